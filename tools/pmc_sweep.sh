#!/bin/bash
# Counter passes (separate rocprofv3 --pmc runs: no tracing beside them) for integrate_multi_kernel on both scenes of tools/probe_sweep_ab.py.
# Usage: tools/pmc_sweep.sh <outdir-name> [PROBE_ROW_FAR]   -> <outdir-name>/summary.txt in the output directory ($OUT below)
OUT=$GRAFT_REPO_ROOT/gpurun_out/$1
export PROBE_ROW_FAR=${2:-1}  # one mode per run: the averages below are per launch
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
pass() { n=$1; shift; timeout -k 10 150 rocprofv3 --pmc "$@" --output-format csv -d $OUT/p$n -- python3 $GRAFT_REPO_ROOT/tools/probe_sweep_ab.py 16 > $OUT/p$n.log 2>&1 || echo "pass $n failed"; }
pass A SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_ACTIVE_INST_VMEM GRBM_GUI_ACTIVE
pass B SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INST_CYCLES_VMEM_RD SQ_INST_CYCLES_VMEM_WR SQ_ACTIVE_INST_LDS SQ_INSTS_LDS SQ_WAIT_ANY
pass C TA_TA_BUSY_sum TA_ADDR_STALLED_BY_TC_CYCLES_sum TA_DATA_STALLED_BY_TC_CYCLES_sum
pass D TCP_PENDING_STALL_CYCLES_sum TCP_TCC_READ_REQ_LATENCY_sum TCP_TCC_READ_REQ_sum TCP_TCP_LATENCY_sum
pass E TCP_TOTAL_ACCESSES_sum TCP_TCR_TCP_STALL_CYCLES_sum TCP_READ_TAGCONFLICT_STALL_CYCLES_sum TCP_GATE_EN1_sum
pass F FETCH_SIZE
pass G WRITE_SIZE
pass H TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum
python3 - > $OUT/summary.txt <<PY
import csv, glob, collections
for d in sorted(glob.glob("$OUT/p?/")):
    for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
        acc = collections.defaultdict(list)
        for r in csv.DictReader(open(f)):
            if "integrate_multi_kernel" in r["Kernel_Name"]:
                acc[r["Counter_Name"]].append(float(r["Counter_Value"]))
        for k, v in acc.items():
            h = len(v) // 2  # first half of the launches: room scene, second half: dpt scene (probe order)
            a, b = v[:h], v[h:]
            print(f"{k:44s} n={len(v):3d} room avg={sum(a) / max(len(a), 1):16.1f}   dpt avg={sum(b) / max(len(b), 1):16.1f}")
PY
cat $OUT/summary.txt
rm -rf $OUT/p?/
