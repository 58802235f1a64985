"""The sparse merge without a GPU: the torch forms of its passes on CPU tensors, two gloo ranks merging raw accumulator planes sparse and dense (bit for
bit; the CPU oracle stands in for the fold kernel, as in tests/test_distributed_cpu.py), the cost model's closed forms, and the argument checks."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest

from test_sparse_merge_gpu import _planes, _same_words, _sums  # the seeded planes and their five sums (host code)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("n, segment", [(1, 64), (512, 256), (385, 64), (385, 256), (10080, 256)])
def test_unpack_of_pack_restores_the_active_voxels_and_leaves_the_rest(n, segment, world):
    import torch
    from hive_amd import distributed as hdist
    n_segments = -(-n // segment)
    active = np.arange(n_segments) % 3 == 0
    active[-1] = True
    sums = _sums(_planes(n, segment, active, seed=n))
    flags = hdist.segment_flags(sums[1], segment)
    assert np.array_equal(flags.numpy(), active.astype(np.uint8))
    seg_list = torch.nonzero(flags).reshape(-1).to(torch.int32)
    per = -(-seg_list.numel() // world)
    pieces = hdist.pack_segments(sums, seg_list, segment, world)
    assert tuple(pieces.shape) == (world, 5, per * segment) and pieces.is_contiguous()
    k = seg_list.numel() - 1  # the last list entry sits in piece k // per at segment slot k % per; the lanes past N are zeros
    last = pieces[k // per, :, (k % per) * segment:(k % per + 1) * segment]
    assert torch.equal(last[:, :n - (n_segments - 1) * segment], sums[:, (n_segments - 1) * segment:]) and not last[:, n - (n_segments - 1) * segment:].any()
    out = torch.full((5, n), -3.0)
    assert hdist.unpack_segments(pieces, seg_list, segment, out) is out
    inside = torch.from_numpy(np.repeat(active, segment)[:n])
    assert torch.equal(out[:, inside], sums[:, inside]) and bool((out[:, ~inside] == -3.0).all())


def test_a_negative_zero_weight_is_active():
    import torch
    from hive_amd import distributed as hdist
    w = torch.zeros(200)
    assert not hdist.segment_flags(w, 64).any()
    w[130] = -0.0
    assert hdist.segment_flags(w, 64).tolist() == [0, 0, 1, 0]


def _fold(mine, round_mode):
    """[5, chunk] summed planes -> [3, chunk] (tsdf, weight, colour) with the oracle's statement of the fold."""
    import torch
    import oracle
    acc = np.ascontiguousarray(mine.numpy())
    chunk = acc.shape[1]
    share = [np.zeros(chunk, np.float32) for _ in range(3)]
    if chunk:
        oracle.lib().oracle_tsdf_accum_finalize(acc.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(chunk), share[0].ctypes.data_as(ctypes.c_void_p),
                                                share[1].ctypes.data_as(ctypes.c_void_p), share[2].ctypes.data_as(ctypes.c_void_p), round_mode)
    return torch.from_numpy(np.stack(share))


def _worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    from hive_amd import distributed as hdist
    hdist.init_from_env(backend="gloo")
    n, out = 10080, {}
    for segment in (256, 64):
        s = np.arange(-(-n // segment))
        accum = _sums(_planes(n, segment, s % (4 if rank == 0 else 3) == 0, seed=100 * rank + segment))  # raw accumulator planes [5, n]
        # dense: every voxel through the two collectives
        part = hdist.VoxelPartition(n)
        share = _fold(hdist.reduce_scatter_pieces(hdist.shard_layout(accum, part), part), 1)
        gathered = hdist.all_gather_pieces(share, part)
        dense = torch.stack([torch.cat([gathered[r, k, :part.count_of(r)] for r in range(world)]) for k in range(3)])
        # sparse: the united active segments alone; the volume keeps its initial values elsewhere
        flags = hdist.unite_segment_flags(hdist.segment_flags(accum[1], segment))
        seg_list = torch.nonzero(flags).reshape(-1).to(torch.int32)
        part = hdist.VoxelPartition(seg_list.numel() * segment, align=segment)
        assert part.chunk == -(-seg_list.numel() // world) * segment
        share = _fold(hdist.reduce_scatter_pieces(hdist.pack_segments(accum, seg_list, segment, world), part), 1)
        gathered = hdist.all_gather_pieces(share, part)
        sparse = torch.stack([torch.ones(n), torch.zeros(n), torch.zeros(n)])
        hdist.unpack_segments(gathered, seg_list, segment, sparse)
        out[f"dense_{segment}"], out[f"sparse_{segment}"] = dense.numpy(), sparse.numpy()
        out[f"stats_{segment}"] = np.array([seg_list.numel(), flags.numel()])
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **out)
    hdist.barrier()
    torch.distributed.destroy_process_group()


def test_two_rank_sparse_and_dense_merges_of_accumulators_agree_bit_for_bit(tmp_path, oracle_lib):
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.start_processes(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    r0, r1 = (np.load(str(tmp_path / f"rank{r}.npz")) for r in range(2))
    for segment in (256, 64):
        active, segments = (int(v) for v in r0[f"stats_{segment}"])
        assert 0.4 <= active / segments <= 0.6
        dense = r0[f"dense_{segment}"]
        assert (dense[1] > 5).any() and (dense[0] != 1.0).any()
        for got in (r0[f"sparse_{segment}"], r1[f"sparse_{segment}"], r1[f"dense_{segment}"]):
            assert _same_words(got, dense)


def test_merge_plan_bytes_match_the_closed_forms_and_the_choice():
    from hive_amd import distributed as hdist
    n = 512 ** 3
    for world in (2, 4, 8):
        for segment in (64, 256, 1024):
            n_segments = n // segment
            for n_active in (0, 1, n_segments // 3, n_segments):
                plan = hdist.merge_plan(n, n_active * segment, world, segment=segment)
                assert plan["segments"] == n_segments and plan["active"] == n_active
                assert plan["bytes_dense"] == (5 + 3) * 4 * n * (world - 1) / world
                assert plan["bytes_sparse"] == (5 + 3) * 4 * n_active * segment * (world - 1) / world + n_segments
                assert plan["mode"] == ("sparse" if plan["ms_sparse"] < plan["ms_dense"] else "dense")
    assert hdist.merge_plan(385, 65, 2, segment=64)["active"] == 2 and hdist.merge_plan(385, 385, 2, segment=64)["segments"] == 7  # (both round up)
    assert hdist.merge_plan(n, n, 8)["mode"] == "dense"  # full activity: the flags and the mark pass are pure overhead
    bench = hdist.merge_plan(n, 45_600_000, 8)  # the benchmark scene: 45.6 M of 134 M voxels carry a weight
    assert bench["mode"] == "sparse" and bench["bytes_sparse"] < 0.36 * bench["bytes_dense"]
    # the rates are arguments: a link ten times as fast shrinks both link terms alike
    slow, fast = hdist.merge_plan(n, n // 3, 8), hdist.merge_plan(n, n // 3, 8, link_gbs=10 * hdist.XGMI_LINKS * hdist.XGMI_LINK_GBS)
    assert fast["ms_dense"] < slow["ms_dense"] and fast["bytes_dense"] == slow["bytes_dense"]


def test_bad_arguments_raise_value_errors():
    from hive_amd import distributed as hdist
    for kwargs in ({"merge": "sparce"}, {"merge": None}, {"segment": 0}, {"segment": 96}, {"segment": 32}, {"segment": 8192}, {"segment": "256"}, {"segment": True}):
        with pytest.raises(ValueError):
            hdist.fuse_sharded(None, **kwargs)  # (before the volume is looked at, and before any collective)
        with pytest.raises(ValueError):
            hdist.tsdf_fusion_fg_bg_sharded(None, **kwargs)
    for args in ((0, 0, 2), (100, 101, 2), (100, -1, 2), (100, 50, 0)):
        with pytest.raises(ValueError):
            hdist.merge_plan(*args)
    with pytest.raises(ValueError):
        hdist.merge_plan(1000, 10, 2, segment=100)
