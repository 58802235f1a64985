#!/usr/bin/env python3
"""Are the kernels of two unbundled gfx950 code objects (make -C hive_amd/csrc _obj/<name>.co) the same machine code?  Hashes the bytes of every FUNC symbol and
every 64-byte .kd kernel descriptor and compares by name; nothing is disassembled.  Bytes 16-23 of a descriptor hold the code's offset RELATIVE to the
descriptor, which moves with anything in .text, so they are zeroed first.  Exit status 1 if a symbol of NEW differs from OLD or is missing there.
Usage: python tools/kernel_bytes.py OLD.co NEW.co"""
import hashlib
import subprocess
import sys

READELF = "/opt/rocm/llvm/bin/llvm-readelf"


def symbols(path):
    data = open(path, "rb").read()
    run = lambda flag: subprocess.run([READELF, flag, "-W", path], capture_output=True, text=True, check=True).stdout.splitlines()
    sec = {}  # section index -> (address, file offset)
    for f in (l.replace("[", " ").replace("]", " ").split() for l in run("-S")):
        if len(f) > 5 and f[0].isdigit() and f[2] != "NOBITS":
            sec[f[0]] = (int(f[3], 16), int(f[4], 16))
    out = {}
    for f in (l.split() for l in run("-s")):  # Num: Value Size Type Bind Vis Ndx Name
        if len(f) == 8 and f[6] in sec and (f[3] == "FUNC" or (f[3] == "OBJECT" and f[7].endswith(".kd"))):
            at = int(f[1], 16) - sec[f[6]][0] + sec[f[6]][1]
            raw = bytearray(data[at : at + int(f[2])])
            if f[3] == "OBJECT":
                raw[16:24] = bytes(8)
            out[f[7]] = hashlib.sha256(raw).hexdigest()
    return out


old, new = symbols(sys.argv[1]), symbols(sys.argv[2])
differ = sorted(n for n in new if n in old and new[n] != old[n])
added, removed = sorted(set(new) - set(old)), sorted(set(old) - set(new))
for tag, names in (("DIFFERS", differ), ("ADDED", added), ("REMOVED", removed)):
    for n in names:
        print(f"{tag:8s}{n}")
print(f"{sys.argv[2]}: {len(new)} symbols, {len(new) - len(differ) - len(added)} equal, {len(differ)} differ, {len(added)} added, {len(removed)} removed")
sys.exit(1 if differ or added else 0)
