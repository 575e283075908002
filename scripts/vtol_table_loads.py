#!/usr/bin/env python3
"""How the vtolUAV kernels read the obstacle table: compile the two vtol translation units to gfx950 ISA (no GPU needed) and
count, per kernel family, the vector memory loads and the scalar loads that sit inside nested loops -- the obstacle loop
within the RK4 step loop, where the only memory the code reads is the table.  A vector load there is the table read through the
vector memory path (a uniform address in every lane); the expected count is 0.

    python scripts/vtol_table_loads.py            # prints one line per family and translation unit; exit 1 on a vector load"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = {"kernels_vtol": ["-ffp-contract=off"], "kernels_vtol_fast": ["-ffp-contract=fast"]}


def count(isa):
    families, cur, nested = {}, None, False
    for line in isa.splitlines():
        m = re.match(r"^_ZN4socp\d+([a-z_]+?)_kernel\S*:", line)
        if m:
            cur, nested = m.group(1), False
            families.setdefault(cur, [0, 0, 0])[0] += 1
            continue
        if ".end_amdhsa_kernel" in line:
            cur = None
        if cur is None:
            continue
        if line.startswith(".LBB") or line.startswith("; %bb"):      # a new block: outside any loop unless its comments say otherwise
            nested = False
        d = re.search(r"Depth=(\d+)", line)                           # "in Loop: Header=.. Depth=N" / "Parent Loop .. Depth=N" / "Inner Loop Header: Depth=N"
        if d:
            nested = int(d.group(1)) >= 2
        if nested:
            if re.search(r"\b(global|flat|buffer)_load", line):
                families[cur][1] += 1
            if "s_load_dword" in line:
                families[cur][2] += 1
    return families


def main():
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for unit, flags in UNITS.items():
            out = os.path.join(tmp, unit + ".s")
            subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S"] + flags +
                                  ["-I" + os.path.join(ROOT, "socp_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                                   os.path.join(ROOT, "socp_amd", "csrc", unit + ".hip"), "-o", out])
            for fam, (n, vec, sca) in count(open(out).read()).items():
                print("%-18s %-14s %2d kernels: vector loads inside nested loops %3d, scalar loads %3d" % (unit, fam, n, vec, sca))
                bad += vec
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
