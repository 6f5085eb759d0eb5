#!/usr/bin/env python3
"""Resource table of every kernel in a built libsimplepath_hip.so, from the code objects' metadata.

    python tools/kernel_resources.py [lib.so] [--md] [--filter REGEX]

One line per kernel: VGPRs, AGPRs, SGPRs, scratch bytes per lane, static LDS bytes, and the size of
its code in bytes.  Two builds whose tables are equal line for line carry the same kernels; DESIGN.md
§13 records the table of the existing kernels before and after the progressive render was added.
Needs llvm-objdump / llvm-readelf / llvm-cxxfilt of the ROCm LLVM (ROCM_PATH, default /opt/rocm).
"""
from __future__ import annotations

import argparse
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def kernels(lib: str) -> dict:
    tmp = tempfile.mkdtemp(prefix="sp_kres_")
    try:
        so = os.path.join(tmp, "lib.so")
        shutil.copy(lib, so)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, cwd=tmp,
                       stdout=subprocess.DEVNULL)
        out = {}
        for co in sorted(glob.glob(os.path.join(tmp, "lib.so.*amdgcn*"))):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True,
                                   capture_output=True, text=True).stdout
            syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", co], check=True,
                                  capture_output=True, text=True).stdout
            size = {}
            for line in syms.splitlines():
                p = line.split()
                if len(p) >= 8 and p[3] == "FUNC":
                    size[p[7]] = int(p[2], 0)
            cur = None
            for line in notes.splitlines():
                m = re.match(r"\s+-?\s*(\.[a-z_]+):\s+(.*)$", line)
                if not m:
                    continue
                k, v = m.group(1), m.group(2).strip().strip("'")
                if k == ".agpr_count":  # first per-kernel field in the metadata's order
                    cur = {}
                if cur is not None and k in FIELDS:
                    cur[k] = int(v)
                if cur is not None and k == ".name":
                    cur["code"] = size.get(v, 0)
                    out[v] = cur
        names = list(out)
        filt = os.path.join(LLVM, "llvm-cxxfilt")
        dem = subprocess.run([filt if os.path.exists(filt) else "c++filt"], input="\n".join(names), capture_output=True,
                             text=True, check=True).stdout.splitlines()
        return {re.sub(r"^void ", "", d): out[n] for d, n in zip(dem, names)}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("lib", nargs="?", default=os.path.join(ROOT, "simplepath_amd", "_build", "libsimplepath_hip.so"))
    ap.add_argument("--md", action="store_true", help="markdown table")
    ap.add_argument("--filter", default="", help="regex on the demangled kernel name")
    a = ap.parse_args()
    ks = kernels(a.lib)
    rows = [(n, k) for n, k in sorted(ks.items()) if re.search(a.filter, n)]
    if a.md:
        print("| kernel | VGPR | AGPR | SGPR | scratch B | LDS B | code B |")
        print("|---|---|---|---|---|---|---|")
    for n, k in rows:
        short = re.sub(r"\(spd::.*$", "", n).replace("spd::mt_blk4::", "").replace("spd::mt_blk1::", "mt_blk1::")
        v = [k.get(f, 0) for f in FIELDS] + [k["code"]]
        if a.md:
            print(f"| `{short}` | " + " | ".join(str(x) for x in v) + " |")
        else:
            print(f"{short:64s} vgpr {v[0]:4d} agpr {v[1]:4d} sgpr {v[2]:4d} scratch {v[3]:6d} lds {v[4]:6d} code {v[5]:7d}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
