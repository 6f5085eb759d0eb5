#!/usr/bin/env python3
"""Counts of direct_nee's checking build: does the decider of sp_nee_black.h ever
disagree with the true cblack(f)?

    make -C simplepath_amd BUILD=_ab/check EXTRA=-DSP_XP_NEE_CHECK=1
    SP_LIB_PATH=simplepath_amd/_ab/check/libsimplepath_hip.so python tools/nee_check_counts.py            # the test scenes
    SP_LIB_PATH=... SP_TILE_DIAG=/tmp/d.bin python bench.py --no-cpu --steps 1 --warmup 0 [--scene S]    # one bench frame
    python tools/nee_check_counts.py S /tmp/d.bin                                                         # its counts

The checking build runs the glossy estimate on the lanes that skip it as well and adds its counts
into words 0..10 of the SP_TILE_DIAG buffer (sp_path.hpp nee_check, sp_mega.hpp).  One NEECHK line
per render.  Words 0..2 (skipped, run, run_unknown_only) count ballots and mean votes only in a build
with -DSP_NEE_SKIP=1.  profiles/r19/nee_order/check_counts_*.txt are this tool's lines."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAMES = ["skipped", "run", "run_unknown_only", "rode_along", "unknown_lanes", "estimate_lanes", "DISAGREE", "nonfinite",
         "lanes_skipped", "skipped_black", "max_w0_bits"]


def show(tag, path):
    d = np.fromfile(path, dtype=np.uint64)[:11]
    r = dict(zip(NAMES, (int(x) for x in d)))
    r["max_w0"] = float(np.array([r.pop("max_w0_bits")], dtype=np.uint32).view(np.float32)[0])
    print("NEECHK", tag, r, flush=True)
    return r


def main():
    if len(sys.argv) == 3:
        show(sys.argv[1], sys.argv[2])
        return 0
    import simplepath_amd as sp
    import tests.test_gpu_nee_order as t
    d = tempfile.mkdtemp(prefix="nee_check_")
    bad = 0
    for lights in (1, 2):
        s = t.load(t.write_scene(d, lights))
        for integ, kw in (("direct_lighting", dict(pipeline="megakernel", tail_fraction=-1.0)), ("whitted", dict(pipeline="megakernel"))):
            f = os.path.join(d, "diag.bin")
            os.environ["SP_TILE_DIAG"] = f
            sp.render_tiles(s, integ, 12, **kw)
            r = show("scene%d %s" % (lights, integ), f)
            bad += r["DISAGREE"] + r["nonfinite"]
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
