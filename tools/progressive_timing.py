#!/usr/bin/env python3
"""What does resuming cost?  One-shot megakernel frames against progressive renders of the same frame
in 1, 4 and 16 passes, HIP-event times, one JSON line per case.

    python tools/progressive_timing.py [--scene bunny] [--width 1920 --height 1080] [--spp 256]
                                       [--integrator direct_lighting] [--bvh 0] [--repeats 5]
                                       [--cases oneshot,1,4,16] [--tree DIR] [--label TEXT]

Cases: `oneshot` is render_tiles(pipeline="megakernel", tail_fraction=-1) -- the form progressive
calls run, without tail chunks; a number N is a progressive render in N equal passes (spp / N samples
each), timed from the first pass's launch to the last one's end with nothing but the passes in
between (no host wait: the calls only enqueue).  Every case renders one warm-up frame first, then
`repeats` timed frames; the line gives their median, min and max, and checks the progressive image
against the one-shot image bit for bit.  A fresh progress object per frame (created outside the timed
window).  --tree imports simplepath_amd from another built checkout (the parent commit's, for the
`oneshot` case there); the line records the library's build id either way.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="bunny")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--integrator", default="direct_lighting")
    ap.add_argument("--bvh", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cases", default="oneshot,1,4,16")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.repeats < 5:
        ap.error("--repeats must be at least 5")
    sys.path.insert(0, os.path.abspath(a.tree))
    import numpy as np
    import torch

    import simplepath_amd as sp
    from simplepath_amd import _abi, scenes

    if not torch.cuda.is_available():
        print("progressive_timing: no GPU", file=sys.stderr)  # a measurement path does not fall back
        return 1
    d = tempfile.mkdtemp(prefix="sp_ptime_")
    path = getattr(scenes, f"write_{a.scene}_scene")(d)
    scene = sp.Scene.from_file(path)
    scene.set_resolution(a.width, a.height)
    scene.upload(device=0, bvh_mode=a.bvh)
    n_tiles = sp.TileScheduler(a.width, a.height).get_num_tiles()
    dev = torch.device("cuda:0")
    out = torch.zeros((n_tiles, 64, 3), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream()
    ident = _abi.build_identity()
    base = {"scene": a.scene, "width": a.width, "height": a.height, "spp": a.spp, "integrator": a.integrator, "bvh": a.bvh,
            "tiles": n_tiles, "repeats": a.repeats, "build_id": ident["build_id"], "so_sha256_16": ident["so_sha256_16"],
            "label": a.label, "device": torch.cuda.get_device_name(0)}

    def timed(enqueue):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        enqueue()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def oneshot():
        sp.render_tiles_device(scene, a.integrator, a.spp, None, out.data_ptr(), stream.cuda_stream, pipeline="megakernel",
                               stats=False, tail_fraction=-1.0)

    # the one-shot image and its ray count: every progressive case must reproduce them
    ref_stats = sp.render_tiles_device(scene, a.integrator, a.spp, None, out.data_ptr(), stream.cuda_stream,
                                       pipeline="megakernel", tail_fraction=-1.0)
    torch.cuda.synchronize()
    ref = out.cpu().numpy().copy()

    for case in a.cases.split(","):
        line = dict(base)
        if case == "oneshot":
            times = [timed(oneshot) for _ in range(a.repeats + 1)][1:]
            line.update(case="oneshot", passes=0, state_bytes=0)
        else:
            passes = int(case)
            if a.spp % passes:
                ap.error("spp must be a multiple of the passes")
            k = a.spp // passes
            times, exact, state_bytes = [], True, 0
            for rep in range(a.repeats + 1):
                prog = sp.Progressive(scene, a.integrator)
                state_bytes = prog.device_bytes
                out.zero_()

                def run():
                    for _ in range(passes):
                        prog.render(k, out.data_ptr(), stream.cuda_stream, stats=False)

                t = timed(run)
                if rep:
                    times.append(t)
                else:
                    exact = bool(np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32)))
                prog.close()
            line.update(case=f"progressive_{passes}x{k}", passes=passes, state_bytes=state_bytes, bit_exact_vs_oneshot=exact)
        med = statistics.median(times)
        line.update(ms_median=round(med, 3), ms_min=round(min(times), 3), ms_max=round(max(times), 3),
                    ms_all=[round(t, 3) for t in times], mrays_per_s=round(ref_stats.rays / med / 1e3, 1))
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
