#!/usr/bin/env python3
"""What does adaptive sampling cost, and what does it save?  (sibling of
tools/progressive_timing.py.)  HIP-event times on one device, one JSON line per case.

    python tools/adaptive_timing.py [--scene bunny] [--width 1920 --height 1080] [--integrator direct_lighting]
                                    [--bvh 0] [--repeats 5] [--cases plain_pass,round_all,round_idle,converge,uniform]
                                    [--step 64] [--threshold 0.05 --min 16 --max 256 --converge-step 32]
                                    [--tree DIR] [--label TEXT]

Cases (each: one warm-up run, then `repeats` timed runs on a fresh object created outside the window):
  plain_pass   one pass of `step` samples on a plain progress object (works on the parent commit's tree: --tree)
  round_all    one adaptive round with every tile active and `step` samples (min = max = step): the
               selection, the compaction, the render kernel with the statistics, no resolve work
  round_idle   one round on a converged object: error + compaction + an empty render launch + the
               resolve of every tile -- the time of the small kernels
  uniform      the uniform frame: one progressive pass of `max` samples on a plain object
  converge     rounds until no tile is active (the host reads active_tiles after each), timed from the
               first round's launch to the last one's end; reports total samples and the histogram of
               per-tile counts
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
    ap.add_argument("--integrator", default="direct_lighting")
    ap.add_argument("--bvh", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cases", default="plain_pass,round_all,round_idle,uniform,converge")
    ap.add_argument("--step", type=int, default=64)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--min", type=int, default=16)
    ap.add_argument("--max", type=int, default=256)
    ap.add_argument("--converge-step", type=int, default=32)
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
        print("adaptive_timing: no GPU", file=sys.stderr)  # a measurement path does not fall back
        return 1
    d = tempfile.mkdtemp(prefix="sp_atime_")
    scene = sp.Scene.from_file(getattr(scenes, f"write_{a.scene}_scene")(d))
    scene.set_resolution(a.width, a.height)
    scene.upload(device=0, bvh_mode=a.bvh)
    n_tiles = sp.TileScheduler(a.width, a.height).get_num_tiles()
    out = torch.zeros((n_tiles, 64, 3), dtype=torch.float32, device=torch.device("cuda:0"))
    stream = torch.cuda.current_stream()
    ident = _abi.build_identity()
    base = {"scene": a.scene, "width": a.width, "height": a.height, "integrator": a.integrator, "bvh": a.bvh, "tiles": n_tiles,
            "repeats": a.repeats, "build_id": ident["build_id"], "so_sha256_16": ident["so_sha256_16"], "label": a.label,
            "device": torch.cuda.get_device_name(0)}

    def timed(enqueue):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        enqueue()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def queued_round(prog, thr, lo, hi, step):
        prog.round(thr, lo, hi, step, out_ptr=out.data_ptr(), stream=stream.cuda_stream, stats=False, result=False)

    for case in a.cases.split(","):
        line, times, extra = dict(base, case=case), [], {}
        for rep in range(a.repeats + 1):
            if case in ("plain_pass", "uniform"):
                k = a.step if case == "plain_pass" else a.max
                prog = sp.Progressive(scene, a.integrator)
                t = timed(lambda: prog.render(k, out.data_ptr(), stream.cuda_stream, stats=False))
                extra = {"samples_per_pixel": k, "state_bytes": prog.device_bytes}
            elif case == "round_all":
                prog = sp.Progressive(scene, a.integrator, adaptive=True)
                t = timed(lambda: queued_round(prog, 0.0, a.step, a.step, a.step))
                extra = {"samples_per_pixel": a.step, "state_bytes": prog.device_bytes,
                         "all_tiles_done": bool((prog.tile_samples() == a.step).all())}
            elif case == "round_idle":
                prog = sp.Progressive(scene, a.integrator, adaptive=True)
                prog.render(2, out.data_ptr(), stream.cuda_stream, stats=False)
                t = timed(lambda: queued_round(prog, 0.0, 2, 2, 1))
                extra = {"active_tiles": prog.round(0.0, 2, 2, 1, out_ptr=out.data_ptr())[2].active_tiles}
            elif case == "converge":
                prog = sp.Progressive(scene, a.integrator, adaptive=True)
                log = []

                def run():
                    while True:
                        _, _, res = prog.round(a.threshold, a.min, a.max, a.converge_step, out_ptr=out.data_ptr(),
                                               stream=stream.cuda_stream, stats=False)
                        log.append(res.active_tiles)
                        if res.active_tiles == 0:
                            return

                t = timed(run)
                done = prog.tile_samples()
                c, n = np.unique(done, return_counts=True)
                extra = {"threshold": a.threshold, "min_samples": a.min, "max_samples": a.max, "step": a.converge_step,
                         "rounds": len(log), "active_per_round": log, "tile_samples_total": int(done.sum(dtype=np.int64)),
                         "uniform_tile_samples_total": int(n_tiles) * a.max,
                         "histogram": {int(k): int(v) for k, v in zip(c, n)}}
            else:
                ap.error(f"unknown case {case}")
            prog.close()
            if rep:
                times.append(t)
        med = statistics.median(times)
        line.update(extra, ms_median=round(med, 3), ms_min=round(min(times), 3), ms_max=round(max(times), 3),
                    ms_all=[round(t, 3) for t in times])
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
