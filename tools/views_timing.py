#!/usr/bin/env python3
"""What one launch of V views gains over V launches.

    python tools/views_timing.py --parent ../parent_checkout
    python tools/views_timing.py --rows 6x128x128,4x1920x1080 --rounds 2

Workload: bunny.sp, DirectLighting, --spp samples, V views of W x H, every view the scene's own
camera, so all arms do equal work and must write equal bytes (asserted: the run fails otherwise).

  views        this build: one sp_render_views call with V copies of the scene's camera
  tiles_mega   --parent's build (a checkout of the parent commit with its library built; this build
               when not given): V sp_render_tiles calls of the frame enqueued back to back with
               stats=None into the V slices of one buffer, pipeline="megakernel"
  tiles_auto   the same with the automatic pipeline

Every arm runs in a child process of its own (a fresh process: library loaded, scene parsed and
uploaded with the default options), each child under its own time limit, and the run ends at the
first child that fails.  A child makes one warm-up call, then --calls timed ones; a call's time is
the host clock from before the first enqueue to after a device synchronise.  The arms of a row
alternate: the row's arms in order, --rounds times.  One JSON line per child goes to stdout, then
one summary line per row and arm: the median and range of all its timed calls."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = "6x128x128,16x256x256,64x256x256,4x1920x1080"
ARMS = ("views", "tiles_mega", "tiles_auto")


def child(spec: dict) -> None:
    sys.path.insert(0, spec["root"])
    import torch
    import simplepath_amd as sp
    scene = sp.Scene.from_file(spec["path"])
    scene.set_resolution(spec["width"], spec["height"])
    scene.upload(device=spec["device"])
    v, spp = spec["views"], spec["spp"]
    n = sp.TileScheduler(spec["width"], spec["height"]).get_num_tiles()
    out = torch.zeros((v, n, 64, 3), dtype=torch.float32, device="cuda")
    arm = spec["arm"]
    if arm == "views":
        cams = [scene.desc().camera] * v

        def call():
            sp.render_views_device(scene, "direct_lighting", spp, cams, None, out.data_ptr(), stats=False)
    else:
        pipeline = "megakernel" if arm == "tiles_mega" else "auto"

        def call():
            for k in range(v):
                sp.render_tiles_device(scene, "direct_lighting", spp, None, out[k].data_ptr(), pipeline=pipeline, stats=False)
    ms = []
    for i in range(1 + spec["calls"]):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if i:
            ms.append((time.perf_counter() - t0) * 1e3)
    res = {"arm": arm, "views": v, "width": spec["width"], "height": spec["height"], "spp": spp, "tiles_per_view": n,
           "ms": ms, "sha256": hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest(),
           "build_id": sp.lib().sp_build_id().decode(), "cus": torch.cuda.get_device_properties(0).multi_processor_count}
    print("views_timing_child " + json.dumps(res), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default=ROWS, help="comma-separated VxWxH")
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--parent", default=None, help="root of the parent commit's checkout, built (the tiles arms)")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--calls", type=int, default=5, help="timed calls per child, after one warm-up call")
    ap.add_argument("--rounds", type=int, default=2, help="times the arms of a row are run in turn")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds per child")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(json.loads(args.child))
        return 0
    sys.path.insert(0, ROOT)
    from simplepath_amd import scenes
    path = scenes.write_bunny_scene(tempfile.mkdtemp(prefix="sp_views_timing_"))
    parent = os.path.abspath(args.parent) if args.parent else ROOT
    for row in args.rows.split(","):
        v, w, h = (int(x) for x in row.split("x"))
        times, shas = {}, set()
        for _ in range(args.rounds):
            for arm in args.arms.split(","):
                spec = dict(arm=arm, views=v, width=w, height=h, spp=args.spp, calls=args.calls, device=args.device, path=path,
                            root=ROOT if arm == "views" else parent)
                line = {"row": row, "arm": arm}
                try:
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", json.dumps(spec)],
                                       capture_output=True, text=True, timeout=args.timeout)
                except subprocess.TimeoutExpired:
                    line["error"] = f"no result within {args.timeout} s"
                    print(json.dumps(line), flush=True)
                    return 1
                if r.returncode != 0:
                    line["error"] = (r.stderr or r.stdout)[-400:]
                    print(json.dumps(line), flush=True)
                    return 1  # nothing more is started on the device after a failed child
                for text in r.stdout.splitlines():
                    if text.startswith("views_timing_child "):
                        line.update(json.loads(text[len("views_timing_child "):]))
                print(json.dumps(line), flush=True)
                times.setdefault(arm, []).extend(line["ms"])
                shas.add(line["sha256"])
        if len(shas) != 1:
            print(json.dumps({"row": row, "error": "the arms wrote different images", "sha256": sorted(shas)}), flush=True)
            return 1
        for arm, ms in times.items():
            print(json.dumps({"row": row, "summary": arm, "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
                              "calls": len(ms)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
