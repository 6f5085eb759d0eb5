#!/usr/bin/env python3
"""What feature buffers cost beside the render they guide.

    python tools/features_timing.py
    python tools/features_timing.py --scene bunny --spp 1,64,256 --passes 5 --out profiles/r24/features/timing.json

One child process (a fresh process: the library is loaded, the scene parsed and uploaded with the
default options) under its own time limit.  On the scene's bench frame (bunny: 1920 x 1080) it times,
for every sample count,

  features   sp_scene_features with all five outputs into device buffers
  render     the DirectLighting sp_render_tiles into a device buffer, on the same build

in alternating passes -- features, render, features, render ... after one warm-up pass of each, so
that whatever else the machine does falls on both alike -- and once, in passes of its own,

  workaround one centre ray per pixel through sp_scene_trace_rays with normals (what a host did
             before this call existed; aliased: not the render's samples)

A pass's time is the library's own kernel_ms (HIP events around the kernels).  Best, median and
worst pass are recorded, and features / render as the ratio of the medians.  One JSON line goes to
stdout, and to --out when given."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# bench.py SCENES: writer, width, height
CONFIGS = {"bunny": ("write_bunny_scene", 1920, 1080), "bunny_scan": ("write_bunny_scan_scene", 1920, 1080),
           "lucy": ("write_lucy_scene", 1920, 1080)}


def summary(ms):
    s = sorted(ms)
    return {"best_ms": s[0], "median_ms": s[len(s) // 2], "worst_ms": s[-1], "passes": len(s)}


def child(spec: dict) -> None:
    sys.path.insert(0, spec["root"])
    import numpy as np
    import torch
    import simplepath_amd as sp
    sys.path.insert(0, os.path.join(spec["root"], "tools"))
    from ray_query_timing import camera_rays
    w, h = spec["width"], spec["height"]
    scene = sp.Scene.from_file(spec["path"])
    scene.set_resolution(w, h)
    scene.upload(device=spec["device"])
    tiles = sp.TileScheduler(w, h).get_num_tiles()
    out = {"width": w, "height": h, "tiles": tiles, "bvh_info": scene.bvh_info(), "build_id": sp.lib().sp_build_id().decode(),
           "spp": {}}
    image = torch.zeros((tiles, 64, 3), dtype=torch.float32, device="cuda")
    bufs = {"ids": torch.zeros((tiles, 64, 4), dtype=torch.int32, device="cuda"),
            "coverage": torch.zeros((tiles, 64), dtype=torch.float32, device="cuda"),
            "depth": torch.zeros((tiles, 64), dtype=torch.float32, device="cuda"),
            "normal": torch.zeros((tiles, 64, 3), dtype=torch.float32, device="cuda"),
            "albedo": torch.zeros((tiles, 64, 3), dtype=torch.float32, device="cuda")}
    ptrs = {k + "_ptr": v.data_ptr() for k, v in bufs.items()}
    torch.cuda.synchronize()
    for spp in spec["spp"]:
        f_ms, r_ms, f_st, r_st = [], [], None, None
        for p in range(1 + spec["passes"]):
            f_st = scene.features_device(spp, **ptrs, stats=True)
            r_st = sp.render_tiles_device(scene, "direct_lighting", spp, None, image.data_ptr())
            if p:
                f_ms.append(f_st["kernel_ms"])
                r_ms.append(r_st.kernel_ms)
        f, r = summary(f_ms), summary(r_ms)
        out["spp"][str(spp)] = {"features": dict(f, camera_rays=f_st["camera_rays"], hits=f_st["hits"],
                                                 mrays_per_s_median=f_st["camera_rays"] / f["median_ms"] / 1e3),
                                "render": dict(r, rays=r_st.rays, pipeline=r_st.pipeline),
                                "features_over_render": f["median_ms"] / r["median_ms"]}
    rays = camera_rays(scene, w, h)
    n = rays.shape[0]
    d_rays = torch.from_numpy(rays.view(np.float32).reshape(n, 8).copy()).cuda()
    d_hits = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    d_nrm = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ms = []
    for p in range(1 + spec["passes"]):
        st = scene.trace_device(d_rays.data_ptr(), n, hits_ptr=d_hits.data_ptr(), normals_ptr=d_nrm.data_ptr(), stats=True)
        if p:
            ms.append(st["kernel_ms"])
    out["workaround"] = dict(summary(ms), rays=n, hits=st["hits"],
                             bytes_moved=n * (32 + 32 + 16))  # ray, hit record and normal per pixel, per sample
    print("features_timing_child " + json.dumps(out), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="bunny", choices=sorted(CONFIGS))
    ap.add_argument("--spp", default="1,64,256")
    ap.add_argument("--passes", type=int, default=5, help="timed passes of each arm, after one warm-up pass")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds for the child")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(json.loads(args.child))
        return 0
    sys.path.insert(0, ROOT)
    from simplepath_amd import scenes
    writer, w, h = CONFIGS[args.scene]
    path = getattr(scenes, writer)(tempfile.mkdtemp(prefix="sp_features_timing_"))
    spec = dict(path=path, width=args.width or w, height=args.height or h, spp=[int(s) for s in args.spp.split(",")],
                passes=args.passes, device=args.device, root=ROOT)
    line = {"scene": args.scene}
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", json.dumps(spec)], capture_output=True, text=True,
                           timeout=args.timeout)
    except subprocess.TimeoutExpired:
        line["error"] = f"no result within {args.timeout} s"
        print(json.dumps(line), flush=True)
        return 1
    if r.returncode != 0:
        line["error"] = (r.stderr or r.stdout)[-600:]
        print(json.dumps(line), flush=True)
        return 1
    for text in r.stdout.splitlines():
        if text.startswith("features_timing_child "):
            line.update(json.loads(text[len("features_timing_child "):]))
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
