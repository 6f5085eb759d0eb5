#!/usr/bin/env python3
"""What the denoiser costs beside the preview frame it cleans.

    python tools/denoise_timing.py
    python tools/denoise_timing.py --scene bunny --iterations 5 --passes 5 --out profiles/r25/denoise/timing.json

One child process (a fresh process: the library is loaded, the scene parsed and uploaded with the
default options) under its own time limit.  On the scene's bench frame (bunny: 1920 x 1080) it
renders a 1-spp DirectLighting frame and its feature buffers into device memory and then times, in
alternating passes after one warm-up pass of each,

  denoise    sp_denoiser_run with all four guides and demodulation, `--iterations` levels
  render     the DirectLighting sp_render_tiles at every count of --spp
  features   sp_scene_features with all five outputs at 1 sample

and, in passes of its own, the denoiser at 1 .. `--iterations` levels, so that the difference of two
neighbouring medians is what one more level costs.  A pass's time is the library's own kernel_ms
(HIP events around the kernels).  Best, median and worst pass are recorded.  Per level the filter
must move the pixel's two 16-byte records in and one out (the last level: 12 bytes of albedo in and
12 of colour out instead); bytes over time is printed as GB/s for comparison with the measured HBM
rate.  One JSON line goes to stdout, and to --out when given."""
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
SIGMAS = dict(sigma_color=0.6, sigma_normal=0.3, sigma_depth=0.2, sigma_coverage=0.4)


def summary(ms):
    s = sorted(ms)
    return {"best_ms": s[0], "median_ms": s[len(s) // 2], "worst_ms": s[-1], "passes": len(s)}


def child(spec: dict) -> None:
    sys.path.insert(0, spec["root"])
    import torch
    import simplepath_amd as sp
    w, h = spec["width"], spec["height"]
    scene = sp.Scene.from_file(spec["path"])
    scene.set_resolution(w, h)
    scene.upload(device=spec["device"])
    tiles = sp.TileScheduler(w, h).get_num_tiles()
    out = {"width": w, "height": h, "tiles": tiles, "build_id": sp.lib().sp_build_id().decode(), "iterations": spec["iterations"]}
    image = torch.zeros((tiles, 64, 3), dtype=torch.float32, device="cuda")
    clean = torch.zeros_like(image)
    scratch = torch.zeros_like(image)
    bufs = {"ids": torch.zeros((tiles, 64, 4), dtype=torch.int32, device="cuda"),
            "coverage": torch.zeros((tiles, 64), dtype=torch.float32, device="cuda"),
            "depth": torch.zeros((tiles, 64), dtype=torch.float32, device="cuda"),
            "normal": torch.zeros((tiles, 64, 3), dtype=torch.float32, device="cuda"),
            "albedo": torch.zeros((tiles, 64, 3), dtype=torch.float32, device="cuda")}
    ptrs = {k + "_ptr": v.data_ptr() for k, v in bufs.items()}
    guides = {k: v for k, v in ptrs.items() if k != "ids_ptr"}
    torch.cuda.synchronize()
    sp.render_tiles_device(scene, "direct_lighting", 1, None, image.data_ptr())
    scene.features_device(1, **ptrs, stats=True)
    den = sp.Denoiser.for_scene(scene, device=spec["device"])
    run = lambda n: den.run_device(image.data_ptr(), clean.data_ptr(), **guides, iterations=n, **SIGMAS, stats=True)
    run(1)  # the first run allocates and builds the map
    d_ms, f_ms, r_ms = [], [], {spp: [] for spp in spec["spp"]}
    d_st = f_st = None
    for p in range(1 + spec["passes"]):
        d_st = run(spec["iterations"])
        f_st = scene.features_device(1, **ptrs, stats=True)
        if p:
            d_ms.append(d_st["kernel_ms"])
            f_ms.append(f_st["kernel_ms"])
        for spp in spec["spp"]:
            r_st = sp.render_tiles_device(scene, "direct_lighting", spp, None, scratch.data_ptr())
            if p:
                r_ms[spp].append(r_st.kernel_ms)
    pixels = d_st["pixels"]
    out["denoise"] = dict(summary(d_ms), pixels=pixels, taps=d_st["taps"], launches=d_st["launches"],
                          device_bytes=den.device_bytes)
    out["features_1spp"] = summary(f_ms)
    out["render"] = {str(spp): summary(ms) for spp, ms in r_ms.items()}
    levels, prev = {}, None
    for n in range(1, spec["iterations"] + 1):
        ms = []
        for p in range(1 + spec["passes"]):
            st = run(n)
            if p:
                ms.append(st["kernel_ms"])
        s = summary(ms)
        step_ms = s["median_ms"] - prev if prev is not None else None
        levels[str(n)] = dict(s, one_more_level_ms=step_ms,
                              one_more_level_gb_per_s=(tiles * 64 * 48 / step_ms / 1e6) if step_ms and step_ms > 0 else None)
        prev = s["median_ms"]
    out["levels"] = levels
    out["bytes_per_level"] = tiles * 64 * 48
    den.close()
    print("denoise_timing_child " + json.dumps(out), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="bunny", choices=sorted(CONFIGS))
    ap.add_argument("--spp", default="1,16", help="sample counts of the renders timed beside the filter")
    ap.add_argument("--iterations", type=int, default=5)
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
    path = getattr(scenes, writer)(tempfile.mkdtemp(prefix="sp_denoise_timing_"))
    spec = dict(path=path, width=args.width or w, height=args.height or h, spp=[int(s) for s in args.spp.split(",")],
                iterations=args.iterations, passes=args.passes, device=args.device, root=ROOT)
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
        if text.startswith("denoise_timing_child "):
            line.update(json.loads(text[len("denoise_timing_child "):]))
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
