#!/usr/bin/env python3
"""What radiance along a caller's rays costs beside a render of the same integrate calls (DESIGN.md
section 28).

    python tools/radiance_timing.py --parent ../parent_checkout
    python tools/radiance_timing.py --integrators direct_lighting --samples 1,16 --rounds 1

Workload: bunny.sp at --size (1920 x 1080), DirectLighting and IterativeRRNEE, 1, 16 and 64 samples.
The rays are the frame's first-sample camera rays, one per pixel, made on the host: the R2 sequence's
first point is (0.75487766, 0.56984029) in every pixel (its seed term is below float precision), the
direction is normalised in float32 (to within rounding of the render's own), and the seed is the
pixel's own, pixel_seed(x, y).

  radiance_morton  this build: one sp_scene_radiance_rays call, the records in the render's order --
                   tile after tile, Morton order inside a tile -- so a wave's 64 records are a tile
  radiance_rows    the same records in row order (y * width + x): a wave's 64 records are a strip
  tiles            --parent's build (a checkout of the parent commit with its library built; this build
                   when not given): sp_render_tiles of the frame, pipeline="megakernel", tail chunks
                   off, at the same sample count: the same number of integrate calls

Every arm runs in a child process of its own (a fresh process: library loaded, scene parsed and
uploaded with the default options), each child under its own time limit, and the run ends at the
first child that fails.  A child makes one warm-up call, then --calls timed ones; a call's time is
the host clock from before the enqueue to after a device synchronise.  The arms of a row alternate:
the row's arms in order, --rounds times.  One JSON line per child goes to stdout, then one summary
line per row and arm with the median and range of all its timed calls, and per integrator the fixed
share of a one-sample call: with t(N) = fixed + N * per_sample fitted through the medians at the two
largest sample counts, fixed / t(1) -- the 312-word seeding of every record's generator, the launch
and the first twist.  The two radiance arms must write the same radiance for every pixel (asserted)."""
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
ARMS = ("radiance_morton", "tiles", "radiance_rows")
R2_FIRST = (0.7548776662466927, 0.5698402909980532)


def pixel_order(width: int, height: int, order: str):
    """(x, y) of every pixel of the frame: row order, or the render's tile-packed order"""
    import numpy as np
    if order == "rows":
        y, x = np.divmod(np.arange(width * height, dtype=np.int64), width)
        return x, y
    tx, ty = (width + 7) // 8, (height + 7) // 8
    m = np.arange(64)
    dx = (m & 1) | (((m >> 2) & 1) << 1) | (((m >> 4) & 1) << 2)
    dy = ((m >> 1) & 1) | (((m >> 3) & 1) << 1) | (((m >> 5) & 1) << 2)
    t = np.arange(tx * ty, dtype=np.int64)
    x = ((t % tx) * 8)[:, None] + dx[None, :]
    y = ((t // tx) * 8)[:, None] + dy[None, :]
    inside = (x < width) & (y < height)
    return x[inside], y[inside]


def camera_rays(sp, scene, x, y):
    """RADIANCE_RAY_DTYPE records: the first-sample camera ray and the sampler seed of pixels (x, y)"""
    import numpy as np
    t = scene.desc().camera.transform
    vx, vy, vz, p = (np.array(list(a), dtype=np.float32) for a in (t.vx, t.vy, t.vz, t.p))
    fx = (x.astype(np.float32) + np.float32(R2_FIRST[0]))[:, None]
    fy = (y.astype(np.float32) + np.float32(R2_FIRST[1]))[:, None]
    d = (fx * vx[None, :] + fy * vy[None, :]) + vz[None, :]
    d = (d / np.sqrt(np.sum(d * d, axis=1, keepdims=True, dtype=np.float32))).astype(np.float32)
    return sp.make_radiance_rays(np.broadcast_to(p, d.shape), d, sp.pixel_seed(x, y))


def child(spec: dict) -> None:
    sys.path.insert(0, spec["root"])
    import numpy as np
    import torch
    import simplepath_amd as sp
    scene = sp.Scene.from_file(spec["path"])
    w, h = spec["width"], spec["height"]
    scene.set_resolution(w, h)
    scene.upload(device=spec["device"])
    arm, integ, spp = spec["arm"], spec["integrator"], spec["samples"]
    res = {"arm": arm, "integrator": integ, "samples": spp, "width": w, "height": h}
    if arm == "tiles":
        n = sp.TileScheduler(w, h).get_num_tiles()
        out = torch.zeros((n, 64, 3), dtype=torch.float32, device="cuda")

        def call():
            return sp.render_tiles_device(scene, integ, spp, None, out.data_ptr(), pipeline="megakernel", tail_fraction=-1.0,
                                          stats=False)
        stats = lambda: sp.render_tiles_device(scene, integ, spp, None, out.data_ptr(), pipeline="megakernel", tail_fraction=-1.0)
    else:
        x, y = pixel_order(w, h, "rows" if arm == "radiance_rows" else "morton")
        rays = camera_rays(sp, scene, x, y)
        n = rays.shape[0]
        d_rays = torch.from_numpy(rays.view(np.int32).reshape(n, 8)).cuda()
        out = torch.zeros((n, 3), dtype=torch.float32, device="cuda")

        def call():
            return scene.radiance_device(d_rays.data_ptr(), n, out.data_ptr(), integ, spp, stats=False)
        stats = lambda: scene.radiance_device(d_rays.data_ptr(), n, out.data_ptr(), integ, spp)
    ms = []
    for i in range(1 + spec["calls"]):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if i:
            ms.append((time.perf_counter() - t0) * 1e3)
    st = stats()  # (after the timed calls: this one waits and reads the counters)
    img = out.cpu().numpy()
    if arm != "tiles":  # to row order, so the two radiance arms hash alike
        rows = np.zeros((h, w, 3), dtype=np.float32)
        rows[y, x] = img
        img = rows
    res.update(ms=ms, records=int(n), rays=int(st.rays), shadow_rays=int(st.shadow_rays), integrate_calls=int(st.samples),
               rng_draws=int(st.rng_draws), kernel_ms=float(st.kernel_ms), sha256=hashlib.sha256(img.tobytes()).hexdigest(),
               build_id=sp.lib().sp_build_id().decode(), cus=torch.cuda.get_device_properties(0).multi_processor_count)
    print("radiance_timing_child " + json.dumps(res), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--integrators", default="direct_lighting,iterative_rrnee")
    ap.add_argument("--samples", default="1,16,64")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--parent", default=None, help="root of the parent commit's checkout, built (the tiles arm)")
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
    path = scenes.write_bunny_scene(tempfile.mkdtemp(prefix="sp_radiance_timing_"))
    parent = os.path.abspath(args.parent) if args.parent else ROOT
    w, h = (int(v) for v in args.size.split("x"))
    samples = sorted(int(v) for v in args.samples.split(","))
    for integ in args.integrators.split(","):
        medians = {}
        for spp in samples:
            row = f"{integ}@{spp}"
            times, shas = {}, {}
            for _ in range(args.rounds):
                for arm in args.arms.split(","):
                    spec = dict(arm=arm, integrator=integ, samples=spp, width=w, height=h, calls=args.calls, device=args.device,
                                path=path, root=parent if arm == "tiles" else ROOT)
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
                        if text.startswith("radiance_timing_child "):
                            line.update(json.loads(text[len("radiance_timing_child "):]))
                    print(json.dumps(line), flush=True)
                    times.setdefault(arm, []).extend(line["ms"])
                    shas.setdefault(arm, set()).add(line["sha256"])
            radiance = set().union(*[v for a, v in shas.items() if a != "tiles"]) if any(a != "tiles" for a in shas) else set()
            if len(radiance) > 1 or any(len(v) != 1 for v in shas.values()):
                print(json.dumps({"row": row, "error": "the radiance arms wrote different radiance",
                                  "sha256": {a: sorted(v) for a, v in shas.items()}}), flush=True)
                return 1
            for arm, ms in times.items():
                medians[(arm, spp)] = statistics.median(ms)
                print(json.dumps({"row": row, "summary": arm, "median_ms": statistics.median(ms), "min_ms": min(ms),
                                  "max_ms": max(ms), "calls": len(ms)}), flush=True)
        if len(samples) >= 3 and samples[0] == 1:
            a, b = samples[-2], samples[-1]
            for arm in args.arms.split(","):
                if (arm, a) not in medians:
                    continue
                per_sample = (medians[(arm, b)] - medians[(arm, a)]) / (b - a)
                fixed = medians[(arm, 1)] - per_sample
                print(json.dumps({"integrator": integ, "summary": arm, "per_sample_ms": per_sample, "fixed_ms": fixed,
                                  "fixed_share_at_1": fixed / medians[(arm, 1)]}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
