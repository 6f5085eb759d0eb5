#!/usr/bin/env python3
"""What a bare walk costs: the rates of sp_scene_trace_rays on a resident scene.

    python tools/ray_query_timing.py --scene bunny
    python tools/ray_query_timing.py --scene bunny --arms camera,random --calls 5

Each arm runs in a child process of its own (a fresh process: the library is loaded, the scene
parsed and uploaded with the default options), each child under its own time limit, and the run
ends at the first child that fails:

  camera          closest hit on one pinhole ray through every pixel centre of the frame, built on the
                  host from desc().camera (origin p, direction (x + 0.5) vx + (y + 0.5) vy + vz,
                  normalised in float32: not the reference's camera rays bit for bit), in row order
  camera_normals  the same rays with the shading normals
  random          any hit, then closest hit, on as many rays from a sphere around the mesh's
                  bounding box towards uniformly random points inside it
  bench           the default render of the same frame (bench.py's configuration of the scene): its
                  Mrays/s counts shading too and stands beside the others as context, not as a bar

Rays and outputs are torch device tensors; a call's time is the library's own kernel_ms (HIP events
around the query kernel), --calls timed calls after one warm-up call.  Mrays/s is rays / kernel_ms;
the best and the median call are recorded.  One JSON line per child goes to stdout."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# bench.py SCENES: writer, width, height, spp, integrator
CONFIGS = {"bunny": ("write_bunny_scene", 1920, 1080, 256, "direct_lighting"),
           "bunny_scan": ("write_bunny_scan_scene", 1920, 1080, 256, "direct_lighting"),
           "lucy": ("write_lucy_scene", 1920, 1080, 256, "direct_lighting")}


def camera_rays(scene, width, height):
    import numpy as np
    import simplepath_amd as sp
    F = np.float32
    cam = scene.desc().camera.transform
    vx, vy, vz, p = (np.array(list(c), dtype=F) for c in (cam.vx, cam.vy, cam.vz, cam.p))
    fx = (np.arange(width, dtype=F) + F(0.5))[None, :, None]
    fy = (np.arange(height, dtype=F) + F(0.5))[:, None, None]
    d = (fx * vx + fy * vy + vz).astype(F).reshape(-1, 3)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    return sp.make_rays(np.broadcast_to(p, d.shape), d)


def random_rays(scene, n, seed=1):
    import numpy as np
    import simplepath_amd as sp
    g = np.random.default_rng(seed)
    d = scene.desc()
    v = np.ctypeslib.as_array(d.vertices, shape=(d.info.num_vertices, 3))
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    u = g.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = 0.5 * (lo + hi) + u * np.linalg.norm(hi - lo)  # a sphere of twice the box's circumradius
    target = g.uniform(lo, hi, (n, 3))
    return sp.make_rays(o, target - o)


def child(spec: dict) -> None:
    sys.path.insert(0, spec["root"])
    import numpy as np
    import torch
    import simplepath_amd as sp
    scene = sp.Scene.from_file(spec["path"])
    scene.set_resolution(spec["width"], spec["height"])
    scene.upload(device=spec["device"])
    out = {"arm": spec["arm"], "width": spec["width"], "height": spec["height"], "bvh_info": scene.bvh_info(),
           "build_id": sp.lib().sp_build_id().decode()}

    def timed(rays, mode, normals):
        n = rays.shape[0]
        d_rays = torch.from_numpy(rays.view(np.float32).reshape(n, 8).copy()).cuda()
        d_hits = torch.zeros((n, 8), dtype=torch.int32, device="cuda") if mode == "closest" else None
        d_nrm = torch.zeros((n, 4), dtype=torch.float32, device="cuda") if normals else None
        d_occ = torch.zeros(n, dtype=torch.int32, device="cuda") if mode == "any" else None
        torch.cuda.synchronize()
        ms, st = [], None
        for call in range(1 + spec["calls"]):
            st = scene.trace_device(d_rays.data_ptr(), n, hits_ptr=d_hits.data_ptr() if d_hits is not None else 0,
                                    normals_ptr=d_nrm.data_ptr() if normals else 0,
                                    occluded_ptr=d_occ.data_ptr() if d_occ is not None else 0, mode=mode, stats=True)
            if call:
                ms.append(st["kernel_ms"])
        ms.sort()
        return {"rays": n, "hits": st["hits"], "stack_depth": st["stack_depth"], "kernel_ms": ms,
                "mrays_per_s_best": n / ms[0] / 1e3, "mrays_per_s_median": n / ms[len(ms) // 2] / 1e3}

    arm = spec["arm"]
    if arm in ("camera", "camera_normals"):
        out["closest"] = timed(camera_rays(scene, spec["width"], spec["height"]), "closest", arm == "camera_normals")
    elif arm == "random":
        rays = random_rays(scene, spec["width"] * spec["height"])
        out["any"] = timed(rays, "any", False)
        out["closest"] = timed(rays, "closest", False)
    elif arm == "bench":
        best = None
        for frame in range(2):
            _, st = sp.render_tiles(scene, spec["integrator"], spec["spp"])
            if frame:
                best = {"kernel_ms": st.kernel_ms, "rays": st.rays, "mrays_per_s": st.rays / st.kernel_ms / 1e3}
        out["render"] = best
    print("ray_query_timing_child " + json.dumps(out), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", action="append", default=None, help="a built-in scene name (repeatable)")
    ap.add_argument("--arms", default="camera,camera_normals,random,bench")
    ap.add_argument("--calls", type=int, default=5, help="timed calls per query, after one warm-up call")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--spp", type=int, default=None, help="samples of the bench arm")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds per child")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(json.loads(args.child))
        return 0
    sys.path.insert(0, ROOT)
    from simplepath_amd import scenes
    work = tempfile.mkdtemp(prefix="sp_ray_query_timing_")
    for name in args.scene or ["bunny"]:
        writer, w, h, spp, integrator = CONFIGS[name]
        path = getattr(scenes, writer)(work)
        base = dict(path=path, width=args.width or w, height=args.height or h, spp=args.spp or spp, integrator=integrator,
                    calls=args.calls, device=args.device, root=ROOT)
        for arm in args.arms.split(","):
            spec = dict(base, arm=arm)
            line = {"scene": name, "arm": arm}
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
                if text.startswith("ray_query_timing_child "):
                    line.update(json.loads(text[len("ray_query_timing_child "):]))
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
