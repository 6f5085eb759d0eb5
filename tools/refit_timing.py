#!/usr/bin/env python3
"""What a moved mesh costs: the device refit against the uploads it replaces, and how the kept
topology traces.

    python tools/refit_timing.py --scene bunny --scene lucy --repeat 2
    python tools/refit_timing.py --scene lucy --parent-root ../parent_checkout

The mesh is bent by a fraction of its bounding box (a parabola in y displacing x).  Per scene and
repeat the arms alternate, each in a child process of its own (a fresh process: the library is
loaded, the scene parsed, one upload timed), each child under its own time limit, and the run
ends at the first child that fails:

  refit         host SAH upload of the rest pose (timed: the upload a refit saves), then per bend
                update_mesh with stats (ms_total and its stages) and a timed render of the refitted tree
  fresh_sah     per bend: the bent mesh uploaded with the host SAH builder, and its render
  device        per bend: the bent mesh uploaded with the device builder and device finish, and its render
  parent_device with --parent-root (a checkout of the parent commit, built): its device upload of the
                rest pose -- the fastest way that build has to show a moved mesh

Renders run at the bench's configuration of the scene (bench.py SCENES: size, samples, integrator)
unless --width / --height / --spp say otherwise; Mrays/s is rays / kernel_ms of the library's own
statistics, the best of --frames after one warm-up frame.  One JSON line per child goes to stdout."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# bench.py SCENES: writer, width, height, spp, integrator
CONFIGS = {"bunny": ("write_bunny_scene", 1920, 1080, 256, "direct_lighting"),
           "bunny_scan": ("write_bunny_scan_scene", 1920, 1080, 256, "direct_lighting"),
           "lucy": ("write_lucy_scene", 1920, 1080, 256, "direct_lighting"),
           "elf": ("write_elf_scene", 4096, 4096, 1024, "iterative_rrnee")}


def bend(v, amount):
    import numpy as np
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = np.maximum(hi - lo, np.float32(1e-20))
    t = ((v[:, 1] - lo[1]) / ext[1]).astype(np.float32)
    out = v.copy()
    out[:, 0] = (v[:, 0] + np.float32(amount) * ext[0] * (np.float32(2.0) * t - np.float32(1.0)) ** 2).astype(np.float32)
    return out


def child(spec: dict) -> None:
    sys.path.insert(0, spec["root"])
    import numpy as np
    import simplepath_amd as sp
    out = {}
    t0 = time.perf_counter()
    scene = sp.Scene.from_file(spec["path"])
    scene.set_resolution(spec["width"], spec["height"])
    out["parse_s"] = time.perf_counter() - t0
    d = scene.desc()
    rest = np.ctypeslib.as_array(d.vertices, shape=(d.info.num_vertices, 3)).astype(np.float32)  # a copy

    def render():
        best = None
        for frame in range(1 + spec["frames"]):
            _, st = sp.render_tiles(scene, spec["integrator"], spec["spp"])
            if frame and (best is None or st.kernel_ms < best[0]):
                best = (st.kernel_ms, st.rays)
        return {"kernel_ms": best[0], "rays": best[1], "mrays_per_s": best[1] / best[0] / 1e3}

    def upload(builder, finish):
        t = time.perf_counter()
        scene.upload(device=spec["device"], builder=builder, finish=finish)
        return time.perf_counter() - t

    arm = spec["arm"]
    if arm == "refit":
        out["upload_s"] = upload("host", "host")
        out["refits"] = []
        for amount in spec["bends"]:
            moved = bend(rest, amount)
            t = time.perf_counter()
            st = scene.update_mesh(moved, stats=True)
            wall = time.perf_counter() - t
            t = time.perf_counter()
            scene.update_mesh(moved)  # the same pose again without stage waits: what a host pays per frame
            plain = time.perf_counter() - t
            out["refits"].append({"bend": amount, "wall_ms": wall * 1e3, "wall_ms_no_stats": plain * 1e3, "stats": st,
                                  "render": render()})
    elif arm in ("fresh_sah", "device"):
        scene.update_mesh(bend(rest, spec["bends"][0]))  # not resident: the host mesh alone
        out["bend"] = spec["bends"][0]
        out["upload_s"] = upload("host", "host") if arm == "fresh_sah" else upload("device", "device")
        out["render"] = render()
    elif arm == "parent_device":
        out["upload_s"] = upload("device", "device")
    out["bvh_info"] = scene.bvh_info()
    out["build_id"] = sp.lib().sp_build_id().decode()
    print("refit_timing_child " + json.dumps(out), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", action="append", default=None, help="a built-in scene name (repeatable)")
    ap.add_argument("--bends", default="0.05,0.2")
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--frames", type=int, default=3, help="timed frames per render, after one warm-up frame")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--spp", type=int, default=None)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--arms", default="refit,device,fresh_sah,parent_device")
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit (arm parent_device)")
    ap.add_argument("--timeout", type=float, default=600.0, help="seconds per child")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(json.loads(args.child))
        return 0
    sys.path.insert(0, ROOT)
    from simplepath_amd import scenes
    work = tempfile.mkdtemp(prefix="sp_refit_timing_")
    bends = [float(x) for x in args.bends.split(",")]
    for name in args.scene or ["bunny"]:
        writer, w, h, spp, integrator = CONFIGS[name]
        path = getattr(scenes, writer)(work)
        base = dict(path=path, width=args.width or w, height=args.height or h, spp=args.spp or spp, integrator=integrator,
                    frames=args.frames, device=args.device, root=ROOT)
        for rep in range(args.repeat):
            for arm in args.arms.split(","):
                if arm == "parent_device" and not args.parent_root:
                    continue
                per_bend = [bends] if arm in ("refit", "parent_device") else [[b] for b in bends]
                for bs in per_bend:
                    spec = dict(base, arm=arm, bends=bs)
                    env = dict(os.environ)
                    env.pop("SP_UPLOAD_TIMING", None)
                    if arm != "refit":  # (under it an update waits after every stage, stats or not)
                        env["SP_UPLOAD_TIMING"] = "1"
                    if arm == "parent_device":
                        spec["root"] = os.path.abspath(args.parent_root)
                        env.pop("SP_LIB_PATH", None)
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", json.dumps(spec)],
                                       capture_output=True, text=True, env=env, timeout=args.timeout)
                    line = {"scene": name, "arm": arm, "repeat": rep}
                    if r.returncode != 0:
                        line["error"] = (r.stderr or r.stdout)[-400:]
                        print(json.dumps(line), flush=True)
                        return 1  # nothing more is started on the device after a failed child
                    for text in r.stderr.splitlines():
                        if text.startswith("sp_upload_timing "):
                            line["upload_stages"] = json.loads(text[len("sp_upload_timing "):])
                    for text in r.stdout.splitlines():
                        if text.startswith("refit_timing_child "):
                            line.update(json.loads(text[len("refit_timing_child "):]))
                    print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
