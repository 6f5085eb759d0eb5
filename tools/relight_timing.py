#!/usr/bin/env python3
"""What a relighting edit costs against the upload it replaces.

    python tools/relight_timing.py --parent ../parent_checkout
    python tools/relight_timing.py --scene spheres --sky 1024x512 --arms set_env_host,set_materials

The sky is the synthetic night map (scenes.night_sky_image, 4096x2048 unless --sky says otherwise)
on material_spheres_ibl.sp ("spheres") and on the bunny with that sky added ("bunny").  Every arm
runs in a child process of its own (a fresh process: library loaded, scene built and uploaded
untimed), does its edit once as a warm-up and then --repeat times (5), and reports the median
(min..max) of the wall time in ms; the run ends at the first child that fails.

  parent_upload   with --parent (a built checkout of the parent commit): Scene.from_desc(edited
                  descriptor) + upload, the only route that build has to any of these edits
  fresh_upload    the same route on this build
  set_env_host    set_env_image with host pixels (two maps alternate), and its sp_env_stats stages
  set_env_device  set_env_image with the pixels in a torch tensor on the device
  set_env_rotate  set_env_image with the transform only
  set_materials   every material replaced
  set_lights      the light list replaced (a sphere light added / removed)
  env_share       the upload of the scene with and without its env image: what the host's
                  build_env_map and the copies of its tables cost inside an upload

One JSON line per child goes to stdout."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = "parent_upload,fresh_upload,set_env_host,set_env_device,set_env_rotate,set_materials,set_lights,env_share"


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def child(spec: dict) -> None:
    sys.path.insert(0, spec["root"])
    import numpy as np
    if spec["arm"] == "set_env_device":
        import torch
    import simplepath_amd as sp
    from simplepath_amd import _abi, scenes
    w, h = spec["sky"]
    skies = [scenes.night_sky_image(w, h, seed=2), scenes.night_sky_image(w, h, seed=3)]
    base = sp.Scene.from_file(spec["path"])
    base.set_resolution(64, 48)
    keep = []

    def with_sky(desc, px, maxr=100.0):
        """the descriptor with env image 0 replaced by px (added, with an image light, when there is none)"""
        d = _abi.sp_scene_desc.from_buffer_copy(desc)
        img = _abi.sp_env_image()
        if desc.num_env_images:
            img = _abi.sp_env_image.from_buffer_copy(desc.env_images[0])
        else:
            for m in (img.light_to_world, img.world_to_light):
                m.vx, m.vy, m.vz = (C.c_float * 3)(1, 0, 0), (C.c_float * 3)(0, 1, 0), (C.c_float * 3)(0, 0, 1)
            n = desc.info.num_lights
            lights = (_abi.sp_light_desc * (n + 1))(*[desc.lights[i] for i in range(n)])
            lights[n].kind, lights[n].image = 2, 0
            lights[n].radiance = (C.c_float * 3)(1, 1, 1)
            d.lights = lights
            d.info.num_lights = n + 1
            keep.append(lights)
        img.width, img.height, img.max_radiance = px.shape[1], px.shape[0], maxr
        img.pixels = px.ctypes.data_as(C.POINTER(C.c_float))
        arr = (_abi.sp_env_image * 1)(img)
        keep.extend([arr, px])
        d.env_images, d.num_env_images = arr, 1
        return d

    def timed(fn, n):
        ms = []
        for k in range(n + 1):
            t = time.perf_counter()
            fn(k)
            if k:
                ms.append((time.perf_counter() - t) * 1e3)
        return summary(ms)

    arm, n, out = spec["arm"], spec["repeat"], {}
    first = with_sky(base.desc(), skies[0])
    if arm in ("parent_upload", "fresh_upload"):
        def route(k):
            s = sp.Scene.from_desc(with_sky(first, skies[k % 2]))
            s.upload(device=spec["device"])
        out["wall"] = timed(route, n)
    elif arm == "env_share":
        def plain(k):
            s = sp.Scene.from_desc(base.desc() if not base.desc().num_env_images else with_sky(first, skies[0][:2, :4].copy()))
            s.upload(device=spec["device"])
        def full(k):
            s = sp.Scene.from_desc(first)
            s.upload(device=spec["device"])
        out["without_env"] = timed(plain, n)
        out["with_env"] = timed(full, n)
    else:
        scene = sp.Scene.from_desc(first)
        scene.upload(device=spec["device"])
        if arm == "set_env_host":
            out["wall"] = timed(lambda k: scene.set_env_image(0, pixels=skies[k % 2]), n)
            out["stages"] = scene.set_env_image(0, pixels=skies[0], stats=True)
            out["check_mismatches"] = scene.env_check(0)["mismatches"]
        elif arm == "set_env_device":
            d_skies = [torch.from_numpy(x).to(f"cuda:{spec['device']}") for x in skies]
            torch.cuda.synchronize()
            out["wall"] = timed(lambda k: scene.set_env_image(0, device_ptr=d_skies[k % 2].data_ptr(), width=w, height=h), n)
            out["stages"] = scene.set_env_image(0, device_ptr=d_skies[0].data_ptr(), width=w, height=h, stats=True)
        elif arm == "set_env_rotate":
            rots = [[[0, 0, 1], [0, 1, 0], [-1, 0, 0]], [[1, 0, 0], [0, 1, 0], [0, 0, 1]]]
            out["wall"] = timed(lambda k: scene.set_env_image(0, light_to_world=rots[k % 2]), n)
        elif arm == "set_materials":
            d = scene.desc()
            mats = [_abi.sp_material_desc.from_buffer_copy(d.materials[i]) for i in range(d.info.num_materials)]
            def edit(k):
                for m in mats:
                    m.lambert_albedo = (C.c_float * 3)(0.1 + 0.05 * (k % 2), 0.2, 0.3)
                scene.set_materials(mats)
            out["wall"] = timed(edit, n)
        elif arm == "set_lights":
            d = scene.desc()
            lights = [_abi.sp_light_desc.from_buffer_copy(d.lights[i]) for i in range(d.info.num_lights)]
            lamp = _abi.sp_light_desc()
            lamp.kind, lamp.image, lamp.radiance = 0, -1, (C.c_float * 3)(20, 20, 20)
            for m in (lamp.object_to_world, lamp.world_to_object, lamp.normal_to_world):
                m.vx, m.vy, m.vz = (C.c_float * 3)(1, 0, 0), (C.c_float * 3)(0, 1, 0), (C.c_float * 3)(0, 0, 1)
            lamp.object_to_world.p, lamp.world_to_object.p = (C.c_float * 3)(3, 4, 6), (C.c_float * 3)(-3, -4, -6)
            out["wall"] = timed(lambda k: scene.set_lights(lights + [lamp] * (k % 2)), n)
        _, st = sp.render_tiles(scene, "direct_lighting", 1)  # the edited scene still renders
        out["render_rays"] = st.rays
    out["build_id"] = sp.lib().sp_build_id().decode()
    print("relight_timing_child " + json.dumps(out), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", action="append", default=None, help="spheres or bunny (repeatable; default both)")
    ap.add_argument("--sky", default="4096x2048")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--arms", default=ARMS)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (arm parent_upload)")
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds per child")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(json.loads(args.child))
        return 0
    sys.path.insert(0, ROOT)
    from simplepath_amd import scenes
    work = tempfile.mkdtemp(prefix="sp_relight_timing_")
    sky = [int(x) for x in args.sky.split("x")]
    paths = {"spheres": scenes.write_material_spheres_scene(work, 96, 48, image="night_96x48.pfm"), "bunny": scenes.write_bunny_scene(work)}
    for name in args.scene or ["spheres", "bunny"]:
        for arm in args.arms.split(","):
            if arm == "parent_upload" and not args.parent:
                continue
            spec = dict(path=paths[name], arm=arm, sky=sky, repeat=args.repeat, device=args.device, root=ROOT)
            env = dict(os.environ)
            if arm == "parent_upload":
                spec["root"] = os.path.abspath(args.parent)
                env.pop("SP_LIB_PATH", None)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", json.dumps(spec)],
                               capture_output=True, text=True, env=env, timeout=args.timeout)
            line = {"scene": name, "arm": arm, "sky": args.sky}
            if r.returncode != 0:
                line["error"] = (r.stderr or r.stdout)[-600:]
                print(json.dumps(line), flush=True)
                return 1  # nothing more is started on the device after a failed child
            for text in r.stdout.splitlines():
                if text.startswith("relight_timing_child "):
                    line.update(json.loads(text[len("relight_timing_child "):]))
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
