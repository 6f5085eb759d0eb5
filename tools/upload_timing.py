#!/usr/bin/env python3
"""Wall time of one scene upload, stage by stage, for the host and the device BVH builders.

    python tools/upload_timing.py --scene bunny --scene lucy --builders host,device --repeat 2
    python tools/upload_timing.py --scene lucy --builders host,device,device_sah --repeat 2
    python tools/upload_timing.py --scene lucy --builders host --finish device

Each upload runs in a child process of its own (a fresh process: the library is loaded, the
scene parsed, and one upload timed), with SP_UPLOAD_TIMING=1, under which the library prints its
stage times: bounds, BVH build, 8-wide collapse, primitive-record packing, copies; and for the
device build its own stages (bounds copy, codes, sort, hierarchy, fit passes, copy-back), the
number of fit passes and the peak device scratch; for the device SAH build ("device_sah") its
stages (bounds copy, levels, handed-over subtrees, numbering, emission, copy-back), the level count,
the nodes the levels split, the handed-over ranges and the peak scratch; and for the device finish (--finish device, or
"auto" with a device builder) its stages (inputs copy, collapse levels, sums, bases, emit,
packing, parents), the level count and its peak scratch.  Builders alternate within a repeat.  One JSON
line per scene, builder and repeat goes to stdout."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRITERS = {"bunny": "write_bunny_scene", "bunny_scan": "write_bunny_scan_scene", "lucy": "write_lucy_scene",
           "elf": "write_elf_scene", "spheres": "write_spheres_scene"}


def child(path: str, builder: str, device: int, finish: str) -> None:
    sys.path.insert(0, ROOT)
    import simplepath_amd as sp
    t0 = time.perf_counter()
    scene = sp.Scene.from_file(path)
    t1 = time.perf_counter()
    if finish == "auto":  # (also what a library from before the device finish understands)
        scene.upload(device=device, builder=builder)
    else:
        scene.upload(device=device, builder=builder, finish=finish)
    t2 = time.perf_counter()
    info = scene.bvh_info()
    print("upload_timing_child " + json.dumps({"parse_s": t1 - t0, "upload_s": t2 - t1, "bvh_info": info,
                                               "device_bytes": scene.device_bytes()}), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", action="append", default=None, help="a built-in scene name or a .sp file (repeatable)")
    ap.add_argument("--builders", default="host,device", help="comma-separated: host, device, device_sah")
    ap.add_argument("--finish", default="auto", choices=["auto", "host", "device"])
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--timeout", type=float, default=900.0, help="seconds per upload")
    ap.add_argument("--child", nargs=2, metavar=("PATH", "BUILDER"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.child[1], args.device, args.finish)
        return 0
    sys.path.insert(0, ROOT)
    from simplepath_amd import scenes
    work = tempfile.mkdtemp(prefix="sp_upload_timing_")
    for name in args.scene or ["bunny"]:
        path = name if name.endswith(".sp") else getattr(scenes, WRITERS[name])(work)
        for rep in range(args.repeat):
            for builder in args.builders.split(","):
                env = dict(os.environ, SP_UPLOAD_TIMING="1")
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--device", str(args.device), "--finish", args.finish,
                                    "--child", path, builder],
                                   capture_output=True, text=True, env=env, timeout=args.timeout)
                line = {"scene": os.path.basename(path), "builder": builder, "finish": args.finish, "repeat": rep}
                if r.returncode != 0:
                    line["error"] = (r.stderr or r.stdout)[-400:]
                    print(json.dumps(line), flush=True)
                    return 1  # nothing more is started on the device after a failed upload
                for text in r.stderr.splitlines():
                    if text.startswith("sp_upload_timing "):
                        line["stages"] = json.loads(text[len("sp_upload_timing "):])
                for text in r.stdout.splitlines():
                    if text.startswith("upload_timing_child "):
                        line.update(json.loads(text[len("upload_timing_child "):]))
                print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
