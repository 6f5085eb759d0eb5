#!/usr/bin/env python3
"""What an upload leaves resident, for every builder x finish combination, as JSON lines: the tree's
sizes (bvh_info), the scene's device bytes, the binary tree's hash (bvh_check) and the three hashes
of the finish's arrays (wide_check).  Run it once per library (SP_LIB_PATH) and compare the outputs:

    python tools/upload_bytes.py --scene bunny --scene lucy > this.jsonl
    SP_LIB_PATH=<other build>/libsimplepath_hip.so python tools/upload_bytes.py ... > other.jsonl

One scene handle per scene goes through all four uploads in turn."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRITERS = {"bunny": "write_bunny_scene", "lucy": "write_lucy_scene", "elf": "write_elf_scene"}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", action="append", default=None, help="a built-in scene name or a .sp file (repeatable)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import simplepath_amd as sp
    from simplepath_amd import scenes
    work = tempfile.mkdtemp(prefix="sp_upload_bytes_")
    for name in args.scene or ["bunny"]:
        path = name if name.endswith(".sp") else getattr(scenes, WRITERS[name])(work)
        scene = sp.Scene.from_file(path)
        for builder in ("host", "device"):
            for finish in ("host", "device"):
                scene.upload(device=args.device, builder=builder, finish=finish)
                wide = scene.wide_check()
                line = {"scene": os.path.basename(path), "builder": builder, "finish": finish, "bvh_info": scene.bvh_info(),
                        "device_bytes": scene.device_bytes(), "bvh_hash": scene.bvh_check()["hash"],
                        "wide_errors": wide["errors"], "records": wide["records"], "wide_depth": wide["depth"],
                        "hash_nodes": wide["hash_nodes"], "hash_records": wide["hash_records"],
                        "hash_parents": wide["hash_parents"]}
                print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
