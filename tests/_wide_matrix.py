"""The scenes x options matrix of the device-finish tests (test_device_finish_host.py,
test_gpu_device_finish.py) and the golden hashes of the host finish over it
(tests/golden/wide_hashes.json, taken from build_wide before it was restated on sp_wide.h).

    python -m tests._wide_matrix OUT.json     writes the hashes of the library as built
"""
import json
import os
import sys
import tempfile

SET_NAMES = [f"tri{n}" for n in (0, 1, 2, 3, 4, 5, 8, 9, 63, 64, 65, 255, 256, 257, 1025)] \
    + ["identical37", "half_dup", "planar", "collinear", "mixed", "spheres_only", "wedge_strip"]
SUITE_NAMES = ["bunny", "lucy_small", "elf_small"]
BUILDERS = ("host", "device")
LEAVES = (1, 4)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide_hashes.json")


def key(name, builder, leaf):
    return f"{name}/{builder}/leaf{leaf}"


def scene_paths(sets, scene_dir):
    paths = {n: sets[n][0] for n in SET_NAMES}
    paths.update({n: os.path.join(scene_dir, n + ".sp") for n in SUITE_NAMES})
    return paths


def host_hashes(paths):
    import simplepath_amd as sp
    out = {}
    for name, path in paths.items():
        scene = sp.Scene.from_file(path)
        for builder in BUILDERS:
            for leaf in LEAVES:
                c = scene.wide_build_check(builder=builder, finish="host", sah_leaf=leaf)
                assert c["errors"] == 0, (name, builder, leaf, c)
                out[key(name, builder, leaf)] = [f"{c['hash_nodes']:016x}", f"{c['hash_records']:016x}"]
    return out


if __name__ == "__main__":
    from simplepath_amd import scenes
    from tests import _lbvh_sets
    d = tempfile.mkdtemp(prefix="wide_matrix_")
    scenes.write_bunny_scene(d)
    scenes.write_lucy_scene(d, n=40, name="lucy_small.sp")
    scenes.write_elf_scene(d, n=24, max_depth=16, name="elf_small.sp")
    with open(sys.argv[1], "w") as fh:
        json.dump(host_hashes(scene_paths(_lbvh_sets.write_all(os.path.join(d, "sets")), d)), fh, indent=0, sort_keys=True)
        fh.write("\n")
