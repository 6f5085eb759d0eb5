"""The refit without a device: the host restatement of the device refit
(sp_scene_refit_build_check: sph::lbvh_fit_boxes and sph::refit_wide on the topology an upload of the
current mesh would make) over constructed sets x deformations x builder x leaf size, checked by
the two structural checkers against the bounds of the MOVED mesh; the host-only update of a scene
that is not resident; and tests/cpp/refit_host_main.cpp, the same code under AddressSanitizer and
UBSan as a stand-alone program."""
import os
import re
import subprocess

import numpy as np
import pytest

import simplepath_amd as sp
from tests import _lbvh_sets, _refit_moves as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BVH_COUNTS = ("nodes", "leaves", "slots", "depth", "max_leaf")
WIDE_COUNTS = ("records", "holes", "slots", "depth")
HASHES = (("b", "hash"), ("w", "hash_nodes"), ("w", "hash_records"), ("w", "hash_parents"))


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    return _lbvh_sets.write_all(str(tmp_path_factory.mktemp("refit_sets")))


def hashes(b, w):
    return tuple({"b": b, "w": w}[which][k] for which, k in HASHES)


@pytest.mark.parametrize("name", R.SETS)
def test_refit_over_the_matrix(sets, name):
    scene = sp.Scene.from_file(sets[name][0])
    v, f = R.mesh_of(scene)
    for builder in R.BUILDERS:
        for leaf in R.LEAVES:
            opts = dict(builder=builder, sah_leaf=leaf)
            b0, w0 = scene.bvh_build_check(**opts), scene.wide_build_check(**opts)
            assert b0["errors"] == 0 and w0["errors"] == 0
            same = {}
            for move, fn in R.MOVES.items():
                moved = fn(v, f)
                assert moved.dtype == np.float32 and moved.shape == v.shape
                b, w = scene.refit_build_check(moved, **opts)
                assert b["errors"] == 0, (name, builder, leaf, move, b)
                assert w["errors"] == 0, (name, builder, leaf, move, w)
                # the topology is the one built from the first pose
                assert [b[k] for k in BVH_COUNTS] == [b0[k] for k in BVH_COUNTS], (move, b, b0)
                assert [w[k] for k in WIDE_COUNTS] == [w0[k] for k in WIDE_COUNTS], (move, w, w0)
                assert w["hash_parents"] == w0["hash_parents"]
                same[move] = hashes(b, w)
            # a device-built tree refitted to unchanged positions: the same fold as lb_emit, the same bytes
            if builder == "device":
                assert same["identity"][0] == b0["hash"], (name, leaf)
            # unchanged positions leave the records as they were, whatever the builder; moved ones do not
            assert same["identity"][2] == w0["hash_records"]
            assert same["shift"][0] != same["identity"][0] and same["shift"][2] != same["identity"][2]
            # after the refits to the other poses, back at A: the bytes of A -> A (the chain on one set of
            # arrays, A -> B -> A in place, runs in tests/cpp/refit_host_main.cpp and on the device)
            assert hashes(*scene.refit_build_check(v, **opts)) == same["identity"]
    # the scene was never modified
    assert np.array_equal(R.mesh_of(scene)[0].view(np.uint32), v.view(np.uint32))


@pytest.mark.parametrize("options", [dict(stackless=True), dict(wide_bvh=False)], ids=["stackless", "no_wide_bvh"])
def test_forced_stackless_and_no_wide_tree(sets, options):
    for name in ("mixed", "tri257"):
        scene = sp.Scene.from_file(sets[name][0])
        v, f = R.mesh_of(scene)
        for builder in R.BUILDERS:
            w0 = scene.wide_build_check(builder=builder, **options)
            for move in ("shift", "permute", "collapse_half"):
                b, w = scene.refit_build_check(R.MOVES[move](v, f), builder=builder, **options)
                assert b["errors"] == 0 and w["errors"] == 0, (name, builder, move, b, w)
                assert (w["records"], w["hash_nodes"]) == (0, 0)
                assert w["hash_parents"] == w0["hash_parents"] and (w["hash_parents"] != 0) == ("stackless" in options)
                assert w["hash_records"] != w0["hash_records"]


def test_suite_scene_bend(scene_dir):
    # shared vertices, three tree levels of wide nodes: the bunny bent by 5 % and 20 % of its box
    scene = sp.Scene.from_file(os.path.join(scene_dir, "bunny.sp"))
    v, f = R.mesh_of(scene)
    for builder in R.BUILDERS:
        for amount in (0.05, 0.2):
            b, w = scene.refit_build_check(R.bend(v, f, amount), builder=builder)
            assert b["errors"] == 0 and w["errors"] == 0 and w["depth"] >= 2, (builder, amount, b, w)


def test_host_only_update_equals_a_scene_made_from_the_moved_mesh(sets):
    # not resident: the call only rewrites the host mesh, and a later build sees nothing of the old one
    for name in ("tri257", "mixed"):
        for move in ("shift", "jitter"):
            scene = sp.Scene.from_file(sets[name][0])
            v, f = R.mesh_of(scene)
            moved = R.MOVES[move](v, f)
            fresh = R.moved_scene(scene, moved)
            st = scene.update_mesh(moved, stats=True)
            assert st["refitted"] == 0
            for builder in R.BUILDERS:
                assert scene.bvh_build_check(builder=builder) == fresh.bvh_build_check(builder=builder)
                assert scene.wide_build_check(builder=builder) == fresh.wide_build_check(builder=builder)
                assert scene.bvh_build_check(builder=builder)["errors"] == 0


def test_refit_host_program_under_sanitizers(tmp_path):
    # lbvh_fit_boxes, refit_wide and both checkers -- a planted stale box included -- under
    # AddressSanitizer and UBSan, as a stand-alone program run directly
    exe = str(tmp_path / "refit_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "simplepath_amd", "csrc", "host", "sp_bvh.cpp"),
                    os.path.join(ROOT, "tests", "cpp", "refit_host_main.cpp"), "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert re.search(r"^0 failing$", r.stdout, re.M), r.stdout[-2000:]
    assert len(re.findall(r"^refit .* ok$", r.stdout, re.M)) >= 3 * 2 * 3, r.stdout[-3000:]
    for kind in ("stale binary box", "stale wide box"):
        assert re.search(rf"^planted {kind}: .* ok$", r.stdout, re.M), r.stdout[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
