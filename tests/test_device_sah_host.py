"""The device SAH builder's surface without a device (include/simplepath_hip.h, SP_HAS_DEVICE_SAH;
DESIGN.md section 22): builder "device_sah" in the host-only check calls runs the level-wise
restatement (sph::build_bvh_sah_levels), another program than the recursive host build, and must
make the same tree byte for byte -- over every suite scene, the constructed sets of
tests/_lbvh_sets.py and tests/_sah_sets.py and every leaf size, through both finishes and through a
refit; the enum, the bvh_mode 1 refusal and the SP_DEVICE_BUILD=2 hook; and
tests/cpp/sah_host_main.cpp, the two builds against each other under AddressSanitizer and UBSan as
a stand-alone program."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import simplepath_amd as sp
from simplepath_amd import _abi
from tests import _lbvh_sets, _refit_moves as R, _sah_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "simplepath_hip.h")
TREE = ("hash", "nodes", "leaves", "depth", "slots", "max_leaf")
WIDE = ("hash_nodes", "hash_records", "hash_parents")
LBVH_SETS = [f"tri{n}" for n in _lbvh_sets.SIZES] + ["identical37", "half_dup", "planar", "collinear", "mixed",
                                                     "spheres_only", "wedge_strip"]
ALL_SETS = LBVH_SETS + list(_sah_sets.NEW)


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    return _sah_sets.write_all(str(tmp_path_factory.mktemp("sah_sets")))


def same_tree(scene, **options):
    dev = scene.bvh_build_check(builder="device_sah", **options)
    host = scene.bvh_build_check(builder="host", **options)
    assert dev["builder"] == "device_sah" and host["builder"] == "host"
    assert dev["errors"] == 0 and host["errors"] == 0, (options, dev, host)
    assert [dev[k] for k in TREE] == [host[k] for k in TREE], (options, dev, host)
    return dev


def same_wide(scene, **options):
    for finish in ("host", "device"):
        dev = scene.wide_build_check(builder="device_sah", finish=finish, **options)
        host = scene.wide_build_check(builder="host", finish=finish, **options)
        assert dev["errors"] == 0 and dev["finish"] == finish, (finish, options, dev)
        assert [dev[k] for k in WIDE] == [host[k] for k in WIDE], (finish, options, dev, host)


def test_header_announces_the_surface():
    text = open(HEADER).read()
    assert re.search(r"^#define SP_HAS_DEVICE_SAH 1\b", text, re.M)
    assert re.search(r"#define SP_ABI_VERSION 6\b", text)  # no new struct, no new field
    assert (_abi.SP_BUILDER_AUTO, _abi.SP_BUILDER_HOST, _abi.SP_BUILDER_DEVICE, _abi.SP_BUILDER_DEVICE_SAH) == (0, 1, 2, 4)
    m = re.search(r"enum \{ SP_BUILDER_AUTO = (\d+), SP_BUILDER_HOST = (\d+), SP_BUILDER_DEVICE = (\d+), "
                  r"SP_BUILDER_DEVICE_SAH = (\d+) \};", text)
    assert m and [int(x) for x in m.groups()] == [0, 1, 2, 4]
    assert _abi.BUILDERS["device_sah"] == 4
    assert C.sizeof(_abi.sp_build_params) == 16 and C.sizeof(_abi.sp_build_params_ex) == 32


def test_same_tree_on_every_suite_scene(scene_dir):
    names = sorted(glob.glob(os.path.join(scene_dir, "*.sp")))
    assert len(names) >= 8
    for path in names:
        scene = sp.Scene.from_file(path)
        for leaf in (1, 2, 3, 4):
            same_tree(scene, sah_leaf=leaf)
        same_tree(scene)
        same_wide(scene)


@pytest.mark.parametrize("name", ALL_SETS)
def test_same_tree_on_constructed_sets(sets, name):
    assert len(LBVH_SETS) == 22
    path, n = sets[name]
    scene = sp.Scene.from_file(path)
    for leaf in (1, 2, 3, 4):
        c = same_tree(scene, sah_leaf=leaf)
        assert n is None or c["slots"] == n
        assert c["max_leaf"] <= leaf
    same_wide(scene)
    same_wide(scene, sah_leaf=1)
    same_wide(scene, stackless=True)


@pytest.mark.parametrize("name", ["tri257", "tri1025", "mixed", "dup_straddle", "two_clusters"])
def test_same_bytes_after_a_refit(sets, name):
    scene = sp.Scene.from_file(sets[name][0])
    v, f = R.mesh_of(scene)
    for move in ("shift", "jitter"):
        moved = R.MOVES[move](v, f)
        for leaf in (1, 4):
            for finish in ("host", "device"):
                bd, wd = scene.refit_build_check(moved, builder="device_sah", finish=finish, sah_leaf=leaf)
                bh, wh = scene.refit_build_check(moved, builder="host", finish=finish, sah_leaf=leaf)
                assert bd["errors"] == 0 and wd["errors"] == 0 and bd["builder"] == "device_sah"
                assert [bd[k] for k in TREE] == [bh[k] for k in TREE], (name, move, leaf, finish)
                assert [wd[k] for k in WIDE] == [wh[k] for k in WIDE], (name, move, leaf, finish)


def test_grid16_ties_are_decided_by_axis_and_bin_order(sets):
    # the lattice is symmetric under x <-> y and under mirroring: the x and y sweeps give equal
    # costs, as do mirror bins, and only "the first strict minimum, axes then bins in order" picks one
    scene = sp.Scene.from_file(sets["grid16"][0])
    c = same_tree(scene, sah_leaf=4)
    assert c["slots"] == 256 and c["leaves"] >= 64
    assert same_tree(scene, sah_leaf=1)["leaves"] == 256


def test_reference_order_and_the_hook(scene_dir, monkeypatch):
    L = sp.lib()
    scene = sp.Scene.from_file(os.path.join(scene_dir, "bunny.sp"))
    b = _abi.sp_build_params()
    b.struct_size = C.sizeof(_abi.sp_build_params)
    b.builder = 4
    up, ref = _abi.sp_upload_params(), _abi.sp_upload_params()
    ref.bvh_mode = 1
    out = _abi.sp_bvh_check()
    out.struct_size = C.sizeof(_abi.sp_bvh_check)
    assert L.sp_scene_bvh_build_check(scene.handle, C.byref(ref), C.byref(b), C.byref(out)) == _abi.SP_ERR_ARG
    assert L.sp_scene_upload_with(scene.handle, 0, C.byref(ref), C.byref(b)) == _abi.SP_ERR_ARG
    assert L.sp_scene_bvh_build_check(scene.handle, C.byref(up), C.byref(b), C.byref(out)) == _abi.SP_OK
    assert out.builder == 4 and out.errors == 0
    b.builder = 3  # still not a builder
    assert L.sp_scene_bvh_build_check(scene.handle, C.byref(up), C.byref(b), C.byref(out)) == _abi.SP_ERR_ARG

    sah = scene.bvh_build_check(builder="auto", bvh_mode=0)
    plain = scene.bvh_build_check(builder="auto", bvh_mode=1)
    assert sah["builder"] == "host"
    monkeypatch.setenv("SP_DEVICE_BUILD", "2")
    hooked = scene.bvh_build_check(builder="auto", bvh_mode=0)
    assert hooked["builder"] == "device_sah" and hooked["hash"] == sah["hash"]
    assert scene.wide_build_check()["finish"] == "device"  # AUTO follows the builder
    same = scene.bvh_build_check(builder="auto", bvh_mode=1)
    assert same["builder"] == "host" and same["hash"] == plain["hash"]
    assert scene.bvh_build_check(builder="host")["builder"] == "host"
    assert scene.bvh_build_check(builder="device")["builder"] == "device"
    monkeypatch.setenv("SP_DEVICE_BUILD", "1")  # keeps its meaning
    assert scene.bvh_build_check(builder="auto")["builder"] == "device"
    assert scene.bvh_build_check(builder="device_sah")["builder"] == "device_sah"


def test_bounds_that_are_not_finite_are_refused(sets):
    # the loader accepts an infinite vertex; its bound has a NaN centroid, and folds over NaN depend
    # on their order: the host builder takes it, the device SAH builder refuses it
    scene = sp.Scene.from_file(sets["tri64"][0])
    v, f = R.mesh_of(scene)
    v[5, 0] = np.float32(np.inf)
    moved = R.moved_scene(scene, v)
    assert moved.bvh_build_check(builder="host")["slots"] == 64
    with pytest.raises(sp.SimplePathError) as e:
        moved.bvh_build_check(builder="device_sah")
    assert e.value.code == _abi.SP_ERR_UNSUPPORTED


def test_both_forms_under_sanitizers(tmp_path):
    # plain g++ with AddressSanitizer and UBSan on the recursive and the level-wise build, run directly
    exe = str(tmp_path / "sah_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "simplepath_amd", "csrc", "host", "sp_bvh.cpp"),
                    os.path.join(ROOT, "tests", "cpp", "sah_host_main.cpp"), "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert re.search(r"^0 failing$", r.stdout, re.M), r.stdout[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
