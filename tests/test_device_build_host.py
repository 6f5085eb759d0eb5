"""The device BVH builder's surface without a device (include/simplepath_hip.h, SP_HAS_DEVICE_BUILD):
the structural checker on every host builder -- binned SAH, the reference's median split, and the
host restatement of the device's linear BVH -- over the suite's scenes and over constructed
primitive sets (tests/_lbvh_sets.py); the new structs' layouts against the compiler's; argument
errors that come back before any device is touched; and tests/cpp/lbvh_host_main.cpp, the same
builders under AddressSanitizer and UBSan as a stand-alone program."""
import ctypes as C
import glob
import os
import re
import subprocess

import pytest

import simplepath_amd as sp
from simplepath_amd import _abi
from tests import _lbvh_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "simplepath_hip.h")


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    return _lbvh_sets.write_all(str(tmp_path_factory.mktemp("lbvh_sets")))


def all_ok(scene, expect_slots=None):
    """errors == 0 for the three host builds; returns the device restatement's check"""
    out = {}
    for builder, mode in (("host", 0), ("host", 1), ("device", 0)):
        c = scene.bvh_build_check(builder=builder, bvh_mode=mode)
        assert c["errors"] == 0, (builder, mode, c)
        assert c["builder"] == builder
        if expect_slots is not None:
            assert c["slots"] == expect_slots, (builder, mode, c)
        assert c["nodes"] == (2 * c["leaves"] - 1 if c["slots"] else 0), c
        out[builder, mode] = c
    return out["device", 0]


def test_header_announces_the_surface():
    text = open(HEADER).read()
    assert re.search(r"^#define SP_HAS_DEVICE_BUILD 1\b", text, re.M)
    assert re.search(r"#define SP_ABI_VERSION 6\b", text)  # new entry points only
    for name in ("sp_scene_upload_with", "sp_scene_bvh_check", "sp_scene_bvh_build_check"):
        assert name in _abi.SIGNATURES and hasattr(sp.lib(), name), name
    assert (_abi.SP_BUILDER_AUTO, _abi.SP_BUILDER_HOST, _abi.SP_BUILDER_DEVICE) == (0, 1, 2)


def test_struct_layouts_match_the_compiler(tmp_path):
    src = tmp_path / "layout.c"
    B = ("struct_size", "builder", "reserved")
    K = ("struct_size", "builder", "nodes", "leaves", "slots", "depth", "max_leaf", "errors", "first_error_kind",
         "reserved", "first_error_node", "hash")
    line = lambda t, fs: ('  printf("%zu' + " %zu" * len(fs) + '\\n", sizeof(' + t + ")"
                          + "".join(f", offsetof({t}, {f})" for f in fs) + ");\n")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "simplepath_hip.h"\nint main(void) {\n'
                   + line("sp_build_params", B) + line("sp_bvh_check", K)
                   + '  printf("%d %d %d\\n", SP_BUILDER_AUTO, SP_BUILDER_HOST, SP_BUILDER_DEVICE);\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, timeout=120)
    a, b, c = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    for got, T, fs in ((a, _abi.sp_build_params, B), (b, _abi.sp_bvh_check, K)):
        assert [int(x) for x in got.split()] == [C.sizeof(T)] + [getattr(T, f).offset for f in fs]
    assert c.split() == ["0", "1", "2"]
    assert C.sizeof(_abi.sp_build_params) == 16 and C.sizeof(_abi.sp_bvh_check) == 72
    assert C.sizeof(_abi.sp_upload_params) == 32  # unchanged


def test_checker_passes_every_suite_scene(scene_dir):
    names = sorted(glob.glob(os.path.join(scene_dir, "*.sp")))
    assert len(names) >= 8
    for path in names:
        scene = sp.Scene.from_file(path)
        dev = all_ok(scene)
        # the checker's walk and the build agree on what bvh_build_info reports for the host SAH
        info = scene.bvh_build_info(0)
        host = scene.bvh_build_check(builder="host")
        assert (host["depth"], host["nodes"], host["slots"]) == (info["depth"], info["nodes"], info["slots"]), path
        assert dev["slots"] == info["slots"]


@pytest.mark.parametrize("name", [f"tri{n}" for n in _lbvh_sets.SIZES]
                         + ["identical37", "half_dup", "planar", "collinear", "mixed", "spheres_only", "wedge_strip"])
def test_checker_passes_constructed_sets(sets, name):
    path, n = sets[name]
    scene = sp.Scene.from_file(path)
    dev = all_ok(scene, expect_slots=n)
    if n is None:
        n = dev["slots"]
        assert n > 100
    # the device restatement: leaves within the leaf size, the same tree on every call
    for leaf in (1, 2, 3, 4):
        c = scene.bvh_build_check(builder="device", sah_leaf=leaf)
        assert c["errors"] == 0 and c["max_leaf"] <= leaf and c["slots"] == n, (leaf, c)
        assert c["hash"] == scene.bvh_build_check(builder="device", sah_leaf=leaf)["hash"]
        if n:
            assert c["leaves"] >= -(-n // leaf) and c["depth"] >= 1
    assert dev["hash"] == scene.bvh_build_check(builder="device", sah_leaf=4)["hash"]  # sah_leaf 0 = 4
    if n == 0:
        assert (dev["nodes"], dev["leaves"], dev["depth"]) == (0, 0, 0)
    if n == 1:
        assert (dev["nodes"], dev["leaves"], dev["depth"], dev["max_leaf"]) == (1, 1, 1, 1)


def test_one_code_for_all_builds_a_balanced_tree(sets):
    # 37 identical triangles share one Morton code: the position tie-break alone makes the tree,
    # which is then as shallow as a tree over 37 positions can be
    scene = sp.Scene.from_file(sets["identical37"][0])
    c = scene.bvh_build_check(builder="device", sah_leaf=1)
    assert c["errors"] == 0 and c["leaves"] == 37 and c["nodes"] == 73
    assert c["depth"] == 7  # ceil(log2 37) + 1 levels


def test_depth_is_consistent_with_the_stack_decision(sets, monkeypatch):
    # sp_scene_bvh_build_info makes the upload's stack / stackless decision on the host; with the
    # device-build hook it sees the linear BVH, whose depth the checker reports
    for name in ("wedge_strip", "tri1025", "mixed"):
        scene = sp.Scene.from_file(sets[name][0])
        c = scene.bvh_build_check(builder="device")
        monkeypatch.setenv("SP_DEVICE_BUILD", "1")
        info = scene.bvh_build_info(0)
        monkeypatch.delenv("SP_DEVICE_BUILD")
        assert info["depth"] == c["depth"] and info["nodes"] == c["nodes"], name
        stackless = c["depth"] + 1 > 96 or info["light_depth"] + 1 > 96
        assert (info["stack_depth"] == 0) == stackless, (name, info)
        # a stack budget below the tree's depth must choose the parent-link walk
        monkeypatch.setenv("SP_DEVICE_BUILD", "1")
        monkeypatch.setenv("SP_STACK_MAX", str(max(1, c["depth"] - 1)))
        assert scene.bvh_build_info(0)["stack_depth"] == 0, name
        monkeypatch.delenv("SP_STACK_MAX")
        monkeypatch.delenv("SP_DEVICE_BUILD")


@pytest.mark.parametrize("hook", ["default", "stack_max", "wide_closest_off"])
@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("name", ["wedge_strip", "tri1025", "mixed"])
def test_walk_plan_is_one_across_entry_points(sets, monkeypatch, name, builder, hook):
    # sp_scene_bvh_build_info and sp_scene_wide_build_check both go through build_trees and
    # walk_plan: what one reports as the stack, the other shows as parent links or a wide tree
    scene = sp.Scene.from_file(sets[name][0])
    depth = scene.bvh_build_check(builder=builder)["depth"]
    if builder == "device":
        monkeypatch.setenv("SP_DEVICE_BUILD", "1")  # (the finish follows: the level-wise collapse)
    if hook == "stack_max":
        monkeypatch.setenv("SP_STACK_MAX", str(max(1, depth - 1)))
    if hook == "wide_closest_off":
        monkeypatch.setenv("SP_WIDE_CLOSEST", "0")
    info = scene.bvh_build_info(0)
    chk = scene.wide_build_check()
    print(name, builder, hook, info, chk)
    assert info["depth"] == depth and chk["errors"] == 0
    assert chk["finish"] == builder
    assert (info["stack_depth"] == 0) == (chk["hash_parents"] != 0), (info, chk)
    assert (info["wide_depth"] == 0) == (chk["records"] == 0), (info, chk)
    assert info["wide_depth"] == chk["depth"]
    stackless = hook == "stack_max" or max(depth, info["light_depth"]) + 1 > 96
    assert (info["stack_depth"] == 0) == stackless
    if stackless:
        assert chk["records"] == 0  # a scene without a stack walks the binary tree only
    elif hook == "wide_closest_off":
        assert info["stack_depth"] == max(depth, info["wide_depth"], info["light_depth"]) + 1
    else:
        assert info["wide_depth"] > 0
        assert info["stack_depth"] == max(2 * (info["wide_depth"] + 1), info["light_depth"] + 1)


def test_device_build_hook_is_ignored_for_the_reference_order(scene_dir, monkeypatch):
    scene = sp.Scene.from_file(os.path.join(scene_dir, "bunny.sp"))
    plain = scene.bvh_build_check(builder="auto", bvh_mode=1)
    sah = scene.bvh_build_check(builder="auto", bvh_mode=0)
    monkeypatch.setenv("SP_DEVICE_BUILD", "1")
    hooked = scene.bvh_build_check(builder="auto", bvh_mode=1)
    assert hooked["builder"] == "host" and hooked["hash"] == plain["hash"]
    # ... and turns AUTO into DEVICE for bvh_mode 0, while an explicit HOST stays
    dev = scene.bvh_build_check(builder="auto", bvh_mode=0)
    assert dev["builder"] == "device" and dev["hash"] == scene.bvh_build_check(builder="device")["hash"] != sah["hash"]
    assert scene.bvh_build_check(builder="host", bvh_mode=0)["hash"] == sah["hash"]


def test_arguments_validated_before_the_device(scene_dir):
    L = sp.lib()
    scene = sp.Scene.from_file(os.path.join(scene_dir, "bunny.sp"))

    def build(**kw):
        b = _abi.sp_build_params()
        b.struct_size = C.sizeof(_abi.sp_build_params)
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    up = _abi.sp_upload_params()
    ref = _abi.sp_upload_params()
    ref.bvh_mode = 1
    out = _abi.sp_bvh_check()
    out.struct_size = C.sizeof(_abi.sp_bvh_check)
    bad = [(up, build(struct_size=0)), (up, build(struct_size=12)), (up, build(struct_size=24)), (up, build(builder=3)),
           (up, build(builder=-1)), (up, build(reserved=(C.c_int32 * 2)(1, 0))), (up, build(reserved=(C.c_int32 * 2)(0, 5))),
           (ref, build(builder=_abi.SP_BUILDER_DEVICE))]
    for p, b in bad:
        assert L.sp_scene_upload_with(scene.handle, 0, C.byref(p), C.byref(b)) == _abi.SP_ERR_ARG
        assert L.sp_scene_bvh_build_check(scene.handle, C.byref(p), C.byref(b), C.byref(out)) == _abi.SP_ERR_ARG
    # sp_upload_params is still validated first, and its reserved word still pinned
    p = _abi.sp_upload_params()
    p.reserved = 3
    assert L.sp_scene_upload_with(scene.handle, 0, C.byref(p), C.byref(build())) == _abi.SP_ERR_ARG
    assert L.sp_scene_upload_with(None, 0, C.byref(up), C.byref(build())) == _abi.SP_ERR_ARG
    # the check calls: NULL arguments, an unknown struct_size, a scene that is not uploaded
    wrong = _abi.sp_bvh_check()
    assert L.sp_scene_bvh_build_check(scene.handle, C.byref(up), None, C.byref(wrong)) == _abi.SP_ERR_ARG
    assert L.sp_scene_bvh_build_check(scene.handle, C.byref(up), None, None) == _abi.SP_ERR_ARG
    assert L.sp_scene_bvh_build_check(None, C.byref(up), None, C.byref(out)) == _abi.SP_ERR_ARG
    assert L.sp_scene_bvh_check(scene.handle, C.byref(wrong)) == _abi.SP_ERR_ARG
    assert L.sp_scene_bvh_check(scene.handle, C.byref(out)) == _abi.SP_ERR_STATE
    # NULL params and NULL build are the defaults
    assert L.sp_scene_bvh_build_check(scene.handle, None, None, C.byref(out)) == _abi.SP_OK
    assert out.errors == 0 and out.builder == _abi.SP_BUILDER_HOST
    with pytest.raises(sp.SimplePathError) as e:
        scene.bvh_build_check(builder="device", bvh_mode=1)
    assert e.value.code == _abi.SP_ERR_ARG


def test_host_builders_under_sanitizers(tmp_path):
    # plain g++ with AddressSanitizer and UBSan on the host builders and the checker, run directly
    exe = str(tmp_path / "lbvh_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "simplepath_amd", "csrc", "host", "sp_bvh.cpp"),
                    os.path.join(ROOT, "tests", "cpp", "lbvh_host_main.cpp"), "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert re.search(r"^0 failing$", r.stdout, re.M), r.stdout[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
