"""The device finish without a device (include/simplepath_hip.h, SP_HAS_DEVICE_FINISH): the golden
hashes of the host finish, taken from build_wide before its per-node work moved into sp_wide.h; the
level-wise restatement (build_wide_levels, what the device runs) against the recursive collapse on
every constructed set and three suite scenes; the wide-tree checker on planted damage; the new
structs' layouts against the compiler's; argument errors that come back before any device is
touched; and tests/cpp/wide_host_main.cpp, the same code under AddressSanitizer and UBSan as a
stand-alone program."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

import simplepath_amd as sp
from simplepath_amd import _abi
from tests import _lbvh_sets, _wide_matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "simplepath_hip.h")
COUNTS = ("records", "holes", "slots", "depth")
NAMES = M.SET_NAMES + M.SUITE_NAMES


@pytest.fixture(scope="module")
def paths(tmp_path_factory, scene_dir):
    return M.scene_paths(_lbvh_sets.write_all(str(tmp_path_factory.mktemp("wide_sets"))), scene_dir)


@pytest.fixture(scope="module")
def golden():
    with open(M.GOLDEN) as fh:
        return json.load(fh)


def test_header_announces_the_surface():
    text = open(HEADER).read()
    assert re.search(r"^#define SP_HAS_DEVICE_FINISH 1\b", text, re.M)
    for name in ("sp_scene_wide_check", "sp_scene_wide_build_check"):
        assert name in _abi.SIGNATURES and hasattr(sp.lib(), name), name
    assert (_abi.SP_FINISH_AUTO, _abi.SP_FINISH_HOST, _abi.SP_FINISH_DEVICE) == (0, 1, 2)


def test_struct_layouts_match_the_compiler(tmp_path):
    src = tmp_path / "layout.c"
    B = ("struct_size", "builder", "reserved", "finish", "reserved2")
    K = ("struct_size", "finish", "records", "holes", "slots", "depth", "reserved", "errors", "first_error_kind", "reserved2",
         "first_error_node", "hash_nodes", "hash_records", "hash_parents")
    line = lambda t, fs: ('  printf("%zu' + " %zu" * len(fs) + '\\n", sizeof(' + t + ")"
                          + "".join(f", offsetof({t}, {f})" for f in fs) + ");\n")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "simplepath_hip.h"\nint main(void) {\n'
                   + line("sp_build_params_ex", B) + line("sp_wide_check", K)
                   + '  printf("%d %d %d\\n", SP_FINISH_AUTO, SP_FINISH_HOST, SP_FINISH_DEVICE);\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, timeout=120)
    a, b, c = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    for got, T, fs in ((a, _abi.sp_build_params_ex, B), (b, _abi.sp_wide_check, K)):
        assert [int(x) for x in got.split()] == [C.sizeof(T)] + [getattr(T, f).offset for f in fs]
    assert c.split() == ["0", "1", "2"]
    # the extended parameters begin as sp_build_params does, which keeps its size
    assert C.sizeof(_abi.sp_build_params) == 16 and C.sizeof(_abi.sp_build_params_ex) == 32
    assert [getattr(_abi.sp_build_params_ex, f).offset for f in ("struct_size", "builder", "reserved")] == \
        [getattr(_abi.sp_build_params, f).offset for f in ("struct_size", "builder", "reserved")]
    assert C.sizeof(_abi.sp_wide_check) == 88


@pytest.mark.parametrize("name", NAMES)
def test_host_finish_still_makes_the_golden_words(paths, golden, name):
    # the refactor guard: these hashes are build_wide's from before it was restated on sp_wide.h
    scene = sp.Scene.from_file(paths[name])
    for builder in M.BUILDERS:
        for leaf in M.LEAVES:
            c = scene.wide_build_check(builder=builder, finish="host", sah_leaf=leaf)
            assert c["errors"] == 0 and c["finish"] == "host", (builder, leaf, c)
            assert [f"{c['hash_nodes']:016x}", f"{c['hash_records']:016x}"] == golden[M.key(name, builder, leaf)], (builder, leaf)


@pytest.mark.parametrize("name", NAMES)
def test_level_wise_collapse_equals_the_recursive_one(paths, golden, name):
    scene = sp.Scene.from_file(paths[name])
    for builder in M.BUILDERS:
        for leaf in M.LEAVES:
            host = scene.wide_build_check(builder=builder, finish="host", sah_leaf=leaf)
            dev = scene.wide_build_check(builder=builder, finish="device", sah_leaf=leaf)
            assert dev["errors"] == 0 and dev["finish"] == "device", (builder, leaf, dev)
            for k in COUNTS + ("hash_nodes", "hash_records", "hash_parents"):
                assert dev[k] == host[k], (builder, leaf, k, host, dev)
            assert [f"{dev['hash_nodes']:016x}", f"{dev['hash_records']:016x}"] == golden[M.key(name, builder, leaf)]


def test_small_ends(paths):
    c = lambda name, **kw: sp.Scene.from_file(paths[name]).wide_build_check(finish="device", **kw)
    none = c("tri0")
    assert (none["records"], none["slots"], none["depth"], none["hash_nodes"], none["errors"]) == (0, 0, 0, 0, 0)
    for builder in M.BUILDERS:
        one = c("tri1", builder=builder)  # the root is a leaf: one record, no child records
        assert (one["records"], one["holes"], one["slots"], one["depth"]) == (1, 0, 1, 1), one
        # up to 8 leaves fit one wide node whatever the builder makes of them; nine single-primitive
        # leaves (leaf size 1; the SAH build may choose them at leaf size 4 too) need a second level
        for n in (2, 3, 4, 5, 8, 9):
            for leaf in (1, 4):
                w = c(f"tri{n}", builder=builder, sah_leaf=leaf)
                assert w["slots"] == n and w["errors"] == 0, (n, leaf, w)
                if n <= 8:
                    assert (w["records"], w["holes"], w["depth"]) == (1, 0, 1), (n, leaf, w)
                elif leaf == 1:
                    assert w["depth"] == 2 and w["records"] > 1, (n, w)
                else:
                    assert (w["depth"] == 1) == (w["records"] == 1) and w["depth"] <= 2, (n, w)
    assert c("spheres_only")["slots"] == 5 and c("mixed")["slots"] == 49


def test_forced_stackless_and_no_wide_tree(paths):
    for name in ("bunny", "mixed", "wedge_strip"):
        scene = sp.Scene.from_file(paths[name])
        for builder in M.BUILDERS:
            host = scene.wide_build_check(builder=builder, finish="host", stackless=True)
            dev = scene.wide_build_check(builder=builder, finish="device", stackless=True)
            assert host["hash_parents"] != 0 and dev["hash_parents"] == host["hash_parents"]
            assert dev["hash_records"] == host["hash_records"]
            assert (dev["records"], dev["hash_nodes"], host["records"], host["hash_nodes"]) == (0, 0, 0, 0)
            flat = scene.wide_build_check(builder=builder, finish="device", wide_bvh=False)
            assert (flat["records"], flat["hash_nodes"], flat["hash_parents"], flat["errors"]) == (0, 0, 0, 0)
            assert flat["hash_records"] == scene.wide_build_check(builder=builder, finish="host", wide_bvh=False)["hash_records"]


def test_finish_resolution_and_hook(paths, monkeypatch):
    scene = sp.Scene.from_file(paths["bunny"])
    monkeypatch.delenv("SP_DEVICE_FINISH", raising=False)
    monkeypatch.delenv("SP_DEVICE_BUILD", raising=False)
    # AUTO follows the builder; explicit values hold with either builder
    assert scene.wide_build_check()["finish"] == "host"
    assert scene.wide_build_check(builder="device")["finish"] == "device"
    assert scene.wide_build_check(builder="device", finish="host")["finish"] == "host"
    assert scene.wide_build_check(builder="host", finish="device")["finish"] == "device"
    assert scene.wide_build_check(bvh_mode=1)["finish"] == "host"
    monkeypatch.setenv("SP_DEVICE_FINISH", "1")
    assert scene.wide_build_check()["finish"] == "device"
    assert scene.wide_build_check(finish="host")["finish"] == "host"
    assert scene.wide_build_check(bvh_mode=1)["finish"] == "host"  # the hook is ignored for the reference order
    monkeypatch.setenv("SP_DEVICE_FINISH", "0")
    assert scene.wide_build_check(builder="device")["finish"] == "host"
    assert scene.wide_build_check(builder="device", finish="device")["finish"] == "device"
    # the plain 16-byte sp_build_params is AUTO as well
    monkeypatch.delenv("SP_DEVICE_FINISH")
    b = _abi.sp_build_params()
    b.struct_size = C.sizeof(_abi.sp_build_params)
    b.builder = _abi.SP_BUILDER_DEVICE
    out = _abi.sp_wide_check()
    out.struct_size = C.sizeof(_abi.sp_wide_check)
    assert sp.lib().sp_scene_wide_build_check(scene.handle, None, C.byref(b), C.byref(out)) == _abi.SP_OK
    assert out.finish == _abi.SP_FINISH_DEVICE and out.errors == 0


def test_arguments_validated_before_the_device(paths):
    L = sp.lib()
    scene = sp.Scene.from_file(paths["bunny"])

    def build(**kw):
        b = _abi.sp_build_params_ex()
        b.struct_size = C.sizeof(_abi.sp_build_params_ex)
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    up = _abi.sp_upload_params()
    ref = _abi.sp_upload_params()
    ref.bvh_mode = 1
    out = _abi.sp_wide_check()
    out.struct_size = C.sizeof(_abi.sp_wide_check)
    as_build = lambda b: C.cast(C.pointer(b), C.POINTER(_abi.sp_build_params))
    bad = [(up, build(struct_size=20)), (up, build(struct_size=28)), (up, build(struct_size=36)), (up, build(finish=3)),
           (up, build(finish=-1)), (up, build(reserved2=(C.c_int32 * 3)(0, 0, 1))), (up, build(reserved=(C.c_int32 * 2)(1, 0))),
           (up, build(builder=3)), (ref, build(finish=_abi.SP_FINISH_DEVICE)),
           (ref, build(builder=_abi.SP_BUILDER_DEVICE, finish=_abi.SP_FINISH_HOST))]
    for p, b in bad:
        assert L.sp_scene_upload_with(scene.handle, 0, C.byref(p), as_build(b)) == _abi.SP_ERR_ARG
        assert L.sp_scene_wide_build_check(scene.handle, C.byref(p), C.byref(b), C.byref(out)) == _abi.SP_ERR_ARG
    with pytest.raises(sp.SimplePathError) as e:
        scene.wide_build_check(finish="device", bvh_mode=1)
    assert e.value.code == _abi.SP_ERR_ARG
    # the check calls: NULL arguments, an unknown struct_size, a scene that is not uploaded
    wrong = _abi.sp_wide_check()
    wrong.struct_size = 96
    assert L.sp_scene_wide_build_check(scene.handle, C.byref(up), None, C.byref(wrong)) == _abi.SP_ERR_ARG
    assert L.sp_scene_wide_build_check(scene.handle, C.byref(up), None, None) == _abi.SP_ERR_ARG
    assert L.sp_scene_wide_build_check(None, C.byref(up), None, C.byref(out)) == _abi.SP_ERR_ARG
    assert L.sp_scene_wide_check(scene.handle, C.byref(wrong)) == _abi.SP_ERR_ARG
    assert L.sp_scene_wide_check(scene.handle, C.byref(out)) == _abi.SP_ERR_STATE
    assert L.sp_scene_wide_build_check(scene.handle, None, None, C.byref(out)) == _abi.SP_OK
    assert out.errors == 0 and out.finish == _abi.SP_FINISH_HOST and out.records > 0


def test_wide_host_program_under_sanitizers(tmp_path):
    # build_wide, build_wide_levels and the checker -- planted damage included -- under
    # AddressSanitizer and UBSan, as a stand-alone program run directly
    exe = str(tmp_path / "wide_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "simplepath_amd", "csrc", "host", "sp_bvh.cpp"),
                    os.path.join(ROOT, "tests", "cpp", "wide_host_main.cpp"), "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert re.search(r"^0 failing$", r.stdout, re.M), r.stdout[-2000:]
    for kind in ("child_base", "meta count", "quantised byte", "hole"):
        assert re.search(rf"^planted {kind}: .* ok$", r.stdout, re.M), r.stdout[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
