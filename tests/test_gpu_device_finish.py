"""The device finish on the GPU (sp_finish.hip; upload(finish="device")).

  * Every array the finish makes on the device -- wnodes, slot_tri, slot_code, wslot_tri, parents --
    read back and hashed, equals the host finish's for the same options, on every constructed set of
    tests/_lbvh_sets.py and on bunny.sp, with the host and the device builder; the wide tree passes
    the structural checker, and the binary tree -- which with the device builder never left the
    device -- still passes its own, depth included.
  * Images of finish="device" against finish="host" on the same builder: bit-identical, with equal
    ray, shadow-ray and draw counts, because the arrays are the same.
  * Re-upload cycles and the SP_DEVICE_FINISH hook."""
import os

import numpy as np
import pytest

import simplepath_amd as sp
from tests import _lbvh_sets, _wide_matrix as M

pytestmark = pytest.mark.gpu

COUNTS = ("records", "holes", "slots", "depth")
HASHES = ("hash_nodes", "hash_records", "hash_parents")


@pytest.fixture(scope="module")
def paths(tmp_path_factory, scene_dir):
    return M.scene_paths(_lbvh_sets.write_all(str(tmp_path_factory.mktemp("wide_sets"))), scene_dir)


def load(path, w=None, h=None, **upload_options):
    s = sp.Scene.from_file(path)
    if w:
        s.set_resolution(w, h)
    s.upload(device=0, **upload_options)
    return s


def same_arrays(dev, host):
    assert dev["errors"] == 0 and host["errors"] == 0, (dev, host)
    for k in COUNTS + HASHES:
        assert dev[k] == host[k], (k, dev, host)


@pytest.mark.parametrize("leaf", M.LEAVES)
@pytest.mark.parametrize("builder", M.BUILDERS)
@pytest.mark.parametrize("name", M.SET_NAMES + ["bunny"])
def test_device_arrays_equal_the_host_finish(paths, name, builder, leaf):
    s = load(paths[name], builder=builder, finish="device", sah_leaf=leaf)
    dev = s.wide_check()
    host = s.wide_build_check(builder=builder, finish="host", sah_leaf=leaf)
    print(name, builder, leaf, dev)
    assert dev["finish"] == "device" and host["finish"] == "host"
    same_arrays(dev, host)
    # the binary tree: with the device builder it never left the device, and its depth is the fit's pass count
    tree = s.bvh_check()
    restated = s.bvh_build_check(builder=builder, sah_leaf=leaf)
    assert tree["errors"] == 0 and tree["builder"] == builder, tree
    assert (tree["hash"], tree["depth"], tree["nodes"], tree["slots"]) == \
        (restated["hash"], restated["depth"], restated["nodes"], restated["slots"]), (tree, restated)
    info = s.bvh_info()
    assert (info["depth"], info["nodes"], info["slots"]) == (tree["depth"], tree["nodes"], tree["slots"])


@pytest.mark.parametrize("builder", M.BUILDERS)
@pytest.mark.parametrize("options", [dict(stackless=True), dict(wide_bvh=False)], ids=["stackless", "no_wide_bvh"])
@pytest.mark.parametrize("name", ["bunny", "mixed", "tri257"])
def test_scenes_without_a_wide_tree(paths, name, options, builder):
    s = load(paths[name], builder=builder, finish="device", **options)
    dev = s.wide_check()
    host = s.wide_build_check(builder=builder, finish="host", **options)
    same_arrays(dev, host)
    assert (dev["records"], dev["hash_nodes"]) == (0, 0)
    assert (dev["hash_parents"] != 0) == ("stackless" in options)
    assert s.bvh_check()["errors"] == 0


@pytest.mark.parametrize("builder", M.BUILDERS)
@pytest.mark.parametrize("scene,w,h,integrator,spp", [
    ("bunny", 64, 40, "direct_lighting", 4),
    ("elf_small", 40, 56, "iterative_rrnee", 2),
])
def test_images_are_bit_identical_across_finishes(paths, scene, w, h, integrator, spp, builder):
    out = {}
    for finish in ("host", "device"):
        s = load(paths[scene], w, h, builder=builder, finish=finish)
        assert s.wide_check()["finish"] == finish
        img, st = sp.render_tiles(s, integrator, spp)
        out[finish] = (img, (st.rays, st.shadow_rays, st.rng_draws, st.samples))
    print(scene, builder, out["host"][1], out["device"][1])
    assert out["host"][1] == out["device"][1]
    assert np.array_equal(out["host"][0].view(np.uint32), out["device"][0].view(np.uint32))


@pytest.mark.parametrize("builder", M.BUILDERS)
def test_one_progress_object_across_two_calls(paths, builder):
    imgs = {}
    for finish in ("host", "device"):
        s = load(paths["bunny"], 64, 40, builder=builder, finish=finish)
        prog = sp.Progressive(s, "direct_lighting")
        prog.render(1)
        imgs[finish], _ = prog.render(3)
        prog.close()
    assert np.array_equal(imgs["host"].view(np.uint32), imgs["device"].view(np.uint32))


def test_reupload_cycle_host_device_host(paths):
    s = load(paths["bunny"], 32, 24, finish="host")
    first = s.wide_check()
    assert first["finish"] == "host" and first["errors"] == 0
    before, _ = sp.render_tiles(s, "direct_lighting", 1)
    s.upload(device=0, finish="device")
    dev = s.wide_check()
    assert dev["finish"] == "device"
    same_arrays(dev, first)
    mid, _ = sp.render_tiles(s, "direct_lighting", 1)
    s.upload(device=0, finish="host")
    last = s.wide_check()
    assert last["finish"] == "host"
    same_arrays(last, first)
    after, _ = sp.render_tiles(s, "direct_lighting", 1)
    assert np.array_equal(before.view(np.uint32), mid.view(np.uint32))
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))


def test_env_hook_selects_the_finish(paths, monkeypatch):
    monkeypatch.setenv("SP_DEVICE_FINISH", "1")
    s = load(paths["bunny"])
    c = s.wide_check()
    assert c["finish"] == "device" and s.bvh_check()["builder"] == "host"
    same_arrays(c, s.wide_build_check(finish="host"))
    monkeypatch.setenv("SP_DEVICE_FINISH", "0")
    s = load(paths["bunny"], builder="device")
    c = s.wide_check()
    assert c["finish"] == "host" and s.bvh_check()["builder"] == "device"
    same_arrays(c, s.wide_build_check(builder="device", finish="device"))
    monkeypatch.delenv("SP_DEVICE_FINISH")
    s = load(paths["bunny"], builder="device")  # AUTO follows the builder
    assert s.wide_check()["finish"] == "device"
