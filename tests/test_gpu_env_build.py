"""The image light's tables built on the device (sp_envbuild.hip; Scene.set_env_image on a resident
scene), against the host builder of the upload (sp_envmap.cpp), word for word.

After set_env_image on the resident 96x48 material_spheres_ibl scene, env_check reads every table
back and compares it with what the host builds from the same pixels: mismatches == 0 and the same
`guided`, over map sizes that cross the row kernel's 64-column and 16-row tiles and constructed
16x8 images that take every special path of the constructor (black, +inf, negative, NaN, the clamp
with each channel the largest, FLT_MAX, a row sum that overflows, denormals), with the guide tables and with
env_replay.  Then the in-place rule for equal sizes, device pixels, the transform-only edit, and
the SP_DEVICE_ENV hook of the upload."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import simplepath_amd as sp
from simplepath_amd import _abi, scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = float(np.finfo(np.float32).max)


def base16x8(seed=11):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.01, 2.0, (8, 16, 3)).astype(np.float32)


def constructed():
    """name -> (pixels [8, 16, 3], max_radiance, guided expected)"""
    out = {}
    out["black"] = (np.zeros((8, 16, 3), np.float32), 100.0, 1)
    img = base16x8()
    img[[2, 5]] = 0.0
    out["black_rows"] = (img, 100.0, 1)
    img = base16x8()
    img[3, 7, 1] = np.inf
    out["inf"] = (img, 100.0, 1)
    img = base16x8()
    img[1, 2] = (-0.5, -0.25, 0.1)
    img[6, 9] = (-3.0, -2.0, -1.0)
    out["negative"] = (img, 100.0, 1)
    img = base16x8()
    img[4, 11, 2] = np.nan
    out["nan"] = (img, 100.0, 0)
    for k, name in enumerate("rgb"):
        img = base16x8()
        c = np.array([10.0, 20.0, 5.0], np.float32)
        c[k] = 9000.0
        img[2 + k, 3 * k + 1] = c
        out[f"clamp_{name}"] = (img, 100.0, 1)
    img = base16x8()
    img[0, 0] = (np.inf, 1.0, 1.0)
    out["flt_max"] = (img, FLT_MAX, None)
    img = base16x8()
    img[3, :] = 3.0e38
    img[4, 2:9] = (3.3e38, 1.0e38, 2.0e38)
    out["near_flt_max"] = (img, FLT_MAX, None)
    # a row sum that overflows: the clamp keeps every entry at or below max_radiance and the sum divides by n,
    # so it takes max_radiance = +inf, under which an infinite texel stays infinite (inf / inf follows)
    img = base16x8()
    img[3, :] = FLT_MAX
    img[6, 4] = (np.inf, 2.0, 1.0)
    out["overflow"] = (img, float("inf"), None)
    img = base16x8() * np.float32(1e-41)
    img[5, 5] = (1e-45, 0.0, 3e-39)
    out["denormal"] = (img.astype(np.float32), 100.0, 1)
    return out


def sized():
    rng = np.random.default_rng(3)
    out = {"1x1": rng.uniform(0.1, 1.0, (1, 1, 3)).astype(np.float32),
           "5x3": rng.uniform(0.0, 1.0, (3, 5, 3)).astype(np.float32),
           "67x33": scenes.night_sky_image(67, 33, seed=4),    # 2w = 134 crosses a 64-column tile and is no multiple of it
           "130x2": rng.uniform(0.0, 300.0, (2, 130, 3)).astype(np.float32),
           "96x48": scenes.night_sky_image(96, 48),
           "1024x512": scenes.night_sky_image(1024, 512)}      # rows of 2048: many tiles, 1024 rows: many blocks
    return {k: (v, 100.0, None) for k, v in out.items()}


CASES = {**sized(), **constructed()}


def load(scene_dir, **upload_options):
    s = sp.Scene.from_file(os.path.join(scene_dir, "material_spheres_ibl.sp"))
    s.set_resolution(24, 16)
    s.upload(device=0, **upload_options)
    return s


@pytest.fixture(scope="module")
def residents(scene_dir):
    return {False: load(scene_dir), True: load(scene_dir, env_replay=True)}


def checked(scene, what):
    c = scene.env_check(0)
    print(what, {k: c[k] for k in ("builder", "guided", "mismatches", "first_table", "first_index")})
    assert c["mismatches"] == 0, (what, c)
    assert c["guided"] == scene.env_build_check(0)["guided"], (what, c)
    return c


@pytest.mark.parametrize("replay", [False, True], ids=["guides", "env_replay"])
@pytest.mark.parametrize("name", list(CASES))
def test_device_tables_equal_the_host_builder(residents, name, replay):
    scene = residents[replay]
    px, maxr, guided = CASES[name]
    st = scene.set_env_image(0, pixels=px, max_radiance=maxr, stats=True)
    assert st["rebuilt"] == 1
    c = checked(scene, (name, replay))
    host = scene.env_build_check(0)
    assert c["builder"] == "device" and (c["width"], c["height"]) == (px.shape[1], px.shape[0])
    assert st["guided"] == c["guided"] and (guided is None or c["guided"] == guided)
    tables = [t for t in _abi.ENV_TABLES if "guide" not in t]
    assert [c["hashes"][t] for t in tables] == [host["hashes"][t] for t in tables]
    assert c["marg_int_bits"] == host["marg_int_bits"]
    for t in ("cond_guide", "marg_guide"):  # with the guides: the host's; with env_replay: absent
        assert c["hashes"][t] == (0 if replay else host["hashes"][t]), t


def test_same_size_edits_keep_the_blocks(residents):
    scene = residents[False]
    a_px, b_px = CASES["96x48"][0], scenes.night_sky_image(96, 48, seed=9)
    scene.set_env_image(0, pixels=a_px, max_radiance=100.0)
    nbytes, first = scene.device_bytes(), checked(scene, "first")
    scene.set_env_image(0, pixels=b_px)
    assert scene.device_bytes() == nbytes and checked(scene, "same size")["hashes"] != first["hashes"]
    scene.set_env_image(0, max_radiance=3.0)  # the current pixels, clamped again
    c = checked(scene, "max_radiance")
    assert scene.device_bytes() == nbytes and c["hashes"]["radiance"] != first["hashes"]["radiance"]
    # another size and back: the first bytes again, in blocks of the first size
    scene.set_env_image(0, pixels=CASES["67x33"][0], max_radiance=100.0)
    assert scene.device_bytes() != nbytes
    checked(scene, "67x33")
    scene.set_env_image(0, pixels=a_px, max_radiance=100.0)
    assert scene.device_bytes() == nbytes and checked(scene, "back")["hashes"] == first["hashes"]
    # and the bytes a fresh upload of this scene holds
    fresh = sp.Scene.from_desc(scene.desc())
    fresh.upload(device=0)
    assert fresh.device_bytes() == nbytes
    f = fresh.env_check(0)
    assert f["builder"] == "host" and f["mismatches"] == 0 and f["hashes"] == first["hashes"]


def test_device_pixels(residents):
    scene = residents[False]
    px = scenes.night_sky_image(67, 33, seed=6)
    scene.set_env_image(0, pixels=px, max_radiance=100.0)
    host_form = checked(scene, "host pixels")
    scene.set_env_image(0, pixels=CASES["5x3"][0])
    t = torch.from_numpy(px).to("cuda:0")
    torch.cuda.synchronize()
    st = scene.set_env_image(0, device_ptr=t.data_ptr(), width=67, height=33, stats=True)
    assert st["rebuilt"] == 1
    c = checked(scene, "device pixels")
    assert c["hashes"] == host_form["hashes"] and c["marg_int_bits"] == host_form["marg_int_bits"]
    e = scene.desc().env_images[0]
    got = np.ctypeslib.as_array(e.pixels, shape=(e.height, e.width, 3))
    assert (e.width, e.height) == (67, 33) and np.array_equal(got.view(np.uint32), px.view(np.uint32))


def test_transform_only_edit_rebuilds_nothing(residents):
    scene = residents[False]
    scene.set_env_image(0, pixels=CASES["96x48"][0], max_radiance=100.0)
    before, nbytes = checked(scene, "before"), scene.device_bytes()
    st = scene.set_env_image(0, light_to_world=[[0, 0, 1], [0, 1, 0], [-1, 0, 0]], stats=True)
    assert st["rebuilt"] == 0 and st["scratch_bytes"] == 0 and st["ms_total"] == 0.0
    assert checked(scene, "after") == before and scene.device_bytes() == nbytes
    assert list(scene.desc().env_images[0].light_to_world.vz) == [-1, 0, 0]


CHILD = """
import os, sys
sys.path.insert(0, sys.argv[1])
import simplepath_amd as sp
s = sp.Scene.from_file(sys.argv[2])
s.set_resolution(24, 16)
s.upload(device=0)
c = s.env_check(0)
print("ENV", c["builder"], c["mismatches"], c["guided"], c["hashes"] == s.env_build_check(0)["hashes"])
"""


def test_device_env_hook_at_upload(scene_dir, tmp_path):
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, SP_DEVICE_ENV="1")
    r = subprocess.run([sys.executable, str(script), ROOT, os.path.join(scene_dir, "material_spheres_ibl.sp")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ENV device 0 1 True" in r.stdout, r.stdout
