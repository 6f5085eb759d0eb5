"""direct_nee traces the shadow ray before the glossy estimate and skips the estimate on the lanes
whose light sample is occluded (sp_path.hpp direct_nee, sp_nee_black.h).
Nothing that can be observed may change: images are compared bit for bit with the CPU oracle, which
keeps the reference's order (evaluate, then trace where f is not black), and rays and shadow rays
must be equal -- the skipped lanes take "is f black?" from the decider, not from the estimate.

The scenes: a glossy plane under two coarse octahedra with smooth normals and a clearcoat over a
glossy base, lit from behind and above by a small sphere light, so that the camera looks at their
self-shadowed sides and at their shadows on the plane: umbra tiles (every lane occluded and
skipping), penumbra tiles (some lanes skip, the others run the estimate) and lit tiles.  The second octahedron's faces are
wound the other way, so all of its normals face away from the camera: the clearcoat seen from behind,
coat Fresnel exactly 1, f black, no shadow ray in the reference.  The second scene adds a light.

Counts of the checking build (-DSP_XP_NEE_CHECK=1) for these inputs at 64 x 64 @ 12 spp (DESIGN.md
§26d), DirectLighting / Whitted.  One light: 41 472 / 44 789 lanes with an estimate, 17 957 / 18 789
skip it, 2 045 / 2 368 of those black, 45 / 51 occluded lanes "unknown".  Two lights: 82 944 / 89 578,
25 675 / 28 219, 2 764 / 3 687, 85 / 92.  Under the wave vote (SP_NEE_SKIP 1) the one-light scene has
43 / 76 skipped votes and 15 205 / 16 035 lanes that ride along, the two-light scene 36 / 218 and
23 371 / 24 814.  No disagreement between the decider and the true cblack(f) in any of them."""
import os

import numpy as np
import pytest

import simplepath_amd as sp
from simplepath_amd import scenes
from tests import _oracle

pytestmark = pytest.mark.gpu

W = H = 64
SPP = 12

SCENE = """version: 1

scene_parameters {
    output_file_name: "nee_order.pfm"
    width: 64
    height: 64
}

perspective_camera {
    origin: 0.0 2.5 6.0
    look_at: 0.0 0.8 0.0
    fov: 45
}

material_glossy {
    name: "glossy_base"
    diffuse: 0.8 0.2 0.8
    ior: 1.8
    roughness: 0.25
}

material_glossy {
    name: "glossy_plane"
    diffuse: 0.6 0.6 0.6
    ior: 1.8
    roughness: 0.3
}

material_clearcoat {
    name: "glossy_clearcoat"
    base: "glossy_base"
    ior: 1.3
    color: 1.0 1.0 1.0
}

mesh {
    file: "octa_out.ply"
    translate: -1.0 1.2 0.0
    material: "glossy_clearcoat"
}

mesh {
    file: "octa_in.ply"
    translate: 1.0 1.2 0.0
    material: "glossy_clearcoat"
}

plane {
    material: "glossy_plane"
}

sphere_light {
    translate: 0.0 4.0 -3.0
    scale: 0.3 0.3 0.3
    radiance: 40.0 40.0 40.0
}
"""

SECOND_LIGHT = """
sphere_light {
    translate: 3.0 3.0 2.0
    scale: 0.3 0.3 0.3
    radiance: 20.0 10.0 10.0
}
"""

OCTA_V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float32)
OCTA_F = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int32)


def write_scene(directory, lights):
    os.makedirs(directory, exist_ok=True)
    scenes.write_ply(os.path.join(directory, "octa_out.ply"), OCTA_V, OCTA_F)
    scenes.write_ply(os.path.join(directory, "octa_in.ply"), OCTA_V, OCTA_F[:, ::-1].copy())
    path = os.path.join(directory, "nee_order%d.sp" % lights)
    with open(path, "w") as fh:
        fh.write(SCENE + (SECOND_LIGHT if lights == 2 else ""))
    return path


def load(path, w=W, h=H):
    s = sp.Scene.from_file(path)
    s.set_resolution(w, h)
    s.upload(device=0, bvh_mode=1)  # the reference-order BVH: bit for bit with the oracle
    return s


_cache = {}


def case(tmp_path_factory, lights, integrator):
    """(scene, oracle image, oracle counts) of one scene and integrator, computed once"""
    key = (lights, integrator)
    if key not in _cache:
        if lights not in _cache:
            _cache[lights] = load(write_scene(str(tmp_path_factory.mktemp("nee_order")), lights))
        s = _cache[lights]
        img, st = _oracle.render(s, sp.string_to_integrator_type(integrator), SPP, None, variant="spm")
        img.setflags(write=False)
        _cache[key] = (s, img, st)
    return _cache[key]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check(img, st, ref, rst):
    print("rays", st.rays, rst["rays"], "shadow", st.shadow_rays, rst["shadow_rays"], "differing values",
          int(np.sum(img.view(np.uint32) != ref.view(np.uint32))))
    assert st.rays == rst["rays"] and st.shadow_rays == rst["shadow_rays"]
    assert same_bits(img, ref)


def test_the_scenes_reach_the_cases(tmp_path_factory):
    # lit, shadowed and black samples in numbers: camera rays that hit geometry each ask for one
    # shadow ray per light unless f is black (only the inward octahedron's clearcoat is)
    for lights in (1, 2):
        s, ref, rst = case(tmp_path_factory, lights, "direct_lighting")
        primary = rst["rays"] - rst["shadow_rays"]
        assert primary == W * H * SPP
        assert 0.05 * primary * lights < rst["shadow_rays"] < 0.97 * primary * lights
        lum = ref.reshape(-1, 3).sum(axis=1)
        assert np.mean(lum == 0.0) > 0.05 and np.mean(lum > 0.0) > 0.2


@pytest.mark.parametrize("lights", [1, 2])
@pytest.mark.parametrize("pipeline", ["megakernel", "chunks"])
def test_direct_lighting_equals_the_oracle(tmp_path_factory, lights, pipeline):
    s, ref, rst = case(tmp_path_factory, lights, "direct_lighting")
    img, st = sp.render_tiles(s, "direct_lighting", SPP, pipeline=pipeline, tail_fraction=-1.0)
    check(img, st, ref, rst)


@pytest.mark.parametrize("lights", [1, 2])
def test_whitted_equals_the_oracle(tmp_path_factory, lights):
    s, ref, rst = case(tmp_path_factory, lights, "whitted")
    img, st = sp.render_tiles(s, "whitted", SPP, pipeline="megakernel")
    check(img, st, ref, rst)


@pytest.mark.parametrize("lights", [1, 2])
def test_resumed_render_equals_the_oracle(tmp_path_factory, lights):
    s, ref, rst = case(tmp_path_factory, lights, "direct_lighting")
    with sp.Progressive(s, "direct_lighting") as prog:
        _, a = prog.render(6)
        img, b = prog.render(6)
    print("rays", a.rays + b.rays, rst["rays"], "shadow", a.shadow_rays + b.shadow_rays, rst["shadow_rays"])
    assert a.rays + b.rays == rst["rays"] and a.shadow_rays + b.shadow_rays == rst["shadow_rays"]
    assert same_bits(img, ref)


@pytest.mark.parametrize("lights", [1, 2])
def test_tail_chunks_equal_the_megakernel_and_the_oracle(tmp_path_factory, lights):
    # tail chunks need more tiles than persistent waves (640 x 512: 5120 tiles), so this render is
    # compared with the plain megakernel's whole frame and with the oracle on every 16th tile
    path = write_scene(str(tmp_path_factory.mktemp("nee_order_tail")), lights)
    s = load(path, 640, 512)
    ref, rst = sp.render_tiles(s, "direct_lighting", 3, pipeline="megakernel", tile_order_factor=2.0, tail_fraction=-1.0)
    img, st = sp.render_tiles(s, "direct_lighting", 3, pipeline="megakernel", tile_order_factor=2.0, tail_fraction=0.4)
    assert rst.tail_tiles == 0 and st.tail_tiles > 0
    assert (st.rays, st.shadow_rays, st.rng_draws) == (rst.rays, rst.shadow_rays, rst.rng_draws)
    assert same_bits(img, ref)
    ids = np.arange(0, ref.shape[0], 16, dtype=np.int32)
    cpu, cst = _oracle.render(s, sp.string_to_integrator_type("direct_lighting"), 3, ids, variant="spm")
    sub, sst = sp.render_tiles(s, "direct_lighting", 3, ids, pipeline="megakernel")
    assert sst.rays == cst["rays"] and sst.shadow_rays == cst["shadow_rays"]
    assert same_bits(sub, cpu) and same_bits(img[ids], cpu)


# ---------------------------------------------------------------------------------------------
# The device unit program (tests/cpp/nee_order_units.hip): one wave per case runs direct_nee and
# the order it replaced -- kept in that file as the specification -- on the same hits and equal
# streams; a replay on a third stream says which path each lane took.  Built once per form of
# SP_NEE_SKIP (0 never skip, 1 the wave vote, 2 each lane on its own: what the library ships).
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORM, OUT = 11, 32
UNKNOWN, BLACK, NOT_BLACK, NO_ESTIMATE = 0, 1, 2, 3
_units = {}


def unit_words(tmp_path_factory, form):
    """[case, lane, word] of nee_order_units_<form>, run once"""
    if "abnormal" in _units:
        pytest.skip("nee_order_units ended abnormally: nothing more is run on the GPU")
    if form not in _units:
        exe = os.path.join(ROOT, "tests", "cpp", "_build", "nee_order_units_%d" % form)
        if not os.path.exists(exe):
            subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "nee_order.mk"], check=True, timeout=900)
        d = tmp_path_factory.mktemp("nee_units")
        t = sp.rsqrt_table()
        table = str(d / "rsqrt_table.bin")
        np.concatenate([np.array([t["bits"], t["zero_result"], t["denorm_result"]], dtype=np.uint32),
                        t["entries"].astype(np.uint32)]).tofile(table)
        out = str(d / "out.bin")
        try:
            r = subprocess.run([exe, table, out], capture_output=True, text=True, timeout=60)
        except subprocess.TimeoutExpired:
            _units["abnormal"] = True
            raise
        if r.returncode != 0:
            if r.returncode not in (1, 2):
                _units["abnormal"] = True
            pytest.fail(f"nee_order_units_{form}: exit {r.returncode}\n{r.stdout}{r.stderr}")
        assert r.stdout.split() == ["nee_order", "9", str(form)], r.stdout
        _units[form] = np.fromfile(out, dtype=np.uint32).reshape(9, 64, OUT)
    return _units[form]


def light_bits(w, light):
    f = (w[..., 22] >> (4 * light)) & 15
    return (f & 1) != 0, (f & 2) != 0, f >> 2  # usable, occluded, the decider's answer


@pytest.mark.parametrize("form", [2, 1, 0])
def test_new_order_equals_the_old_order_bit_for_bit(tmp_path_factory, form):
    w = unit_words(tmp_path_factory, form)
    lanes = np.arange(64)
    active = np.ones((9, 64), dtype=bool)
    active[8] = lanes % 3 != 0
    # L, shadow, rays, rng.draws, the stream index, buffer and readiness, and the next two numbers drawn
    new, old = w[..., :FORM], w[..., FORM:2 * FORM]
    bad = np.argwhere((new != old) & active[..., None])
    assert bad.size == 0, f"first differing (case, lane, word): {bad[:8].tolist()}"
    assert np.all(w[8][~active[8]] == 0xEEEEEEEE)  # divergent entry: a lane without a hit wrote nothing
    assert np.all(w[active][:, 5] >= 2)


def test_the_unit_cases_take_their_paths(tmp_path_factory):
    w = unit_words(tmp_path_factory, 2)
    lanes = np.arange(64)
    use0, occ0, known0 = light_bits(w, 0)
    use1, occ1, known1 = light_bits(w, 1)
    wo_y = w[..., 23].view(np.float32)
    draws, shadow, first = w[..., 5], w[..., 3], w[..., 24]
    # 0: every lane occluded with a firm answer: the whole wave skips
    assert np.all(use0[0] & occ0[0] & (known0[0] == NOT_BLACK)) and np.all(shadow[0] == 1) and np.all(draws[0] == 2 + 32)
    # 1: a mixed wave
    assert 8 < np.sum(occ0[1]) < 56 and np.all(known0[1] == NOT_BLACK)
    # 2: two occluded lanes the decider cannot tell (|wo.y| < 2^-10) among lanes that skip
    assert np.all(occ0[2]) and np.all(known0[2][[5, 37]] == UNKNOWN) and np.sum(known0[2] == UNKNOWN) == 2
    assert np.all(np.abs(wo_y[2][[5, 37]]) < 2.0 ** -10)
    # 3: the clearcoat seen from behind: black whatever the estimate, no shadow ray counted, 32 words drawn
    behind = lanes % 2 == 0
    assert np.all(wo_y[3][behind] < 0) and np.all(known0[3][behind] == BLACK) and np.all(shadow[3][behind] == 0)
    assert np.any(occ0[3][behind]) and np.any(~occ0[3][behind]) and np.all(draws[3][behind] == 34)
    assert np.all(known0[3][~behind] == NOT_BLACK) and np.all(shadow[3][~behind] == 1)
    # 4: wo.y == 0 draws nothing for the estimate and is "unknown"; occluded and visible lanes of both kinds
    flat = lanes % 4 == 0
    assert np.all(wo_y[4][flat] == 0.0) and np.all(draws[4][flat] == 2) and np.all(known0[4][flat] == UNKNOWN)
    assert np.all(draws[4][~flat] == 34) and np.any(occ0[4][~flat]) and np.any(~occ0[4][~flat])
    # 5, 6: the first estimate starts at word 300 of 312, so its 32 words cross a generation, on lanes
    # that skip and lanes that run; the second light's sample and estimate follow (6: generation ready)
    for c in (5, 6):
        at300 = lanes < 32 if c == 5 else lanes >= 0
        assert np.all(first[c][at300] == 300) and np.all(use1[c]) and np.all(draws[c] == 2 * 34)
        assert np.any(occ0[c][at300]) and np.any(~occ0[c][at300])
        assert np.all(w[c][at300][:, 6] == (300 + 32 + 2 + 32) - 312)  # the index afterwards: in the next generation
    # 7: the first light occluded, the second visible
    assert np.all(occ0[7]) and np.sum(use1[7] & ~occ1[7]) > 32
    # 8: divergent entry, three materials
    act = lanes % 3 != 0
    assert np.any(known0[8][act] == NO_ESTIMATE) and np.any(known0[8][act] == NOT_BLACK) and np.any(occ0[8][act]) and np.any(~occ0[8][act])
