"""Lanes on a special case beside ordinary lanes in one wave, bit for bit against the CPU oracle.

The libm (sp_libm.h) and the glossy BRDF helpers (sp_path.hpp) compute their main path for every
lane and override the special cases afterwards; the oracle keeps the reference's early returns.
The scene below puts both kinds of lane into the same 8 x 8 tiles (one wave each):

  * a wall the camera faces head on, glossy at the smallest roughness the parser keeps (it clamps
    at 1e-3): its centre pixels take beckmann_sample11's steep branch, the pixels around them the
    Newton one, and its narrow lobe sends lm_expf in beck_D to 0 and through the subnormals;
  * a floor 0.0005 below the camera, roughness 0.01: grazing outgoing directions (|wo.y| < 1e-3),
    reflections into the other hemisphere (!same_hemisphere), and Smith lambda on both sides of
    a = 1.6;
  * balls of roughness 1 (the top of the reference's [0, 1] scale; the parser sets no upper
    limit), of a glossy material with ior < 1 and of a clearcoat with ior < 1: total internal
    reflection (sin_t >= 1) in fresnel_dielectric.

That the oracle really takes each of these paths on this scene was counted once in a scratch build
of the oracle (with the counts).  Three guards no camera ray of a valid scene was
found to reach stay uncovered here: dp < 0 (the visible-normal sample never produced one), an
infinite tangent (a w.y that underflows), and mf_eval's zero half vector."""
import os

import numpy as np
import pytest

import simplepath_amd as sp
from tests import _oracle

pytestmark = pytest.mark.gpu

SCENE = """version: 1

scene_parameters {
    output_file_name: "fixup.pfm"
    width: 16
    height: 16
    max_depth: 4
}

perspective_camera {
    origin: 0.0 0.0005 0.0
    look_at: 0.0 0.0005 -1.0
    fov: 60
}

material_glossy {
    name: "wall"
    diffuse: 0.6 0.6 0.6
    ior: 1.8
    roughness: 0.0001
}

material_glossy {
    name: "floor"
    diffuse: 0.5 0.5 0.6
    ior: 1.8
    roughness: 0.01
}

material_glossy {
    name: "rough"
    diffuse: 0.8 0.3 0.3
    ior: 1.8
    roughness: 1.0
}

material_glossy {
    name: "inside_out"
    diffuse: 0.3 0.8 0.3
    ior: 0.7
    roughness: 0.25
}

material_clearcoat {
    name: "coat"
    base: "inside_out"
    ior: 0.8
    color: 1.0 1.0 1.0
}

plane {
    material: "floor"
    translate: 0.0 0.0 0.0
}

plane {
    material: "wall"
    translate: 0.0 0.0 -6.0
    rotate: 1 0 0 90
}

sphere {
    translate: -1.2 0.5 -4.0
    scale: 0.5 0.5 0.5
    material: "rough"
}

sphere {
    translate: 0.0 0.5 -3.0
    scale: 0.5 0.5 0.5
    material: "inside_out"
}

sphere {
    translate: 1.2 0.5 -4.0
    scale: 0.5 0.5 0.5
    material: "coat"
}

sphere_light {
    translate: 0.0 3.0 -3.0
    scale: 0.5 0.5 0.5
    radiance: 8.0 8.0 8.0
}
"""
SPP = 8


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    path = os.path.join(str(tmp_path_factory.mktemp("fixup")), "fixup.sp")
    with open(path, "w") as fh:
        fh.write(SCENE)
    s = sp.Scene.from_file(path)
    s.set_resolution(16, 16)
    s.upload(device=0, bvh_mode=1)
    return s


@pytest.fixture(scope="module")
def oracle_frames(scene):
    # computed once per integrator and libm variant, shared and left unchanged
    frames = {}
    for integrator in ("direct_lighting", "iterative_rrnee"):
        for variant in ("spm", "glibc"):
            frames[integrator, variant] = _oracle.render(scene, sp.string_to_integrator_type(integrator), SPP, variant=variant)
    return frames


@pytest.mark.parametrize("integrator", ["direct_lighting", "iterative_rrnee"])
def test_special_lanes_beside_ordinary_ones(scene, oracle_frames, integrator):
    assert sp.TileScheduler(16, 16).get_num_tiles() == 4
    g, gst = sp.render_tiles(scene, integrator, SPP)
    assert np.all(np.isfinite(g)) and np.any(g > 0)
    for variant in ("spm", "glibc"):
        c, cst = oracle_frames[integrator, variant]
        assert gst.rays == cst["rays"], variant
        assert gst.shadow_rays == cst["shadow_rays"], variant
        assert gst.samples == cst["samples"] == 16 * 16 * SPP, variant
        assert g.shape == c.shape and np.array_equal(g.view(np.uint32), c.view(np.uint32)), variant


def test_draw_counts_agree_between_pipelines(scene, oracle_frames):
    # the megakernel and the chunked pipeline consume every pixel's stream alike: same draw count
    c, cst = oracle_frames["direct_lighting", "spm"]
    draws = set()
    for pipeline in ("megakernel", "chunks"):
        g, gst = sp.render_tiles(scene, "direct_lighting", SPP, pipeline=pipeline)
        assert np.array_equal(g.view(np.uint32), c.view(np.uint32)), pipeline
        assert gst.rays == cst["rays"] and gst.shadow_rays == cst["shadow_rays"], pipeline
        draws.add(gst.rng_draws)
    assert len(draws) == 1 and draws.pop() > 0
