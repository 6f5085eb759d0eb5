"""Camera edits on a resident scene (sp_scene_set_camera, include/simplepath_hip.h): after an upload
the camera is replaced in turn by one from camera_look_at and a hand-made transform, and each render
is the CPU oracle's image of the scene's descriptor, bit for bit, with its ray counts -- nothing is
uploaded or rebuilt (a progress object made after the edit survives a following upload with the
same options), progress objects made before it are retired, and a refitted mesh stays moved."""
import os

import numpy as np
import pytest

import simplepath_amd as sp
from simplepath_amd import _abi
from tests import _oracle

pytestmark = pytest.mark.gpu


def load(scene_dir, name, w, h, bvh=0):
    s = sp.Scene.from_file(os.path.join(scene_dir, name))
    s.set_resolution(w, h)
    s.upload(device=0, bvh_mode=bvh)
    return s


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def hand_made(scene):
    """the scene's camera sheared by (3, -2) pixels and zoomed out by a quarter: no look_at gives it"""
    c = _abi.sp_camera_desc.from_buffer_copy(scene.desc().camera)
    t = c.transform
    for k in range(3):
        t.vz[k] = np.float32(t.vz[k]) + np.float32(3.0) * np.float32(t.vx[k]) - np.float32(2.0) * np.float32(t.vy[k])
        t.vx[k] = np.float32(1.25) * np.float32(t.vx[k])
        t.vy[k] = np.float32(1.25) * np.float32(t.vy[k])
    return c


def bunny_cameras(scene):
    # bunny.sp looks from (0, 2, 5) at (-0.25, 1, 0): another side, closer, a tilted up vector
    return [sp.camera_look_at((2.5, 1.75, 3.5), (-0.25, 0.75, 0.0), (0.125, 1.0, 0.0), 38.0, scene.width, scene.height),
            hand_made(scene)]


def check_against_oracle(s, integrator, spp):
    img, st = sp.render_tiles(s, integrator, spp)
    ref, rst = _oracle.render(s, sp.string_to_integrator_type(integrator), spp, variant="spm")
    print(integrator, "rays", st.rays, rst["rays"], "shadow", st.shadow_rays, rst["shadow_rays"], "differing values",
          int(np.sum(img.view(np.uint32) != ref.view(np.uint32))))
    assert same_bits(img, ref)
    assert (st.rays, st.shadow_rays) == (rst["rays"], rst["shadow_rays"])
    return img


@pytest.mark.parametrize("bvh", [0, 1])
@pytest.mark.parametrize("integrator,spp", [("direct_lighting", 5), ("iterative_rrnee", 3)])
def test_renders_after_set_camera_match_the_oracle(scene_dir, integrator, spp, bvh):
    s = load(scene_dir, "bunny.sp", 40, 24, bvh=bvh)
    first = check_against_oracle(s, integrator, spp)
    for cam in bunny_cameras(s):
        s.set_camera(cam)
        d = s.desc().camera
        assert bytes(d) == bytes(cam)
        img = check_against_oracle(s, integrator, spp)
        assert not same_bits(img, first)  # another view, not the loaded one again


def test_progress_objects_and_residency(scene_dir):
    s = load(scene_dir, "bunny.sp", 40, 24)
    cams = bunny_cameras(s)
    old = sp.Progressive(s, "direct_lighting")
    old.render(1)
    s.set_camera(cams[0])
    with pytest.raises(sp.SimplePathError) as e:
        old.render(1)
    assert e.value.code == _abi.SP_ERR_STATE
    old.close()
    # made after the edit: an upload with the same options finds the scene resident (a rebuild would
    # bump the generation and retire the object), and the passes see the new camera
    new = sp.Progressive(s, "direct_lighting")
    new.render(2)
    s.upload(device=0, bvh_mode=0)
    img, _ = new.render(3)
    new.close()
    ref, _ = _oracle.render(s, sp.string_to_integrator_type("direct_lighting"), 5, variant="spm")
    assert same_bits(img, ref)


def test_set_camera_keeps_a_refitted_mesh(scene_dir):
    s = load(scene_dir, "bunny.sp", 40, 24)
    d = s.desc()
    v = np.ctypeslib.as_array(d.vertices, shape=(d.info.num_vertices, 3)).copy()
    moved = (v * np.float32([1.0, 1.125, 0.875]) + np.float32([0.125, 0.0, 0.0])).astype(np.float32)
    assert s.update_mesh(moved, stats=True)["refitted"] == 1
    before = check_against_oracle(s, "direct_lighting", 5)  # the oracle renders desc(): the moved mesh
    s.set_camera(bunny_cameras(s)[0])
    d = s.desc()
    assert np.array_equal(np.ctypeslib.as_array(d.vertices, shape=(d.info.num_vertices, 3)), moved)
    after = check_against_oracle(s, "direct_lighting", 5)
    assert not same_bits(after, before)
    # the unmoved mesh through the same camera is another image: the refit is what was rendered
    fresh = sp.Scene.from_file(os.path.join(scene_dir, "bunny.sp"))
    fresh.set_resolution(40, 24)
    fresh.set_camera(s.desc().camera)
    unmoved, _ = _oracle.render(fresh, sp.string_to_integrator_type("direct_lighting"), 5, variant="spm")
    assert not same_bits(after, unmoved)
