"""What an upload leaves on the scene handle (sp_capi.hip).

  * A failed upload is not resident: the handle is as it was before any upload, whatever it held
    before, and the same upload fails again instead of being taken for the resident one.  No test
    here renders after a failure.
  * One handle taken through every kind of residency -- both builders, both finishes, the
    parent-link walk, no wide tree, the reference order -- holds after each upload exactly what a
    fresh handle holds: no size and no array survives from one residency into the next."""
import os

import pytest

import simplepath_amd as sp
from simplepath_amd import _abi
from tests import _lbvh_sets

pytestmark = pytest.mark.gpu

# the clearcoat pass resolves `base` in file order, so the second coat finds the first
NESTED_CLEARCOAT = """version: 1

scene_parameters {
    output_file_name: "nested.pfm"
    width: 16
    height: 16
    max_depth: 3
}

perspective_camera {
    origin: 0.0 0.0 3.0
    look_at: 0.0 0.0 0.0
    fov: 45
}

material_lambertian {
    name: "paint"
    diffuse: 0.8 0.3 0.3
}

material_clearcoat {
    name: "coat"
    base: "paint"
}

material_clearcoat {
    name: "coat_on_coat"
    base: "coat"
}

sphere {
    scale: 0.5 0.5 0.5
    material: "coat_on_coat"
}

sphere_light {
    translate: 0.0 3.0 3.0
    scale: 0.5 0.5 0.5
    radiance: 8.0 8.0 8.0
}
"""


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    return _lbvh_sets.write_all(str(tmp_path_factory.mktemp("lbvh_sets")))


def fails_with(code, call, *args, **kwargs):
    with pytest.raises(sp.SimplePathError) as e:
        call(*args, **kwargs)
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def assert_not_resident(scene):
    fails_with(_abi.SP_ERR_STATE, scene.device_bytes)
    fails_with(_abi.SP_ERR_STATE, scene.bvh_check)
    fails_with(_abi.SP_ERR_STATE, scene.wide_check)
    fails_with(_abi.SP_ERR_STATE, scene.bvh_info)


def test_a_failed_upload_is_not_resident():
    scene = sp.Scene.from_string(NESTED_CLEARCOAT)
    first = fails_with(_abi.SP_ERR_UNSUPPORTED, scene.upload, device=0)
    assert "clearcoat over clearcoat" in first
    # the same options again: a resident scene would answer SP_OK without building anything
    second = fails_with(_abi.SP_ERR_UNSUPPORTED, scene.upload, device=0)
    assert second == first
    assert_not_resident(scene)
    # No option lets this scene upload, so this handle cannot hold a valid residency first; the
    # nearest it gets is a failure under other options, which must leave the same state ...
    for options in (dict(builder="device"), dict(bvh_mode=1), dict(stackless=True, builder="host", finish="device")):
        fails_with(_abi.SP_ERR_UNSUPPORTED, scene.upload, device=0, **options)
        fails_with(_abi.SP_ERR_UNSUPPORTED, scene.upload, device=0, **options)
        assert_not_resident(scene)


def test_a_refused_argument_leaves_the_residency(sets):
    # ... and a handle that does hold one keeps it through an upload refused for its arguments
    scene = sp.Scene.from_file(sets["mixed"][0])
    scene.upload(device=0, builder="device")
    held = (scene.device_bytes(), scene.bvh_info(), scene.bvh_check(), scene.wide_check())
    fails_with(_abi.SP_ERR_ARG, scene.upload, device=0, sah_leaf=9)
    fails_with(_abi.SP_ERR_ARG, scene.upload, device=0, bvh_mode=1, builder="device")
    fails_with(_abi.SP_ERR_ARG, scene.upload, device=1 << 20)
    assert (scene.device_bytes(), scene.bvh_info(), scene.bvh_check(), scene.wide_check()) == held
    assert held[2]["builder"] == "device" and held[3]["finish"] == "device"


RESIDENCIES = [
    dict(builder="host", finish="host"),
    dict(builder="device", finish="device"),
    dict(builder="host", finish="device"),
    dict(builder="device", finish="host"),
    dict(builder="host", finish="host", stackless=True),
    dict(builder="device", finish="device", stackless=True),
    dict(wide_bvh=False),
    dict(bvh_mode=1),
    dict(builder="host", finish="host"),
]


@pytest.mark.parametrize("name", ["mixed", "tri1025"])
def test_one_handle_through_every_residency(sets, name):
    path = sets[name][0]
    scene = sp.Scene.from_file(path)
    for options in RESIDENCIES:
        scene.upload(device=0, **options)
        tree_options = {k: v for k, v in options.items() if k != "finish"}
        wide, built = scene.wide_check(), scene.wide_build_check(**options)
        print(name, options, wide)
        assert wide["errors"] == 0 and built["errors"] == 0, (options, wide, built)
        for k in ("hash_nodes", "hash_records", "hash_parents"):
            assert wide[k] == built[k], (options, k, wide, built)
        assert (wide["hash_parents"] != 0) == bool(options.get("stackless")), (options, wide)
        assert (wide["records"] != 0) == (not options.get("stackless") and options.get("wide_bvh", True)
                                          and not options.get("bvh_mode")), (options, wide)
        assert scene.bvh_check()["hash"] == scene.bvh_build_check(**tree_options)["hash"], options
        fresh = sp.Scene.from_file(path)
        fresh.upload(device=0, **options)
        assert scene.bvh_info() == fresh.bvh_info(), options
        assert scene.device_bytes() == fresh.device_bytes(), options
        assert wide == fresh.wide_check() and scene.bvh_check() == fresh.bvh_check(), options
