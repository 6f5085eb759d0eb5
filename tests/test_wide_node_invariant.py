"""What spw::visit_plain (simplepath_amd/csrc/common/sp_wide_visit.h) takes from the builders: on every
occupied slot of every 8-wide node the lower quantised byte is <= the upper one on each axis, and no
scale byte is 255.  The structural checker counts a violation as an error of kind 10
(sph::check_wide; sp_wide_check.first_error_kind), so the trees of every builder are held to it
here: about 2 000 triangles, and degenerate sets -- coplanar, duplicated, identical, collinear.

  * CPU: the host SAH builder, the host LBVH builder (the restatement of the device LBVH build), the
    restatement of the device SAH build, each with the host collapse and the restatement of the device
    finish, at leaf sizes 1 and 4; and the restatement of the refit after the vertices moved.
  * GPU: the same builders and finishes on the device, read back, and a device refit after a move.
  * The checker itself: tests/cpp/wide_visit_plain_main.cpp plants a swapped byte pair and a scale
    byte of 255 in a real tree and must be told kind 10 (test_wide_visit_plain_host.py runs it)."""
import pytest

import simplepath_amd as sp
from tests import _lbvh_sets, _refit_moves as R

W, H = 64, 48
BUILDERS = ("host", "device", "device_sah")
FINISHES = ("host", "device")
MOVES = ("jitter", "shrink", "collapse_half")


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("wide_invariant"))
    return {
        "tri2000": _lbvh_sets.write_set(d, "tri2000", _lbvh_sets.separated_triangles(2000)),
        "planar": _lbvh_sets.write_set(d, "planar", _lbvh_sets.planar_centroids(100)),
        "half_dup": _lbvh_sets.write_set(d, "half_dup", _lbvh_sets.half_duplicated(64)),
        "identical": _lbvh_sets.write_set(d, "identical", _lbvh_sets.identical_triangles(37)),
        "collinear": _lbvh_sets.write_set(d, "collinear", _lbvh_sets.collinear_centroids(90)),
    }


NAMES = ("tri2000", "planar", "half_dup", "identical", "collinear")


def clean(w, what):
    assert w["errors"] == 0, (what, w)
    assert w["records"] > 0, (what, w)


@pytest.mark.parametrize("name", NAMES)
def test_every_host_built_tree_keeps_the_invariant(sets, name):
    scene = sp.Scene.from_file(sets[name])
    v, f = R.mesh_of(scene)
    deep = 0
    for builder in BUILDERS:
        for finish in FINISHES:
            for leaf in (1, 4):
                opts = dict(builder=builder, finish=finish, sah_leaf=leaf)
                w = scene.wide_build_check(**opts)
                clean(w, (name, opts))
                deep = max(deep, w["depth"])
                if builder == "device_sah":
                    continue  # a refit keeps the topology of the host SAH or the device LBVH build
                for move in MOVES:
                    clean(scene.refit_build_check(R.MOVES[move](v, f), **opts)[1], (name, opts, move))
    if name == "tri2000":
        assert deep >= 3  # several levels of wide nodes, not a root alone


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_every_device_built_tree_keeps_the_invariant(sets, name):
    first = sp.Scene.from_file(sets[name])
    v, f = R.mesh_of(first)
    for builder in BUILDERS:
        for finish in FINISHES:
            opts = dict(builder=builder, finish=finish)
            s = sp.Scene.from_file(sets[name])
            s.set_resolution(W, H)
            s.upload(device=0, **opts)
            w = s.wide_check()
            clean(w, (name, opts))
            assert w["finish"] == finish
            if builder == "device_sah":
                continue
            for move in MOVES:
                assert s.update_mesh(R.MOVES[move](v, f), stats=True)["refitted"] == 1
                clean(s.wide_check(), (name, opts, move))
