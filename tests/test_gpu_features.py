"""Feature buffers on the render's own camera samples (sp_scene_camera_rays, sp_scene_features,
sp_features.hip).  The camera rays are compared bit for bit with the numpy
restatement of the sample (tests/_features.py) and anchored to the verified render; the features
with the reduction, one sample at a time in numpy float32, of the brute force's first hits
(tests/_ray_query.py) -- every float in every bit, the ids and |H| equal.  Sphere normals have no
bit-exact host restatement: they come from a ray query on the same rays."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import simplepath_amd as sp
from simplepath_amd import _abi
from tests import _features as ft, _lbvh_sets, _ray_query as rq, _refit_moves

pytestmark = pytest.mark.gpu

F = np.float32
ALL = tuple(sp.FEATURE_OUTPUTS)

# the walks of one scene (tests/test_gpu_ray_query.py)
WALKS = {
    "reference": dict(bvh_mode=1),
    "reference_stackless": dict(bvh_mode=1, stackless=True),
    "wide": dict(),
    "binary": dict(wide_bvh=False),
    "binary_closest": dict(binary_closest=True),
    "device_lbvh": dict(builder="device"),
    "device_sah": dict(builder="device_sah"),
}
SAMPLES = {"extra": 17, "extra_horizon": 17, "mixed": 5}  # the samples every test of a scene draws from
# `extra` seen from the side, across the floor plane's horizon.  From the file's own camera the
# floor plane fills the frame (every sample of every pixel hits), so the pixels without a hit and
# the partly covered ones that the reduction's edge cases need are taken from this view.
HORIZON = dict(eye=(0.2, -3.0, 0.5), look_at=(0.0, 0.0, 0.35), up=(0.0, 0.0, 1.0), fov_degrees=45.0)


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("features"))
    return {"mixed": _lbvh_sets.write_all(d)["mixed"][0], "extra": rq.write_extra_scene(d)}


def load(path, size=None, **upload_options):
    s = sp.Scene.from_file(path)
    if size:
        s.set_resolution(*size)
    s.upload(device=0, **(upload_options or dict(bvh_mode=1)))
    return s


def restated_rays(scene, tile_ids=None, first=0, num=1, camera=None):
    cam = ft.camera_array(camera if camera is not None else scene.desc().camera)
    return ft.camera_rays(cam, scene.width, scene.height, tile_ids, first, num)


class Case:
    """One scene resident in the reference order: its restated camera rays and the brute force's
    first hits for every sample, made once and left unchanged."""

    def __init__(self, path, n, camera=None):
        self.path, self.n = path, n
        self.scene = sp.Scene.from_file(path)
        if camera:
            self.scene.set_camera(sp.camera_look_at(width=self.scene.width, height=self.scene.height, **camera))
        self.scene.upload(device=0, bvh_mode=1)
        self.prims, self.mats = rq.Prims(self.scene), ft.Materials(self.scene)
        self.rays = restated_rays(self.scene, num=n)
        self.inside = ft.pixels(self.scene.width, self.scene.height, None)[2]
        flat = self.rays.reshape(-1)
        _, normals = self.scene.trace(flat["o"], flat["d"], flat["tmin"], flat["tmax"], normals=True)
        self.samples = ft.samples_from_brute(self.prims, self.rays, self.inside, self.mats, normals.reshape(self.rays.shape + (3,)))


@pytest.fixture(scope="module")
def cases(paths):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(paths[name.split("_")[0]], SAMPLES[name], HORIZON if name == "extra_horizon" else None)
        return made[name]
    return get


# ---------------------------------------------------------------- 1. camera rays
def assert_rays(got, want, what):
    assert got.shape == want.shape and got.dtype == sp.RAY_DTYPE, (what, got.shape, want.shape)
    g, w = got.view(np.uint32).reshape(-1, 8), want.view(np.uint32).reshape(-1, 8)
    bad = np.flatnonzero((g != w).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {g.shape[0]} records differ, first {bad[:4]}: {got.reshape(-1)[bad[:4]]} != {want.reshape(-1)[bad[:4]]}"


@pytest.mark.parametrize("size", [(48, 32), (20, 12)])
def test_camera_rays_match_the_restatement(paths, size):
    scene = load(paths["extra"], size)
    n_tiles = sp.TileScheduler(*size).get_num_tiles()
    inside = ft.pixels(*size, None)[2]
    assert (size == (48, 32)) == bool(inside.all())  # 20 x 12: partial tiles in both axes
    assert_rays(scene.camera_rays(num_samples=17), restated_rays(scene, num=17), f"{size}: samples 0..16")
    rays = scene.camera_rays(num_samples=17)
    assert not rays.view(np.uint32).reshape(n_tiles, 17, 64, 8)[~np.broadcast_to(inside[:, None, :], rays.shape)].any()
    live = rays[np.broadcast_to(inside[:, None, :], rays.shape)]
    assert (live["tmin"] == F(0.001)).all() and (live["tmax"] == np.finfo(F).max).all()
    assert_rays(scene.camera_rays(first_sample=5, num_samples=3), rays[:, 5:8], f"{size}: a range that starts at 5")
    # a permuted subset with one tile repeated
    g = np.random.default_rng(3)
    ids = g.permutation(n_tiles)[: max(3, n_tiles // 2)]
    ids = np.concatenate([ids, ids[1:2]]).astype(np.int32)
    assert_rays(scene.camera_rays(ids, num_samples=17), rays[ids], f"{size}: a tile list")
    assert_rays(scene.camera_rays(ids, num_samples=17), restated_rays(scene, ids, num=17), f"{size}: a tile list, restated")
    # another camera: set on the scene, and for one call only
    cam = sp.camera_look_at((0.4, 0.9, 2.8), (0.1, -0.1, 0.2), (0.0, 1.0, 0.1), 52.0, *size)
    before = bytes(scene.desc().camera)
    over = scene.camera_rays(ids, num_samples=4, camera=cam)
    assert_rays(over, restated_rays(scene, ids, num=4, camera=cam), f"{size}: the per-call camera")
    assert bytes(scene.desc().camera) == before
    assert_rays(scene.camera_rays(num_samples=17), rays, f"{size}: the override left the scene's camera alone")
    scene.set_camera(cam)
    assert_rays(scene.camera_rays(ids, num_samples=4), over, f"{size}: set_camera")
    assert not np.array_equal(over["d"], rays[ids][:, :4]["d"])


# ---------------------------------------------------------------- 2. the verified render
@pytest.mark.parametrize("size", [(48, 32), (20, 12)])
def test_sample_0_rays_are_the_renders(paths, size):
    scene = load(paths["extra"], size)
    image, _ = sp.render_tiles(scene, "direct_lighting", 1)
    rays = scene.camera_rays()[:, 0, :]
    px, py, inside = ft.pixels(*size, None)
    L, _ = scene.radiance(rays["o"].reshape(-1, 3), rays["d"].reshape(-1, 3), sp.pixel_seed(px, py).reshape(-1), "direct_lighting", samples=1)
    assert L.reshape(image.shape).tobytes() == image.tobytes()
    assert image[inside].max() > 0.0 and not image[~inside].view(np.uint32).any()


# ---------------------------------------------------------------- 3. the brute force
def brute_conditions(case, spp):
    """what the issue asks of `extra` at spp 17, from the brute force alone"""
    s = case.samples
    hits = (s.hit[:, :spp, :] & case.inside[:, None, :]).sum(axis=1)
    live = s.hit[:, :spp, :]
    kinds = set(np.unique(s.kind[:, :spp, :][live]).tolist())
    coat = case.mats.kind[s.material[:, :spp, :][live]] == 2
    figures = {"partial": int(((hits > 0) & (hits < spp)).sum()), "empty": int(((hits == 0) & case.inside).sum()),
               "kinds": sorted(kinds), "clearcoat_hits": int(coat.sum()), "sphere_pixels": int(ft.sphere_pixels(s, spp).sum())}
    print(f"spp {spp}: {figures}")
    return figures


@pytest.mark.parametrize("name,spp", [("extra", 1), ("extra", 2), ("extra", 17), ("extra_horizon", 17), ("mixed", 5)])
def test_features_equal_the_brute_force(cases, name, spp):
    """Conditions asserted from the brute force before anything is compared.  `extra` at 17 spp has
    hits of all three primitive kinds and on the clearcoat material; from its own camera the floor
    plane fills the frame (measured: 0 partly covered and 0 empty pixels), so the two coverage
    conditions are asserted of the same scene from the HORIZON camera (19 partly covered, 277 empty),
    which is compared in every bit like the others."""
    case = cases(name)
    figures = brute_conditions(case, spp)
    if spp == 17:
        assert figures["clearcoat_hits"] >= 1 and figures["kinds"] == [rq.TRI, rq.SPHERE, rq.PLANE]
    if name == "extra_horizon":
        assert figures["partial"] >= 1 and figures["empty"] >= 1
    want = ft.reduce(case.samples, spp)
    got, st = case.scene.features(spp, stats=True)
    assert set(got) == set(ALL)
    sphere = ft.sphere_pixels(case.samples, spp)
    assert 0 < sphere.sum() < sphere.size
    ft.assert_equal(got, want, f"{name} spp {spp}: no sphere among the hits", where=~sphere)
    ft.assert_equal(got, want, f"{name} spp {spp}: sphere normals from the ray query", where=sphere)
    assert (st["launches"], st["camera_rays"], st["hits"]) == (1, int(case.inside.sum()) * spp, int(want["ids"]["hits"].sum()))
    assert st["kernel_ms"] > 0.0 and st["stack_depth"] > 0
    empty = want["ids"]["hits"] == 0
    assert (got["ids"][empty] == np.array((-1, -1, -1, 0), dtype=sp.FEATURE_IDS_DTYPE)).all()
    for k in ft.FLOAT_OUTPUTS:
        assert not got[k][empty].view(np.uint32).any(), k


# ---------------------------------------------------------------- 4. every walk
FROM_WALK = ("depth", "coverage", "albedo")


@pytest.mark.parametrize("walk", list(WALKS))
def test_every_walk(cases, walk):
    case = cases("extra")
    base = case.scene.features(5)
    scene = load(case.path, **WALKS[walk])
    got = scene.features(5)
    ft.assert_equal(got, base, f"{walk} against the reference order", names=FROM_WALK)
    assert np.array_equal(got["ids"]["hits"], base["ids"]["hits"])
    own = ft.reduce(ft.samples_from_trace(scene, case.rays[:, :5], case.inside, case.mats), 5)
    ft.assert_equal(got, own, f"{walk} against its own ray query")


def test_the_stackless_walk_of_a_deep_tree(scene_dir):
    scene = load(os.path.join(scene_dir, "wedge_strip.sp"), (48, 40))
    assert scene.bvh_info()["depth"] == 172
    got, st = scene.features(3, stats=True)
    assert st["stack_depth"] == 0  # stackless
    inside = ft.pixels(48, 40, None)[2]
    rays = scene.camera_rays(num_samples=3)
    own = ft.reduce(ft.samples_from_trace(scene, rays, inside, ft.Materials(scene)), 3)
    assert own["ids"]["hits"].sum() > 0
    # the strip's largest triangles give hits at t = NaN (tests/test_gpu_device_build.py): a NaN is
    # a NaN, whatever its bits
    nan = np.isnan(own["depth"])
    print(f"wedge_strip: {int(own['ids']['hits'].sum())} hits, {int(nan.sum())} pixels with a NaN depth")
    assert np.array_equal(np.isnan(got["depth"]), nan)
    got["depth"][nan] = own["depth"][nan]
    ft.assert_equal(got, own, "wedge_strip against its own ray query")


# ---------------------------------------------------------------- 5. per-tile sample counts
def test_per_tile_sample_counts(cases):
    case = cases("extra")
    scene = case.scene
    n_tiles = case.rays.shape[0]
    counts = np.resize(np.array([0, 1, 3, 17, 2], dtype=np.uint32), n_tiles)
    got = scene.features(99, tile_samples=counts)
    ft.assert_equal(got, ft.reduce(case.samples, counts), "per-tile counts against the brute force")
    one_shots = {int(c): scene.features(int(c)) for c in np.unique(counts)}
    for c, one_shot in one_shots.items():
        for k in ALL:
            assert got[k][counts == c].tobytes() == one_shot[k][counts == c].tobytes(), (k, c)
    zero = counts == 0
    assert (got["ids"][zero] == np.array((-1, -1, -1, 0), dtype=sp.FEATURE_IDS_DTYPE)).all()
    assert all(not got[k][zero].view(np.uint32).any() for k in ft.FLOAT_OUTPUTS)
    # a tile list beside the counts: the counts belong to the slots
    ids = np.array([7, 2, 2, 19, 11], dtype=np.int32)
    listed = scene.features(99, tile_ids=ids, tile_samples=counts[:5])
    for k in ALL:
        for slot, (tile, c) in enumerate(zip(ids, counts[:5])):
            assert listed[k][slot].tobytes() == one_shots[int(c)][k][tile].tobytes(), (k, slot)
    # the device form of the counts
    d_counts = torch.from_numpy(counts.view(np.int32).copy()).cuda()
    bufs = device_buffers(n_tiles)
    scene.features_device(99, **pointers(bufs), d_tile_samples=d_counts.data_ptr(), stats=True)
    for k in ALL:
        assert payload(bufs[k]).tobytes() == got[k].tobytes(), k


# ---------------------------------------------------------------- 6. optional outputs
GUARD = 4  # words on either side of every buffer (ids stay 16-byte aligned)
FILL = 0x5A5A5A5A
WORDS = {"ids": 4, "coverage": 1, "depth": 1, "normal": 3, "albedo": 3}


def device_buffers(n_tiles):
    return {k: torch.full((n_tiles * 64 * WORDS[k] + 2 * GUARD,), FILL, dtype=torch.int32, device="cuda:0") for k in ALL}


def pointers(bufs, names=ALL):
    return {k + "_ptr": bufs[k].data_ptr() + 4 * GUARD for k in names}


def payload(buf):
    return buf.cpu().numpy()[GUARD:-GUARD]


def guards_intact(buf):
    a = buf.cpu().numpy()
    return bool((a[:GUARD] == FILL).all() and (a[-GUARD:] == FILL).all())


@pytest.mark.parametrize("names", [(k,) for k in ALL] + [("ids", "depth"), ("coverage", "normal", "albedo"), ALL])
def test_optional_outputs(cases, names):
    case = cases("extra")
    want = case.scene.features(3)
    bufs = device_buffers(case.rays.shape[0])
    torch.cuda.synchronize()
    st = case.scene.features_device(3, **pointers(bufs, names), stats=True)
    assert st["launches"] == 1 and st["hits"] == int(want["ids"]["hits"].sum())
    for k in ALL:
        assert guards_intact(bufs[k]), k
        if k in names:
            assert payload(bufs[k]).tobytes() == want[k].tobytes(), k
        else:
            assert (payload(bufs[k]) == FILL).all(), k


# ---------------------------------------------------------------- 7. the device form
def test_device_form_is_stream_ordered_with_renders(cases):
    case = cases("extra")
    scene = case.scene
    n_tiles = case.rays.shape[0]
    want = scene.features(17)
    want_rays = scene.camera_rays(num_samples=2)
    ref = torch.zeros((n_tiles, 64, 3), dtype=torch.float32, device="cuda:0")
    sp.render_tiles_device(scene, "direct_lighting", 4, None, ref.data_ptr())
    out = torch.zeros_like(ref)
    bufs = device_buffers(n_tiles)
    d_rays = torch.zeros((n_tiles, 2, 64, 8), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        h = stream.cuda_stream
        assert sp.render_tiles_device(scene, "direct_lighting", 4, None, out.data_ptr(), h, stats=False) is None
        assert scene.features_device(17, **pointers(bufs), stream=h) is None  # only enqueued
        assert scene.camera_rays_device(d_rays.data_ptr(), num_samples=2, stream=h) is None
        out2 = torch.zeros_like(ref)
        assert sp.render_tiles_device(scene, "direct_lighting", 4, None, out2.data_ptr(), h, stats=False) is None
    stream.synchronize()
    for k in ALL:
        assert guards_intact(bufs[k]) and payload(bufs[k]).tobytes() == want[k].tobytes(), k
    assert d_rays.cpu().numpy().tobytes() == want_rays.tobytes()
    assert torch.equal(out, ref) and torch.equal(out2, ref)
    # a device tile list
    ids = np.array([5, 0, 23, 5], dtype=np.int32)
    d_ids = torch.from_numpy(ids).cuda()
    bufs = device_buffers(ids.size)
    with torch.cuda.stream(stream):
        st = scene.features_device(17, **pointers(bufs), d_tile_ids=d_ids.data_ptr(), num_tiles=ids.size, stream=stream.cuda_stream, stats=True)
    assert st["launches"] == 1 and st["camera_rays"] == ids.size * 64 * 17
    for k in ALL:
        assert payload(bufs[k]).tobytes() == want[k][ids].tobytes(), k


# ---------------------------------------------------------------- 8. scene state
def test_features_follow_a_moved_mesh_and_edited_materials(paths):
    scene = load(paths["mixed"], None, builder="device")
    before = scene.features(3)
    v, f = _refit_moves.mesh_of(scene)
    scene.update_mesh(_refit_moves.jitter(v, f))
    moved = scene.features(3)
    assert moved["depth"].tobytes() != before["depth"].tobytes()
    fresh = sp.Scene.from_desc(scene.desc())
    fresh.upload(device=0, builder="device")
    ft.assert_equal(moved, fresh.features(3), "after update_mesh against a fresh upload")
    d = scene.desc()
    mats = [_abi.sp_material_desc.from_buffer_copy(d.materials[i]) for i in range(d.info.num_materials)]
    for k, m in enumerate(mats):
        m.lambert_albedo = (C.c_float * 3)(0.05 + 0.03 * k, 0.2, 0.11)
    scene.set_materials(mats)
    edited = scene.features(3)
    assert edited["albedo"].tobytes() != moved["albedo"].tobytes() and edited["depth"].tobytes() == moved["depth"].tobytes()
    fresh = sp.Scene.from_desc(scene.desc())
    fresh.upload(device=0, builder="device")
    ft.assert_equal(edited, fresh.features(3), "after set_materials against a fresh upload")


def test_a_progress_object_survives_the_calls(cases):
    case = cases("mixed")
    scene = case.scene
    one_shot, _ = sp.render_tiles(scene, "direct_lighting", 4)
    with sp.Progressive(scene, "direct_lighting") as prog:
        prog.render(2)
        got = scene.features(5)
        scene.camera_rays(num_samples=2)
        ft.assert_equal(got, ft.reduce(case.samples, 5), "beside a progress object")
        tiles, _ = prog.render(2)  # still valid, and still the one-shot image
        assert np.array_equal(tiles.view(np.uint32), one_shot.view(np.uint32))


def test_adaptive_counts_feed_the_features(cases):
    case = cases("extra")
    scene = case.scene
    with sp.Progressive(scene, "direct_lighting", adaptive=True) as prog:
        prog.converge(0.05, 2, 17, 5)
        counts = prog.tile_samples()
    assert counts.shape == (case.rays.shape[0],) and 2 <= counts.min() and counts.max() <= 17
    print(f"adaptive counts: {np.unique(counts, return_counts=True)}")
    ft.assert_equal(scene.features(1, tile_samples=counts), ft.reduce(case.samples, counts), "Progressive.tile_samples()")


# ---------------------------------------------------------------- 9. empty work
def test_empty_work_launches_nothing(cases):
    scene = cases("extra").scene
    word = torch.full((64,), FILL, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    st = scene.features_device(4, depth_ptr=word.data_ptr(), d_tile_ids=word.data_ptr(), num_tiles=0, stats=True)
    assert (st["launches"], st["camera_rays"], st["hits"]) == (0, 0, 0)
    st = scene.camera_rays_device(word.data_ptr(), d_tile_ids=word.data_ptr(), num_tiles=0, num_samples=3, stats=True)
    assert (st["launches"], st["camera_rays"]) == (0, 0)
    st = scene.camera_rays_device(word.data_ptr(), num_samples=0, stats=True)
    assert (st["launches"], st["camera_rays"]) == (0, 0)
    assert scene.camera_rays_device(0, num_samples=0) is None  # nothing to write: no buffer needed
    torch.cuda.synchronize()
    assert (word.cpu().numpy() == FILL).all()
    assert scene.camera_rays(num_samples=0).shape == (24, 0, 64)
