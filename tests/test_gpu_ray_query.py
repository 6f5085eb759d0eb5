"""Ray queries on the resident scene (sp_scene_trace_rays, sp_query.hip) against the
brute force composed from the oracle's leaf functions (tests/_ray_query.py): for every ray and every
primitive one orc_unit row, the smallest accepted t and "any flag set".  Every walk an upload can
choose answers the same rays: t must be the brute force's bit for bit under each of them, and so
bit-equal across them; only which of several primitives at exactly that t is reported may differ.

Figures measured on the device when these tests were written, each printed before it is asserted:
sphere normals deviate from unit length by at most 1.3e-7 and from the direction hit point - centre
by at most 1.6e-6 (the bounds, 1e-6 and 1e-5, are float32 rounding of a normalised vector)."""
import ctypes as C

import numpy as np
import pytest
import torch

import simplepath_amd as sp
from simplepath_amd import _abi
from tests import _lbvh_sets, _ray_query as rq, _refit_moves

pytestmark = pytest.mark.gpu

F = np.float32

# the walks of one scene: reference order with the stack and with parent links, the 8-wide SAH walk,
# the binary SAH walk for every query or for closest hits only, and both device builders
WALKS = {
    "reference": dict(bvh_mode=1),
    "reference_stackless": dict(bvh_mode=1, stackless=True),
    "wide": dict(),
    "binary": dict(wide_bvh=False),
    "binary_closest": dict(binary_closest=True),
    "device_lbvh": dict(builder="device"),
    "device_sah": dict(builder="device_sah"),
}
LEAF_WALKS = {"leaf1": dict(sah_leaf=1), "leaf4": dict(sah_leaf=4), "leaf1_binary": dict(sah_leaf=1, wide_bvh=False)}

# set -> rays: every count of {0, 1, 63, 64, 65, 255, 256, 257, 1000} occurs (0 and 1 also below)
SETS = {"tri1": 257, "tri2": 63, "tri5": 65, "tri64": 255, "tri65": 256, "tri257": 1000, "identical37": 64,
        "half_dup": 257, "mixed": 1000, "extra": 1000, "spheres_only": 1}


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ray_query"))
    out = {name: path for name, (path, _) in _lbvh_sets.write_all(d).items()}
    out["extra"] = rq.write_extra_scene(d)
    return out


class Case:
    """One set: its scene, primitives, rays and brute force, made once and left unchanged."""

    def __init__(self, path, n_rays, seed):
        self.scene = sp.Scene.from_file(path)
        self.prims = rq.Prims(self.scene)
        self.rays = rq.make_rays(self.prims, n_rays, seed)
        self.brute = rq.Brute(self.prims, self.rays)


@pytest.fixture(scope="module")
def cases(paths):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(paths[name], SETS[name], 100 + len(made))
        return made[name]
    return get


def trace_all(scene, rays):
    """closest with normals, closest without, any: the three kernels on the same rays"""
    hits_n, normals = scene.trace(rays["o"], rays["d"], rays["tmin"], rays["tmax"], normals=True)
    hits = scene.trace(rays["o"], rays["d"], rays["tmin"], rays["tmax"])
    occluded = scene.trace(rays["o"], rays["d"], rays["tmin"], rays["tmax"], mode="any")
    return hits_n, normals, hits, occluded


def check_walk(case, what):
    hits_n, normals, hits, occluded = trace_all(case.scene, case.rays)
    rq.check_closest(case.prims, case.rays, hits, case.brute, what)
    assert hits_n.tobytes() == hits.tobytes(), f"{what}: normals=False returns the same hit records"
    rq.check_any(case.rays, occluded, case.brute, what)
    print(f"{what}: {case.rays.shape[0]} rays, {int((hits['kind'] != rq.MISS).sum())} hits, {int(occluded.sum())} occluded")
    rq.check_normals(case.prims, case.rays, hits_n, normals, what)
    return hits


@pytest.mark.parametrize("walk", list(WALKS))
@pytest.mark.parametrize("name", list(SETS))
def test_every_walk_answers_the_brute_force(cases, name, walk):
    case = cases(name)
    case.scene.upload(device=0, **WALKS[walk])
    check_walk(case, f"{name}/{walk}")


@pytest.mark.parametrize("name", list(SETS))
def test_t_is_bit_equal_across_the_walks(cases, name):
    case = cases(name)
    t_bits = {}
    for walk, options in {**WALKS, **(LEAF_WALKS if name == "tri257" else {})}.items():
        case.scene.upload(device=0, **options)
        t_bits[walk] = rq.bits(case.scene.trace(case.rays["o"], case.rays["d"], case.rays["tmin"], case.rays["tmax"])["t"]).copy()
    for walk, t in t_bits.items():
        assert np.array_equal(t, t_bits["reference"]), f"{name}: t differs between the walks reference and {walk}"


@pytest.mark.parametrize("walk", list(LEAF_WALKS))
def test_sah_leaf_sizes(cases, walk):
    case = cases("tri257")
    case.scene.upload(device=0, **LEAF_WALKS[walk])
    check_walk(case, f"tri257/{walk}")


# Finite rays whose slab tests meet 0 * inf: the 8-wide walk orders children by entry distance, and
# a NaN one must be entered, not lose the walk its way.  Every walk answers
# them as the brute force does.
@pytest.mark.parametrize("walk", ["wide", "binary_closest", "device_lbvh", "device_sah", "leaf1", "binary", "reference"])
@pytest.mark.parametrize("name", ["tri257", "half_dup", "mixed", "extra"])
def test_rays_in_a_box_plane_are_walked(paths, name, walk):
    scene = sp.Scene.from_file(paths[name])
    p = rq.Prims(scene)
    scene.upload(device=0, **{**WALKS, **LEAF_WALKS}[walk])
    for axis in (2, 1, 0):
        rays = rq.plane_rays(p, axis)
        assert rq.usable(rays).all()
        brute = rq.Brute(p, rays)
        hits_n, normals, hits, occluded = trace_all(scene, rays)
        what = f"{name}/{walk}: rays in a plane of axis {axis}"
        print(f"{what}: {rays.shape[0]} rays, {int(brute.occluded.sum())} hit")
        rq.check_closest(p, rays, hits, brute, what)
        rq.check_any(rays, occluded, brute, what)
        rq.check_normals(p, rays, hits_n, normals, what)
        assert hits_n.tobytes() == hits.tobytes()


@pytest.mark.parametrize("n", [0, 1])
def test_smallest_counts(cases, n):
    case = cases("mixed")
    case.scene.upload(device=0)
    rays = case.rays[:n]
    hits_n, normals, hits, occluded = trace_all(case.scene, rays)
    assert hits.shape == (n,) and normals.shape == (n, 3) and occluded.shape == (n,)
    brute = rq.Brute(case.prims, rays)
    rq.check_closest(case.prims, rays, hits, brute, f"{n} rays")
    rq.check_any(rays, occluded, brute, f"{n} rays")
    st = _abi.sp_ray_query_stats()
    st.struct_size = C.sizeof(st)
    q = _abi.sp_ray_query()
    q.struct_size, q.mode, q.num_rays = C.sizeof(q), _abi.SP_QUERY_ANY, 0
    assert sp.lib().sp_scene_trace_rays(case.scene.handle, C.byref(q), C.byref(st)) == _abi.SP_OK
    assert (st.launches, st.rays, st.hits) == (0, 0, 0)  # num_rays == 0 succeeds and launches nothing


def with_limits(rays, tmin=None, tmax=None):
    r = rays.copy()
    if tmin is not None:
        r["tmin"] = tmin
    if tmax is not None:
        r["tmax"] = tmax
    return r


@pytest.mark.parametrize("walk", ["reference", "wide", "binary", "device_lbvh"])
@pytest.mark.parametrize("name", ["mixed", "identical37", "extra"])
def test_exact_limits(cases, name, walk):
    case = cases(name)
    p, scene = case.prims, case.scene
    scene.upload(device=0, **WALKS[walk])
    base = scene.trace(case.rays["o"], case.rays["d"], case.rays["tmin"], case.rays["tmax"])
    sel = np.flatnonzero(base["kind"] != rq.MISS)
    assert sel.size > case.rays.shape[0] // 2
    rays, t = case.rays[sel], base["t"][sel].copy()
    first = (base["kind"][sel], base["index"][sel])

    def run(r, what):
        brute = rq.Brute(p, r)
        hits = scene.trace(r["o"], r["d"], r["tmin"], r["tmax"])
        occluded = scene.trace(r["o"], r["d"], r["tmin"], r["tmax"], mode="any")
        rq.check_closest(p, r, hits, brute, f"{name}/{walk}: {what}")
        rq.check_any(r, occluded, brute, f"{name}/{walk}: {what}")
        return hits, occluded

    hits, occluded = run(with_limits(rays, tmax=t), "tmax = t")
    assert np.array_equal(rq.bits(hits["t"]), rq.bits(t)) and occluded.all()
    below = np.nextafter(t, F(0.0))
    hits, occluded = run(with_limits(rays, tmax=below), "tmax = nextafter(t, 0)")
    h = hits["kind"] != rq.MISS
    assert (hits["t"][h] <= below[h]).all() and (hits["t"][h] < t[h]).all()  # that primitive is no longer reported
    hits, occluded = run(with_limits(rays, tmin=t), "tmin = t")
    assert np.array_equal(rq.bits(hits["t"]), rq.bits(t)) and occluded.all()
    above = np.nextafter(t, F(np.inf))
    hits, occluded = run(with_limits(rays, tmin=above), "tmin = nextafter(t, inf)")
    h = hits["kind"] != rq.MISS
    assert (hits["t"][h] >= above[h]).all()
    same = h & (hits["kind"] == first[0]) & (hits["index"] == first[1])
    assert (hits["t"][same] > t[same]).all()  # a sphere's far side at most, never the hit at t
    hits, occluded = run(with_limits(rays, tmin=(t * F(2.0)).astype(F), tmax=t), "tmin > tmax")
    assert (hits["kind"] == rq.MISS).all() and not occluded.any()


@pytest.mark.parametrize("walk", ["reference", "reference_stackless", "wide", "binary", "device_lbvh"])
def test_degenerate_rays_are_safe_misses(cases, walk):
    case = cases("mixed")
    scene = case.scene
    scene.upload(device=0, **WALKS[walk])
    base = scene.trace(case.rays["o"], case.rays["d"], case.rays["tmin"], case.rays["tmax"])
    good = case.rays[np.flatnonzero(base["kind"] != rq.MISS)[:8]].copy()
    nan, inf = F(np.nan), F(np.inf)
    bad = np.concatenate([good, good, good])[:20].copy()
    bad["d"][0] = 0.0                       # zero direction
    bad["d"][1] = [-0.0, 0.0, -0.0]
    bad["o"][2, 0] = nan                    # NaN in the origin
    bad["o"][3] = nan
    bad["d"][4, 1] = nan                    # NaN in the direction
    bad["d"][5] = nan
    bad["o"][6, 2] = inf                    # infinite origin, infinite direction
    bad["d"][7, 0] = -inf
    bad["tmin"][8] = nan                    # NaN limits
    bad["tmax"][9] = nan
    bad["tmax"][10] = 0.25                  # (an ordinary short ray among them)
    n_bad = 10
    hits, normals = scene.trace(bad["o"], bad["d"], bad["tmin"], bad["tmax"], normals=True)   # returns: SP_OK
    occluded = scene.trace(bad["o"], bad["d"], bad["tmin"], bad["tmax"], mode="any")
    assert not rq.usable(bad[:n_bad]).any() and rq.usable(bad[n_bad:]).all()
    assert (hits["kind"][:n_bad] == rq.MISS).all() and not occluded[:n_bad].any()
    assert np.array_equal(rq.bits(hits["t"][:n_bad]), rq.bits(bad["tmax"][:n_bad]))
    assert not rq.bits(normals[:n_bad]).any()
    brute = rq.Brute(case.prims, bad)
    rq.check_closest(case.prims, bad, hits, brute, f"degenerate/{walk}")
    rq.check_any(bad, occluded, brute, f"degenerate/{walk}")
    # an infinite tmax works: the hits of the finite limit, and a miss reports the ray's own +inf
    far = with_limits(case.rays, tmax=inf)
    hits_inf = scene.trace(far["o"], far["d"], far["tmin"], far["tmax"])
    occ_inf = scene.trace(far["o"], far["d"], far["tmin"], far["tmax"], mode="any")
    hit = base["kind"] != rq.MISS
    assert hits_inf[hit].tobytes() == base[hit].tobytes()
    assert (hits_inf["kind"][~hit] == rq.MISS).all() and np.isposinf(hits_inf["t"][~hit]).all()
    assert np.array_equal(occ_inf, hit)


@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("name", ["tri65", "mixed"])
def test_after_a_refit_the_moved_mesh_answers(paths, name, builder):
    scene = sp.Scene.from_file(paths[name])
    scene.upload(device=0, builder=builder)
    v, f = _refit_moves.mesh_of(scene)
    moved = _refit_moves.jitter(v, f)
    assert not np.array_equal(moved, v)
    scene.update_mesh(moved)
    p = rq.Prims(scene)
    assert np.array_equal(p.vertices, moved)
    rays = rq.make_rays(p, 257, 77)
    brute = rq.Brute(p, rays)
    hits_n, normals, hits, occluded = trace_all(scene, rays)
    rq.check_closest(p, rays, hits, brute, f"{name}/{builder} refitted")
    rq.check_any(rays, occluded, brute, f"{name}/{builder} refitted")
    rq.check_normals(p, rays, hits_n, normals, f"{name}/{builder} refitted")
    assert (hits["kind"] == rq.TRI).sum() > 50
    # and not the first pose's answers
    old = rq.Brute(rq.Prims(sp.Scene.from_file(paths[name])), rays)
    assert not np.array_equal(rq.bits(old.t_closest), rq.bits(brute.t_closest))


def test_device_buffers_are_stream_ordered_with_renders(cases):
    case = cases("extra")
    scene, rays = case.scene, case.rays
    scene.upload(device=0)
    n = rays.shape[0]
    host_hits, host_normals = scene.trace(rays["o"], rays["d"], rays["tmin"], rays["tmax"], normals=True)
    host_occ = scene.trace(rays["o"], rays["d"], rays["tmin"], rays["tmax"], mode="any")
    n_tiles = sp.TileScheduler(scene.width, scene.height).get_num_tiles()
    ref = torch.zeros((n_tiles, 64, 3), dtype=torch.float32, device="cuda:0")
    ref_stats = sp.render_tiles_device(scene, "direct_lighting", 4, None, ref.data_ptr())
    torch.cuda.synchronize()

    d_rays = torch.from_numpy(rays.view(np.float32).reshape(n, 8).copy()).cuda()
    d_hits = torch.zeros((n, 8), dtype=torch.int32, device="cuda:0")
    d_normals = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
    d_occ = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    out = torch.zeros_like(ref)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        h = stream.cuda_stream
        assert scene.trace_device(d_rays.data_ptr(), n, hits_ptr=d_hits.data_ptr(), normals_ptr=d_normals.data_ptr(), stream=h) is None
        assert sp.render_tiles_device(scene, "direct_lighting", 4, None, out.data_ptr(), h, stats=False) is None
        assert scene.trace_device(d_rays.data_ptr(), n, occluded_ptr=d_occ.data_ptr(), mode="any", stream=h) is None
    stream.synchronize()
    assert d_hits.cpu().numpy().tobytes() == host_hits.tobytes()
    assert np.array_equal(d_normals.cpu().numpy()[:, :3].view(np.uint32), host_normals.view(np.uint32))
    assert not d_normals.cpu().numpy()[:, 3].view(np.uint32).any()
    assert np.array_equal(d_occ.cpu().numpy() != 0, host_occ)
    assert set(np.unique(d_occ.cpu().numpy())) <= {0, 1}
    assert torch.equal(out, ref)
    # the same sequence with the render's statistics: its rays are those of the render alone
    d_hits.zero_()
    with torch.cuda.stream(stream):
        scene.trace_device(d_rays.data_ptr(), n, hits_ptr=d_hits.data_ptr(), stream=h)
        st = sp.render_tiles_device(scene, "direct_lighting", 4, None, out.data_ptr(), h)
        q_any = scene.trace_device(d_rays.data_ptr(), n, occluded_ptr=d_occ.data_ptr(), mode="any", stream=h, stats=True)
        q_closest = scene.trace_device(d_rays.data_ptr(), n, hits_ptr=d_hits.data_ptr(), stream=h, stats=True)
    stream.synchronize()
    assert (st.rays, st.shadow_rays, st.samples) == (ref_stats.rays, ref_stats.shadow_rays, ref_stats.samples)
    assert torch.equal(out, ref)
    n_hit = int((host_hits["kind"] != rq.MISS).sum())
    assert (q_closest["rays"], q_closest["hits"], q_closest["launches"]) == (n, n_hit, 1)
    assert (q_any["rays"], q_any["hits"], q_any["launches"]) == (n, int(host_occ.sum()), 1)
    assert q_closest["kernel_ms"] > 0.0 and q_closest["stack_depth"] >= q_any["stack_depth"] > 0
    assert d_hits.cpu().numpy().tobytes() == host_hits.tobytes()


def test_a_progress_object_survives_a_query(cases):
    case = cases("mixed")
    scene = case.scene
    scene.upload(device=0)
    one_shot, _ = sp.render_tiles(scene, "direct_lighting", 4)
    with sp.Progressive(scene, "direct_lighting") as prog:
        prog.render(2)
        hits = scene.trace(case.rays["o"], case.rays["d"])
        rq.check_closest(case.prims, case.rays, hits, case.brute, "beside a progress object")
        tiles, _ = prog.render(2)  # still valid, and still the one-shot image
        assert np.array_equal(tiles.view(np.uint32), one_shot.view(np.uint32))


def test_a_scene_that_is_not_resident_refuses():
    from tests.test_gpu_upload_state import NESTED_CLEARCOAT
    scene = sp.Scene.from_string(NESTED_CLEARCOAT)
    with pytest.raises(sp.SimplePathError) as e:
        scene.upload(device=0)  # the upload releases what was resident, then fails: nothing is
    assert e.value.code == _abi.SP_ERR_UNSUPPORTED
    for mode in ("closest", "any"):
        with pytest.raises(sp.SimplePathError) as e:
            scene.trace(np.zeros((2, 3)), np.ones((2, 3)), mode=mode)
        assert e.value.code == _abi.SP_ERR_STATE
    with pytest.raises(sp.SimplePathError) as e:
        scene.trace_device(0x1000, 2, hits_ptr=0x1000)
    assert e.value.code == _abi.SP_ERR_STATE
