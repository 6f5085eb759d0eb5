"""TEST INFRASTRUCTURE for the feature-buffer tests (tests/test_gpu_features.py): the
render's camera sample restated step by step in numpy float32 (rseq_component and tail_camera_ray,
csrc/common/sp_rng.h and csrc/hip/sp_mega.hpp), the per-sample first hits from the brute force of
tests/_ray_query.py or from a residency's own ray query, and the reduction of sp_scene_features one
sample at a time.  Only samples_from_trace touches a device."""
import numpy as np

from tests import _ray_query as rq, _units

F = np.float32
U = np.uint32
VARIANT = "glibc"
PI_F = F(3.14159274)
FLT_MAX = F(np.finfo(np.float32).max)
SEED_2D = 0x6184FAF4  # RSequenceSampler m_seed_2D (main.cpp:67)
FLOAT_OUTPUTS = ("coverage", "depth", "normal", "albedo")


def _unit1(name: str, *cols) -> np.ndarray:
    r = np.stack([np.ascontiguousarray(c, dtype=F).reshape(-1) for c in cols], axis=1).view(U)
    return _units.oracle_unit(VARIANT, name, r)[:, 0].view(F)


def _powf(x, y) -> np.float32:
    return _unit1("powf", np.array([x], dtype=F), np.array([y], dtype=F))[0]


def alphas():
    """sph::rsequence_alphas' alpha2 (RSequence<2>'s constructor, math/Sampler.h) with glibc's powf"""
    x = F(2.0)
    third = F(1.0) / (F(2.0) + F(1.0))
    for _ in range(10):
        x = _powf(F(1.0) + x, third)
    inv = F(1.0) / x
    out = []
    for k in (F(1.0), F(2.0)):
        v = _powf(inv, k)
        out.append(F(v - np.trunc(v)))
    return out[0], out[1]


def rseq_component(seed: np.ndarray, alpha: np.float32, n: int) -> np.ndarray:
    """sp_rng.h rseq_component: (float)seed / FLT_MAX, + alpha * ((float)n + 1), fractional part"""
    fseed = seed.astype(U).astype(F) / FLT_MAX
    f = (fseed + F(alpha) * (F(n) + F(1.0))).astype(F)
    return (f - np.trunc(f)).astype(F)


def _morton1(a: np.ndarray) -> np.ndarray:
    out = np.zeros_like(a)
    for b in range(3):
        out |= ((a >> (2 * b)) & 1) << b
    return out


def pixels(width: int, height: int, tile_ids) -> tuple:
    """px, py [slots, 64] (int64) and which of them lie inside the image; tile_ids None: every tile"""
    tiles_x = (width + 7) // 8
    if tile_ids is None:
        tile_ids = np.arange(tiles_x * ((height + 7) // 8))
    t = np.asarray(tile_ids, dtype=np.int64)[:, None]
    lane = np.arange(64, dtype=np.int64)[None, :]
    px = (t % tiles_x) * 8 + _morton1(lane)
    py = (t // tiles_x) * 8 + _morton1(lane >> 1)
    return px, py, (px < width) & (py < height)


def camera_array(cam) -> np.ndarray:
    """[4, 3] float32 {vx, vy, vz, p} of a sp_camera_desc"""
    t = cam.transform
    return np.array([list(t.vx), list(t.vy), list(t.vz), list(t.p)], dtype=F)


def camera_rays(cam: np.ndarray, width: int, height: int, tile_ids, first_sample: int, num_samples: int) -> np.ndarray:
    """tail_camera_ray for every (slot, sample, lane): a RAY_DTYPE array [slots, num_samples, 64];
    all-zero records outside the image"""
    import simplepath_amd as sp
    px, py, inside = pixels(width, height, tile_ids)
    a0, a1 = alphas()
    seed = (((px << 16) | py) ^ SEED_2D).astype(U)
    rays = np.zeros((px.shape[0], num_samples, 64), dtype=sp.RAY_DTYPE)
    vx, vy, vz, p = cam
    for s in range(num_samples):
        i = first_sample + s
        fx = (px.astype(F) + rseq_component(seed, a0, i)).astype(F)
        fy = (py.astype(F) + rseq_component(seed, a1, i)).astype(F)
        v = ((fx[..., None] * vx + fy[..., None] * vy).astype(F) + vz).astype(F)  # add(add(scale, scale), vz)
        flat = v.reshape(-1, 3)
        r = _unit1("rsqrt_ref_u32", _unit1("dot", flat[:, 0], flat[:, 1], flat[:, 2], flat[:, 0], flat[:, 1], flat[:, 2]))
        d = (flat * r[:, None]).astype(F).reshape(v.shape)
        rec = rays[:, s, :]
        rec["o"], rec["d"], rec["tmin"], rec["tmax"] = p, d, F(0.001), FLT_MAX
        rec[~inside] = np.zeros((), dtype=sp.RAY_DTYPE)
    return rays


class Materials:
    """a(m) of the issue: lambert_albedo * pi (float32), a clearcoat's from its base"""

    def __init__(self, scene):
        d = scene.desc()
        n = d.info.num_materials
        kind = np.array([d.materials[i].kind for i in range(n)])
        base = np.array([d.materials[i].base for i in range(n)])
        lam = np.array([list(d.materials[i].lambert_albedo) for i in range(n)], dtype=F).reshape(n, 3)
        src = np.where(kind == 2, base, np.arange(n))
        assert (kind[src] != 2).all()
        self.kind = kind
        self.albedo = (lam[src] * PI_F).astype(F)


class Samples:
    """The first hits of rays [slots, n, 64], per sample: hit, t, kind, index, material, normal,
    albedo ([slots, n, 64(, 3)]); sphere: pixels-by-sample whose normal came from a ray query"""

    def __init__(self, rays, inside):
        self.rays, self.inside = rays, inside
        shape = rays.shape
        self.hit = np.zeros(shape, dtype=bool)
        self.t = np.zeros(shape, dtype=F)
        self.kind = np.full(shape, -1, dtype=np.int32)
        self.index = np.full(shape, -1, dtype=np.int32)
        self.material = np.full(shape, -1, dtype=np.int32)
        self.normal = np.zeros(shape + (3,), dtype=F)
        self.albedo = np.zeros(shape + (3,), dtype=F)


def samples_from_trace(scene, rays, inside, mats: Materials) -> Samples:
    """a residency's own answers: scene.trace(..., normals=True) on the rays"""
    s = Samples(rays, inside)
    flat = rays.reshape(-1)
    hits, normals = scene.trace(flat["o"], flat["d"], flat["tmin"], flat["tmax"], normals=True)
    hit = hits["kind"] != rq.MISS
    s.hit = hit.reshape(rays.shape)
    assert not s.hit[~np.broadcast_to(inside[:, None, :], rays.shape)].any()  # an all-zero record is a miss
    s.t = np.where(hit, hits["t"], F(0)).astype(F).reshape(rays.shape)
    s.kind, s.index, s.material = (hits[k].reshape(rays.shape) for k in ("kind", "index", "material"))
    s.normal = normals.reshape(rays.shape + (3,))
    s.albedo = np.where(hit[:, None], mats.albedo[np.where(hit, hits["material"], 0)], F(0)).astype(F).reshape(rays.shape + (3,))
    s.sphere = s.hit & (s.kind == rq.SPHERE)
    return s


def samples_from_brute(prims: rq.Prims, rays, inside, mats: Materials, sphere_normals=None) -> Samples:
    """the brute force's: closest t and the one primitive that attains it (asserted unique), the
    triangle and plane normals restated on the host; sphere normals, which have no bit-exact host
    restatement, from sphere_normals [slots, n, 64, 3] (a ray query's) where given"""
    s = Samples(rays, inside)
    flat = rays.reshape(-1)
    live = np.flatnonzero(np.broadcast_to(inside[:, None, :], rays.shape).reshape(-1))
    brute = rq.Brute(prims, flat[live])
    hit = brute.occluded
    attains = brute.flag & (brute.t == brute.t_closest[:, None])
    assert (attains.sum(axis=1)[hit] == 1).all(), "the reported primitive is unambiguous"
    col = attains.argmax(axis=1)
    kind = np.where(col < prims.nt, rq.TRI, prims.shape_kind[np.maximum(col - prims.nt, 0)]).astype(np.int32)
    index = np.where(col < prims.nt, col, col - prims.nt).astype(np.int32)
    material = np.where(col < prims.nt, prims.tri_material[np.minimum(col, max(prims.nt - 1, 0))] if prims.nt else 0,
                        prims.shape_material[np.maximum(col - prims.nt, 0)]).astype(np.int32)
    normal = np.zeros((live.size, 3), dtype=F)
    tri = np.flatnonzero(hit & (kind == rq.TRI))
    if tri.size:
        rec = np.zeros(tri.size, dtype=[("index", "<i4"), ("beta", "<f4"), ("gamma", "<f4")])
        rec["index"], rec["beta"], rec["gamma"] = index[tri], brute.beta[tri, index[tri]], brute.gamma[tri, index[tri]]
        normal[tri] = rq.triangle_normals(prims, rec)
    pl = np.flatnonzero(hit & (kind == rq.PLANE))
    normal[pl] = prims.normal_vy[index[pl]]
    sph = np.flatnonzero(hit & (kind == rq.SPHERE))
    if sphere_normals is not None:
        normal[sph] = sphere_normals.reshape(-1, 3)[live[sph]]

    def put(dst, values, fill):
        out = np.full((flat.shape[0],) + values.shape[1:], fill, dtype=dst.dtype)
        out[live] = np.where(hit.reshape((-1,) + (1,) * (values.ndim - 1)), values, fill)
        return out.reshape(dst.shape)

    s.hit = put(s.hit, hit, False)
    s.t = put(s.t, brute.t_closest, F(0))
    s.kind, s.index, s.material = put(s.kind, kind, -1), put(s.index, index, -1), put(s.material, material, -1)
    s.normal = put(s.normal, normal, F(0))
    s.albedo = put(s.albedo, mats.albedo[material], F(0))
    s.sphere = put(np.zeros(rays.shape, dtype=bool), kind == rq.SPHERE, False)
    return s


def _sum_next(total, x, first, act):
    """a sum's next term: the first as it is, the others added in order (float32)"""
    return np.where(first, x, np.where(act, (total + x).astype(F), total)).astype(F)


def reduce(s: Samples, counts) -> dict:
    """sp_scene_features' outputs from per-sample first hits, one sample at a time.  counts: n of
    every slot (an int) or per slot.  Returns ids [slots, 64] FEATURE_IDS_DTYPE and the float buffers."""
    import simplepath_amd as sp
    slots = s.rays.shape[0]
    n = np.broadcast_to(np.asarray(counts, dtype=np.int64), (slots,))[:, None]  # [slots, 1]
    assert n.max(initial=0) <= s.rays.shape[1]
    cnt = np.zeros((slots, 64), dtype=np.int64)
    tsum = np.zeros((slots, 64), dtype=F)
    nsum = np.zeros((slots, 64, 3), dtype=F)
    asum = np.zeros((slots, 64, 3), dtype=F)
    ids = np.zeros((slots, 64), dtype=sp.FEATURE_IDS_DTYPE)
    ids["kind"] = ids["index"] = ids["material"] = -1
    for i in range(int(n.max(initial=0))):
        act = s.hit[:, i, :] & (i < n) & s.inside
        first = act & (cnt == 0)
        tsum = _sum_next(tsum, s.t[:, i, :], first, act)
        nsum = _sum_next(nsum, s.normal[:, i], first[..., None], act[..., None])
        asum = _sum_next(asum, s.albedo[:, i], first[..., None], act[..., None])
        if i == 0:
            for k in ("kind", "index", "material"):
                ids[k] = np.where(act, getattr(s, k)[:, 0, :], -1)
        cnt += act
    ids["hits"] = cnt
    any_hit = cnt > 0
    fh = np.where(any_hit, cnt, 1).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        coverage = np.where(any_hit, cnt.astype(F) / np.maximum(n, 1).astype(F), F(0)).astype(F)
    return {"ids": ids, "coverage": coverage,
            "depth": np.where(any_hit, tsum / fh, F(0)).astype(F),
            "normal": np.where(any_hit[..., None], nsum / fh[..., None], F(0)).astype(F),
            "albedo": np.where(any_hit[..., None], asum / fh[..., None], F(0)).astype(F)}


def sphere_pixels(s: Samples, counts) -> np.ndarray:
    """[slots, 64]: a sphere is among the pixel's hit samples"""
    n = np.broadcast_to(np.asarray(counts, dtype=np.int64), (s.rays.shape[0],))[:, None, None]
    return (s.sphere & (np.arange(s.rays.shape[1])[None, :, None] < n)).any(axis=1)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a).view(U)


def assert_equal(got: dict, want: dict, what: str, names=None, where=None) -> None:
    """every bit of the float buffers and every word of the ids; where: a [slots, 64] pixel mask"""
    for name in names or got:
        g, w = got[name], want[name]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if where is not None:
            g, w = g[where], w[where]
        words = {"ids": 4, "normal": 3, "albedo": 3}.get(name, 1)
        g, w = bits(g).reshape(-1, words), bits(w).reshape(-1, words)
        bad = np.flatnonzero((g != w).any(axis=1))
        assert bad.size == 0, f"{what}: {name} differs in {bad.size} of {g.shape[0]} pixels, first {bad[:4]}: {g[bad[:4]]} != {w[bad[:4]]}"
