"""TEST INFRASTRUCTURE for the denoiser tests: the edge-avoiding a-trous filter of
include/simplepath_hip.h ("denoising", THE RULE) restated in numpy float32 on tile-packed arrays,
one tap at a time over all pixels at once.  Written from the rule, not from the C header: expf is
glibc's through the oracle (numpy's exp is not glibc's), every other step is one float32 numpy
operation, which neither contracts nor reorders.  Returns the image and the number of counted taps.
Also the synthetic buffers the host and the device tests share.  Nothing here touches a device."""
import numpy as np

from tests import _units

F = np.float32
U = np.uint32
H = (F(1.0 / 16.0), F(1.0 / 4.0), F(3.0 / 8.0), F(1.0 / 4.0), F(1.0 / 16.0))
GUIDES = ("albedo", "normal", "depth", "coverage")
DEFAULTS = dict(iterations=4, sigma_color=0.6, sigma_normal=0.3, sigma_depth=0.2, sigma_coverage=0.4, albedo_floor=0.0,
                depth_floor=0.0)


def expf(x: np.ndarray) -> np.ndarray:
    """glibc's expf on a float32 array of any shape"""
    x = np.ascontiguousarray(x, dtype=F)
    if x.size == 0:
        return x.copy()
    return _units.oracle_unit("glibc", "expf", x.reshape(-1, 1).view(U))[:, 0].view(F).reshape(x.shape)


def _spread(v):
    return (v & 1) | ((v & 2) << 1) | ((v & 4) << 2)


def morton_lane(x, y):
    """the pixel's Morton index in its 8x8 tile: x in the even bits, y in the odd ones"""
    return _spread(x & 7) | (_spread(y & 7) << 1)


def layout(width: int, height: int, tile_ids):
    """px, py [slots, 64], which pixel slots lie inside the image, and slot_of_tile (-1: absent; a
    repeated id: its lowest slot).  tile_ids None: every tile; an id outside the frame: no pixel."""
    tiles_x, tiles_y = (width + 7) // 8, (height + 7) // 8
    total = tiles_x * tiles_y
    ids = np.arange(total, dtype=np.int64) if tile_ids is None else np.asarray(tile_ids, dtype=np.int64).reshape(-1)
    valid = (ids >= 0) & (ids < total)
    safe = np.where(valid, ids, 0)
    lx = np.zeros(64, dtype=np.int64)
    ly = np.zeros(64, dtype=np.int64)
    for y in range(8):
        for x in range(8):
            lane = int(morton_lane(np.int64(x), np.int64(y)))
            lx[lane], ly[lane] = x, y
    px = (safe % tiles_x)[:, None] * 8 + lx[None, :]
    py = (safe // tiles_x)[:, None] * 8 + ly[None, :]
    inside = valid[:, None] & (px < width) & (py < height)
    slot_of_tile = np.full(total, -1, dtype=np.int64)
    for s in range(ids.size - 1, -1, -1):
        if valid[s]:
            slot_of_tile[ids[s]] = s
    return px, py, inside, slot_of_tile, tiles_x


def denoise(width, height, tile_ids, color, albedo=None, normal=None, depth=None, coverage=None, iterations=4, sigma_color=0.6,
            sigma_normal=0.3, sigma_depth=0.2, sigma_coverage=0.4, albedo_floor=0.0, depth_floor=0.0, demodulate=True):
    """THE RULE on tile-packed float32 arrays ([slots, 64, 3] and [slots, 64]); returns (out, taps)"""
    px, py, inside, slot_of_tile, tiles_x = layout(width, height, tile_ids)
    n = px.shape[0]
    c = np.ascontiguousarray(color, dtype=F).reshape(n, 64, 3)
    arr = lambda v, *shape: None if v is None else np.ascontiguousarray(v, dtype=F).reshape((n, 64) + shape)
    a, nrm, z, k = arr(albedo, 3), arr(normal, 3), arr(depth), arr(coverage)
    albedo_floor = F(albedo_floor) if F(albedo_floor) != 0 else F(0.01)
    depth_floor = F(depth_floor) if F(depth_floor) != 0 else F(1e-3)
    one = F(1.0)
    with np.errstate(all="ignore"):
        # prepare
        if demodulate:
            s = (k[..., None] * a) + (one - k)[..., None]
            m = np.where(s > albedo_floor, s, albedo_floor).astype(F)  # a NaN gives the floor
            x = c / m
        else:
            m, x = None, c.copy()
        if z is not None:
            g = one / (F(sigma_depth) * np.where(z > depth_floor, z, depth_floor).astype(F))
        taps = 0
        for i in range(int(iterations)):
            step = 1 << i
            sc = F(sigma_color) * F(2.0 ** -i)
            inv_c = one / (sc * sc)
            inv_n = one / (F(sigma_normal) * F(sigma_normal)) if nrm is not None else None
            inv_k = one / (F(sigma_coverage) * F(sigma_coverage)) if k is not None else None
            acc = np.zeros((n, 64, 3), dtype=F)
            wsum = np.zeros((n, 64), dtype=F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qx, qy = px + dx * step, py + dy * step
                    ok = inside & (qx >= 0) & (qx < width) & (qy >= 0) & (qy < height)
                    qtile = np.where(ok, (qy // 8) * tiles_x + qx // 8, 0)
                    sq = slot_of_tile[qtile]
                    ok &= sq >= 0  # q's tile is not in the list: skipped
                    sq = np.where(ok, sq, 0)
                    lq = np.where(ok, morton_lane(qx, qy), 0)
                    h2 = H[dx + 2] * H[dy + 2]
                    xq = x[sq, lq]
                    d = xq - x
                    e = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * inv_c
                    zero = np.zeros_like(e)
                    if nrm is not None:
                        d = nrm[sq, lq] - nrm
                        e = e + ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * inv_n
                    else:
                        e = e + zero
                    if z is not None:
                        dz = (z[sq, lq] - z) * g
                        e = e + dz * dz
                    else:
                        e = e + zero
                    if k is not None:
                        dk = k[sq, lq] - k
                        e = e + (dk * dk) * inv_k
                    else:
                        e = e + zero
                    w = h2 * expf(-e)
                    counted = ok & (w > 0)  # NaN and 0 fail the comparison
                    acc = np.where(counted[..., None], acc + w[..., None] * xq, acc)
                    wsum = np.where(counted, wsum + w, wsum)
                    taps += int(counted.sum())
            x = np.where((wsum > 0)[..., None], acc / wsum[..., None], x).astype(F)
        out = x * m if demodulate else x
        out = np.where(inside[..., None], out, F(0.0)).astype(F)
    return out, taps


def relative_l2(image, truth) -> float:
    """||image - truth||_2 / ||truth||_2 in float64"""
    image, truth = np.asarray(image, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    return float(np.sqrt(np.sum((image - truth) ** 2) / np.sum(truth ** 2)))


def synthetic(width: int, height: int, slots: int, seed: int = 20250, planted: bool = True) -> dict:
    """Fixed-seed buffers for `slots` tile slots: a smooth colour under noise, a textured albedo,
    unit-ish normals, a depth with a step, coverage in [0, 1].  planted: a NaN colour, a +inf colour,
    -0 components, a zero-coverage region, zero albedo at full coverage (the floor) and exact
    zeros in the depth (its floor)."""
    g = np.random.default_rng(seed)
    shape = (slots, 64)
    albedo = g.uniform(0.05, 0.95, shape + (3,)).astype(F)
    color = (albedo * g.uniform(0.2, 1.5, shape + (1,)).astype(F) + g.normal(0.0, 0.15, shape + (3,)).astype(F)).astype(F)
    normal = g.normal(0.0, 1.0, shape + (3,)).astype(F)
    normal = (normal / np.linalg.norm(normal, axis=-1, keepdims=True)).astype(F)
    depth = g.uniform(2.0, 3.0, shape).astype(F)
    depth[slots // 2:] += F(4.0)  # a depth step between the slots' halves
    coverage = np.clip(g.uniform(-0.3, 1.3, shape), 0.0, 1.0).astype(F)
    if planted:
        flat = lambda v: v.reshape(slots * 64, -1)
        pick = g.permutation(slots * 64)
        flat(color)[pick[0]] = np.nan
        flat(color)[pick[1]] = np.inf
        flat(color)[pick[2:6], 0] = F(-0.0)
        flat(color)[pick[6], :] = F(-0.0)
        flat(coverage)[pick[10:40]] = F(0.0)
        coverage[slots - 1] = F(0.0)  # a zero-coverage region: one whole slot
        flat(depth)[pick[10:40]] = F(0.0)
        flat(albedo)[pick[40:60]] = F(0.0)
        flat(coverage)[pick[40:50]] = F(1.0)  # s = 0: the floor
    return dict(color=color, albedo=albedo, normal=normal, depth=depth, coverage=coverage,
                planted=(np.unravel_index(pick[:2], shape) if planted else None))
