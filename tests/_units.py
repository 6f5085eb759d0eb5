"""TEST INFRASTRUCTURE: the rows the device unit tests evaluate (tests/test_units_host.py,
tests/test_gpu_units.py).

FUNCTIONS tables every leaf function once: words per input row (k) and per output row (m), the
name oracle/sp_oracle.c orc_unit knows it by, how a NaN is compared, which RSQRTSS table form the
device gets, and the builder of its input rows.  tests/cpp/device_units.hip and orc_unit each
restate k and m in code; test_units_host.py checks orc_unit's against this table.

Row formats (32-bit words, floats as their bits):
    unary libm / sqrt / sqrt_unit / erfinv / rsqrt*   x -> f(x)          sincosf*: x -> sin, cos
    powf  x, y -> x^y        atan2f  y, x -> atan2(y, x)   powf_unit  x, y -> powf_unit, powf
    div  a, b -> a / b       fma, muladd  a, b, c          dop1  a, b, c, d
    dot  a3, b3 -> 1         cross  a3, b3 -> 3
    fresnel  cos_i, eta_i, eta_t                            beck11  cos_theta_i, U1, U2 -> x, y
    beck11_pre  wo3, alpha_x, alpha_y, U1, U2 -> x, y of the precomputed form, x, y of beck11
    uniform_sphere, uniform_hemisphere, cosine_hemisphere  u2 -> 3     concentric_disk  u2 -> 2
    onb_of_unit  v3 -> u3, v3, w3
    beck_D, beck_lambda  alpha_x, alpha_y, w3               beck_pdf  alpha_x, alpha_y, wo3, wh3
    mf_eval  alpha_x, alpha_y, ior, wo3, wi3 -> rgb         mf_pdf  alpha_x, alpha_y, wo3, wi3
    spherical_phi  v3        ray_offset  n3, d3
    tri_hit  p0, p1, p2, o3, d3, tmin, tmax -> flag, t, beta, gamma   (zeros after a miss)
    sphere_t, plane_t  world_to_object (vx, vy, vz, p), o3, d3, tmin, tmax -> flag, t
    box_hit  lo3, hi3, o3, d3, tmin, tmax -> flag
    stream  seed, seeding, 200 steps -> count, the values drawn   (section f below)
    the stream-fed layer (rho16 .. material_pdf: seed, skip, a material record, directions -> the words,
    the stream words consumed, one further draw; the light units) and the image environment light
    against small images: sections g and h below, which state their row formats

Kernel option sets.  sp_path.hpp is compiled under five sets of options (tests/cpp/Makefile SET_*);
the evaluator is built once per set, and the stream and the units that own a generator (DRAWING)
run in every set that compiles them.

NaN rule.  For every lm_* function, fmod1, round_f and rsqrtss_emulated the header restates the x86
result explicitly: all bits are compared for every input, NaN inputs and NaN results included
(rule ALL).  For everything else plain arithmetic decides a NaN's sign and payload: an output word
that is a NaN in the reference only has to be a NaN on the device (rule CLASS), such rows are
counted, and at most NAN_CAP of a function's rows may hold a reference NaN -- except for `div` and
the rsqrt_ref forms, whose special-value cross products are the point (their random rows are built
from finite, for rsqrt_ref positive, values and so meet the cap on their own).

Everything is made at run time from fixed seeds; rows are shuffled so that every wave holds special
and ordinary arguments side by side, and no row count is a multiple of 64.
"""
from __future__ import annotations

import ctypes as C
import os as _os
import re as _re
from collections import namedtuple

import numpy as np

ALL, CLASS = "all", "class"
NAN_CAP = 1e-3
STRIDE = 4099          # every 4099th of all 2^32 bit patterns
N_RANDOM = 1 << 19

F32_MAX = 0x7f7fffff
POWF_UNIT_X = (0x33800000, 0x3f7fffef)   # sp_libm.h POWF_UNIT_X_LO / HI: 2^-24, 1 - 1e-6f
POWF_FIT = (0x3ee3e95c, 0x3f7cd99d)      # sp_libm.h POWF_FIT_LO / HI (tests/golden/libm_forms_full.txt fitrange)

# The constants each function's source compares (the magnitude of) its argument with, as float
# bits (sp_libm.h; abstop limits are given as the first float of the next class).  The standard
# set holds the 65 floats within +-32 ulps of each, in both signs.
FRINGES = {
    "expf": [0x42b00000, 0x42b17217, 0xc2cff1b4 & 0x7fffffff, 0xc2ce8ecf & 0x7fffffff, 0x7f800000],
    "logf": [0x00800000, 0x3f800000, 0x7f800000, 0x3f330000],
    "sinf": [0x39800000, 0x3f400000, 0x42f00000, 0x7f800000],
    "cosf": [0x39800000, 0x3f400000, 0x42f00000, 0x7f800000],
    "sincosf": [0x39800000, 0x3f400000, 0x42f00000, 0x7f800000],
    "sincosf_bounded": [0x39800000, 0x3f400000],
    "erff": [0x04000000, 0x31800000, 0x3f580000, 0x3fa00000, 0x4036db6e, 0x40c00000, 0x7f800000],
    "acosf": [0x32800001, 0x3f000000, 0x3f800000, 0x7f800000],
    "atanf": [0x31000000, 0x3ee00000, 0x3f300000, 0x3f980000, 0x401c0000, 0x4c000000, 0x7f800000],
    "fmod1": [0x3f800000, 0x4b000000, 0x7f7fffff],
    "roundf": [0x3f000000, 0x3f800000, 0x3fc00000, 0x40200000, 0x4affffff, 0x4b000000, 0x4b800000],
    "sqrt": [0x00800000, 0x0f800000, 0x7f800000],
    "rsqrt": [0x00800000, 0x3f800000, 0x40000000, 0x7f800000],
    # erfinv switches polynomial at |log(1 - a^2)| = 6.125: a = sqrt(1 - exp(-6.125)) = 0x3f7fb848 to
    # the ulp; the fringe is wide enough (+-64) to hold the switch whichever way the log rounds
    "erfinv": [0x3f7fb848],
}

Spec = namedtuple("Spec", "k m oracle rule table nan_exempt rows image", defaults=(None,))  # image: a key of IMAGES (section h)


def _rng(name: str) -> np.random.Generator:
    return np.random.default_rng([0x5eed, *name.encode()])


def f2u(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def u2f(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint32).view(np.float32)


def _finish(name: str, parts, k: int) -> np.ndarray:
    """Stack the parts, shuffle the rows with a fixed seed, keep the count off the multiples of 64."""
    rows = np.concatenate([np.ascontiguousarray(p, dtype=np.uint32).reshape(-1, k) for p in parts])
    if rows.shape[0] % 64 == 0:
        rows = np.concatenate([rows, rows[:1]])
    _rng(name + "/shuffle").shuffle(rows, axis=0)
    return np.ascontiguousarray(rows)


def _fringe(consts, width=32) -> np.ndarray:
    out = []
    for c in consts:
        b = np.clip(np.arange(c - width, c + width + 1, dtype=np.int64), 0, 0x7fffffff).astype(np.uint32)
        out += [b, b | np.uint32(0x80000000)]
    return np.concatenate(out) if out else np.zeros(0, np.uint32)


def _classes() -> np.ndarray:
    """Every biased exponent with mantissas 0, 1, 0x400000 and 0x7fffff in both signs (+-0, +-inf, the
    smallest and largest denormals, quiet and signalling NaNs among them), and NaNs of further payloads."""
    e = np.arange(256, dtype=np.uint32)[:, None] << np.uint32(23)
    m = np.array([0, 1, 0x400000, 0x7fffff], dtype=np.uint32)[None, :]
    pos = (e | m).ravel()
    nans = np.array([0x7f800002, 0x7f812345, 0x7fa00000, 0x7fbfffff, 0x7fc00001, 0x7fc12345, 0x7fe00000,
                     0x7fffffff & ~0x1000], dtype=np.uint32)
    pos = np.concatenate([pos, nans])
    return np.concatenate([pos, pos | np.uint32(0x80000000)])


def standard_set(name: str, fringes=(), width=32) -> np.ndarray:
    """The standard set for one float argument, as bit patterns."""
    stride = np.arange(0, 1 << 32, STRIDE, dtype=np.uint64).astype(np.uint32)
    rand = _rng(name).integers(0, 1 << 32, N_RANDOM, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([_classes(), _fringe(fringes, width), stride, rand])


def _finite(bits: np.ndarray) -> np.ndarray:
    return bits[(bits & np.uint32(0x7f800000)) != np.uint32(0x7f800000)]


def _specials_then_finite(name: str, fringes, positive=False) -> np.ndarray:
    """Standard set for a CLASS function: every class and fringe value, the strided and random
    patterns without their NaNs and infinities (positive: without their sign)."""
    stride = np.arange(0, 1 << 32, STRIDE, dtype=np.uint64).astype(np.uint32)
    rand = _rng(name).integers(0, 1 << 32, N_RANDOM, dtype=np.uint64).astype(np.uint32)
    body = _finite(np.concatenate([stride, rand]))
    if positive:
        body = body & np.uint32(0x7fffffff)
    return np.concatenate([_classes(), _fringe(fringes), body])


# ------------------------------------------------------------------ a. libm
def _unary(name):
    return lambda: _finish(name, [standard_set(name, FRINGES[name])], 1)


def _rows_sincosf_bounded():
    # |y| < 120 only (abstop <= 0x42e): the standard set below 0x42f00000, the fringe just inside it
    s = standard_set("sincosf_bounded", FRINGES["sincosf_bounded"])
    s = s[(s & np.uint32(0x7fffffff)) < np.uint32(0x42f00000)]
    inside = np.arange(0x42f00000 - 64, 0x42f00000, dtype=np.uint32)
    return _finish("sincosf_bounded", [s, inside, inside | np.uint32(0x80000000)], 1)


PAIR_SPECIALS = u2f(np.array([
    0x00000000, 0x80000000, 0x3f800000, 0xbf800000, 0x7f800000, 0xff800000,            # +-0, +-1, +-inf
    0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fc12345, 0x7fa00000,            # NaNs
    0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000,            # denormals, FLT_MIN
    0x7f7fffff, 0xff7fffff,                                                            # +-FLT_MAX
    0x40400000, 0xc0400000, 0x40a00000, 0xc0a00000, 0x4b7fffff, 0xcb7fffff,            # odd: +-3, +-5, +-(2^24 - 1)
    0x40000000, 0xc0000000, 0x40800000, 0xc0800000,                                    # even: +-2, +-4
    0x3f000000, 0xbf000000, 0x3fc00000, 0xbfc00000, 0x40200000, 0xc0200000,            # half: +-.5, +-1.5, +-2.5
    0x4b800000, 0xcb800000, 0x4b000001, 0xcb000001,                                    # +-2^24, +-(2^23 + 1)
    0x3f7fffff, 0x3f800001, 0x41200000, 0x3dcccccd,                                    # 1 -+ ulp, 10, 0.1
], dtype=np.uint32))


def _cross2(v) -> np.ndarray:
    a, b = np.meshgrid(f2u(v), f2u(v), indexing="ij")
    return np.stack([a.ravel(), b.ravel()], axis=1)


def _random_pairs(name, n=N_RANDOM) -> np.ndarray:
    return _rng(name).integers(0, 1 << 32, (n, 2), dtype=np.uint64).astype(np.uint32)


def _box_pairs(name, n) -> np.ndarray:
    """x from [2^-24, 1 - 1e-6f] (half uniform in the bits, half uniform in the value), y uniform in
    the bits of the fit range."""
    g = _rng(name)
    xb = g.integers(POWF_UNIT_X[0], POWF_UNIT_X[1] + 1, n // 2, dtype=np.uint64).astype(np.uint32)
    lo, hi = u2f([POWF_UNIT_X[0]])[0], u2f([POWF_UNIT_X[1]])[0]
    xv = np.clip(g.uniform(lo, hi, n - n // 2).astype(np.float32), lo, hi)
    y = g.integers(POWF_FIT[0], POWF_FIT[1] + 1, n, dtype=np.uint64).astype(np.uint32)
    return np.stack([np.concatenate([xb, f2u(xv)]), y], axis=1)


def _rows_powf():
    return _finish("powf", [_cross2(PAIR_SPECIALS), _random_pairs("powf"), _box_pairs("powf/box", 1 << 18)], 2)


def _rows_atan2f():
    g = _rng("atan2f/unit")
    th = g.uniform(-np.pi, np.pi, 1 << 18)
    unit = np.stack([f2u(np.sin(th)), f2u(np.cos(th))], axis=1)  # y first, x second
    return _finish("atan2f", [_cross2(PAIR_SPECIALS), _random_pairs("atan2f"), unit], 2)


def _rows_powf_unit():
    # the box lm_powf_unit claims, both faces of each interval included
    g = _rng("powf_unit")
    n = 1 << 13
    body = _box_pairs("powf_unit/box", N_RANDOM)
    faces = []
    for xf in POWF_UNIT_X:
        y = g.integers(POWF_FIT[0], POWF_FIT[1] + 1, n, dtype=np.uint64).astype(np.uint32)
        y[:2] = POWF_FIT
        faces.append(np.stack([np.full(n, xf, np.uint32), y], axis=1))
    for yf in POWF_FIT:
        x = g.integers(POWF_UNIT_X[0], POWF_UNIT_X[1] + 1, n, dtype=np.uint64).astype(np.uint32)
        faces.append(np.stack([x, np.full(n, yf, np.uint32)], axis=1))
    return _finish("powf_unit", [body] + faces, 2)


# ------------------------------------------------------------------ b. arithmetic under the build flags
def _finite_bits(g, shape) -> np.ndarray:
    """Random finite bit patterns: any sign, biased exponent 0..254, any mantissa."""
    b = g.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)
    e = g.integers(0, 255, shape, dtype=np.uint64).astype(np.uint32)
    return (b & np.uint32(0x807fffff)) | (e << np.uint32(23))


def _denormal_bits(g, shape) -> np.ndarray:
    b = g.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)
    return b & np.uint32(0x807fffff)


def _scaled(g, n, lo_exp, hi_exp) -> np.ndarray:
    """Random-sign floats with a uniform mantissa and a binary exponent uniform in [lo_exp, hi_exp]."""
    m = g.uniform(1.0, 2.0, n) * np.where(g.integers(0, 2, n) == 1, -1.0, 1.0)
    return (m * np.exp2(g.integers(lo_exp, hi_exp + 1, n).astype(np.float64))).astype(np.float32)


def _rows_div():
    g = _rng("div")
    n = 1 << 17
    rand = _finite_bits(g, (N_RANDOM, 2))
    den_a = np.stack([_denormal_bits(g, n), _finite_bits(g, n)], axis=1)          # denormal / any
    den_b = np.stack([_finite_bits(g, n), _denormal_bits(g, n)], axis=1)          # any / denormal
    tiny_large = np.stack([f2u(_scaled(g, n, -126, -100)), f2u(_scaled(g, n, 10, 40))], axis=1)  # denormal results
    return _finish("div", [_cross2(PAIR_SPECIALS), rand, den_a, den_b, tiny_large], 2)


def _rows_sqrt():
    g = _rng("sqrt/denormal")
    den = _denormal_bits(g, 1 << 17) & np.uint32(0x7fffffff)                       # sqrt of a denormal
    return _finish("sqrt", [_specials_then_finite("sqrt", FRINGES["sqrt"], positive=True), den], 1)


TRIPLE_SPECIALS = u2f(np.array([0x00000000, 0x80000000, 0x3f800000, 0xbf800000, 0x7f800000, 0xff800000, 0x7fc00000,
                                0x7f800001, 0x00000001, 0x807fffff, 0x7f7fffff, 0x00800000], dtype=np.uint32))


def _rows_fma(name):
    def build():
        g = _rng("fma")  # fma and muladd run the same rows
        n = 1 << 17
        a, b, c = np.meshgrid(f2u(TRIPLE_SPECIALS), f2u(TRIPLE_SPECIALS), f2u(TRIPLE_SPECIALS), indexing="ij")
        cross = np.stack([a.ravel(), b.ravel(), c.ravel()], axis=1)
        rand = _finite_bits(g, (N_RANDOM, 3))
        # denormal operands; tiny x tiny with a denormal or zero addend: denormal products and results
        den = np.stack([_denormal_bits(g, n), _finite_bits(g, n), _denormal_bits(g, n)], axis=1)
        tt = np.stack([f2u(_scaled(g, n, -75, -64)), f2u(_scaled(g, n, -75, -64)),
                       np.where(g.integers(0, 2, n) == 1, _denormal_bits(g, n), np.uint32(0))], axis=1)
        # c = -(a * b rounded): the fused form leaves the product's rounding error, the unfused one +0
        x, y = _scaled(g, n, -20, 20), _scaled(g, n, -20, 20)
        cancel = np.stack([f2u(x), f2u(y), f2u(-(x * y))], axis=1)
        return _finish(name, [cross, rand, den, tt, cancel], 3)
    return build


def _rows_sqrt_unit():
    # its domain: +-0, every exponent from 2^-96 up with the four mantissas, every float in
    # [1 - 2^-10, 1], random values in [2^-96, FLT_MAX]
    g = _rng("sqrt_unit")
    e = np.arange(31, 255, dtype=np.uint32)[:, None] << np.uint32(23)
    cls = (e | np.array([0, 1, 0x400000, 0x7fffff], dtype=np.uint32)[None, :]).ravel()
    near1 = np.arange(0x3f7fc000, 0x3f800001, dtype=np.uint32)
    rand = g.integers(0x0f800000, F32_MAX + 1, N_RANDOM, dtype=np.uint64).astype(np.uint32)
    zeros = np.array([0, 0x80000000], dtype=np.uint32)
    return _finish("sqrt_unit", [zeros, cls, near1, rand], 1)


def _vectors(g, n, lo_exp=-10, hi_exp=10) -> np.ndarray:
    return np.stack([_scaled(g, n, lo_exp, hi_exp) for _ in range(3)], axis=1)


def _rows_dot_cross(name):
    def build():
        g = _rng("dot")  # dot and cross run the same rows
        a, b = _vectors(g, N_RANDOM), _vectors(g, N_RANDOM)
        # cancelling pairs: b orthogonal to a up to rounding (a . b near 0), and b parallel to a (a x b near 0)
        n = 1 << 18
        ca = _vectors(g, n, -3, 3)
        orth = np.cross(ca.astype(np.float64), _vectors(g, n, -3, 3).astype(np.float64)).astype(np.float32)
        par = (ca.astype(np.float64) * g.uniform(-4, 4, (n, 1))).astype(np.float32)
        cb = np.where((np.arange(n) % 2 == 0)[:, None], orth, par)
        return _finish(name, [np.concatenate([f2u(a), f2u(b)], axis=1), np.concatenate([f2u(ca), f2u(cb)], axis=1)], 6)
    return build


def _rows_dop1():
    g = _rng("dop1")
    rand = np.stack([f2u(_scaled(g, N_RANDOM, -10, 10)) for _ in range(4)], axis=1)
    n = 1 << 18
    a, b = _scaled(g, n, -10, 10), _scaled(g, n, -10, 10)
    # a * b - c * d with c * d within a few ulps of a * b
    c = u2f(f2u(a) + g.integers(0, 3, n, dtype=np.uint64).astype(np.uint32))
    d = u2f(f2u(b) - g.integers(0, 3, n, dtype=np.uint64).astype(np.uint32))
    return _finish("dop1", [rand, np.stack([f2u(a), f2u(b), f2u(c), f2u(d)], axis=1)], 4)


# ------------------------------------------------------------------ c. RSQRTSS
def _rows_rsqrt(name):
    def build():
        g = _rng("rsqrt")  # all four forms run the same rows
        pos = g.integers(0x00800000, F32_MAX + 1, N_RANDOM, dtype=np.uint64).astype(np.uint32)
        return _finish(name, [standard_set("rsqrt", FRINGES["rsqrt"]), pos], 1)
    return build


# ------------------------------------------------------------------ d. shading leaf functions
ETA_PAIRS = [(1.0, 1.5), (1.5, 1.0), (1.0, 0.7), (1.0, 0.8), (1.0, 1.0)]
ALPHAS = [1e-3, 0.01, 0.25, 1.0]  # 1e-3: the parser's clamp


def _rows_fresnel():
    g = _rng("fresnel")
    n = 1 << 17
    edge = u2f(np.array([0x00000000, 0x80000000, 0x3f800000, 0xbf800000, 0x3f7fffff, 0xbf7fffff, 0x3f800001,
                         0xbf800001, 0x40000000, 0xc0000000, 0x00000001, 0x80000001, 0x00800000, 0x33800000,
                         0xb3800000, 0x3f000000, 0xbf000000], dtype=np.uint32))
    parts = []
    for ei, et in ETA_PAIRS:
        # cosines where sin_t crosses 1 (total internal reflection) for this pair, either orientation
        crit = []
        for a, b in ((ei, et), (et, ei)):
            if a > b:
                cc = np.float32(np.sqrt(1.0 - (b / a) ** 2))
                crit.append(u2f(f2u([cc])[0] + np.arange(-32, 33).astype(np.uint32)))
        crit = np.concatenate(crit + [np.zeros(0, np.float32)])
        ci = np.concatenate([g.uniform(-1.0, 1.0, n).astype(np.float32), edge, crit, -crit])
        parts.append(np.stack([f2u(ci), np.full(ci.size, f2u([ei])[0]), np.full(ci.size, f2u([et])[0])], axis=1))
    return _finish("fresnel", parts, 3)


def _rows_erfinv():
    # (-1, 1), both ends, and the fringes of its branch point
    g = _rng("erfinv")
    uni = g.uniform(-1.0, 1.0, 1 << 18).astype(np.float32)
    uni = uni[np.abs(uni) < 1.0]
    bits = g.integers(0, 0x3f800000, 1 << 18, dtype=np.uint64).astype(np.uint32)   # uniform in the bits of [0, 1)
    bits |= (g.integers(0, 2, bits.size, dtype=np.uint64).astype(np.uint32) << np.uint32(31))
    ends = np.array([0x3f7fffff, 0xbf7fffff, 0x3f800000, 0xbf800000, 0, 0x80000000, 1, 0x80000001], dtype=np.uint32)
    top = np.arange(0x3f800000 - 64, 0x3f800000, dtype=np.uint32)
    return _finish("erfinv", [f2u(uni), bits, ends, top, top | np.uint32(0x80000000), _fringe(FRINGES["erfinv"], 64)], 1)


def _neighbours(x, r=2) -> np.ndarray:
    return u2f(f2u([np.float32(x)])[0] + np.arange(-r, r + 1).astype(np.uint32))


def _beck11_columns(g, n):
    cos_sp = np.concatenate([[0.0, 1.0, 0.5, 1e-3], _neighbours(.9999), u2f([0x3f7fffff, 0x00000001, 0x00800000])]).astype(np.float32)
    u_sp = np.concatenate([[0.0, 0.5, 1.0 - 2.0 ** -24], _neighbours(1e-6)]).astype(np.float32)
    cti = g.uniform(0.0, 1.0, n).astype(np.float32)
    # a third of the cosines near 1 (the branch at .9999f and the steep end)
    cti = np.where(g.integers(0, 3, n) == 0, (1.0 - g.uniform(0, 4e-4, n)).astype(np.float32), cti)
    U1 = np.minimum(g.uniform(0.0, 1.0, n).astype(np.float32), np.float32(1.0 - 2.0 ** -24))
    U2 = np.minimum(g.uniform(0.0, 1.0, n).astype(np.float32), np.float32(1.0 - 2.0 ** -24))
    pick = lambda col, sp: np.where(g.integers(0, 8, n) == 0, sp[g.integers(0, sp.size, n)], col)  # noqa: E731
    # cos_theta_i = 0 and the smallest denormal give the reference a NaN (tan = inf): they stay in the
    # cross product of the edge values below and out of the random picks, for the NaN cap
    cti, U1, U2 = pick(cti, cos_sp[cos_sp > np.float32(1e-40)]), pick(U1, u_sp), pick(U2, u_sp)
    a, b, c = np.meshgrid(cos_sp, u_sp, u_sp, indexing="ij")
    return (np.concatenate([a.ravel(), cti]).astype(np.float32), np.concatenate([b.ravel(), U1]).astype(np.float32),
            np.concatenate([c.ravel(), U2]).astype(np.float32))


def _rows_beck11():
    cti, U1, U2 = _beck11_columns(_rng("beck11"), 1 << 18)
    return _finish("beck11", [np.stack([f2u(cti), f2u(U1), f2u(U2)], axis=1)], 3)


def _unit_vectors(g, n) -> np.ndarray:
    v = g.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _rows_beck11_pre():
    # the beck11 rows as wo = (sin, cos, 0) with alpha 1, and random directions (both hemispheres)
    # under the roughness set, isotropic and not
    g = _rng("beck11")
    cti, U1, U2 = _beck11_columns(g, 1 << 18)
    s = np.sqrt(np.maximum(0.0, 1.0 - cti.astype(np.float64) ** 2)).astype(np.float32)
    one = np.ones_like(cti)
    same = np.stack([f2u(s), f2u(cti), f2u(np.zeros_like(cti)), f2u(one), f2u(one), f2u(U1), f2u(U2)], axis=1)
    g = _rng("beck11_pre")
    n = 1 << 17
    wo = _unit_vectors(g, n)
    al = np.array(ALPHAS, dtype=np.float32)
    ax = al[g.integers(0, al.size, n)]
    ay = np.where(g.integers(0, 2, n) == 0, ax, al[g.integers(0, al.size, n)])
    _, V1, V2 = _beck11_columns(g, n)
    rnd = np.stack([f2u(wo[:, 0]), f2u(wo[:, 1]), f2u(wo[:, 2]), f2u(ax), f2u(ay), f2u(V1[-n:]), f2u(V2[-n:])], axis=1)
    return _finish("beck11_pre", [same, rnd], 7)


U_TOP = np.float32(1.0 - 2.0 ** -24)
U_SPECIALS = np.array([0.0, 2.0 ** -24, 0.25, 0.5, 0.75, U_TOP, 0.5 - 2.0 ** -25, 0.5 + 2.0 ** -24, 1e-6], dtype=np.float32)


def _u2_rows(name):
    def build():
        g = _rng("u2")  # the four sampling maps run the same rows
        top, sp = U_TOP, U_SPECIALS
        a, b = np.meshgrid(sp, sp, indexing="ij")
        n = 1 << 16
        u = np.minimum(g.uniform(0, 1, (N_RANDOM, 2)).astype(np.float32), top)
        t = np.minimum(g.uniform(0, 1, n).astype(np.float32), top)
        half = np.full(n, 0.5, np.float32)
        parts = [np.stack([a.ravel(), b.ravel()], axis=1), u,
                 np.stack([t, t], axis=1), np.stack([t, np.minimum(np.float32(1.0) - t, top)], axis=1),  # |a| = |b|
                 np.stack([t, half], axis=1), np.stack([half, t], axis=1)]                                # the axes
        return _finish(name, [f2u(p) for p in parts], 2)
    return build


def _rows_onb():
    g = _rng("onb_of_unit")
    v = _unit_vectors(g, N_RANDOM)
    n = 1 << 15
    th = g.uniform(0, 2 * np.pi, n)
    eq = np.stack([np.cos(th), np.sin(th), np.zeros(n)], axis=1).astype(np.float32)     # z = +0 and -0: the branch
    eqn = eq.copy()
    eqn[:, 2] = -0.0
    z = 1.0 - np.exp2(g.uniform(-24, -2, n))                                             # near the poles
    r = np.sqrt(1 - z * z)
    cap = np.stack([r * np.cos(th), r * np.sin(th), z], axis=1).astype(np.float32)
    poles = np.array([[0, 0, 1], [0, 0, -1], [0, 1, 0], [0, -1, 0], [1, 0, 0], [-1, 0, 0], [0, 1, -0.0], [1, 0, -0.0]],
                     dtype=np.float32)
    return _finish("onb_of_unit", [f2u(v), f2u(eq), f2u(eqn), f2u(cap), f2u(cap * np.float32(-1)), f2u(poles)], 3)


def _shading_dirs(g, n) -> np.ndarray:
    """Unit directions with |w.y| from 1 down to 1e-6, in both hemispheres."""
    y = np.exp(g.uniform(np.log(1e-6), 0.0, n)) * np.where(g.integers(0, 2, n) == 1, -1.0, 1.0)
    y = np.where(g.integers(0, 4, n) == 0, g.uniform(-1, 1, n), y)
    th = g.uniform(0, 2 * np.pi, n)
    r = np.sqrt(np.maximum(0.0, 1 - y * y))
    return np.stack([r * np.cos(th), y, r * np.sin(th)], axis=1).astype(np.float32)


def _alpha_columns(g, n):
    al = np.array(ALPHAS, dtype=np.float32)
    ax = al[g.integers(0, al.size, n)]
    ay = np.where(g.integers(0, 2, n) == 0, ax, al[g.integers(0, al.size, n)])
    return ax, ay


DIR_SPECIALS = np.array([[0, 1, 0], [0, -1, 0], [1, 0, 0], [0, 0, 1], [1, -0.0, 0], [0.6, 0.8, 0], [0, 0.8, 0.6],
                         [0.6, 1e-6, 0.8], [0.6, -1e-6, 0.8], [0.6, 1e-38, 0.8]], dtype=np.float32)


def _rows_beck_w(name):
    def build():
        g = _rng("beck_w")  # beck_D and beck_lambda run the same rows
        n = 1 << 18
        ax, ay = _alpha_columns(g, n)
        w = _shading_dirs(g, n)
        rnd = np.concatenate([f2u(ax)[:, None], f2u(ay)[:, None], f2u(w)], axis=1)
        # both sides of a = 1 / (alpha |tan theta|) = 1.6 (beck_lambda's limit), isotropic alphas
        m = 1 << 16
        al = np.array(ALPHAS, dtype=np.float64)[g.integers(0, len(ALPHAS), m)]
        tan = 1.0 / (1.6 * al) * (1.0 + g.uniform(-1e-5, 1e-5, m))
        y = 1.0 / np.sqrt(1 + tan * tan)
        th = g.uniform(0, 2 * np.pi, m)
        r = np.sqrt(np.maximum(0.0, 1 - y * y))
        wl = np.stack([r * np.cos(th), y, r * np.sin(th)], axis=1).astype(np.float32)
        lim = np.concatenate([f2u(al.astype(np.float32))[:, None], f2u(al.astype(np.float32))[:, None], f2u(wl)], axis=1)
        sp = [np.concatenate([f2u(np.full((len(DIR_SPECIALS), 2), a, np.float32)), f2u(DIR_SPECIALS)], axis=1) for a in ALPHAS]
        return _finish(name, [rnd, lim] + sp, 5)
    return build


def _dir_pairs(g, n):
    wo, wi = _shading_dirs(g, n), _shading_dirs(g, n)
    k = np.arange(n) % 64
    wi = np.where((k == 0)[:, None], -wo, wi)                      # wi = -wo: a zero half vector
    # (a grazing wo.y = 0 makes beck_pdf 0 / 0 in the reference: rare enough for the NaN cap)
    wo = np.where((np.arange(n) % 512 == 1)[:, None], DIR_SPECIALS[g.integers(0, len(DIR_SPECIALS), n)], wo)
    wi = np.where((k == 2)[:, None], DIR_SPECIALS[g.integers(0, len(DIR_SPECIALS), n)], wi)
    wi = np.where((k == 3)[:, None], wo, wi)                       # wi = wo
    return wo.astype(np.float32), wi.astype(np.float32)


def _rows_wo_w(name, with_ior):
    def build():
        g = _rng("wo_w")  # beck_pdf, mf_pdf and mf_eval run the same directions
        n = 1 << 18
        ax, ay = _alpha_columns(g, n)
        wo, wi = _dir_pairs(g, n)
        cols = [f2u(ax)[:, None], f2u(ay)[:, None]]
        if with_ior:
            ior = np.array([1.5, 1.33, 2.4, 1.0], dtype=np.float32)[g.integers(0, 4, n)]
            cols.append(f2u(ior)[:, None])
        if name == "beck_pdf":  # second direction: a half vector (unit)
            h = wo.astype(np.float64) + wi.astype(np.float64)
            ln = np.linalg.norm(h, axis=1, keepdims=True)
            wi = np.where(ln > 0, h / np.where(ln > 0, ln, 1.0), wi).astype(np.float32)
        return _finish(name, [np.concatenate(cols + [f2u(wo), f2u(wi)], axis=1)], 9 if with_ior else 8)
    return build


def _rows_spherical_phi():
    g = _rng("spherical_phi")
    v = _unit_vectors(g, N_RANDOM)
    ax = np.array([[1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, -1], [0, 1, 0], [1, 0, -0.0], [-1, 0, -0.0], [-1, 0, 0.0],
                   [-0.0, 0, 1], [0.0, 1, 0.0], [-0.0, 1, -0.0], [-0.0, 1, 0.0], [1e-30, 0, -1e-30], [-1, 0, -1e-45]],
                  dtype=np.float32)
    n = 1 << 12
    th = g.uniform(-np.pi, np.pi, n)
    ring = np.stack([np.cos(th), np.zeros(n), np.sin(th)], axis=1).astype(np.float32)
    return _finish("spherical_phi", [f2u(v), f2u(ax), f2u(ring)], 3)


def _rows_ray_offset():
    g = _rng("ray_offset")
    nrm, d = _unit_vectors(g, N_RANDOM), _unit_vectors(g, N_RANDOM)
    n = 1 << 15
    a = _unit_vectors(g, n)
    orth = np.cross(a.astype(np.float64), _unit_vectors(g, n).astype(np.float64))
    orth = (orth / np.linalg.norm(orth, axis=1, keepdims=True)).astype(np.float32)   # grazing: dot near 0
    ex = np.array([[0, 1, 0, 1, 0, 0], [0, 1, 0, 0, 1, 0], [0, 1, 0, 0, -1, 0], [0, 1, 0, 1, 1e-40, 0],
                   [0, 1, 0, 1, -1e-38, 0], [1, 0, 0, 0, 0, 1], [0, 1, 0, 1, 1e-30, 0]], dtype=np.float32)  # dot == 0, tiny
    return _finish("ray_offset", [np.concatenate([f2u(nrm), f2u(d)], axis=1), np.concatenate([f2u(a), f2u(orth)], axis=1),
                                  f2u(ex)], 6)


# ------------------------------------------------------------------ e. hit tests
TMIN, TMAX = np.float32(1e-3), np.float32(3.40282347e38)


def _with_exact_limits(name, rows, t_word, tmin_word, limit=1 << 13):
    """Rows whose t equals tmin, and tmax, exactly: the reference's own t of the first `limit` hits is
    written back as the row's tmin, and as its tmax (inputs only: the expectation is computed anew)."""
    out = oracle_unit("glibc", name, rows)
    hit = np.flatnonzero(out[:, 0] == 1)[:limit]
    lo, hi = rows[hit].copy(), rows[hit].copy()
    lo[:, tmin_word] = out[hit, t_word]
    hi[:, tmin_word + 1] = out[hit, t_word]
    return [rows, lo, hi]


def _rows_tri_hit():
    g = _rng("tri_hit")
    n = 1 << 17

    def rays_to(target, m):
        o = (target.astype(np.float64) + _unit_vectors(g, m) * g.uniform(0.5, 20, (m, 1))).astype(np.float32)
        return o, target.astype(np.float32) - o  # float subtraction: the ray passes the target as closely as floats allow

    def pack(p0, p1, p2, o, d):
        m = p0.shape[0]
        lim = np.tile(np.array([TMIN, TMAX], dtype=np.float32), (m, 1))
        return f2u(np.concatenate([p0, p1, p2, o, d, lim], axis=1).astype(np.float32))

    p0, p1, p2 = (g.uniform(-1, 1, (n, 3)).astype(np.float32) for _ in range(3))
    bc = g.dirichlet([1, 1, 1], n)
    inside = (bc[:, :1] * p0 + bc[:, 1:2] * p1 + bc[:, 2:] * p2)
    o, d = rays_to(inside, n)
    miss = g.integers(0, 4, n) == 0
    d = np.where(miss[:, None], _unit_vectors(g, n), d)
    parts = [pack(p0, p1, p2, o, d)]
    m = 1 << 14
    q0, q1, q2, q3 = (g.uniform(-1, 1, (m, 3)).astype(np.float32) for _ in range(4))
    o, d = rays_to(q0, m)
    parts += [pack(q0, q1, q2, o, d), pack(q1, q0, q2, o, d), pack(q2, q1, q0, o, d)]      # at a vertex, in each slot
    s = g.uniform(0, 1, (m, 1))
    o, d = rays_to(q0 + s * (q1.astype(np.float64) - q0), m)
    parts += [pack(q0, q1, q2, o, d), pack(q1, q0, q3, o, d)]                               # an edge two triangles share
    inpl = q0 + g.uniform(-2, 2, (m, 1)) * (q1.astype(np.float64) - q0) + g.uniform(-2, 2, (m, 1)) * (q2.astype(np.float64) - q0)
    parts += [pack(q0, q1, q2, inpl.astype(np.float32), q1 - q0)]                           # along the plane: denom 0 or tiny
    zeros = np.zeros((m, 3), np.float32)
    ex, ey = np.tile(np.float32([1, 0, 0]), (m, 1)), np.tile(np.float32([0, 1, 0]), (m, 1))
    oz = np.concatenate([g.uniform(-1, 2, (m, 2)), np.ones((m, 1))], axis=1).astype(np.float32)
    parts += [pack(zeros, ex, ey, oz, ex), pack(zeros, ex, ey, oz * np.float32([1, 1, 0]), ey)]  # exactly in / parallel to the plane
    o, d = rays_to(q0, m)
    parts += [pack(q0, q1, q1, o, d), pack(q0, q0, q0, o, d),
              pack(q0, q1, (q0 + np.float32(0.5) * (q1 - q0)).astype(np.float32), o, d)]    # degenerate triangles
    return _finish("tri_hit", _with_exact_limits("tri_hit", np.concatenate(parts), 1, 15), 17)


def _affines(g, n, kind):
    """world_to_object rows (vx, vy, vz, p): kind 0 identity, 1 uniform scale + translation, 2 a rotation
    with per-axis scales + translation."""
    eye = np.tile(np.eye(3), (n, 1, 1))
    if kind == 0:
        m, p = eye, np.zeros((n, 3))
    elif kind == 1:
        m, p = eye * np.exp2(g.uniform(-4, 4, (n, 1, 1))), g.uniform(-3, 3, (n, 3))
    else:
        q, _ = np.linalg.qr(g.normal(size=(n, 3, 3)))
        m, p = q * np.exp2(g.uniform(-3, 3, (n, 1, 3))), g.uniform(-3, 3, (n, 3))
    return np.concatenate([m.reshape(n, 9), p], axis=1).astype(np.float32)


def _obj_to_world(aff, pts, vec=False):
    """Points (or vectors) given in object space, mapped to world space through the inverse of the
    world_to_object rows (float64; the tests only need them near where they aim)."""
    n = aff.shape[0]
    m = aff[:, :9].astype(np.float64).reshape(n, 3, 3)  # rows vx, vy, vz: x' = p.x vx + p.y vy + p.z vz + p
    inv = np.linalg.inv(np.transpose(m, (0, 2, 1)))
    rhs = pts if vec else pts - aff[:, 9:].astype(np.float64)
    return np.einsum("nij,nj->ni", inv, rhs)


def _rows_sphere_t():
    g = _rng("sphere_t")
    n = 1 << 16
    parts = []
    lim = np.tile(np.array([TMIN, TMAX], dtype=np.float32), (n, 1))
    for kind in (0, 1, 2):
        aff = _affines(g, n, kind)
        dirs = _unit_vectors(g, n).astype(np.float64)
        perp = np.cross(dirs, _unit_vectors(g, n))
        perp /= np.linalg.norm(perp, axis=1, keepdims=True)
        # impact parameter: a third random, a third grazing (1 -+ 2^-4 .. 2^-26: disc near 0, both signs), a third inside
        sel = g.integers(0, 3, n)
        graze = 1.0 + np.exp2(g.uniform(-26, -4, n)) * np.where(g.integers(0, 2, n) == 1, -1.0, 1.0)
        b = np.where(sel == 0, g.uniform(0, 1.5, n), graze)
        back = np.where(sel == 2, g.uniform(0, 0.9, n), g.uniform(1.5, 30, n))     # origin inside the sphere
        b = np.where(sel == 2, g.uniform(0, 0.4, n), b)
        o_obj = perp * b[:, None] - dirs * back[:, None]
        o = _obj_to_world(aff, o_obj).astype(np.float32)
        d = _obj_to_world(aff, dirs, vec=True).astype(np.float32)
        parts.append(f2u(np.concatenate([aff, o, d, lim], axis=1)))
    return _finish("sphere_t", _with_exact_limits("sphere_t", np.concatenate(parts), 1, 18), 20)


def _rows_plane_t():
    g = _rng("plane_t")
    n = 1 << 16
    parts = []
    lim = np.tile(np.array([TMIN, TMAX], dtype=np.float32), (n, 1))
    for kind in (0, 1, 2):
        aff = _affines(g, n, kind)
        o = g.uniform(-5, 5, (n, 3)).astype(np.float32)
        d = _unit_vectors(g, n)
        if kind < 2:  # axis-aligned transforms: d.y = +0 and -0 survive them
            k = np.arange(n) % 8
            d[:, 1] = np.where(k == 0, np.float32(0.0), np.where(k == 1, np.float32(-0.0), d[:, 1]))
            o[:, 1] = np.where(k == 2, np.float32(0.0), o[:, 1])     # origin in the plane
        parts.append(f2u(np.concatenate([aff, o, d, lim], axis=1)))
    return _finish("plane_t", _with_exact_limits("plane_t", np.concatenate(parts), 1, 18), 20)


def _rows_box_hit():
    g = _rng("box_hit")
    n = 1 << 18
    c, h = g.uniform(-2, 2, (n, 3)), np.exp2(g.uniform(-6, 1, (n, 3)))
    k = np.arange(n) % 16
    h = np.where((k == 0)[:, None] & (np.arange(3) == (np.arange(n) // 16 % 3)[:, None]), 0.0, h)   # flat boxes
    lo, hi = (c - h).astype(np.float32), (c + h).astype(np.float32)
    o = g.uniform(-4, 4, (n, 3)).astype(np.float32)
    aim = (c + g.uniform(-1.2, 1.2, (n, 3)) * h)
    d = (aim - o).astype(np.float32)
    d = np.where((g.integers(0, 4, n) == 0)[:, None], _unit_vectors(g, n), d)
    axis = np.arange(3) == g.integers(0, 3, n)[:, None]
    zero = np.where(g.integers(0, 2, n) == 1, np.float32(-0.0), np.float32(0.0))[:, None]
    d = np.where(axis & ((k >= 1) & (k <= 4))[:, None], zero, d)                 # a zero component: inv = +-inf
    face = np.where(g.integers(0, 2, n)[:, None] == 1, lo, hi)
    o = np.where(axis & ((k >= 3) & (k <= 6))[:, None], face, o)                 # origin on a face (0 x inf with k 3, 4)
    tmin = np.where(k == 7, g.uniform(0, 4, n), 1e-3).astype(np.float32)
    tmax = np.where(k == 8, g.uniform(0, 4, n), TMAX).astype(np.float32)
    return _finish("box_hit", [f2u(np.concatenate([lo, hi, o, d, tmin[:, None], tmax[:, None]], axis=1).astype(np.float32))], 14)


# ------------------------------------------------------------------ f. the pixel stream
# Row: seed, seeding (0 rng_seed, 1 rng_seed_twisted), STREAM_STEPS steps of op | prepare << 4 | n << 8.
# Output: the number of values drawn, the values (next1D floats), zeros up to STREAM_OUT words.
MT_N = 312
RNG_MARGIN = 96                      # sp_path.hpp SP_RNG_MARGIN: rng_prepare twists ahead this close to the end
STREAM_STEPS, STREAM_OUT = 200, 2048
STREAM_LANES = 3 * 256               # three blocks of four full waves
STREAM_WORDS = 2000                  # words a script consumes at least: more than six generations
OP_NOP, OP_DRAW, OP_RAW2, OP_SKIP, OP_RESERVE_DRAW, OP_RESERVE_SKIP = range(6)
SKIP_COUNTS = (0, 1, 311, 312, 313)


def step_words(op: int, n: int):
    """Words of the stream one step consumes, and how many of them it draws (writes out)."""
    return {OP_NOP: (0, 0), OP_DRAW: (n, n), OP_RAW2: (2, 2), OP_SKIP: (n, 0), OP_RESERVE_DRAW: (n, n),
            OP_RESERVE_SKIP: (n, 0)}[op]


def _lane_script(g, lane: int):
    """One lane's operations [(op, n)]: random steps toward each 312-word boundary, one of nine
    boundary scenarios at it, in an order of the lane's own."""
    ops, p = [], 0

    def add(op, n=0):
        nonlocal p
        ops.append((op, int(n)))
        p += step_words(op, int(n))[0]

    order = list(g.permutation(9))
    gen = 0
    while p < STREAM_WORDS and len(ops) < STREAM_STEPS - 40:
        bound = (p // MT_N + 1) * MT_N
        while bound - p > 60:  # random steps that stay at least 24 words short of the boundary
            room = bound - p - 24
            r = int(g.integers(0, 6))
            if r == 0:
                add(OP_DRAW, g.integers(1, min(24, room) + 1))
            elif r == 1:
                add(OP_RAW2)
            elif r == 2:
                add(OP_SKIP, g.integers(0, min(90, room) + 1))
            elif r == 3:
                add(OP_RESERVE_DRAW, g.integers(1, min(32, room) + 1))
            elif r == 4:
                add(OP_RESERVE_SKIP, g.integers(1, min(32, room) + 1))
            else:
                add(OP_NOP)
        d = bound - p  # 24 .. 60 words to the boundary
        scen = order[gen % 9]
        gen += 1
        a, e = int(g.integers(1, 17)), int(g.integers(1, 17))
        if scen == 0:    # draws at buffer index 311, then 312 (the switch: word 0), then 1
            add(OP_DRAW, d), add(OP_DRAW, 1), add(OP_DRAW, 1)
        elif scen == 1:  # rng_raw2 straddling the boundary
            add(OP_SKIP, d - 1), add(OP_RAW2)
        elif scen == 2:  # rng_reserve spanning it, then the reserved draws
            add(OP_SKIP, d - a), add(OP_RESERVE_DRAW, a + e)
        elif scen == 3:  # rng_reserve + rng_skip_reserved spanning it
            add(OP_SKIP, d - a), add(OP_RESERVE_SKIP, a + e), add(OP_DRAW, 3)
        elif scen == 4:  # rng_skip of 0, 1, 311, 312, 313 from the middle of a generation
            add(OP_SKIP, SKIP_COUNTS[lane % 5]), add(OP_DRAW, 2)
        elif scen == 5:  # one run of draws across the boundary: the draw-ahead window emptied by the switch
            add(OP_DRAW, d + 3)
        elif scen == 6:  # skipped exactly to the boundary, then rng_raw2 there
            add(OP_SKIP, d), add(OP_RAW2)
        elif scen == 7:  # the last word skipped, a draw at the switch
            add(OP_DRAW, d - 1), add(OP_SKIP, 1), add(OP_DRAW, 1)
        else:            # rng_skip of 0, 1, 311, 312, 313 from the boundary itself
            add(OP_SKIP, d), add(OP_SKIP, SKIP_COUNTS[(lane // 5) % 5]), add(OP_DRAW, 2)
    assert len(ops) <= STREAM_STEPS and p >= STREAM_WORDS, (lane, len(ops), p)
    return ops + [(OP_NOP, 0)] * (STREAM_STEPS - len(ops))


def stream_seed(row: int) -> int:
    x, y = 3 + row % 61, 5 + row // 61  # pixel coordinates, as the renderer seeds a pixel's stream
    return (((x << 16) | y) ^ 0xB0AE9D99) & 0xffffffff


def _rows_stream():
    g = _rng("stream")
    r = np.zeros((STREAM_LANES, 2 + STREAM_STEPS), dtype=np.uint32)
    for row in range(STREAM_LANES):
        r[row, 0] = stream_seed(row)
        r[row, 1] = row & 1  # half the lanes rng_seed, half rng_seed_twisted, side by side in every wave
        r[row, 2:] = [op | (n << 8) for op, n in _lane_script(g, row)]
    # rng_prepare before a step, for all 64 lanes of a wave at once (it is a wave-synchronous call)
    prep = g.integers(0, 5, (STREAM_LANES // 64, STREAM_STEPS)) == 0
    r[:, 2:] |= np.repeat(prep, 64, axis=0).astype(np.uint32) << np.uint32(4)
    return r


def stream_positions(row_words) -> list:
    """Stream positions (0 = the first word after seeding) of the values one row's script draws."""
    pos, p = [], 0
    for step in row_words[2:]:
        used, drawn = step_words(int(step) & 15, int(step) >> 8)
        pos += range(p, p + drawn)
        p += used
    return pos


def stream_expected(variant: str, r: np.ndarray) -> np.ndarray:
    """Every drawn value is a position of orc_mt_stream(seed, N) (pinned to libstdc++ by
    tests/golden/sampler_golden.npy): no other reference code."""
    from tests import _oracle
    L = _oracle.load(variant)
    out = np.zeros((r.shape[0], STREAM_OUT), dtype=np.uint32)
    for i, row in enumerate(r):
        pos = stream_positions(row)
        assert 0 < len(pos) < STREAM_OUT
        s = np.zeros(pos[-1] + 1, dtype=np.float32)
        L.orc_mt_stream(int(row[0]), s.size, s.ctypes.data_as(C.POINTER(C.c_float)))
        out[i, 0] = len(pos)
        out[i, 1:1 + len(pos)] = s.view(np.uint32)[pos]
    return out


# ------------------------------------------------------------------ g. the stream-fed layer
# Rows that draw: seed, skip, a material record (ROW_MAT words), then directions.  Output: the
# function's words, the number of stream words it consumed, one further next1D.
#   material record  kind, albedo3, microfacet_r3, alpha_x, alpha_y, ior, sample_visible_area,
#                    coat_ior, coat_color3, base record (kind .. sample_visible_area, 11 words)
#   rho16 (and rho16_served)             + local wo -> rgb
#   glossy_weights (and weights_served)  + local wo -> w0, w1
#   mf_sample, mf_sample_pre             + local wo -> colour3, dir3, pdf, props
#   material_sample  + n, wo -> colour3, dir3, pdf, props     (world form)
#   material_eval    + n, wo, wi -> rgb       material_pdf  + n, wo, wi -> pdf
# Lights (no draws): a light record (ROW_LIGHT words: kind, radiance3, object_to_world 12,
# world_to_object 12, normal_to_world 9), the observer, then
#   sphere_pdf  -> pdf      light_pdf  + wi -> pdf
#   light_sample  + the observer's normal, u2 -> L3, pdf, direction3, tmin, tmax
# sample_visible_area is 1 in every row: the scene parser sets nothing else (sp_scene.cpp blank_material).
ROW_MAT, ROW_LIGHT = 26, 37
N_DRAW = 1 << 16
IORS = [1.5, 1.33, 2.4, 1.0, 0.7]
COAT_IORS = [1.5, 1.0, 0.8]
MAT_LAMBERTIAN, MAT_GLOSSY, MAT_CLEARCOAT = 0, 1, 2
LIGHT_SPHERE, LIGHT_ENVIRONMENT = 0, 1
SPHERE_PDF_SWITCH = 1.0 / 0.00068523     # sphere_pdf's small-angle form below sin^2 = 0.00068523: squared distance above this
ONE_ULP = np.nextafter(np.float32(1), np.float32(2))


def _skips(g, n) -> np.ndarray:
    """Stream positions: anywhere in the first two generations (even and odd); every start from
    312 - 33 to 312 + 1, so the 32 words of an estimate straddle the boundary in every way at both
    parities; exactly 0 and 311; the same around the second boundary."""
    c = np.arange(n) % 8
    s = g.integers(0, 2 * MT_N + 80, n)
    s = np.where(c == 0, g.integers(MT_N - 33, MT_N + 2, n), s)
    s = np.where(c == 1, g.integers(2 * MT_N - 33, 2 * MT_N + 2, n), s)
    s = np.where(c == 2, np.where(g.integers(0, 2, n) == 0, 0, MT_N - 1), s)
    s = np.where(c == 3, g.integers(MT_N - 3, MT_N + 1, n), s)     # 309 .. 312: the coat's draw, a sample's pair at the boundary
    return s.astype(np.uint32)


def _records(g, n, kinds) -> np.ndarray:
    """n material records without a coat (11 words): float columns as bits."""
    kind = np.asarray(kinds)[g.integers(0, len(kinds), n)]
    i = np.arange(n)
    # albedo classes: zero in 1 of 32 (with it the weights are rho / rho, a NaN whenever the estimate is
    # 0 or infinite, about one such row in 80: thinned for the NaN cap), above 1 in 1 of 8
    ac, rc = g.integers(0, 32, n), g.integers(0, 8, n)
    alb = g.uniform(0.02, 1.0, (n, 3)) / np.pi                     # ordinary (albedo / pi)
    alb = np.where(((ac >= 1) & (ac <= 4))[:, None], g.uniform(1.0, 4.0, (n, 3)), alb)   # above 1
    R = g.uniform(0.05, 1.0, (n, 3)).astype(np.float32)            # coloured: rc 5, 6, 7
    R[rc <= 1] = 1.0                                               # grey, the scene files' own
    R[rc == 2] = 0.5                                               # grey
    near = rc == 3                                                 # one channel an ulp off grey: no shortcut
    R[near] = 1.0
    R[near, i[near] % 3] = ONE_ULP
    R[rc == 4] = 0.0                                               # a black microfacet colour
    # a zero albedo; where the other lobe is black too (or there is none) `weights` divides 0 by 0:
    # those rows are thinned to 1 in 64 for the NaN cap
    lone = (kind == MAT_LAMBERTIAN) | (rc == 4)
    zero = (ac == 0) & (~lone | (i % 64 == 0))
    alb = np.where(zero[:, None], 0.0, alb)
    ax, ay = _alpha_columns(g, n)
    ior = np.array(IORS, dtype=np.float32)[g.integers(0, len(IORS), n)]
    return np.concatenate([kind.astype(np.uint32)[:, None], f2u(alb.astype(np.float32)), f2u(R), f2u(ax)[:, None],
                           f2u(ay)[:, None], f2u(ior)[:, None], np.ones((n, 1), np.uint32)], axis=1)


def _materials(g, n, kinds) -> np.ndarray:
    """n full records (ROW_MAT words).  A clearcoat's own lobes are unused (zero); its base is a
    Lambertian or a glossy record."""
    top = _records(g, n, [k for k in kinds if k != MAT_CLEARCOAT])
    base = _records(g, n, [MAT_LAMBERTIAN, MAT_GLOSSY])
    coat = (g.integers(0, 3, n) == 0) if MAT_CLEARCOAT in kinds else np.zeros(n, bool)
    top[coat, 0] = MAT_CLEARCOAT
    cior = np.array(COAT_IORS, dtype=np.float32)[g.integers(0, len(COAT_IORS), n)]
    ccol = np.where((g.integers(0, 2, n) == 0)[:, None], 1.0, g.uniform(0.1, 1.0, (n, 3))).astype(np.float32)
    return np.concatenate([top, f2u(cior)[:, None], f2u(ccol), base], axis=1)


def _local_wo(g, n) -> np.ndarray:
    """Local outgoing directions: _shading_dirs (both hemispheres), DIR_SPECIALS, wo.y = +0 and -0
    (nothing is drawn), |wo.y| down to 1e-38."""
    wo = _shading_dirs(g, n)
    k = np.arange(n) % 512   # the grazing classes give the reference infinities and NaNs: rare, for the NaN cap
    wo = np.where((k == 1)[:, None], DIR_SPECIALS[g.integers(0, len(DIR_SPECIALS), n)], wo)
    th = g.uniform(0, 2 * np.pi, n)
    ring = np.stack([np.cos(th), np.zeros(n), np.sin(th)], axis=1).astype(np.float32)
    ring[:, 1] = np.where(g.integers(0, 2, n) == 0, np.float32(0.0), np.float32(-0.0))
    wo = np.where((k % 256 == 2)[:, None], ring, wo)   # with a zero albedo on top, wo.y = 0 leaves `weights` 0 / 0
    tiny = ring.copy()
    tiny[:, 1] = (10.0 ** g.uniform(-38, -6, n) * np.where(g.integers(0, 2, n) == 0, 1.0, -1.0)).astype(np.float32)
    wo = np.where((k == 3)[:, None], tiny, wo)
    return wo.astype(np.float32)


def _local_pairs(g, n):
    """wo as _local_wo; wi: any direction, -wo, wo, a special, the hemisphere opposite to wo."""
    wo, wi = _local_wo(g, n), _shading_dirs(g, n)
    j = np.arange(n) % 64
    wi = np.where((j == 5)[:, None], -wo, wi)
    wi = np.where((j == 6)[:, None], wo, wi)
    wi = np.where((j == 7)[:, None], DIR_SPECIALS[g.integers(0, len(DIR_SPECIALS), n)], wi)
    opp = wi.copy()
    opp[:, 1] = -np.copysign(np.abs(wi[:, 1]), wo[:, 1])
    wi = np.where(((j >= 8) & (j < 12))[:, None], opp, wi)
    return wo, wi.astype(np.float32)


def _to_world(g, n, *local):
    """A shading normal per row and the local directions in its frame.  Half the rows: n = (0, 1, 0),
    whose frame (onb_of_unit) is the exact permutation local = (-w.z, w.y, w.x), so every special
    value of the local directions survives; the others: a random normal of length 1, 0.37 or 3."""
    nrm = _unit_vectors(g, n).astype(np.float64)
    a = np.cross(nrm, _unit_vectors(g, n))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = np.cross(nrm, a)
    even = (g.integers(0, 2, n) == 0)[:, None]
    out = []
    for l in local:
        exact = np.stack([l[:, 2], l[:, 1], -l[:, 0]], axis=1)
        rot = (l[:, :1] * a + l[:, 1:2] * nrm + l[:, 2:] * b).astype(np.float32)
        out.append(np.where(even, exact, rot).astype(np.float32))
    length = np.array([1.0, 1.0, 0.37, 3.0])[g.integers(0, 4, n)][:, None]
    nw = np.where(even, np.float32([0, 1, 0]), (nrm * length).astype(np.float32)).astype(np.float32)
    return [nw] + out


def _draw_head(g, n, kinds):
    seed = g.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([seed[:, None], _skips(g, n)[:, None], _materials(g, n, kinds)], axis=1)


def _rows_local_draw():
    g = _rng("local_draw")  # rho16, glossy_weights, mf_sample and their other forms run the same rows
    n = N_DRAW
    return _finish("local_draw", [np.concatenate([_draw_head(g, n, [MAT_GLOSSY]), f2u(_local_wo(g, n))], axis=1)], 31)


def _rows_material(name):
    def build():
        g = _rng("material")  # material_sample, material_eval and material_pdf run the same records and directions
        n = N_DRAW
        head = _draw_head(g, n, [MAT_LAMBERTIAN, MAT_GLOSSY, MAT_CLEARCOAT])
        nw, wo, wi = _to_world(g, n, *_local_pairs(g, n))
        cols = [head, f2u(nw), f2u(wo)] + ([] if name == "material_sample" else [f2u(wi)])
        return _finish("material", [np.concatenate(cols, axis=1)], 34 if name == "material_sample" else 37)
    return build


# serve_rho (rrnee set): 64 consecutive rows are one wave, each row one lane's request:
#   seed, skip, material record, n, wo, flags -> served?, wA0, wA1, words of the bounce's site,
#   wE0, wE1, wP0, wP1, wS0, wS1, words of the light's three sites, one further next1D
# flags: 1 wants the light's eval / pdf / sample estimates, 2 wants the bounce's own sample's, 4 the lane
# is absent (it leaves before the call).  Wave classes, by wave index % 8:
#   0 every lane wants both (256 requests for 64 lanes: the deal loop runs four times)
#   1 one lane only        2 lanes 0 and 63 only       3 half the lanes absent, the others want at random
#   4 wants at random, nobody absent                   5 48 lanes absent, the 16 others want both (64 requests for 16)
#   6 every lane wants both, at positions whose estimates straddle the generation boundary
#   7 wants and absences at random
# In classes 0, 4 and 6 the lanes with lane % 16 == 5 have wo.y == 0 (dc 0: nothing drawn); a third of
# the owners are clearcoats.  Every material has a glossy lobe, as material_has_rho demands of an owner.
SERVE_WAVES = 512
WANT_B, WANT_A, ABSENT = 1, 2, 4


def _rows_serve_rho():
    g = _rng("serve_rho")
    n = SERVE_WAVES * 64
    mat = _materials(g, n, [MAT_GLOSSY, MAT_CLEARCOAT])
    mat[:, 15] = MAT_GLOSSY                                   # a coat's base: glossy
    nw, wo = _to_world(g, n, _local_wo(g, n))
    lane, wave = np.arange(n) % 64, np.arange(n) // 64
    cls = wave % 8
    rnd = g.integers(0, 4, n)
    flags = np.where(cls == 0, 3, rnd)
    one = g.integers(0, 64, SERVE_WAVES)[wave]
    flags = np.where(cls == 1, np.where(lane == one, 1 + 2 * (wave // 8 % 2), 0), flags)
    flags = np.where(cls == 2, np.where((lane == 0) | (lane == 63), 3, 0), flags)
    flags = np.where((cls == 3) & (g.integers(0, 2, n) == 0), ABSENT, flags)
    perm = np.argsort(g.random((SERVE_WAVES, 64)), axis=1).ravel()   # a random rank per lane of each wave
    flags = np.where(cls == 5, np.where(perm < 48, ABSENT, 3), flags)
    flags = np.where(cls == 6, 3, flags)
    flags = np.where((cls == 7) & (g.integers(0, 4, n) == 0), ABSENT, flags)
    skip = _skips(g, n)
    skip = np.where(cls == 6, g.integers(MT_N - 110, MT_N + 1, n), skip).astype(np.uint32)
    dc0 = np.isin(cls, (0, 4, 6)) & (lane % 16 == 5)
    th = g.uniform(0, 2 * np.pi, n)
    flat = np.stack([np.cos(th), np.where(g.integers(0, 2, n) == 0, 0.0, -0.0), np.sin(th)], axis=1).astype(np.float32)
    nw = np.where(dc0[:, None], np.float32([0, 1, 0]), nw)
    wo = np.where(dc0[:, None], flat, wo)
    ordinary = f2u(np.full(3, 0.2, np.float32))               # with nothing drawn a zero albedo leaves 0 / 0: not here
    mat[dc0, 1:4] = ordinary
    mat[dc0, 16:19] = ordinary
    seed = g.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    r = np.concatenate([seed[:, None], skip[:, None], mat, f2u(nw), f2u(wo), flags.astype(np.uint32)[:, None]], axis=1)
    return np.ascontiguousarray(r.astype(np.uint32))


def _light_records(g, n):
    """Light records and observers in the light's object space -> (records [n, 37], observers in world space).
    Transforms as _affines kinds 1 and 2, identity where the observer sits within 32 ulps of the sphere."""
    c = np.arange(n) % 8                                 # observer class
    tk = np.where(c == 2, 0, 1 + (np.arange(n) // 8) % 2)
    w2o = np.where((tk == 0)[:, None], _affines(g, n, 0), np.where((tk == 1)[:, None], _affines(g, n, 1), _affines(g, n, 2)))
    A = np.transpose(w2o[:, :9].astype(np.float64).reshape(n, 3, 3), (0, 2, 1))     # x' = A x + p
    Ai = np.linalg.inv(A)
    o2w = np.concatenate([np.transpose(Ai, (0, 2, 1)).reshape(n, 9), -np.einsum("nij,nj->ni", Ai, w2o[:, 9:].astype(np.float64))], axis=1)
    nrm = A.reshape(n, 9)                                # columns of inverse(o2w.linear) transposed = rows of A
    d = _unit_vectors(g, n).astype(np.float64)
    r = g.uniform(1.05, 30.0, n)                                                   # outside
    r = np.where(c == 1, g.uniform(0.0, 0.95, n), r)                               # inside
    sw = np.sqrt(SPHERE_PDF_SWITCH) * (1.0 + 10.0 ** g.uniform(-7, -2, n) * np.where(g.integers(0, 2, n) == 0, 1.0, -1.0))
    r = np.where((c == 3) | (c == 4), sw, r)                                       # both sides of the small-angle switch
    obj = d * r[:, None]
    obs = _obj_to_world(w2o, obj).astype(np.float32)
    # on the unit sphere (identity transform: object space is world space): the float32 unit vector
    # stretched in steps of 2^-24, so dot(o, o) takes the values within some ulps of 1 on both sides
    near = (_unit_vectors(g, n).astype(np.float64) * (1.0 + g.integers(-16, 17, n)[:, None] * 2.0 ** -24)).astype(np.float32)
    obs = np.where((c == 2)[:, None], near, obs)
    kind = np.where(np.arange(n) % 4 == 3, LIGHT_ENVIRONMENT, LIGHT_SPHERE).astype(np.uint32)
    rad = g.uniform(0.1, 50.0, (n, 3)).astype(np.float32)
    rad[np.arange(n) % 16 == 5] = 0.0                                              # black radiance
    rec = np.concatenate([kind[:, None], f2u(rad), f2u(o2w.astype(np.float32)), f2u(w2o), f2u(nrm.astype(np.float32))], axis=1)
    return rec, obs


def _rows_light(name):
    def build():
        g = _rng("light")  # sphere_pdf, light_sample and light_pdf run the same lights and observers
        n = N_DRAW
        rec, obs = _light_records(g, n)
        on = _unit_vectors(g, n)
        u = np.minimum(g.uniform(0, 1, (n, 2)).astype(np.float32), U_TOP)
        sp = U_SPECIALS[g.integers(0, U_SPECIALS.size, (n, 2))]
        u = np.where((np.arange(n) % 8 == 6)[:, None], sp, u)                      # the special values of _u2_rows, crossed
        wi = _unit_vectors(g, n)
        tail = {"sphere_pdf": [], "light_sample": [f2u(on), f2u(u)], "light_pdf": [f2u(wi)]}[name]
        return _finish("light", [np.concatenate([rec, f2u(obs)] + tail, axis=1)], ROW_LIGHT + 3 + sum(t.shape[1] for t in tail))
    return build


# ------------------------------------------------------------------ h. the image environment light
# env_sample  u2 -> L3, pdf, wi3      env_pdf  wi3 -> pdf      env_radiance  dir3 -> rgb
# against one of IMAGES; `<unit>_replay` is the same function without the guide tables.  A unit's
# name carries its image: env_sample@a16.  The evaluator gets the image as a file (image_words) and
# builds the tables with the upload's host builder; the oracle builds its own from the same pixels.
IMAGE_NAMES = ("a16", "b64", "zero16")
ENV_MAX_RADIANCE = np.float32(100.0)


def image(name: str) -> dict:
    """16 x 8 and 64 x 32 images of dim texels with a zero row, a zero column, one texel thousands of
    times brighter and one above max_radiance (b64: a block of zeros too, and a rotated, scaled light);
    zero16 is all zero."""
    g = _rng("image/" + name)
    w, h = {"a16": (16, 8), "b64": (64, 32), "zero16": (16, 8)}[name]
    px = g.uniform(0.005, 0.02, (h, w, 3)).astype(np.float32)
    l2w = np.eye(3)
    if name == "zero16":
        px[:] = 0
    else:
        px[h // 3, :, :] = 0
        px[:, w // 4, :] = 0
        px[1, 2] = (40, 50, 30)
        px[h - 2, w - 3] = (900, 200, 100)
    if name == "b64":
        px[10:14, 20:41] = 0
        q, _ = np.linalg.qr(g.normal(size=(3, 3)))
        l2w = q * np.array([1.0, 2.0, 0.5])
    l2w32 = l2w.astype(np.float32)
    w2l32 = np.linalg.inv(l2w32.astype(np.float64)).astype(np.float32)
    # sp_linear holds columns: vx, vy, vz
    return dict(w=w, h=h, pixels=np.ascontiguousarray(px), max_radiance=ENV_MAX_RADIANCE,
                l2w=np.ascontiguousarray(l2w32.T).ravel(), w2l=np.ascontiguousarray(w2l32.T).ravel())


def image_words(name: str) -> np.ndarray:
    im = image(name)
    return np.concatenate([np.array([im["w"], im["h"]], np.uint32), f2u([im["max_radiance"]]), f2u(im["l2w"]), f2u(im["w2l"]),
                           f2u(im["pixels"]).ravel()])


class _EnvImage(C.Structure):  # include/simplepath_hip.h sp_env_image
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("pixels", C.POINTER(C.c_float)), ("max_radiance", C.c_float),
                ("reserved", C.c_int32), ("light_to_world", C.c_float * 9), ("world_to_light", C.c_float * 9)]


def oracle_set_image(variant: str, name: str):
    from tests import _oracle
    L, im = _oracle.load(variant), image(name)
    d = _EnvImage(im["w"], im["h"], im["pixels"].ctypes.data_as(C.POINTER(C.c_float)), float(im["max_radiance"]), 0,
                  (C.c_float * 9)(*im["l2w"].tolist()), (C.c_float * 9)(*im["w2l"].tolist()))
    L.orc_unit_env.restype = C.c_int
    L.orc_unit_env.argtypes = [C.POINTER(_EnvImage)]
    assert L.orc_unit_env(C.byref(d)) == 0
    return L, im


def env_cdfs(name: str):
    """The oracle's own marginal [nv + 1] and conditional [nv, nu + 1] cdf tables of an image."""
    L, im = oracle_set_image("glibc", name)
    nu, nv = 2 * im["w"], 2 * im["h"]
    marg, cond = np.zeros(nv + 1, np.float32), np.zeros((nv, nu + 1), np.float32)
    L.orc_unit_env_cdf.restype = C.c_int
    L.orc_unit_env_cdf.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float)]
    assert L.orc_unit_env_cdf(marg.ctypes.data_as(C.POINTER(C.c_float)), cond.ctypes.data_as(C.POINTER(C.c_float))) == 0
    return marg, cond


def _around(vals) -> np.ndarray:
    """Each value of [0, 1) and its two neighbours, as floats kept inside [0, 1 - 2^-24]."""
    b = f2u(np.asarray(vals, np.float32)).astype(np.int64)
    b = np.concatenate([b - 1, b, b + 1])
    return u2f(np.clip(b, 0, int(f2u([U_TOP])[0])).astype(np.uint32))


def guide_bits(n: int) -> int:  # sp_envmap.cpp guide_bits
    b = 0
    while (1 << b) < n and b < 16:
        b += 1
    return b


def _rows_env_sample(img):
    def build():
        im = image(img)
        nu, nv = 2 * im["w"], 2 * im["h"]
        marg, cond = env_cdfs(img)
        g = _rng("env_sample/" + img)
        rnd = lambda n: np.minimum(g.uniform(0, 1, n).astype(np.float32), U_TOP)  # noqa: E731
        a, b = np.meshgrid(U_SPECIALS, U_SPECIALS, indexing="ij")                  # 0 and 1 - 2^-24 among them
        parts = [np.stack([rnd(1 << 14), rnd(1 << 14)], axis=1), np.stack([a.ravel(), b.ravel()], axis=1)]
        my = np.tile(_around(marg[:nv]), 4)                                        # u.y on the marginal's entries
        parts.append(np.stack([rnd(my.size), my], axis=1))
        for v in range(nv):  # u.y inside row v's interval, u.x on that row's entries
            lo, hi = (marg[v - 1] if v else np.float32(0)), marg[v]
            uy = np.float32((np.float64(lo) + np.float64(hi)) / 2)
            if lo <= uy < hi:
                ux = _around(cond[v, :nu])
                parts.append(np.stack([ux, np.full(ux.size, uy, np.float32)], axis=1))
        for bits in sorted({guide_bits(nu), guide_bits(nv)}):                      # the guides' bucket edges
            e = _around(np.arange(1 << bits, dtype=np.float64) / (1 << bits))
            parts += [np.stack([e, rnd(e.size)], axis=1), np.stack([rnd(e.size), e], axis=1), np.stack([e, e], axis=1)]
        return _finish("env_sample/" + img, [f2u(p.astype(np.float32)) for p in parts], 2)
    return build


def _rows_env_dirs(img):
    def build():
        im = image(img)
        w, h = im["w"], im["h"]
        g = _rng("env_dirs/" + img)  # env_pdf and env_radiance run the same directions
        # texel borders of the nearest-neighbour fetch and of the pdf's bins, the poles and phi = 0 = 2 pi
        # among them: every quarter step of the 2w x 2h grid, and the same angles a few ulps off
        th = np.pi * np.arange(0, 2 * h + 0.25, 0.25) / (2 * h)
        ph = 2 * np.pi * np.arange(0, 2 * w + 0.25, 0.25) / (2 * w)
        T, P = (x.ravel() for x in np.meshgrid(th, ph, indexing="ij"))
        grid = np.stack([np.sin(T) * np.cos(P), np.cos(T), np.sin(T) * np.sin(P)], axis=1).astype(np.float32)
        jit = u2f((f2u(grid).astype(np.int64) + g.integers(-2, 3, grid.shape)).astype(np.uint32))
        jit = np.where(grid == 0, grid, jit)
        ax = np.array([[0, 1, 0], [0, -1, 0], [1, 0, 0], [1, 0, -0.0], [-1, 0, 0], [-1, 0, -0.0], [1, 0, 1e-45], [1, 0, -1e-45],
                       [1, 0, 1e-8], [1, 0, -1e-8], [0, 0, 1], [0, 0, -1], [1e-30, 1, 0], [0, 1, -1e-30], [0.6, 0.8, -0.0]], dtype=np.float32)
        local = np.concatenate([_unit_vectors(g, 1 << 14), grid, jit, ax]).astype(np.float64)
        l2w = im["l2w"].astype(np.float64).reshape(3, 3).T                          # columns vx, vy, vz
        world = np.where(np.allclose(l2w, np.eye(3)), local, local @ l2w.T).astype(np.float32)
        return _finish("env_dirs/" + img, [f2u(world)], 3)
    return build


# (no env_pdf of the all-zero image: the reference divides its zero function by its zero integral,
# a NaN in every row, which the NaN cap does not admit; env_sample's pdf of it is 0 and is compared)
ENV_UNITS = {f"{fn}{form}@{img}": (fn, img) for img in IMAGE_NAMES for fn in ("env_sample", "env_pdf", "env_radiance")
             for form in ("", "_replay") if (fn, img) != ("env_pdf", "zero16")}


def device_name(name: str) -> str:
    """The name the evaluator knows a unit by (a unit's image is an argument, not part of the name)."""
    return name.split("@")[0]


# ------------------------------------------------------------------ the kernel option sets
# tests/cpp/Makefile states each set once (SET_<name> := -D...), beside the translation units it
# mirrors, and builds one evaluator per set.
_ROOT = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))


def option_sets() -> dict:
    """{set: {macro: value}} as tests/cpp/Makefile states them."""
    sets = {}
    for line in open(_os.path.join(_ROOT, "tests", "cpp", "Makefile")):
        m = _re.match(r"SET_(\w+)\s*:=\s*(.*)$", line)
        if m:
            sets[m.group(1)] = {k: int(v) for k, v in _re.findall(r"-D(\w+)=(-?\d+)", m.group(2))}
            assert len(sets[m.group(1)]) == len(m.group(2).split()), line
    return sets


# read when this module is imported: a SET_ line of the Makefile that is not a list of -DNAME=integer
# flags fails the import (the assert in option_sets), and with it every test of the unit modules
OPTION_SETS = option_sets()
# units that exist in some sets only: the served forms need SP_SERVE_RHO
ONLY_IN = {"rho16_served": ("rrnee",), "weights_served": ("rrnee",), "serve_rho": ("rrnee",)}
WHOLE_WAVES = ("stream", "serve_rho")  # units whose rows are whole waves of 64; every other row count is off the multiples


def evaluator(option_set: str) -> str:
    return _os.path.join(_ROOT, "tests", "cpp", "_build", "device_units" + ("" if option_set == "default" else "_" + option_set))


def units_of(option_set: str) -> list:
    return [n for n in FUNCTIONS if option_set in ONLY_IN.get(n, (option_set,))]


# ------------------------------------------------------------------ the table
FUNCTIONS = {
    # a. libm: all bits
    **{f: Spec(1, 1, f, ALL, None, False, _unary(f)) for f in
       ("expf", "logf", "sinf", "cosf", "erff", "acosf", "atanf", "fmod1", "roundf")},
    "sincosf": Spec(1, 2, "sincosf", ALL, None, False, _unary("sincosf")),
    "sincosf_bounded": Spec(1, 2, "sincosf_bounded", ALL, None, False, _rows_sincosf_bounded),
    "powf": Spec(2, 1, "powf", ALL, None, False, _rows_powf),
    "atan2f": Spec(2, 1, "atan2f", ALL, None, False, _rows_atan2f),
    "powf_unit": Spec(2, 2, "powf_unit", ALL, None, False, _rows_powf_unit),
    # b. arithmetic under the build flags
    "div": Spec(2, 1, "div", CLASS, None, True, _rows_div),
    "sqrt": Spec(1, 1, "sqrt", CLASS, None, False, _rows_sqrt),
    "fma": Spec(3, 1, "fma", CLASS, None, False, _rows_fma("fma")),
    "muladd": Spec(3, 1, "muladd", CLASS, None, False, _rows_fma("muladd")),
    "sqrt_unit": Spec(1, 1, "sqrt_unit", CLASS, None, False, _rows_sqrt_unit),
    "dot": Spec(6, 1, "dot", CLASS, None, False, _rows_dot_cross("dot")),
    "cross": Spec(6, 3, "cross", CLASS, None, False, _rows_dot_cross("cross")),
    "dop1": Spec(4, 1, "dop1", CLASS, None, False, _rows_dop1),
    # c. RSQRTSS from the packed and from the 32-bit LDS table
    "rsqrtss_packed": Spec(1, 1, "rsqrtss", ALL, "packed", False, _rows_rsqrt("rsqrtss_packed")),
    "rsqrtss_u32": Spec(1, 1, "rsqrtss", ALL, "u32", False, _rows_rsqrt("rsqrtss_u32")),
    "rsqrt_ref_packed": Spec(1, 1, "rsqrt_ref", CLASS, "packed", True, _rows_rsqrt("rsqrt_ref_packed")),
    "rsqrt_ref_u32": Spec(1, 1, "rsqrt_ref", CLASS, "u32", True, _rows_rsqrt("rsqrt_ref_u32")),
    # d. shading leaf functions
    "fresnel": Spec(3, 1, "fresnel", CLASS, None, False, _rows_fresnel),
    "erfinv": Spec(1, 1, "erfinv", CLASS, None, False, _rows_erfinv),
    "beck11": Spec(3, 2, "beck11", CLASS, None, False, _rows_beck11),
    "beck11_pre": Spec(7, 4, "beck11_pre", CLASS, "packed", False, _rows_beck11_pre),
    "uniform_sphere": Spec(2, 3, "uniform_sphere", CLASS, None, False, _u2_rows("uniform_sphere")),
    "uniform_hemisphere": Spec(2, 3, "uniform_hemisphere", CLASS, None, False, _u2_rows("uniform_hemisphere")),
    "concentric_disk": Spec(2, 2, "concentric_disk", CLASS, None, False, _u2_rows("concentric_disk")),
    "cosine_hemisphere": Spec(2, 3, "cosine_hemisphere", CLASS, None, False, _u2_rows("cosine_hemisphere")),
    "onb_of_unit": Spec(3, 9, "onb_of_unit", CLASS, None, False, _rows_onb),
    "beck_D": Spec(5, 1, "beck_D", CLASS, None, False, _rows_beck_w("beck_D")),
    "beck_lambda": Spec(5, 1, "beck_lambda", CLASS, None, False, _rows_beck_w("beck_lambda")),
    "beck_pdf": Spec(8, 1, "beck_pdf", CLASS, None, False, _rows_wo_w("beck_pdf", False)),
    "mf_eval": Spec(9, 3, "mf_eval", CLASS, "packed", False, _rows_wo_w("mf_eval", True)),
    "mf_pdf": Spec(8, 1, "mf_pdf", CLASS, "packed", False, _rows_wo_w("mf_pdf", False)),
    "spherical_phi": Spec(3, 1, "spherical_phi", CLASS, None, False, _rows_spherical_phi),
    "ray_offset": Spec(6, 1, "ray_offset", CLASS, None, False, _rows_ray_offset),
    # e. hit tests
    "tri_hit": Spec(17, 4, "tri_hit", CLASS, None, False, _rows_tri_hit),
    "sphere_t": Spec(20, 2, "sphere_t", CLASS, None, False, _rows_sphere_t),
    "plane_t": Spec(20, 2, "plane_t", CLASS, None, False, _rows_plane_t),
    "box_hit": Spec(14, 1, "box_hit", CLASS, None, False, _rows_box_hit),
    # f. the pixel stream (no orc_unit entry: the expectation is orc_mt_stream, stream_expected)
    "stream": Spec(2 + STREAM_STEPS, STREAM_OUT, None, ALL, None, False, _rows_stream),
    # g. the stream-fed layer; mf_sample_pre and the served forms are compared with the same reference
    # words as the form they restate
    "rho16": Spec(31, 5, "rho16", CLASS, "packed", False, _rows_local_draw),
    "rho16_served": Spec(31, 5, "rho16", CLASS, "packed", False, _rows_local_draw),
    "glossy_weights": Spec(31, 4, "glossy_weights", CLASS, "packed", False, _rows_local_draw),
    "weights_served": Spec(31, 4, "glossy_weights", CLASS, "packed", False, _rows_local_draw),
    "mf_sample": Spec(31, 10, "mf_sample", CLASS, "packed", False, _rows_local_draw),
    "mf_sample_pre": Spec(31, 10, "mf_sample", CLASS, "packed", False, _rows_local_draw),
    "material_sample": Spec(34, 10, "material_sample", CLASS, "packed", False, _rows_material("material_sample")),
    "material_eval": Spec(37, 5, "material_eval", CLASS, "packed", False, _rows_material("material_eval")),
    "material_pdf": Spec(37, 3, "material_pdf", CLASS, "packed", False, _rows_material("material_pdf")),
    "serve_rho": Spec(2 + ROW_MAT + 7, 12, "serve_rho", CLASS, "packed", False, _rows_serve_rho),
    "sphere_pdf": Spec(40, 1, "sphere_pdf", CLASS, None, False, _rows_light("sphere_pdf")),
    "light_sample": Spec(45, 9, "light_sample", CLASS, "packed", False, _rows_light("light_sample")),
    "light_pdf": Spec(43, 1, "light_pdf", CLASS, None, False, _rows_light("light_pdf")),
    # h. the image environment light: per image, the guided and the replayed lookup against the same reference words
    **{name: {"env_sample": Spec(2, 7, "env_sample", CLASS, "packed", False, _rows_env_sample(img), img),
              "env_pdf": Spec(3, 1, "env_pdf", CLASS, "packed", False, _rows_env_dirs(img), img),
              "env_radiance": Spec(3, 3, "env_radiance", CLASS, "packed", False, _rows_env_dirs(img), img)}[fn]
       for name, (fn, img) in ENV_UNITS.items()},
}

# the units that own a generator (section g's rows that draw): with the stream, the ones that read a kernel option
DRAWING = ("rho16", "rho16_served", "glossy_weights", "weights_served", "mf_sample", "mf_sample_pre", "material_sample",
           "material_eval", "material_pdf", "serve_rho")
STREAM_FED = DRAWING + ("sphere_pdf", "light_sample", "light_pdf") + tuple(ENV_UNITS)  # sections g and h

# Named exceptions: argument classes in which the device knowingly differs from
# the reference and no valid scene can reach.  Their rows are counted, printed and left out of the
# comparison; everything else of the function is asserted.
def _negative_denormal(r: np.ndarray) -> np.ndarray:
    return ((r[:, 0] & np.uint32(0xff800000)) == np.uint32(0x80000000)) & ((r[:, 0] & np.uint32(0x007fffff)) != 0)


# RSQRTSS reads a denormal as a zero of its sign, so the instruction gives -inf for a negative
# denormal; rsqrtss_emulated (sp_math.h) gives the default NaN of a negative argument.  The kernels
# only take rsqrt of dot(a, a), which is never negative, and the one-comparison fix changed the
# registers or scratch of 52 render kernels, so the kernels stay as they are.
EXCEPTIONS = {name: ("negative denormal argument", _negative_denormal)
              for name in ("rsqrtss_packed", "rsqrtss_u32", "rsqrt_ref_packed", "rsqrt_ref_u32")}


def rows(name: str) -> np.ndarray:
    """The input rows of one function: uint32 [n, k]."""
    r = FUNCTIONS[name].rows()
    assert r.dtype == np.uint32 and r.ndim == 2 and r.shape[1] == FUNCTIONS[name].k
    assert (r.shape[0] % 64 != 0) != (name in WHOLE_WAVES)  # a partial last wave; the stream and serve_rho: whole waves
    return r


# ------------------------------------------------------------------ the reference side
def oracle_arity(variant: str, oracle_name: str):
    from tests import _oracle
    L = _oracle.load(variant)
    k, m = C.c_int(), C.c_int()
    L.orc_unit_arity.restype = C.c_int
    L.orc_unit_arity.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    rc = L.orc_unit_arity(oracle_name.encode(), C.byref(k), C.byref(m))
    return None if rc != 0 else (k.value, m.value)


def oracle_unit(variant: str, name: str, r: np.ndarray) -> np.ndarray:
    """orc_unit of liboracle_<variant>.so on the rows of function `name`: uint32 [n, m]."""
    from tests import _oracle
    spec = FUNCTIONS[name]
    L = _oracle.load(variant)
    if spec.image:
        oracle_set_image(variant, spec.image)
    L.orc_unit.restype = C.c_int
    L.orc_unit.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.c_int64, C.POINTER(C.c_uint32)]
    r = np.ascontiguousarray(r, dtype=np.uint32)
    assert r.shape[1] == spec.k
    out = np.zeros((r.shape[0], spec.m), dtype=np.uint32)
    rc = L.orc_unit(spec.oracle.encode(), r.ctypes.data_as(C.POINTER(C.c_uint32)), r.shape[0],
                    out.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == 0, (name, rc)
    return out


def is_nan(words: np.ndarray) -> np.ndarray:
    return (words & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)


def mismatches(name: str, r: np.ndarray, got: np.ndarray, ref: np.ndarray):
    """Rows of `got` that differ from `ref` under the function's NaN rule, the number of rows whose
    reference holds a NaN, and the number of rows left out as the function's named exception.  Flags
    and other integer outputs never look like NaNs (0 or 1)."""
    nan_ref = is_nan(ref)
    if FUNCTIONS[name].rule == ALL:
        bad = got != ref
    else:
        bad = np.where(nan_ref, ~is_nan(got), got != ref)
    bad = bad.any(axis=1)
    excepted = EXCEPTIONS[name][1](r) if name in EXCEPTIONS else np.zeros(r.shape[0], dtype=bool)
    return np.flatnonzero(bad & ~excepted), int(nan_ref.any(axis=1).sum()), int(excepted.sum())


def reference(variant: str, name: str, r: np.ndarray) -> np.ndarray:
    """The expected output words of function `name` on rows r, from liboracle_<variant>.so."""
    return stream_expected(variant, r) if name == "stream" else oracle_unit(variant, name, r)
