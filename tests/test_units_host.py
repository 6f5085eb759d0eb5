"""The reference side and the inputs of the device unit tests (tests/test_gpu_units.py), without a GPU.

For every function of tests/_units.py the two oracles -- liboracle_glibc.so (the reference
semantics) and liboracle_spm.so (the device headers compiled for the host) -- evaluate the full
input set and must agree bit for bit, NaNs included: whatever the device then differs in is a
matter of the device compilation alone.  The NaN rule of _units.py is kept honest here: a function
whose NaNs are compared by class only may have a reference NaN in at most 0.1 % of its rows
(`div` and the rsqrt_ref forms excepted)."""
import numpy as np
import pytest

from tests import _units

NAMES = [n for n, spec in _units.FUNCTIONS.items() if spec.oracle]  # all but the pixel stream


@pytest.fixture(scope="module", params=NAMES)
def evaluated(request):
    name = request.param
    r = _units.rows(name)
    return name, r, _units.oracle_unit("glibc", name, r), _units.oracle_unit("spm", name, r)


def _hex(a):
    return " ".join(f"{int(v):08x}" for v in a)


def test_oracles_agree_bit_for_bit(evaluated):
    name, r, glibc, spm = evaluated
    bad = np.flatnonzero((glibc != spm).any(axis=1))
    msg = "\n".join(f"  in {_hex(r[i])}  glibc {_hex(glibc[i])}  spm {_hex(spm[i])}" for i in bad[:8])
    assert bad.size == 0, f"{name}: {bad.size} of {r.shape[0]} rows differ between the oracles\n{msg}"


def test_nan_share(evaluated):
    name, r, glibc, _ = evaluated
    spec = _units.FUNCTIONS[name]
    nan_rows = int(_units.is_nan(glibc).any(axis=1).sum())
    print(f"{name}: {r.shape[0]} rows, {nan_rows} with a NaN in the reference")
    if spec.rule == _units.CLASS and not spec.nan_exempt:
        assert nan_rows <= _units.NAN_CAP * r.shape[0], (name, nan_rows, r.shape[0])


def test_rows_are_shaped_for_the_kernel(evaluated):
    name, r, glibc, _ = evaluated
    spec = _units.FUNCTIONS[name]
    assert r.shape[1] == spec.k and glibc.shape == (r.shape[0], spec.m)
    # a partial last wave (serve_rho: whole waves), more than one block
    assert (r.shape[0] % 64 != 0) != (name in _units.WHOLE_WAVES) and r.shape[0] > 256
    for variant in ("glibc", "spm"):
        assert _units.oracle_arity(variant, spec.oracle) == (spec.k, spec.m), name


def test_unknown_function_is_refused():
    assert _units.oracle_arity("glibc", "no_such_function") is None


def test_powf_unit_rows_lie_in_the_claimed_box():
    r = _units.rows("powf_unit")
    (xlo, xhi), (ylo, yhi) = _units.POWF_UNIT_X, _units.POWF_FIT
    assert ((r[:, 0] >= xlo) & (r[:, 0] <= xhi) & (r[:, 1] >= ylo) & (r[:, 1] <= yhi)).all()
    for face, col in ((xlo, 0), (xhi, 0), (ylo, 1), (yhi, 1)):  # both faces of each interval
        assert (r[:, col] == face).any()
    # the box is the one the header claims and the recorded full sweep covered
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "simplepath_amd", "csrc", "common", "sp_libm.h")).read()
    log = open(os.path.join(root, "tests", "golden", "libm_forms_full.txt")).read()
    assert f"POWF_UNIT_X_LO = 0x{xlo:08x}u, POWF_UNIT_X_HI = 0x{xhi:08x}u" in hdr
    assert f"POWF_FIT_LO = 0x{ylo:08x}u, POWF_FIT_HI = 0x{yhi:08x}u" in hdr
    assert f"powf_unit x=[0x{xlo:08x},0x{xhi:08x}] y=[0x{ylo:08x},0x{yhi:08x}]" in log


def test_sincosf_bounded_rows_are_bounded():
    r = _units.rows("sincosf_bounded")
    mag = r[:, 0] & np.uint32(0x7fffffff)
    assert (mag < 0x42f00000).all() and (mag == 0x42f00000 - 1).any()


def test_sqrt_unit_rows_lie_in_its_domain():
    r = _units.rows("sqrt_unit")[:, 0]
    mag = r & np.uint32(0x7fffffff)
    assert ((mag == 0) | ((r >= 0x0f800000) & (r <= _units.F32_MAX))).all()
    assert np.isin(np.arange(0x3f7fc000, 0x3f800001, dtype=np.uint32), r).all()  # every float in [1 - 2^-10, 1]


# ------------------------------------------------------------------ the pixel stream's scripts
class _RngModel:
    """The position bookkeeping of sp_path.hpp's Rng, restated from rng_raw / rng_skip /
    rng_skip_reserved: idx within the generation, the number of buffer switches."""

    def __init__(self):
        self.idx, self.switches = _units.MT_N, 0

    def position(self):
        return (self.switches - 1) * _units.MT_N + self.idx

    def raw(self):
        if self.idx >= _units.MT_N:
            self.switches, self.idx = self.switches + 1, 0
        self.idx += 1
        return self.position() - 1, self.idx - 1  # stream position and buffer index of the word drawn

    def skip(self, n):
        while n > 0:
            if self.idx >= _units.MT_N:
                self.switches, self.idx = self.switches + 1, 0
            take = min(n, _units.MT_N - self.idx)
            self.idx, n = self.idx + take, n - take

    def skip_reserved(self, n):
        t = self.idx + n
        if t > _units.MT_N:
            self.switches, self.idx = self.switches + 1, t - _units.MT_N
        else:
            self.idx = t


def test_stream_scripts_consume_what_the_expectation_assumes():
    U = _units
    r = U.rows("stream")
    assert r.shape == (U.STREAM_LANES, 2 + U.STREAM_STEPS) and U.STREAM_LANES % 256 == 0
    assert len(set(r[:, 0].tolist())) == r.shape[0]                       # every lane its own seed
    assert all((r[w * 64:(w + 1) * 64, 1] == 1).sum() == 32 for w in range(r.shape[0] // 64))
    seen = set()
    first_switch_step = []
    # every margin an option set compiles rng_prepare with (96, and 144 in the rrnee set)
    margins = sorted({s.get("SP_RNG_MARGIN", U.RNG_MARGIN) for s in U.OPTION_SETS.values()})
    assert U.RNG_MARGIN in margins and 144 in margins
    for row in r:
        m, drawn = _RngModel(), []
        switch_steps = []
        for si, step in enumerate(row[2:]):
            op, n, prepare = int(step) & 15, int(step) >> 8, bool(int(step) & 16)
            before, sw = m.position(), m.switches
            if prepare:
                seen.add("prepare in the margin" if U.MT_N - U.RNG_MARGIN <= m.idx < U.MT_N else
                         "prepare at the boundary" if m.idx == U.MT_N else
                         "prepare just after a boundary" if m.idx < 8 else "prepare early")
                for mg in margins:  # the same scripts, read with each set's margin
                    seen.add(f"margin {mg}: " + ("prepare in the margin" if U.MT_N - mg <= m.idx < U.MT_N else
                                                 "prepare within 16 words before the margin" if U.MT_N - mg - 16 <= m.idx < U.MT_N - mg
                                                 else "prepare elsewhere"))
                    if m.idx in (U.MT_N - mg - 1, U.MT_N - mg):
                        seen.add(f"margin {mg}: prepare at idx = N - margin{' - 1' if m.idx == U.MT_N - mg - 1 else ''}")
                if U.MT_N - max(margins) <= m.idx < U.MT_N - min(margins):
                    seen.add("prepare inside the wide margin and outside the narrow one")
            if op == U.OP_DRAW:
                for _ in range(n):
                    pos, idx = m.raw()
                    drawn.append(pos)
                    seen.add(f"draw at {idx}") if idx in (0, 1, 311) else None
                if n > 2 and sw != m.switches and before % U.MT_N != 0:
                    seen.add("run of draws across a boundary")
            elif op == U.OP_RAW2:
                a, b = m.raw(), m.raw()
                drawn += [a[0], b[0]]
                seen.add("raw2 straddling") if (a[1], b[1]) == (311, 0) else None
                seen.add("raw2 at the switch") if a[1] == 0 else None
            elif op == U.OP_SKIP:
                idx0 = m.idx
                m.skip(n)
                if n in U.SKIP_COUNTS:
                    seen.add(f"skip {n} from " + ("the boundary" if idx0 == U.MT_N else "inside"))
            elif op == U.OP_RESERVE_DRAW:
                assert 0 < n <= U.MT_N
                seen.add("reserved draws spanning") if m.idx < U.MT_N < m.idx + n else None
                drawn += [m.raw()[0] for _ in range(n)]
            elif op == U.OP_RESERVE_SKIP:
                assert 0 < n <= U.MT_N
                seen.add("reserved skip spanning") if m.idx < U.MT_N < m.idx + n else None
                m.skip_reserved(n)
            else:
                assert op == U.OP_NOP and n == 0
            assert m.position() - before == U.step_words(op, n)[0]      # the count the expectation assumes
            if sw != m.switches:
                switch_steps.append(si)
        assert drawn == U.stream_positions(row)
        assert m.position() >= U.STREAM_WORDS > 6 * U.MT_N and len(drawn) < U.STREAM_OUT
        first_switch_step.append(tuple(switch_steps[1:4]))
    # lanes of one wave reach the boundaries at steps of their own
    assert all(len(set(first_switch_step[w * 64:(w + 1) * 64])) > 48 for w in range(r.shape[0] // 64))
    want = {"draw at 311", "draw at 0", "draw at 1", "raw2 straddling", "raw2 at the switch", "reserved draws spanning",
            "reserved skip spanning", "run of draws across a boundary", "prepare in the margin", "prepare at the boundary",
            "prepare just after a boundary"}
    want |= {f"skip {n} from {where}" for n in U.SKIP_COUNTS for where in ("the boundary", "inside")}
    # rng_prepare's window in every set: a prepare inside each margin, one just short of it (no lane of
    # its own makes the call urgent), one on either side of its first word, and one that only the wide
    # margin of the rrnee set takes
    want |= {f"margin {mg}: {what}" for mg in margins for what in
             ("prepare in the margin", "prepare within 16 words before the margin", "prepare at idx = N - margin",
              "prepare at idx = N - margin - 1")}
    want.add("prepare inside the wide margin and outside the narrow one")
    assert want <= seen, sorted(want - seen)


# ------------------------------------------------------------------ the kernel option sets
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_DIR = os.path.join(ROOT, "simplepath_amd", "csrc", "hip")
# Preamble macros no unit reads: sp_wave.hip's own constant, the number of stream rows wf_shade touches
# ahead of a glossy hit.  It is used in sp_wave.hip alone (asserted below), so the wave set's evaluator
# is built without it.
PRIVATE = {"SP_WAVE_RNG_TOUCH"}


def _preamble(path):
    """The SP_ macros a translation unit defines before its first #include, with macros that only
    forward another one (#define SP_RNG_PF SP_CHUNK_RNG_PF) resolved and the forwarded name dropped."""
    raw = {}
    for line in open(path):
        if line.startswith("#include"):
            break
        m = re.match(r"#\s*define\s+(SP_\w+)\s+(\S+)", line)
        if m:
            raw[m.group(1)] = m.group(2)
    forwarded = {v for v in raw.values() if v in raw}
    out = {}
    for k, v in raw.items():
        if k in forwarded:
            continue
        while v in raw:
            v = raw[v]
        out[k] = int(v)
    return out


def test_every_translation_unit_is_compiled_under_a_stated_option_set():
    sets = _units.OPTION_SETS
    assert set(sets) == {"default", "direct", "rrnee", "chunk", "wave"}
    # the default set restates the headers' own defaults
    headers = "".join(open(os.path.join(HIP_DIR, h)).read() for h in ("sp_path.hpp", "sp_device.hpp"))
    for macro, value in sets["default"].items():
        assert re.search(rf"#ifndef {macro}\n#define {macro} {value}\n", headers), (macro, value)
    # the private macro is read by its own translation unit alone
    for name in os.listdir(HIP_DIR):
        if name != "sp_wave.hip":
            assert not (PRIVATE & set(re.findall(r"SP_\w+", open(os.path.join(HIP_DIR, name)).read()))), name
    used = {}
    for name in sorted(os.listdir(HIP_DIR)):
        if not name.endswith(".hip"):
            continue
        pre = {k: v for k, v in _preamble(os.path.join(HIP_DIR, name)).items() if k not in PRIVATE}
        match = [s for s, opts in sets.items() if (opts == pre if pre else s == "default")]
        assert len(match) == 1, f"{name}: its preamble {pre} is none of the option sets of tests/cpp/Makefile: {sets}"
        used.setdefault(match[0], []).append(name)
    print({s: len(v) for s, v in used.items()})
    assert set(used) == set(sets), "an option set no translation unit uses"
    # no two sets are the same options: none could share a binary
    assert len({tuple(sorted(o.items())) for o in sets.values()}) == len(sets)
    assert "sp_mega_direct.hip" in used["direct"] and "sp_mega_rrnee.hip" in used["rrnee"]
    assert used["chunk"] == ["sp_chunk.hip"] and used["wave"] == ["sp_wave.hip"] and "sp_mega.hip" in used["default"]


def test_units_of_every_set():
    for s in _units.OPTION_SETS:
        names = _units.units_of(s)
        assert "stream" in names and all(n in names for n in _units.STREAM_FED if n not in _units.ONLY_IN)
        assert all(n in names for n in _units.DRAWING if n not in _units.ONLY_IN)
        assert ("weights_served" in names) == ("rho16_served" in names) == (_units.OPTION_SETS[s].get("SP_SERVE_RHO", 0) == 1)
        assert ("serve_rho" in names) == (_units.OPTION_SETS[s].get("SP_SERVE_RHO", 0) == 1)


# ------------------------------------------------------------------ the stream-fed layer's rows hold their edges
def _f(words):
    return _units.u2f(words)


def test_stream_positions_hold_every_straddle():
    U = _units
    for name in ("rho16", "material_eval", "material_sample"):
        skip = U.rows(name)[:, 1].astype(np.int64)
        idx = skip % U.MT_N
        assert (idx % 2 == 0).any() and (idx % 2 == 1).any()                      # even and odd inside a generation
        for bound in (U.MT_N, 2 * U.MT_N):                                        # the first boundary, and a second further on
            starts = set(skip[(skip >= bound - 33) & (skip <= bound + 1)].tolist())
            assert starts == set(range(bound - 33, bound + 2)), (name, bound, sorted(set(range(bound - 33, bound + 2)) - starts))
        assert (skip == 0).any() and (skip == U.MT_N - 1).any()
    # an estimate (32 words) whose words straddle the boundary at an odd and at an even index, with a wo that draws
    r = U.rows("rho16")
    skip, wy = r[:, 1].astype(np.int64) % U.MT_N, _f(r[:, 29])
    straddle = (skip + 32 > U.MT_N) & (skip < U.MT_N) & (wy != 0)
    assert (straddle & (skip % 2 == 1)).any() and (straddle & (skip % 2 == 0) & (skip > 0)).any()
    assert ((skip == U.MT_N - 1) & (wy != 0)).any()                              # a sample's pair split across the boundary


def test_material_rows_hold_every_class():
    U = _units
    for name, kinds in (("glossy_weights", {U.MAT_GLOSSY}), ("material_eval", {U.MAT_LAMBERTIAN, U.MAT_GLOSSY, U.MAT_CLEARCOAT})):
        r = U.rows(name)
        mat = r[:, 2:2 + U.ROW_MAT]
        assert set(mat[:, 0].tolist()) == kinds
        assert (mat[:, 10] == 1).all() and (mat[:, 25] == 1).all()               # sample_visible_area: the parser's only value
        coat = mat[:, 0] == U.MAT_CLEARCOAT
        rec = np.where(coat[:, None], mat[:, 15:26], mat[:, 0:11])               # the record whose lobes are read
        glossy = rec[:, 0] == U.MAT_GLOSSY
        alb, R = _f(rec[:, 1:4]), rec[:, 4:7]
        one, half, up = (U.f2u([v])[0] for v in (1.0, 0.5, U.ONE_ULP))
        grey = (R[:, 0] == R[:, 1]) & (R[:, 1] == R[:, 2])
        assert (glossy & (R == one).all(axis=1)).any() and (glossy & (R == half).all(axis=1)).any()
        for ch in range(3):  # an ulp off grey in each channel: no shortcut may be taken
            assert (glossy & (R[:, ch] == up) & (np.delete(R, ch, axis=1) == one).all(axis=1)).any(), (name, ch)
        assert (glossy & ~grey & (np.abs(_f(R) - 1.0) > 0.01).any(axis=1)).any()  # coloured
        assert (glossy & (_f(R) == 0).all(axis=1) & (alb > 0).all(axis=1)).any()  # black R alone
        assert (glossy & (_f(R) == 0).all(axis=1) & (alb == 0).all(axis=1)).any()  # both black: 0 / 0
        assert (alb == 0).all(axis=1).any() and (alb > 1).all(axis=1).any() and ((alb > 0) & (alb < 1)).all(axis=1).any()
        ax, ay, ior = _f(rec[:, 7]), _f(rec[:, 8]), _f(rec[:, 9])
        for a in U.ALPHAS:
            assert (glossy & (ax == np.float32(a)) & (ay == ax)).any() and (glossy & (ax == np.float32(a)) & (ay != ax)).any()
        assert set(ior[glossy].tolist()) == {float(np.float32(v)) for v in U.IORS}
        if coat.any():
            assert set(_f(mat[coat, 11]).tolist()) == {float(np.float32(v)) for v in U.COAT_IORS}
            cc = _f(mat[coat, 12:15])
            assert (cc == 1).all(axis=1).any() and (cc != 1).any(axis=1).any()
            assert (mat[coat, 15] == U.MAT_LAMBERTIAN).any() and (mat[coat, 15] == U.MAT_GLOSSY).any()
            lam = (mat[:, 0] == U.MAT_LAMBERTIAN)
            assert (lam & (_f(mat[:, 1:4]) == 0).all(axis=1)).any()              # a Lambertian of zero albedo: its weight is 0 / 0


def test_direction_rows_hold_every_class():
    U = _units
    wo = _f(U.rows("rho16")[:, 28:31])
    y = wo[:, 1]
    assert ((y == 0) & ~np.signbit(y)).any() and ((y == 0) & np.signbit(y)).any()  # wo.y = +0, -0: nothing is drawn
    assert ((np.abs(y) < 1e-30) & (y != 0)).any() and ((np.abs(y) < 1e-5) & (np.abs(y) > 1e-7)).any()
    assert (y < -0.5).any() and (y > 0.5).any()                                  # below and above the surface
    for d in U.DIR_SPECIALS:
        assert (wo.view(np.uint32) == U.f2u(d)).all(axis=1).any(), d
    # world form: in the rows whose normal is (0, 1, 0) the local directions are an exact permutation
    r = U.rows("material_eval")
    n, wo, wi = _f(r[:, 28:31]), _f(r[:, 31:34]), _f(r[:, 34:37])
    axis = (n == np.float32([0, 1, 0])).all(axis=1)
    assert axis.any() and (~axis).any() and (np.abs(np.linalg.norm(n[~axis], axis=1) - 3.0) < 1e-3).any()
    assert (axis & (wo[:, 1] == 0)).any() and (axis & (np.abs(wo[:, 1]) < 1e-30) & (wo[:, 1] != 0)).any()
    assert (axis & (wi == wo).all(axis=1)).any() and (axis & (wi == -wo).all(axis=1)).any()
    assert (axis & (wi[:, 1] * wo[:, 1] < 0)).any() and (axis & (wi[:, 1] * wo[:, 1] > 0)).any()  # the other hemisphere, the same


def test_light_rows_hold_every_class():
    U = _units
    r = U.rows("light_sample")
    kind, rad = r[:, 0], _f(r[:, 1:4])
    assert set(kind.tolist()) == {U.LIGHT_SPHERE, U.LIGHT_ENVIRONMENT}
    sphere = kind == U.LIGHT_SPHERE
    assert (sphere & (rad == 0).all(axis=1)).any() and (sphere & (rad > 0).all(axis=1)).any()
    w2o = _f(r[:, 16:28]).astype(np.float64)
    obs = _f(r[:, U.ROW_LIGHT:U.ROW_LIGHT + 3]).astype(np.float64)
    A = np.transpose(w2o[:, :9].reshape(-1, 3, 3), (0, 2, 1))
    obj = np.einsum("nij,nj->ni", A, obs) + w2o[:, 9:]
    sq = (obj * obj).sum(axis=1)
    ulp = 2.0 ** -23
    assert (sphere & (sq < 0.95)).any() and (sphere & (sq > 1.1)).any()          # inside, outside
    ident = (_f(r[:, 16:28]) == np.float32([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])).all(axis=1)
    for lo, hi in ((1 - 32 * ulp, 1), (1, 1 + 32 * ulp)):                        # within 32 ulps of the sphere, either side
        assert (sphere & ident & (sq > lo) & (sq < hi)).any()
    sq32 = (_f(r[:, U.ROW_LIGHT:U.ROW_LIGHT + 3]) ** 2).sum(axis=1, dtype=np.float32)
    assert (sphere & ident & (sq32 == 1)).any()                                  # and on it
    sw = U.SPHERE_PDF_SWITCH
    assert (sphere & (sq > sw * (1 - 1e-4)) & (sq < sw)).any() and (sphere & (sq > sw) & (sq < sw * (1 + 1e-4))).any()
    # o2w is the inverse of w2o
    o2w = _f(r[:, 4:16]).astype(np.float64)
    B = np.transpose(o2w[:, :9].reshape(-1, 3, 3), (0, 2, 1))
    assert np.abs(np.einsum("nij,njk->nik", A, B) - np.eye(3)).max() < 1e-4
    u = _f(r[:, U.ROW_LIGHT + 6:U.ROW_LIGHT + 8])
    assert (u >= 0).all() and (u <= U.U_TOP).all()
    for v in U.U_SPECIALS:
        assert (u[:, 0] == v).any() and (u[:, 1] == v).any(), v
    assert (U.rows("sphere_pdf")[:, 0] == U.LIGHT_SPHERE).any()


def test_images_and_their_rows_hold_every_class():
    U = _units
    assert {(U.image(i)["w"], U.image(i)["h"]) for i in U.IMAGE_NAMES} == {(16, 8), (64, 32)}
    for img in U.IMAGE_NAMES:
        im = U.image(img)
        px, nu, nv = im["pixels"], 2 * im["w"], 2 * im["h"]
        marg, cond = U.env_cdfs(img)
        lum = px.sum(axis=2)
        r = U.rows(f"env_sample@{img}")
        ref = U.oracle_unit("glibc", f"env_sample@{img}", r)
        u = _f(r)
        assert (u >= 0).all() and (u <= U.U_TOP).all()
        assert (u == 0).any(axis=0).all() and (u == U.U_TOP).any(axis=0).all()     # u at 0 and at 1 - 2^-24, both coordinates
        if img == "zero16":
            assert (px == 0).all() and (ref[:, 3] == 0).all()                      # an all-zero image: pdf 0 everywhere
            continue
        assert (lum == 0).all(axis=1).any() and (lum == 0).all(axis=0).any()      # a zero row, a zero column
        dim = np.median(lum[lum > 0])
        assert (lum > 1000 * dim).sum() >= 1 and (0.2126 * px[..., 0] + 0.7152 * px[..., 1] + 0.0722 * px[..., 2] > im["max_radiance"]).any()
        assert (np.diff(cond[:, :nu], axis=1) == 0).any() and (np.diff(marg[:nv]) == 0).any() == (lum == 0).all(axis=1).any()
        # u on the oracle's own table entries and their neighbours: the marginal's, and each selectable row's
        for e in marg[:nv][(marg[:nv] > 0) & (marg[:nv] < 1)][:: max(1, nv // 8)]:
            b = int(U.f2u([e])[0])
            assert {b - 1, b, b + 1} <= set(r[:, 1].tolist())
        v = nv // 2 + 1
        uy = np.float32((np.float64(marg[v - 1]) + np.float64(marg[v])) / 2)
        on_row = r[r[:, 1] == U.f2u([uy])[0], 0]
        for e in cond[v, 1:nu:7]:
            if not 0 < e < U.U_TOP:  # an entry at 1 is out of u's range: its rows sit at 1 - 2^-24
                continue
            b = int(U.f2u([e])[0])
            assert {b - 1, b, b + 1} <= set(on_row.tolist()), (img, v)
        for bits in (U.guide_bits(nu), U.guide_bits(nv)):                          # the guides' bucket edges
            for k in (1, (1 << bits) // 2, (1 << bits) - 1):
                b = int(U.f2u([k / (1 << bits)])[0])
                assert {b - 1, b, b + 1} <= set(r[:, 0].tolist()) and {b - 1, b, b + 1} <= set(r[:, 1].tolist())
        assert (ref[:, 3] != 0).all()   # zero texels are never chosen (the reference's shifted cdf can make the pdf negative)
        d = _f(U.rows(f"env_pdf@{img}"))
        if img == "a16":  # identity transform: the special directions arrive as they are
            for s in ([0, 1, 0], [0, -1, 0], [1, 0, 0], [1, 0, -0.0], [1, 0, 1e-45], [1, 0, -1e-45]):
                assert (d.view(np.uint32) == U.f2u(np.float32(s))).all(axis=1).any(), s
            phi = np.arctan2(d[:, 2].astype(np.float64), d[:, 0].astype(np.float64)) % (2 * np.pi)
            border = 2 * np.pi * 2.5 / im["w"]                                     # a texel border of the nearest-neighbour fetch
            assert (np.abs(phi - border) < 1e-6).sum() >= 3


def test_reference_pdf_of_the_all_zero_image_is_a_nan_everywhere():
    """Why there is no env_pdf unit of zero16: the reference's pdf_impl divides the zero function by
    the zero integral for every direction off the poles (at a pole it returns 0 before dividing).
    Nothing is specified for the device there, and nothing is compared."""
    import ctypes as C
    U = _units
    d = U.rows("env_pdf@a16")
    for variant in ("glibc", "spm"):
        L, _ = U.oracle_set_image(variant, "zero16")
        out = np.zeros((d.shape[0], 1), np.uint32)
        L.orc_unit.restype = C.c_int
        L.orc_unit.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.c_int64, C.POINTER(C.c_uint32)]
        assert L.orc_unit(b"env_pdf", d.ctypes.data_as(C.POINTER(C.c_uint32)), d.shape[0], out.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
        nan = U.is_nan(out[:, 0])
        assert nan.mean() > 0.99 and (out[~nan, 0] == 0).all()
    # env_sample of the same image is specified and compared: pdf 0, black, no direction
    r = U.rows("env_sample@zero16")
    assert (U.oracle_unit("glibc", "env_sample@zero16", r) == 0).all()


def test_directions_of_the_transformed_image_keep_their_classes():
    """b64's light is rotated and scaled: its direction rows are taken back through world_to_light (as
    env_pdf does) and must still hold the poles, phi 0 = 2 pi from both sides, and the borders of the
    texels and of the pdf's bins, to within the rounding of the two 3x3 products."""
    U = _units
    im = U.image("b64")
    w2l = im["w2l"].astype(np.float64).reshape(3, 3).T
    assert not np.allclose(w2l, np.eye(3))
    d = _f(U.rows("env_pdf@b64")).astype(np.float64) @ w2l.T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    theta = np.arccos(np.clip(d[:, 1], -1, 1))
    phi = np.arctan2(d[:, 2], d[:, 0]) % (2 * np.pi)
    eps = 2e-6
    assert (theta < eps).any() and (theta > np.pi - eps).any()                     # both poles
    mid = (theta > 0.3) & (theta < np.pi - 0.3)
    assert (mid & (phi < eps)).any() and (mid & (phi > 2 * np.pi - eps)).any()     # phi 0 and 2 pi
    for k in (3, 40.5, 100):  # borders of the pdf's 2w bins (integers) and of the w texels' rounding (half texels: odd halves)
        assert (mid & (np.abs(phi - 2 * np.pi * k / (2 * im["w"])) < eps)).sum() >= 3, k
    for k in (5, 20.5, 47):
        assert (np.abs(theta - np.pi * k / (2 * im["h"])) < eps).sum() >= 3, k


def test_serve_rho_waves_hold_every_class():
    U = _units
    r = U.rows("serve_rho")
    assert r.shape == (U.SERVE_WAVES * 64, 35) and U.SERVE_WAVES % 4 == 0          # whole waves, whole blocks
    ref = U.oracle_unit("glibc", "serve_rho", r)
    flags = r[:, 34].reshape(-1, 64)
    assert set(flags.ravel().tolist()) == {0, 1, 2, 3, 4}
    want, want_a, absent = (flags & 1) != 0, (flags & 2) != 0, flags == U.ABSENT
    active = (~absent).sum(axis=1)
    requests = 3 * want.sum(axis=1) + want_a.sum(axis=1)
    assert ((flags == 3).all(axis=1)).any()                                        # full waves where every lane wants
    assert ((want | want_a).sum(axis=1) == 1).any()                                # one lane only
    only = np.zeros(64, bool)
    only[[0, 63]] = True
    assert (((want | want_a) == only).all(axis=1)).any()                           # wants in lanes 0 and 63
    assert ((absent.sum(axis=1) >= 24) & (absent.sum(axis=1) <= 40) & (requests > 0)).any()   # half the lanes absent
    assert ((absent.sum(axis=1) == 48) & (requests == 64)).any()                   # 64 requests dealt to 16 lanes
    assert (requests > active).any() and (requests > 3 * active).any() and ((requests > 0) & (requests <= active)).any()
    assert (absent[:, 0] & (requests > 0)).any() and (absent[:, 63] & (requests > 0)).any()   # ranks differ from lane ids
    # owners: the estimates of the three sites straddle the generation boundary; dc 0; coats
    skip = r[:, 1].astype(np.int64).reshape(-1, 64)
    mat0 = r[:, 2].reshape(-1, 64)
    coat = mat0 == U.MAT_CLEARCOAT
    assert set(mat0.ravel().tolist()) == {U.MAT_GLOSSY, U.MAT_CLEARCOAT} and (r[:, 17] == U.MAT_GLOSSY).all()
    served_a = ref[:, 0].reshape(-1, 64) == 1
    words_b = ref[:, 10].reshape(-1, 64).astype(np.int64)
    start_b = skip + np.where(served_a, ref[:, 3].reshape(-1, 64).astype(np.int64) + 3, 0) + 2
    idx = start_b % U.MT_N
    for k in (0, 1, 2):  # the boundary inside the eval, the pdf and the sample site's estimate
        lo, hi = idx + 32 * k, idx + 32 * (k + 1)
        assert (want & (words_b >= 96) & (lo < U.MT_N) & (hi > U.MT_N)).any(), k
    assert (want_a & served_a & (skip % U.MT_N + 33 > U.MT_N) & (skip % U.MT_N < U.MT_N)).any()   # and inside the bounce's
    assert (want & (words_b == 0)).any() and (want & coat & (words_b == 1)).any()  # dc 0 owners, with a coat too
    assert (want & coat & (words_b == 97)).any() and (want & ~coat & (words_b == 96)).any()
    assert (want_a & ~served_a & coat).any() and (want_a & served_a & coat).any()  # a specular pick wants nothing after all
    assert (ref[absent.ravel()] == 0).all()
    # the same estimate at the same position gives the same weights: a check of the expectation itself
    w = ref.reshape(-1, 64, 12)
    dc0 = want & (words_b <= 1)
    assert (w[dc0][:, 4:6] == w[dc0][:, 6:8]).all()


def test_stream_expectation_is_the_same_in_both_oracles():
    r = _units.rows("stream")[:64]
    assert np.array_equal(_units.stream_expected("glibc", r), _units.stream_expected("spm", r))


def test_evaluator_refuses_bad_calls(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "cpp", "_build", "device_units")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(root, "tests", "cpp"), "_build/device_units"], check=True, timeout=600)
    rows = tmp_path / "in.bin"
    np.arange(7, dtype=np.uint32).tofile(rows)  # 7 words: no rows of 2
    for args, text in ((["no_such_function", str(rows), str(tmp_path / "o")], "unknown function"),
                       (["powf", str(rows), str(tmp_path / "o")], "short file"),
                       (["expf", str(tmp_path / "missing"), str(tmp_path / "o")], "cannot read"),
                       (["rsqrt_ref_packed", str(rows), str(tmp_path / "o")], "needs the RSQRTSS table")):
        p = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and text in p.stderr, (args, p.returncode, p.stderr)
