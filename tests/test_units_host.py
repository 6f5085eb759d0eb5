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
    assert r.shape[0] % 64 != 0 and r.shape[0] > 256  # a partial last wave, more than one block
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
    assert want <= seen, sorted(want - seen)


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
