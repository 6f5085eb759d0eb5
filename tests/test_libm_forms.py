"""lm_powf_unit, the powf entry of beckmann_sample11's one call site (sp_libm.h), against lm_powf.

The entry is lm_powf without its tests for zero, inf, NaN, negative and subnormal arguments and
for overflow / underflow, all of which are dead on the box of arguments the call site can pass:
x = 1 - max(U1, 1e-6f) in [2^-24, 1 - 1e-6f] and y = fit(acosf(c)), c in [0, .9999f].
tools/libm_exhaustive.cpp

  fitrange   evaluates fit for every float c of that interval (about 1.07e9 values) and fails if one
             leaves the y interval the entry claims,
  powf_unit  compares the entry with spm::lm_powf bit for bit for every float x of the x interval
             (2.0e8 values; here every 127th) at both ends of the y interval and 38 values between,
             and checks that arguments one step outside each face of the box, and the special values
             lm_powf tests for, are not claimed by lm_powf_unit_claims().

The full runs (stride 1) are recorded in tests/golden/libm_forms_full.txt; lm_powf itself stays
checked against glibc by tests/test_libm_exact.py."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X_LO, X_HI = 0x33800000, 0x3F7FFFEF  # 2^-24, 1 - 1e-6f
N_Y = 40


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("libm_forms") / "libm_ex")
    subprocess.run(["g++", "-O2", "-std=c++17", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-builtin", "-pthread",
                    os.path.join(ROOT, "tools", "libm_exhaustive.cpp"), "-o", exe, "-lm"], check=True, timeout=300)
    return exe


def box(text):
    m = re.search(r"powf_unit x=\[0x([0-9a-f]{8}),0x([0-9a-f]{8})\] y=\[0x([0-9a-f]{8}),0x([0-9a-f]{8})\] ys=(\d+) claimed_outside=(\d+)", text)
    assert m, text
    return [int(g, 16) for g in m.groups()[:4]] + [int(m.group(5)), int(m.group(6))]


def test_powf_unit_matches_lm_powf_on_its_box(checker):
    out = subprocess.run([checker, "powf_unit", "127", "4"], capture_output=True, text=True, timeout=240)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    x_lo, x_hi, y_lo, y_hi, n_y, outside = box(out.stdout)
    assert (x_lo, x_hi) == (X_LO, X_HI) and n_y == N_Y
    assert outside == 0  # nothing outside the box is claimed
    n_x = len(range(0, X_HI - X_LO + 1, 127))
    assert f"powf_unit checked={n_x * N_Y} mismatches=0" in out.stdout


def test_fit_interval_is_the_claimed_one(checker):
    # every 61st c, plus the recorded full run below: the claimed y interval is exactly the range of fit
    out = subprocess.run([checker, "fitrange", "61", "4"], capture_output=True, text=True, timeout=240)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    assert "mismatches=0" in out.stdout


def test_full_run_log(checker):
    text = open(os.path.join(ROOT, "tests", "golden", "libm_forms_full.txt")).read()
    x_lo, x_hi, y_lo, y_hi, n_y, outside = box(text)
    assert (x_lo, x_hi) == (X_LO, X_HI) and n_y == N_Y and outside == 0
    assert f"powf_unit checked={(X_HI - X_LO + 1) * N_Y} mismatches=0" in text
    # the recorded fit range is the y interval of the recorded sweep and of today's build
    m = re.search(r"fitrange lo=0x([0-9a-f]{8}) \S+ hi=0x([0-9a-f]{8})", text)
    assert m and (int(m.group(1), 16), int(m.group(2), 16)) == (y_lo, y_hi)
    assert f"fitrange checked={0x3F7FF972 + 1} mismatches=0" in text  # every c in [0, .9999f]
    now = subprocess.run([checker, "powf_unit", "1000003", "2"], capture_output=True, text=True, timeout=120)
    assert box(now.stdout)[:4] == [x_lo, x_hi, y_lo, y_hi]
    # the single-exit forms of the functions the kernels' hot loops call, against glibc over all 2^32 inputs
    for fn in ["expf", "logf"]:
        assert f"{fn} checked=4294967296 mismatches=0" in text
