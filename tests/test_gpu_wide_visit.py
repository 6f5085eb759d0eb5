"""The device's wide_visit (sp_path.hpp: node fetch + the one-exit visit of sp_wide_visit.h, compiled
with the library's flags) on 1e5 of the (node, ray) pairs of tests/cpp/wide_visit_main.cpp, once with
a record per lane and once with a record per wave (the two forms of the function, see below): every
output word -- inner, leaf, nearest, the bits of t_rest, without and with NAN_SAFE -- equals the
words of the branching specification that the host program keeps.  No tolerance."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "wide_visit_units")
PAIRS = 100_000


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "wide_visit.mk"], check=True, timeout=600)
    return EXE


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("wide_visit") / "wide_visit_host")
    subprocess.run(["g++", "-std=c++17", "-O2", "-mfma", "-ffp-contract=off", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "simplepath_amd", "csrc", "host", "sp_bvh.cpp"),
                    os.path.join(ROOT, "tests", "cpp", "wide_visit_main.cpp"), "-o", path], check=True, timeout=600)
    return path


def wanted_slots(rows):
    """the occupied-and-wanted mask of each row's record and filter, as the visit computes it"""
    w = rows.astype(np.uint64)
    nz = np.zeros(rows.shape[0], dtype=np.uint64)
    for k in range(8):
        nz |= (((w[:, 6 + k // 4] >> np.uint64(8 * (k % 4))) & np.uint64(0xff)) != 0).astype(np.uint64) << np.uint64(k)
    return ((w[:, 3] >> np.uint64(24)) | nz) & w[:, 28] & np.uint64(0xff)


# dump: every lane its own record, so a wave wants all eight slots and runs the block of eight;
# dumpw: the 64 lanes of a wave share a record and a filter, so the wave steps over the slots that
# nobody wants by scalar branches (sp_wide_visit.h wave_slots) -- the other form of the same function
@pytest.mark.parametrize("mode", ["dump", "dumpw"])
def test_device_visit_equals_the_host_specification(exe, host, tmp_path, mode):
    fin, fwant, fgot = (str(tmp_path / n) for n in ("in.bin", "want.bin", "got.bin"))
    subprocess.run([host, mode, str(PAIRS), fin, fwant], check=True, timeout=120)
    r = subprocess.run([exe, fin, fgot], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, f"wide_visit_units: exit {r.returncode}\n{r.stdout}{r.stderr}"
    assert r.stdout.split() == ["wide_visit", str(PAIRS)]
    rows = np.fromfile(fin, dtype=np.uint32).reshape(PAIRS, 32)
    want = np.fromfile(fwant, dtype=np.uint32).reshape(PAIRS, 8)
    got = np.fromfile(fgot, dtype=np.uint32).reshape(PAIRS, 8)
    slots = wanted_slots(rows)
    full = PAIRS // 64 * 64
    uniform = (slots[:full].reshape(-1, 64) == slots[:full:64, None]).all(axis=1)
    skipping = int((uniform & (slots[:full:64] != 0xff)).sum())
    print(f"{mode}: {PAIRS} pairs: {int((want[:, 0] != 0).sum())} with inner hits, {int((want[:, 1] != 0).sum())} with leaf hits, "
          f"{int((want[:, :4] != want[:, 4:]).any(axis=1).sum())} where NAN_SAFE changes a word; "
          f"{skipping} of {full // 64} waves step over slots")
    assert (want[:, 0] != 0).sum() > PAIRS // 1000 and (want[:, 1] != 0).sum() > PAIRS // 1000
    assert (want[:, :4] != want[:, 4:]).any()  # NaN entry distances: the NAN_SAFE form has something to differ by
    if mode == "dumpw":
        assert uniform.all() and skipping > full // 64 // 2
    else:
        assert skipping < full // 64 // 100
    bad = np.flatnonzero((want != got).any(axis=1))
    hx = lambda a: " ".join(f"{int(v):08x}" for v in a)
    assert bad.size == 0, (f"{bad.size} of {PAIRS} pairs differ; first {bad[0]}:\n  in   {hx(rows[bad[0]])}\n"
                           f"  want {hx(want[bad[0]])}\n  got  {hx(got[bad[0]])}")
