"""The plain node visit on the device (sp_wide_visit.h visit_plain; sp_path.hpp SP_VISIT_PLAIN), through
tests/cpp/wide_visit_plain_units.hip built once with SP_VISIT_PLAIN=1 (the library's default) and once
with 0 (the walks before the plain form).

  * Visits: spw::visit_plain on 1e5 (node, ray) pairs inside its contract, dumped by
    tests/cpp/wide_visit_plain_main.cpp, against that program's spw::visit<false> words: inner, leaf and
    nearest equal, t_rest the same float value.  The other build runs spw::visit<false> on the same
    rows and must give the host's words bit for bit.
  * Walks: wide_closest and wide_any over one tree four wide levels deep (600 triangles), 256 rays =
    four waves: plain rays (the wave votes plain), plain rays but for one lane with d.y = 0 that starts
    in a box plane (the wave votes general), axis-parallel rays (no lane is plain), and rays that start
    exactly in decoded planes of the root's children with plain directions (plain, with slab distances
    of zero).  Hit primitive, the bits of t and the any-hit answer are equal between the two builds,
    lane for lane: a lane's answer does not depend on its wave's vote.

The merged-query walk of IterativeRRNEE is not reached by the unit program (its queries are posted by
integrate()'s own LDS bookkeeping); the rrnee tests of the suite run it with the vote."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
PAIRS = 100_000


@pytest.fixture(scope="module")
def exes():
    paths = [os.path.join(BUILD, f"wide_visit_plain_units_{k}") for k in (0, 1)]
    if not all(os.path.exists(p) for p in paths):
        subprocess.run(["make", "-s", "-j", "2", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "wide_visit_plain.mk"], check=True, timeout=600)
    return paths


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("wide_visit_plain") / "wide_visit_plain_host")
    subprocess.run(["g++", "-std=c++17", "-O2", "-mfma", "-ffp-contract=off", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "simplepath_amd", "csrc", "host", "sp_bvh.cpp"),
                    os.path.join(ROOT, "tests", "cpp", "wide_visit_plain_main.cpp"), "-o", path], check=True, timeout=600)
    return path


def run(exe, mode, fin, fout, expect):
    r = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, f"{os.path.basename(exe)} {mode}: exit {r.returncode}\n{r.stdout}{r.stderr}"
    assert r.stdout.split() == expect, r.stdout


def test_device_plain_visit_equals_the_general_form(exes, host, tmp_path):
    fin, fwant = str(tmp_path / "in.bin"), str(tmp_path / "want.bin")
    subprocess.run([host, "dump", str(PAIRS), fin, fwant], check=True, timeout=120)
    want = np.fromfile(fwant, dtype=np.uint32).reshape(PAIRS, 4)
    got = []
    for k, exe in enumerate(exes):
        fgot = str(tmp_path / f"got{k}.bin")
        run(exe, "visits", fin, fgot, ["visits", str(PAIRS), "plain", str(k)])
        got.append(np.fromfile(fgot, dtype=np.uint32).reshape(PAIRS, 4))
    inner, leaf = int((want[:, 0] != 0).sum()), int((want[:, 1] != 0).sum())
    second = int(((want[:, 0] & (want[:, 0] - 1)) != 0).sum())
    zero_sign = int(((got[1][:, 3] != want[:, 3]) & (got[1][:, 3].view(np.float32) == want[:, 3].view(np.float32))).sum())
    print(f"{PAIRS} pairs: {inner} with inner hits, {leaf} with leaf hits, {second} with two or more inner hits, "
          f"{zero_sign} where t_rest is the other zero")
    assert min(inner, leaf, second) > PAIRS // 1000
    hx = lambda a: " ".join(f"{int(v):08x}" for v in a)
    # the general form on the device: the host's words
    bad = np.flatnonzero((got[0] != want).any(axis=1))
    assert bad.size == 0, f"visit<false>: {bad.size} pairs differ; first {bad[0]}: want {hx(want[bad[0]])} got {hx(got[0][bad[0]])}"
    # the plain form: the contract
    differ = (got[1][:, :3] != want[:, :3]).any(axis=1) | (got[1][:, 3].view(np.float32) != want[:, 3].view(np.float32))
    bad = np.flatnonzero(differ)
    assert bad.size == 0, f"visit_plain: {bad.size} pairs differ; first {bad[0]}: want {hx(want[bad[0]])} got {hx(got[1][bad[0]])}"


def test_walks_answer_the_same_whatever_the_vote(exes, host, tmp_path):
    fwalk = str(tmp_path / "walk.bin")
    r = subprocess.run([host, "walk", fwalk], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    head = np.fromfile(fwalk, dtype=np.uint32, count=4)
    records, slots, depth, rays = (int(x) for x in head)
    assert depth >= 3 and rays == 256 and slots == 600
    out = []
    for k, exe in enumerate(exes):
        fgot = str(tmp_path / f"walk{k}.bin")
        run(exe, "walks", fwalk, fgot, ["walks", str(rays), "plain", str(k)])
        out.append(np.fromfile(fgot, dtype=np.uint32).reshape(rays, 3))
    general, plain = out
    hit = general[:, 0] != 0xffffffff
    per_wave = hit.reshape(4, 64).sum(axis=1)
    print(f"tree: {records} records, depth {depth}; closest hits per wave {per_wave.tolist()}, any hits {int(general[:, 2].sum())}")
    # every wave finds something and misses something: the walks went down and came back
    assert (per_wave > 4).all() and (per_wave < 64).all()
    assert (general[hit, 0] < slots).all() and set(np.unique(general[:, 2])) == {0, 1}
    bad = np.flatnonzero((general != plain).any(axis=1))
    assert bad.size == 0, (f"{bad.size} rays differ between the builds; first: ray {bad[0]} (wave {bad[0] // 64}, lane {bad[0] % 64}) "
                           f"general {general[bad[0]].tolist()} plain {plain[bad[0]].tolist()}")
