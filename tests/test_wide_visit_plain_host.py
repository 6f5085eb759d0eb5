"""spw::visit_plain against spw::visit<false> on the host (simplepath_amd/csrc/common/sp_wide_visit.h;
tests/cpp/wide_visit_plain_main.cpp): inside visit_plain's contract -- finite origin, finite non-zero
1 / d, limits no NaN, finite node origin, scale bytes <= 254, qlo <= qhi on occupied-and-wanted slots
-- inner, leaf and nearest are equal and t_rest is the same float value, over more than 1e7 pairs of
real wide nodes (both host builders, leaf sizes 1 and 4; scattered, planar, duplicated and point sets)
and synthetic records, with camera-like, random, wildly scaled and in-plane rays.  The program counts
what the pairs inside the contract exercise, and every class must occur.  Rays the predicate rejects
must make the two forms differ somewhere, or the predicate would not be needed.  The same program
once more under AddressSanitizer and UBSan."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "simplepath_amd", "csrc", "host", "sp_bvh.cpp"), os.path.join(ROOT, "tests", "cpp", "wide_visit_plain_main.cpp")]
FLAGS = ["g++", "-std=c++17", "-mfma", "-ffp-contract=off", "-pthread", "-I", os.path.join(ROOT, "include")]
CLASSES = ("inner", "leaf", "second", "equal_min", "in_plane", "zero_dist", "overflow", "tmax_inf", "neg_x", "neg_y", "neg_z")


def build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.run(FLAGS + extra + SOURCES + ["-o", exe], check=True, timeout=600)
    return exe


def check(r, pairs, inside_at_least):
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    for line in ("clean tree: ok", "plain_ray: ok", "0 failing"):
        assert re.search(rf"^{line}$", r.stdout, re.M), r.stdout[-2000:]
    assert re.search(r"^planted swapped bytes: errors \d+ kind 10 ok$", r.stdout, re.M), r.stdout[-2000:]
    assert re.search(r"^planted scale byte: errors \d+ kind 10 ok$", r.stdout, re.M), r.stdout[-2000:]
    m = re.search(r"^(\d+) pairs \((\d+) real nodes\): (\d+) inside the contract, (\d+) rejected rays$", r.stdout, re.M)
    assert m, r.stdout[-2000:]
    n, nodes, inside, rejected = (int(x) for x in m.groups())
    assert n == pairs and nodes > 1000 and inside >= inside_at_least and rejected > pairs // 100
    m = re.search(r"^inside: (.*)$", r.stdout, re.M)
    counts = dict(zip(m.group(1).split()[::2], (int(x) for x in m.group(1).split()[1::2])))
    for c in CLASSES:  # a green run is not vacuous: each class the contract is about occurs
        assert counts[c] > 0, (c, counts)
    assert counts["nan"] == 0  # no slab distance inside the contract is a NaN
    m = re.search(r"^rejected: (\d+) differ$", r.stdout, re.M)
    assert m and int(m.group(1)) > 0, r.stdout[-2000:]  # outside the contract the general form is needed


def test_plain_visit_equals_the_general_form_inside_the_contract(tmp_path):
    exe = build(tmp_path, "wide_visit_plain", ["-O2"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:])
    check(r, 16_000_000, 10_000_000)


def test_plain_visit_program_under_sanitizers(tmp_path):
    exe = build(tmp_path, "wide_visit_plain_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, "400000"], capture_output=True, text=True, timeout=300)
    check(r, 400_000, 250_000)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
