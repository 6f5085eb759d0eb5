"""The one-exit visit of an 8-wide node (simplepath_amd/csrc/common/sp_wide_visit.h) against the
branching wide_visit + slab_box it replaced, on the host: tests/cpp/wide_visit_main.cpp keeps the old
form as the specification and compares inner, leaf, nearest and the bits of t_rest under both
NAN_SAFE values, on real wide nodes (both builders, several leaf sizes, planar / duplicated / point
sets; camera-like, random and in-box-plane rays) and on synthetic records (random bytes, every
empty / leaf / inner slot pattern, filters, duplicated and zero-extent child boxes; ray components
+-0, denormals, infinities, NaN, an origin exactly in a decoded plane, tmax FLT_MAX and +inf).
1.2e7 pairs in the plain build; the same program once more under AddressSanitizer and UBSan."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "simplepath_amd", "csrc", "host", "sp_bvh.cpp"), os.path.join(ROOT, "tests", "cpp", "wide_visit_main.cpp")]
FLAGS = ["g++", "-std=c++17", "-mfma", "-ffp-contract=off", "-pthread", "-I", os.path.join(ROOT, "include")]


def build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.run(FLAGS + extra + SOURCES + ["-o", exe], check=True, timeout=600)
    return exe


def check(r, pairs):
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert re.search(r"^nonzero_bytes: ok$", r.stdout, re.M), r.stdout[-2000:]
    assert re.search(r"^0 failing$", r.stdout, re.M), r.stdout[-2000:]
    m = re.search(r"^(\d+) pairs \((\d+) real nodes\): (\d+) with inner hits, (\d+) with leaf hits, (\d+) with a ranked rest, "
                  r"(\d+) where NAN_SAFE changes a word", r.stdout, re.M)
    assert m, r.stdout[-2000:]
    n, nodes, inner, leaf, rest, nan_safe = (int(x) for x in m.groups())
    assert n == pairs and nodes > 1000
    # the inputs reach what the contract is about: hits of both kinds, an ordering with a rest, NaN distances
    assert min(inner, leaf, rest, nan_safe) > pairs // 1000, r.stdout[-2000:]


def test_new_visit_equals_the_branching_form(tmp_path):
    exe = build(tmp_path, "wide_visit", ["-O2"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-1000:])
    check(r, 12_000_000)


def test_wide_visit_program_under_sanitizers(tmp_path):
    exe = build(tmp_path, "wide_visit_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, "400000"], capture_output=True, text=True, timeout=300)
    check(r, 400_000)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
