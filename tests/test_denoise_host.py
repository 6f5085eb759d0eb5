"""The denoiser's expressions (simplepath_amd/csrc/common/sp_denoise.h) on the host:
tests/cpp/denoise_host_main.cpp runs the header the device kernels are made of, in plain loops, over
case files written here, and every output bit and the tap count must equal the numpy restatement of
the rule (tests/_denoise.py, glibc's expf through the oracle).  This closes, without a device, the
link between the rule and the text the kernels compile.  The same program once more under
AddressSanitizer and UBSan."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _denoise as dn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "denoise_host_main.cpp")
FLAGS = ["g++", "-std=c++17", "-mfma", "-ffp-contract=off"]


def build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.run(FLAGS + extra + [SOURCE, "-o", exe], check=True, timeout=600)
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build(tmp_path_factory.mktemp("denoise_host"), "denoise_host", ["-O2"])


def run_case(exe, tmp_path, width, height, ids, buffers, demodulate, **params):
    """the program's (image, taps) on one case"""
    p = dict(dn.DEFAULTS, **params)
    ids = np.asarray(ids, dtype=np.int32)
    n = ids.size
    case, out = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(case, "wb") as f:
        has = [int(buffers.get(g) is not None) for g in dn.GUIDES]
        np.array([width, height, n, p["iterations"], int(demodulate)] + has, dtype=np.int32).tofile(f)
        np.array([p[k] for k in ("sigma_color", "sigma_normal", "sigma_depth", "sigma_coverage", "albedo_floor", "depth_floor")],
                 dtype=np.float32).tofile(f)
        ids.tofile(f)
        for name in ("color",) + dn.GUIDES:
            if buffers.get(name) is not None:
                np.ascontiguousarray(buffers[name], dtype=np.float32).tofile(f)
    r = subprocess.run([exe, case, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"^taps (\d+)$", r.stdout, re.M)
    assert m, r.stdout[-2000:]
    return np.fromfile(out, dtype=np.float32).reshape(n, 64, 3), int(m.group(1)), r


def check_case(exe, tmp_path, width, height, ids, buffers, demodulate=True, **params):
    got, taps, _ = run_case(exe, tmp_path, width, height, ids, buffers, demodulate, **params)
    guides = {g: buffers.get(g) for g in dn.GUIDES}
    ref, ref_taps = dn.denoise(width, height, ids, buffers["color"], demodulate=demodulate, **guides, **dict(dn.DEFAULTS, **params))
    bad = np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32))
    print(f"{width}x{height} {len(ids)} slots: {bad.size} of {got.size} words differ, taps {taps} (restatement {ref_taps})")
    assert bad.size == 0, (bad[:8], got.reshape(-1)[bad[:8]], ref.reshape(-1)[bad[:8]])
    assert taps == ref_taps
    return got, taps


def all_tiles(width, height):
    return np.arange(((width + 7) // 8) * ((height + 7) // 8), dtype=np.int32)


def test_planted_frame_every_bit_and_the_tap_count(program, tmp_path):
    """48x32, four levels (step 8 crosses tiles and leaves the image), every planted special"""
    ids = all_tiles(48, 32)
    b = dn.synthetic(48, 32, ids.size)
    got, taps = check_case(program, tmp_path, 48, 32, ids, b)
    assert 0 < taps < 4 * 25 * 48 * 32
    flat = got.reshape(-1, 3)
    nan_i, inf_i = (int(s) * 64 + int(l) for s, l in zip(*b["planted"]))
    assert np.isnan(flat[nan_i]).all() and np.isposinf(flat[inf_i]).all()  # the centre passes through
    rest = np.delete(flat, [nan_i, inf_i], axis=0)
    assert np.isfinite(rest).all()  # and spreads to no neighbour


@pytest.mark.parametrize("guide", dn.GUIDES[1:] + ("none", "no_demodulation", "floors", "eight_levels"))
def test_each_edge_term_alone_on_a_clipped_frame(program, tmp_path, guide):
    """20x12 (3x2 tiles, clipped in both axes): one guide at a time, none, the flag off, floors of
    the caller's, and the most levels the call takes"""
    ids = all_tiles(20, 12)
    b = dn.synthetic(20, 12, ids.size, seed=7)
    if guide in dn.GUIDES:
        check_case(program, tmp_path, 20, 12, ids, {"color": b["color"], guide: b[guide]}, demodulate=False)
    elif guide == "none":
        check_case(program, tmp_path, 20, 12, ids, {"color": b["color"]}, demodulate=False)
    elif guide == "no_demodulation":
        check_case(program, tmp_path, 20, 12, ids, b, demodulate=False)
    elif guide == "floors":
        check_case(program, tmp_path, 20, 12, ids, b, albedo_floor=0.25, depth_floor=2.5)
    else:
        check_case(program, tmp_path, 20, 12, ids, b, iterations=8)


def test_tile_lists_subset_and_device_list_semantics(program, tmp_path):
    """a permuted subset with absent neighbours (their taps are skipped), and a list with an id
    outside the frame and a repeat (served from its lowest slot)"""
    subset = np.array([17, 2, 9, 23, 0, 10, 14], dtype=np.int32)  # of 6 x 4 tiles
    b = dn.synthetic(48, 32, subset.size, seed=11)
    _, taps = check_case(program, tmp_path, 48, 32, subset, b)
    odd = np.array([4, 1, 99, 4, -3, 0], dtype=np.int32)  # of 3 x 2 tiles
    b = dn.synthetic(20, 12, odd.size, seed=12)
    got, _ = check_case(program, tmp_path, 20, 12, odd, b)
    assert not got[2].view(np.uint32).any() and not got[4].view(np.uint32).any()  # +0 everywhere


def test_denoise_program_under_sanitizers(tmp_path):
    exe = build(tmp_path, "denoise_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    odd = np.array([4, 1, 99, 4, -3, 0], dtype=np.int32)
    b = dn.synthetic(20, 12, odd.size, seed=12)
    _, taps, r = run_case(exe, tmp_path, 20, 12, odd, b, True)
    assert taps > 0
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
