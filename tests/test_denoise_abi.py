"""The denoiser's surface without a device (include/simplepath_hip.h, "denoising"): the announcement
in the header, the structs' layouts in C and ctypes, and every refusal of sp_denoiser_create and
sp_denoiser_run in the order the header states, with stand-in pointers that are never read.  The
object touches no device before its first run, so it can be made anywhere; it is made for a device
ordinal no machine has, so a run that is in order ends in SP_ERR_HIP at the device selection, with
or without a GPU, which is how "everything else was accepted" shows."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import simplepath_amd as sp
from simplepath_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "simplepath_hip.h")
NAMES = ("sp_denoiser_create", "sp_denoiser_free", "sp_denoiser_device_bytes", "sp_denoiser_run", "sp_denoiser_run_host")
ARG = _abi.SP_ERR_ARG
ALIGNED, ODD = 0x100000, 0x100002  # stand-in device addresses: validation never reads through them
SLOT = 64 * 3 * 4                  # bytes of one tile slot's colour
NO_DEVICE = 4096                   # an ordinal no machine has: a call that is in order ends at hipSetDevice
POINTERS = ("d_color", "d_albedo", "d_normal", "d_depth", "d_coverage", "d_out")


def test_header_announces_the_surface():
    text = open(HEADER).read()
    assert re.search(r"^#define SP_HAS_DENOISE 1\b", text, re.M)
    assert re.search(r"#define SP_ABI_VERSION 6\b", text)  # new entry points only
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _abi.SIGNATURES and hasattr(sp.lib(), name), name
    for name in ("Denoiser", "DENOISE_GUIDES"):
        assert name in sp.__all__
    # the rule and its consequences are stated where the restatements are written from
    for phrase in ("THE RULE", "never spreads to its neighbours", "passes through unchanged", "ORDINARY STREAM ORDER",
                   "lm_expf", "atomicMin"):
        assert phrase in text, phrase


def fields(struct):
    return [C.sizeof(struct)] + [getattr(struct, name).offset for name, _ in struct._fields_[1:]]


def test_struct_layouts_match_the_compiler(tmp_path):
    structs = (_abi.sp_denoiser_params, _abi.sp_denoise_params, _abi.sp_denoise_stats)
    lines = []
    for s in structs:
        name = s.__name__
        offs = ", ".join(f"offsetof({name}, {f})" for f, _ in s._fields_[1:])
        lines.append(f'  printf("%zu{" %zu" * (len(s._fields_) - 1)}\\n", sizeof({name}), {offs});\n')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "simplepath_hip.h"\nint main(void) {\n' + "".join(lines)
                   + "  return SP_HAS_DENOISE == 1 && SP_DENOISE_DEMODULATE == %d && SP_DENOISE_MAX_ITERATIONS == 8 ? 0 : 1;\n}\n"
                   % _abi.SP_DENOISE_DEMODULATE)
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, timeout=120)
    out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    for s, line in zip(structs, out):
        assert [int(x) for x in line.split()] == fields(s), s.__name__
    assert [C.sizeof(s) for s in structs] == [56, 112, 32]  # the sizes the header states


def create_params(width=20, height=12, **fields_):
    p = _abi.sp_denoiser_params()
    p.struct_size = C.sizeof(p)
    p.width, p.height = width, height
    for k, v in fields_.items():
        setattr(p, k, v)
    return p


def test_create_refuses_in_the_stated_order():
    L = sp.lib()
    h = C.c_void_p()
    create = lambda p: L.sp_denoiser_create(None if p is None else C.byref(p), C.byref(h))
    ids = (C.c_int32 * 3)(0, 5, 2)
    bad_ids = (C.c_int32 * 3)(0, 6, 2)
    twice = (C.c_int32 * 3)(4, 1, 4)
    # 1. null arguments -- before anything in them is looked at
    assert create(None) == ARG and b"null" in L.sp_last_error()
    assert L.sp_denoiser_create(C.byref(create_params()), None) == ARG and b"null" in L.sp_last_error()
    # 2. struct_size and reserved words -- before the counts
    assert create(create_params(struct_size=48, width=0)) == ARG and b"struct_size" in L.sp_last_error()
    for k in range(4):
        p = create_params(width=0)
        p.reserved[k] = 1
        assert create(p) == ARG and b"reserved" in L.sp_last_error()
    # 3. counts, then the tile-list rules
    assert create(create_params(device=-1, width=0)) == ARG and b"device" in L.sp_last_error()
    assert create(create_params(width=0, num_tiles=-1)) == ARG and b"width" in L.sp_last_error()
    assert create(create_params(height=0)) == ARG and b"height" in L.sp_last_error()
    assert create(create_params(tile_ids=bad_ids, num_tiles=-1)) == ARG and b"num_tiles" in L.sp_last_error()
    assert create(create_params(d_tile_ids=ALIGNED, num_tiles=1 << 31)) == ARG and b"num_tiles" in L.sp_last_error()
    assert create(create_params(tile_ids=ids, d_tile_ids=ALIGNED, num_tiles=3)) == ARG and b"not both" in L.sp_last_error()
    assert create(create_params(tile_ids=bad_ids, num_tiles=3)) == ARG and b"out of range" in L.sp_last_error()
    assert create(create_params(tile_ids=twice, num_tiles=3)) == ARG and b"repeated" in L.sp_last_error()
    assert create(create_params(d_tile_ids=ODD, num_tiles=3)) == ARG and b"aligned" in L.sp_last_error()
    assert not h.value  # nothing was made
    # what is in order makes an object, on a machine without a device too; its size is known at once
    for p, slots in ((create_params(), 6), (create_params(tile_ids=ids, num_tiles=3), 3), (create_params(d_tile_ids=ALIGNED, num_tiles=9), 9),
                     (create_params(tile_ids=ids, num_tiles=0), 0)):
        assert create(p) == 0, L.sp_last_error()
        b = C.c_int64(-1)
        assert L.sp_denoiser_device_bytes(h, C.byref(b)) == 0
        listed = 4 * slots if (p.tile_ids or p.d_tile_ids) else 0
        assert b.value == (slots * 64 * 48 + listed + 6 * 4 + 16 if slots else 0)
        L.sp_denoiser_free(h)
    assert L.sp_denoiser_device_bytes(None, C.byref(b)) == ARG
    L.sp_denoiser_free(None)  # as free(NULL)
    with pytest.raises(sp.SimplePathError) as e:
        sp.Denoiser(20, 12, tile_ids=[1, 1])
    assert e.value.code == ARG


def run_params(slots=6, **fields_):
    p = _abi.sp_denoise_params()
    p.struct_size = C.sizeof(p)
    p.iterations = 3
    p.sigma_color = 0.5
    p.d_color, p.d_out = ALIGNED, ALIGNED + 16 * slots * SLOT
    for k, v in fields_.items():
        setattr(p, k, v)
    return p


def stats(size=None):
    st = _abi.sp_denoise_stats()
    st.struct_size = C.sizeof(st) if size is None else size
    return st


@pytest.mark.parametrize("form", ["sp_denoiser_run", "sp_denoiser_run_host"])
def test_run_refuses_in_the_stated_order(form):
    L = sp.lib()
    device_form = form == "sp_denoiser_run"
    dn = sp.Denoiser(20, 12, device=NO_DEVICE)  # 6 slots
    fn = getattr(L, form)
    call = lambda p, st=None, h=dn.handle: fn(h, None if p is None else C.byref(p), None if st is None else C.byref(st))
    accepted = lambda rc: rc == _abi.SP_ERR_HIP  # everything was in order: the call went on to the device
    guides = dict(d_albedo=ALIGNED + SLOT * 1000, d_normal=ALIGNED + SLOT * 2000, d_depth=ALIGNED + SLOT * 3000,
                  d_coverage=ALIGNED + SLOT * 4000)  # (d_out lies 96 slots behind d_color)
    sigmas = dict(sigma_normal=0.3, sigma_depth=0.2, sigma_coverage=0.4)
    assert accepted(call(run_params()))
    assert accepted(call(run_params(**guides, **sigmas, flags=1), stats()))
    # 1. null arguments
    assert call(run_params(struct_size=0), h=None) == ARG and b"null" in L.sp_last_error()
    assert call(None) == ARG and b"null" in L.sp_last_error()
    # 2. struct sizes, reserved words, unknown flags -- before the ranges
    assert call(run_params(struct_size=104, iterations=0)) == ARG and b"sp_denoise_params.struct_size" in L.sp_last_error()
    assert call(run_params(iterations=0), stats(0)) == ARG and b"sp_denoise_stats" in L.sp_last_error()
    assert call(run_params(reserved0=1, iterations=0)) == ARG and b"reserved" in L.sp_last_error()
    for k in range(4):
        p = run_params(iterations=0)
        p.reserved[k] = 1
        assert call(p) == ARG and b"reserved" in L.sp_last_error()
    assert call(run_params(flags=2, iterations=0)) == ARG and b"flags" in L.sp_last_error()
    # 4. iterations, then the sigmas and the floors -- before the pointers
    for it in (0, 9, -1):
        assert call(run_params(iterations=it, sigma_color=0.0)) == ARG and b"iterations" in L.sp_last_error()
    assert accepted(call(run_params(iterations=1))) and accepted(call(run_params(iterations=8)))
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(run_params(sigma_color=bad, d_color=0)) == ARG and b"sigma_color" in L.sp_last_error()
        for guide, sigma in (("d_normal", "sigma_normal"), ("d_depth", "sigma_depth"), ("d_coverage", "sigma_coverage")):
            p = run_params(**{guide: guides[guide], sigma: bad, "d_color": 0})
            assert call(p) == ARG and sigma.encode() in L.sp_last_error()
            assert accepted(call(run_params(**{sigma: bad})))  # not looked at without its guide
    for bad in (-0.5, float("inf"), float("nan")):
        assert call(run_params(albedo_floor=bad, d_color=0)) == ARG and b"albedo_floor" in L.sp_last_error()
        assert call(run_params(depth_floor=bad, d_color=0)) == ARG and b"depth_floor" in L.sp_last_error()
    assert accepted(call(run_params(albedo_floor=0.5, depth_floor=2.0)))
    # 5. missing buffers, then the flag without its guides -- before the alignment
    odd = ODD if device_form else ALIGNED
    assert call(run_params(d_color=0, d_out=odd)) == ARG and b"d_color" in L.sp_last_error()
    assert call(run_params(d_out=0, d_color=odd)) == ARG and b"d_out" in L.sp_last_error()
    for missing in ("d_albedo", "d_coverage"):
        g = dict(guides, **{missing: 0, "d_normal": odd})
        assert call(run_params(flags=1, **g, **sigmas)) == ARG and b"DEMODULATE" in L.sp_last_error()
    # 6. alignment (device pointers only), then a forbidden overlap
    for name in POINTERS:
        p = run_params(**guides, **sigmas)
        setattr(p, name, getattr(p, name) + 2)
        p.d_out = p.d_out if name == "d_out" else p.d_color + 4  # an overlap as well: the alignment is named first
        rc = call(p)
        if name == "d_out" and not device_form:
            assert accepted(rc)  # no alignment is asked of a host array, and this one overlaps nothing
        else:
            assert rc == ARG and (b"aligned" in L.sp_last_error()) == device_form, name
    assert accepted(call(run_params(d_out=ALIGNED)))  # d_out may equal d_color
    assert call(run_params(d_out=ALIGNED + 4)) == ARG and b"overlaps d_color" in L.sp_last_error()
    assert call(run_params(d_out=ALIGNED + 6 * SLOT - 4)) == ARG and b"overlaps d_color" in L.sp_last_error()
    assert accepted(call(run_params(d_out=ALIGNED + 6 * SLOT)))  # adjacent
    for name in POINTERS[1:5]:
        g = dict(guides, **{name: ALIGNED + 16 * 6 * SLOT + 8})
        assert call(run_params(**g, **sigmas)) == ARG and b"d_out overlaps" in L.sp_last_error(), name
    # an empty list succeeds whatever the device is, and launches nothing
    empty = sp.Denoiser(20, 12, tile_ids=[], device=NO_DEVICE)
    st = stats()
    assert call(run_params(d_color=0, d_out=0), st, h=empty.handle) == 0 and st.launches == 0 and st.pixels == 0
    assert call(run_params(iterations=0, d_color=0, d_out=0), h=empty.handle) == ARG
    assert empty.run(np.zeros((0, 64, 3), dtype=np.float32), demodulate=False).shape == (0, 64, 3)
    empty.close()
    dn.close()
    dn.close()  # idempotent


def test_wrapper_checks_shapes():
    with sp.Denoiser(20, 12) as dn:
        assert dn.num_tiles == 6 and dn.device_bytes == 6 * 64 * 48 + 24 + 16
        with pytest.raises(ValueError):
            dn.run(np.zeros((5, 64, 3), dtype=np.float32), demodulate=False)
        with pytest.raises(ValueError):
            dn.run(np.zeros((6, 64, 3), dtype=np.float32), depth=np.zeros((6, 64, 3), dtype=np.float32), demodulate=False)
        with pytest.raises(sp.SimplePathError) as e:
            dn.run(np.zeros((6, 64, 3), dtype=np.float32))  # demodulate without albedo and coverage
        assert e.value.code == ARG
