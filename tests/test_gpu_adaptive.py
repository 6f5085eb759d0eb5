"""Adaptive sampling on progress objects (sp_adaptive_round).

The reference side of every test is built without the code under test: the plain progress API gives
each pixel's per-sample radiance exactly (a one-sample pass onto a zeroed sum is 0 + L_i), a numpy
float32 restatement of the issue's arithmetic turns those into running statistics, tile errors and
the selection rule, and the CPU oracle renders the tiles one-shot at the counts the rule gives."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import simplepath_amd as sp
from simplepath_amd import _abi
from tests import _oracle

pytestmark = pytest.mark.gpu

f32 = np.float32
ALL_INTEGRATORS = ["mandelbrot", "brute_force", "brute_force_iterative", "brute_force_iterative_rr", "iterative_rrnee",
                   "direct_lighting", "whitted"]
FLOOR = f32(0.01)  # floor = 0 means this


def load(scene_dir, name, w, h, bvh=0):
    s = sp.Scene.from_file(os.path.join(scene_dir, name))
    s.set_resolution(w, h)
    s.upload(device=0, bvh_mode=bvh)
    return s


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def counts(st):
    return np.array([st.rays, st.shadow_rays, st.samples, st.rng_draws], dtype=np.int64)


def one_shot(s, integrator, spp, ids=None, **kw):
    return sp.render_tiles(s, integrator, spp, ids, pipeline="megakernel", tail_fraction=-1.0, **kw)


def inside_mask(w, h, ids):
    """[tiles, 64] bool: which morton lanes of each slot are pixels of the image"""
    m = np.arange(64)
    dx = (m & 1) | ((m >> 1) & 2) | ((m >> 2) & 4)
    dy = ((m >> 1) & 1) | ((m >> 2) & 2) | ((m >> 3) & 4)
    tw = (w + 7) // 8
    ids = np.asarray(ids, dtype=np.int64)
    x = (ids % tw)[:, None] * 8 + dx[None, :]
    y = (ids // tw)[:, None] * 8 + dy[None, :]
    return (x < w) & (y < h)


def all_ids(w, h):
    return np.arange(((w + 7) // 8) * ((h + 7) // 8), dtype=np.int32)


def per_sample_radiance(s, integrator, n, ids=None):
    """[n, tiles, 64, 3] float32: L_i of every pixel slot, exactly, from plain progress objects.
    Sample i is rendered alone onto a zeroed sum from the state after i samples."""
    out = []
    with sp.Progressive(s, integrator, ids) as a, sp.Progressive(s, integrator, ids) as b:
        for i in range(n):
            if i == 0:
                a.render(1)
                state, done = a.export_state()
                out.append(state["sum"].copy())
                continue
            start = state.copy()
            start["sum"] = 0
            b.import_state(start, i)
            b.render(1)
            out.append(b.export_state()[0]["sum"].copy())
            a.render(1)
            state, done = a.export_state()
            assert done == i + 1
    return np.stack(out).reshape(n, -1, 64, 3)


def luminance(L):
    return ((f32(0.2126) * L[..., 0]) + (f32(0.7152) * L[..., 1])) + (f32(0.0722) * L[..., 2])


class Replay:
    """The issue's arithmetic in numpy float32, every operation rounded on its own."""

    def __init__(self, L, inside):
        self.y = luminance(L.astype(f32))          # [n, tiles, 64]
        self.inside = inside
        t = self.y.shape[1]
        self.mean = np.zeros((t, 64), f32)
        self.m2 = np.zeros((t, 64), f32)
        self.done = np.zeros(t, np.uint32)

    def push(self, t, k):
        for _ in range(k):
            n = int(self.done[t]) + 1
            y = self.y[n - 1, t]
            if n == 1:
                self.mean[t], self.m2[t] = y, f32(0)
            else:
                d = y - self.mean[t]
                mean = self.mean[t] + d / f32(n)
                self.m2[t] = self.m2[t] + d * (y - mean)
                self.mean[t] = mean
            self.done[t] = n

    def errors(self, floor=FLOOR):
        E = np.zeros(self.done.size, f32)
        with np.errstate(all="ignore"):
            for t, n in enumerate(self.done):
                if not self.inside[t].any():
                    continue
                if n < 2:
                    E[t] = np.inf
                    continue
                e = np.sqrt((self.m2[t] / f32(n - 1)) / f32(n)) / (np.abs(self.mean[t]) + f32(floor))
                e = np.where(np.isfinite(e), e, f32(np.inf)).astype(f32)
                E[t] = e[self.inside[t]].max()
        return E

    def round(self, threshold, lo, hi, step, floor=FLOOR):
        """returns (active slots, tile errors before the round)"""
        E = self.errors(floor)
        n = self.done.astype(np.int64)
        active = (n < hi) & ((n < lo) | ~(E <= f32(threshold)))
        for t in np.flatnonzero(active):
            self.push(t, min(step, hi - int(self.done[t])))
        return np.flatnonzero(active), E

    def noise(self):
        mean = np.where(self.inside, self.mean, f32(0))
        m2 = np.where(self.inside, self.m2, f32(0))
        return mean.reshape(-1), m2.reshape(-1)


def check_state(prog, rep, floor=0.0):
    noise, done = prog.export_noise()
    mean, m2 = rep.noise()
    assert np.array_equal(done, rep.done)
    assert same_bits(noise["mean"], mean) and same_bits(noise["m2"], m2)
    assert same_bits(prog.tile_errors(floor), rep.errors(floor if floor else FLOOR))
    assert np.array_equal(prog.tile_samples(), rep.done)


# ---- 1. the statistics are the reference's arithmetic ------------------------------------------

@pytest.mark.parametrize("scene_name,w,h,integrator,n", [
    ("bunny.sp", 24, 16, "direct_lighting", 9),
    ("elf_small.sp", 16, 16, "iterative_rrnee", 6),
    ("bunny.sp", 20, 12, "direct_lighting", 5),  # clipped: lanes outside the image are not in E
])
def test_statistics_match_the_restated_arithmetic(scene_dir, scene_name, w, h, integrator, n):
    s = load(scene_dir, scene_name, w, h, bvh=1)
    inside = inside_mask(w, h, all_ids(w, h))
    assert inside.all() == (w % 8 == 0 and h % 8 == 0)
    L = per_sample_radiance(s, integrator, n)
    assert float(luminance(L).std(axis=0).max()) > 0  # the samples do differ somewhere
    # uniformly, in one call: the image is the plain one, the statistics the replay's
    rep = Replay(L, inside)
    for t in range(rep.done.size):
        rep.push(t, n)
    with sp.Progressive(s, integrator, adaptive=True) as prog:
        img, _ = prog.render(n)
        assert same_bits(img, one_shot(s, integrator, n)[0]) and prog.samples == n
        check_state(prog, rep)
        check_state(prog, rep, floor=0.25)
    # in rounds that select every tile (min = max), two samples at a time, checked at every stop
    rep = Replay(L, inside)
    with sp.Progressive(s, integrator, adaptive=True) as prog:
        while True:
            img, st, res = prog.round(0.0, n, n, 2)
            act, E = rep.round(0.0, n, n, 2)
            assert res.active_tiles == act.size
            check_state(prog, rep)
            if act.size == 0:
                break
        assert same_bits(img, one_shot(s, integrator, n)[0])


# ---- 2. every tile is the oracle's one-shot tile at its own count -------------------------------

ADAPT_SCENE = ("bunny.sp", 40, 64, "direct_lighting")  # under the bunny: glossy floor; above: whole tiles of sky
ADAPT_RULE = dict(threshold=0.3, min_samples=2, max_samples=11, step=3)
_cache = {}


def adapt_reference(scene_dir):
    """per-sample radiance of ADAPT_SCENE (both BVH modes render the same bits: the parity suite)"""
    if "L" not in _cache:
        name, w, h, integrator = ADAPT_SCENE
        _cache["L"] = per_sample_radiance(load(scene_dir, name, w, h), integrator, ADAPT_RULE["max_samples"])
        _cache["L"].setflags(write=False)
    return _cache["L"]


@pytest.mark.parametrize("bvh", [0, 1])
def test_converged_tiles_are_the_oracles_tiles_at_their_counts(scene_dir, bvh):
    name, w, h, integrator = ADAPT_SCENE
    rule = ADAPT_RULE
    L = adapt_reference(scene_dir)
    inside = inside_mask(w, h, all_ids(w, h))
    # the scene must exercise both ends of the rule, judged on the reference side alone
    probe = Replay(L, inside)
    for t in range(probe.done.size):
        probe.push(t, rule["min_samples"])
    E_min = probe.errors()
    for t in range(probe.done.size):
        probe.push(t, rule["max_samples"] - rule["step"] - rule["min_samples"])
    E_late = probe.errors()
    print(f"tiles with E == 0 at {rule['min_samples']} samples: {int((E_min == 0).sum())}; above {rule['threshold']} at "
          f"{rule['max_samples'] - rule['step']}: {int((E_late > f32(rule['threshold'])).sum())} of {E_late.size}")
    assert (E_min == 0).any(), "no whole tile of constant luminance"
    assert (E_late > f32(rule["threshold"])).any(), "no tile still above the threshold one step before max_samples"

    rep = Replay(L, inside)
    s = load(scene_dir, name, w, h, bvh=bvh)
    total = np.zeros(4, np.int64)
    with sp.Progressive(s, integrator, adaptive=True) as prog:
        rounds = 0
        while True:
            img, st, res = prog.round(rule["threshold"], rule["min_samples"], rule["max_samples"], rule["step"])
            act, E = rep.round(rule["threshold"], rule["min_samples"], rule["max_samples"], rule["step"])
            total += counts(st)
            rounds += 1
            assert res.active_tiles == act.size, rounds
            assert np.array_equal(prog.tile_samples(), rep.done), rounds
            assert res.max_error == E.max() and (res.min_done, res.max_done) == (rep.done.min(), rep.done.max())
            assert res.samples_total == int((rep.done.astype(np.int64) * inside.sum(axis=1)).sum())
            if act.size == 0:
                break
        done = prog.tile_samples()
        assert prog.samples == done.max()
    groups = sorted(set(done.tolist()))
    print("per-tile counts:", {c: int((done == c).sum()) for c in groups})
    assert len(groups) >= 3 and groups[0] >= rule["min_samples"] and groups[-1] == rule["max_samples"]
    integ = sp.string_to_integrator_type(integrator)
    rays = shadow = 0
    for c in groups:
        ids = np.flatnonzero(done == c).astype(np.int32)
        ref, rst = _oracle.render(s, integ, c, tile_ids=ids)
        assert same_bits(img[ids], ref), c
        rays += rst["rays"]
        shadow += rst["shadow_rays"]
    assert (int(total[0]), int(total[1])) == (rays, shadow)


# ---- 3. degenerate settings reduce to what exists ----------------------------------------------

@pytest.mark.parametrize("integrator", ALL_INTEGRATORS)
def test_min_equals_max_is_the_one_shot_render(scene_dir, integrator):
    s = load(scene_dir, "closed_room.sp", 40, 24)
    ref, rst = one_shot(s, integrator, 8)
    with sp.Progressive(s, integrator, adaptive=True) as prog:
        img, rounds = prog.converge(0.5, 8, 8, 3)
        assert [r.active_tiles for _, r in rounds] == [15, 15, 15, 0]
        assert np.array_equal(prog.tile_samples(), np.full(15, 8, np.uint32))
    assert same_bits(img, ref)
    assert np.array_equal(sum(counts(st) for st, _ in rounds), counts(rst))


@pytest.mark.parametrize("integrator,waves", [("direct_lighting", 1), ("direct_lighting", 2), ("direct_lighting", 3),
                                              ("iterative_rrnee", 2), ("iterative_rrnee", 4)])
def test_occupancy_variants(scene_dir, integrator, waves):
    s = load(scene_dir, "elf_small.sp", 40, 24)
    ref, rst = one_shot(s, integrator, 7)
    with sp.Progressive(s, integrator, adaptive=True, waves_per_simd=waves) as prog:
        img, rounds = prog.converge(0.0, 7, 7, 4)
    assert same_bits(img, ref) and np.array_equal(sum(counts(st) for st, _ in rounds), counts(rst))


@pytest.mark.parametrize("integrator", ["direct_lighting", "iterative_rrnee", "whitted"])
def test_uniform_passes_on_an_adaptive_object(scene_dir, integrator):
    s = load(scene_dir, "elf_small.sp", 40, 24, bvh=1)
    with sp.Progressive(s, integrator) as plain, sp.Progressive(s, integrator, adaptive=True) as prog:
        assert prog.device_bytes - plain.device_bytes == 15 * (64 * 8 + 16) + 4
        for k in (1, 3, 4):
            ref, rst = plain.render(k)
            img, st = prog.render(k)
            assert same_bits(img, ref) and np.array_equal(counts(st), counts(rst))
        assert prog.samples == plain.samples == 8
        a, b = prog.export_state(), plain.export_state()
        assert a[1] == b[1] and a[0].tobytes() == b[0].tobytes()


def test_threshold_zero_keeps_only_constant_tiles(scene_dir):
    name, w, h, integrator = ADAPT_SCENE
    L = adapt_reference(scene_dir)
    inside = inside_mask(w, h, all_ids(w, h))
    probe = Replay(L, inside)
    for t in range(probe.done.size):
        probe.push(t, 2)
    constant = probe.errors() == 0
    assert constant.any() and not constant.all()
    s = load(scene_dir, name, w, h)
    with sp.Progressive(s, integrator, adaptive=True) as prog:
        img, rounds = prog.converge(0.0, 2, 6, 2)
        done = prog.tile_samples()
    assert np.array_equal(done, np.where(constant, 2, 6))
    assert [r.active_tiles for _, r in rounds] == [constant.size, int((~constant).sum()), int((~constant).sum()), 0]
    assert same_bits(img[constant], one_shot(s, integrator, 2, np.flatnonzero(constant).astype(np.int32))[0])
    assert same_bits(img[~constant], one_shot(s, integrator, 6, np.flatnonzero(~constant).astype(np.int32))[0])


# ---- 4. compaction and lists at awkward sizes (Mandelbrot: cheap, and its tile errors vary) ------

MB_W, MB_H, MB_MAX = 264, 256, 5
MB_RULE = dict(threshold=0.02, min_samples=2, max_samples=MB_MAX, step=1)


def mandelbrot_reference(scene_dir):
    """[MB_MAX, 1056, 64, 3]: Mandelbrot draws nothing, so sample i needs only the R2 index"""
    if "mb" not in _cache:
        s = load(scene_dir, "bunny.sp", MB_W, MB_H)
        out = []
        with sp.Progressive(s, "mandelbrot") as b:
            zero = np.zeros(b.num_tiles * 64, dtype=sp.PIXEL_STATE_DTYPE)
            for i in range(MB_MAX):
                b.import_state(zero, i)
                b.render(1)
                out.append(b.export_state()[0]["sum"].copy())
        _cache["mb"] = np.stack(out).reshape(MB_MAX, -1, 64, 3)
        _cache["mb"].setflags(write=False)
    return _cache["mb"]


def run_rule(prog, rule):
    """the device's (active_tiles, counts) after every round until it converges"""
    log = []
    while True:
        _, _, res = prog.round(rule["threshold"], rule["min_samples"], rule["max_samples"], rule["step"])
        log.append((res.active_tiles, prog.tile_samples().tolist()))
        if res.active_tiles == 0:
            return log


def replay_rule(rep, rule):
    log = []
    while True:
        act, _ = rep.round(rule["threshold"], rule["min_samples"], rule["max_samples"], rule["step"])
        log.append((act.size, rep.done.tolist()))
        if act.size == 0:
            return log


def mandelbrot_ids(case):
    rng = np.random.default_rng(7)
    total = all_ids(MB_W, MB_H)
    if case == "one":
        return total[500:501]
    if case == "63":
        return total[470:533]
    if case == "65":
        return total[470:535]
    if case == "shuffled_with_duplicates":
        ids = rng.permutation(total)[:300]
        return np.concatenate([ids, ids[:77]])[rng.permutation(377)].astype(np.int32)
    return None  # the whole frame: 1056 tiles, more than the compaction's 1024 per step


@pytest.mark.parametrize("case", ["one", "63", "65", "frame", "shuffled_with_duplicates", "device_list"])
def test_lists_and_compaction(scene_dir, case):
    L = mandelbrot_reference(scene_dir)
    s = load(scene_dir, "bunny.sp", MB_W, MB_H)
    ids = mandelbrot_ids("shuffled_with_duplicates" if case == "device_list" else case)
    slots = all_ids(MB_W, MB_H) if ids is None else ids
    expect = replay_rule(Replay(L[:, slots], inside_mask(MB_W, MB_H, slots)), MB_RULE)
    final = np.array(expect[-1][1])
    assert len(expect) > 2 and (len(set(final.tolist())) > 1 or slots.size == 1), "the rule selects nothing of interest"
    runs = []
    for _ in range(2):
        kw = {}
        if case == "device_list":
            d_ids = torch.from_numpy(ids).to("cuda:0")
            kw = dict(d_tile_ids=d_ids.data_ptr(), num_tiles=ids.size)
        elif ids is not None:
            kw = dict(tile_ids=ids)
        with sp.Progressive(s, "mandelbrot", adaptive=True, **kw) as prog:
            runs.append(run_rule(prog, MB_RULE))
    assert runs[0] == expect
    assert runs[1] == runs[0]


def test_forced_tile_order_keeps_the_selection(scene_dir):
    # Only DirectLighting and IterativeRRNEE have a probe kernel, and it runs only with more tiles than
    # persistent waves: too many for per-sample references.  The order permutes the queue and the
    # active list, nothing else: rounds on a probed object equal those of one in queue order.
    s = load(scene_dir, "bunny.sp", 640, 512)
    rule = (0.05, 2, 6, 2)
    logs = []
    for factor in (-1.0, 2.0, 2.0):
        with sp.Progressive(s, "direct_lighting", adaptive=True, tile_order_factor=factor) as prog:
            log = []
            for _ in range(4):
                img, st, res = prog.round(*rule)
                log.append((res.active_tiles, st.launches, tuple(counts(st)[:3].tolist()), prog.tile_samples().tobytes(),
                            img.tobytes()))
            logs.append(log)
    assert [r[1] for r in logs[0]] == [4, 4, 4, 4] and [r[1] for r in logs[1]] == [6, 4, 4, 4]
    assert 0 < logs[0][2][0] < 5120 and logs[0][3][0] == 0
    strip = lambda log: [(r[0],) + r[2:] for r in log]
    assert strip(logs[1]) == strip(logs[0]) and logs[2] == logs[1]


# ---- 5. boundary ---------------------------------------------------------------------------------

def test_queued_rounds_and_a_dependent_kernel(scene_dir):
    name, w, h, integrator = ADAPT_SCENE
    s = load(scene_dir, name, w, h)
    rule = (0.05, 2, 11, 3)
    with sp.Progressive(s, integrator, adaptive=True) as prog:
        imgs = [prog.round(*rule)[0] for _ in range(3)]
        want = prog.tile_samples()
    dev = torch.device("cuda:0")
    outs = [torch.zeros((imgs[0].shape[0], 64, 3), dtype=torch.float32, device=dev) for _ in range(3)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with sp.Progressive(s, integrator, adaptive=True) as prog:
        with torch.cuda.stream(stream):
            for out in outs:
                assert prog.round(*rule, out_ptr=out.data_ptr(), stream=stream.cuda_stream, stats=False,
                                  result=False) == (None, None, None)
            both = outs[0] + outs[2]  # a dependent kernel behind them, without a host wait
        stream.synchronize()
        assert np.array_equal(prog.tile_samples(), want) and len(set(want.tolist())) > 1
    for out, img in zip(outs, imgs):
        assert same_bits(out.cpu().numpy(), img)
    assert np.array_equal(both.cpu().numpy(), imgs[0] + imgs[2])


def test_checkpoint_round_trip_into_a_fresh_scene(scene_dir):
    name, w, h, integrator = ADAPT_SCENE
    rule = (0.05, 2, 11, 3)
    s = load(scene_dir, name, w, h, bvh=1)
    with sp.Progressive(s, integrator, adaptive=True) as prog:
        prog.round(*rule)
        prog.round(*rule)
        state, n = prog.export_state()
        noise, done = prog.export_noise()
        assert n == done.max() and len(set(done.tolist())) > 1
        ref_img, ref_rounds = prog.converge(*rule)
        ref_done = prog.tile_samples()
    del s
    s2 = load(scene_dir, name, w, h, bvh=1)
    with sp.Progressive(s2, integrator, adaptive=True) as prog:
        prog.import_state(state, n)
        assert np.array_equal(prog.tile_samples(), np.full(done.size, n, np.uint32))
        L = sp.lib()
        for count, tiles in ((noise.size - 1, done.size), (noise.size, done.size - 1)):
            assert L.sp_adaptive_import(prog._h, C.c_void_p(noise.ctypes.data), count,
                                        done.ctypes.data_as(C.POINTER(C.c_uint32)), tiles) == _abi.SP_ERR_ARG
        prog.import_noise(noise, done)
        assert np.array_equal(prog.tile_samples(), done) and prog.samples == n
        img, rounds = prog.converge(*rule)
        assert same_bits(img, ref_img) and np.array_equal(prog.tile_samples(), ref_done)
        assert [r.active_tiles for _, r in rounds] == [r.active_tiles for _, r in ref_rounds]
        assert all(np.array_equal(counts(a), counts(b)) for (a, _), (b, _) in zip(rounds, ref_rounds))


def test_errors_and_invalidation(scene_dir):
    s = load(scene_dir, "bunny.sp", 24, 16)
    L = sp.lib()
    good = sp.Progressive._adaptive_params(0.1, 1, 4, 1, 0.0)
    with sp.Progressive(s, "direct_lighting") as plain:
        buf = np.zeros(64, np.uint32)
        with pytest.raises(sp.SimplePathError) as e:
            plain.round(0.1, 1, 4, 1)
        assert e.value.code == _abi.SP_ERR_STATE
        for call in (plain.tile_samples, plain.tile_errors, plain.export_noise):
            with pytest.raises(sp.SimplePathError) as e:
                call()
            assert e.value.code == _abi.SP_ERR_STATE
        assert L.sp_adaptive_round(plain._h, C.byref(good), None, None, None, None) == _abi.SP_ERR_STATE
    prog = sp.Progressive(s, "direct_lighting", adaptive=True)
    bad = [dict(threshold=float("nan")), dict(threshold=-1.0), dict(threshold=float("inf")), dict(step=0),
           dict(min_samples=5, max_samples=4), dict(max_samples=0, min_samples=0), dict(floor=float("nan")),
           dict(struct_size=0), dict(struct_size=C.sizeof(_abi.sp_adaptive_params) + 4)]
    for change in bad:
        p = sp.Progressive._adaptive_params(0.1, 1, 4, 1, 0.0)
        for k, v in change.items():
            setattr(p, k, v)
        assert L.sp_adaptive_round(prog._h, C.byref(p), None, None, None, None) == _abi.SP_ERR_ARG, change
    p = sp.Progressive._adaptive_params(0.1, 1, 4, 1, 0.0)
    p.reserved[1] = 1
    assert L.sp_adaptive_round(prog._h, C.byref(p), None, None, None, None) == _abi.SP_ERR_ARG
    assert L.sp_adaptive_round(None, C.byref(good), None, None, None, None) == _abi.SP_ERR_ARG
    assert L.sp_adaptive_round(prog._h, None, None, None, None, None) == _abi.SP_ERR_ARG
    small = np.zeros(prog.num_tiles - 1, np.uint32)
    assert L.sp_adaptive_tile_samples(prog._h, small.ctypes.data_as(C.POINTER(C.c_uint32)), small.size) == _abi.SP_ERR_ARG
    assert prog.samples == 0 and not prog.tile_samples().any()  # the refused calls rendered nothing
    _, _, res = prog.round(0.1, 1, 4, 1)
    assert res.active_tiles == prog.num_tiles and res.max_error == np.inf
    s.set_resolution(24, 16)
    for call in (lambda: prog.round(0.1, 1, 4, 1), prog.tile_samples, prog.tile_errors, prog.export_noise,
                 lambda: prog.render(1)):
        with pytest.raises(sp.SimplePathError) as e:
            call()
        assert e.value.code == _abi.SP_ERR_STATE
    prog.close()


def test_one_shot_renders_unchanged_beside_an_adaptive_object(scene_dir):
    s = load(scene_dir, "bunny.sp", 64, 40)
    before, bst = sp.render_tiles(s, "direct_lighting", 8)
    with sp.Progressive(s, "direct_lighting", adaptive=True) as prog:
        prog.round(0.05, 2, 8, 3)
        mid, mst = sp.render_tiles(s, "direct_lighting", 8)
        img, _ = prog.converge(0.05, 8, 8, 3)
    after, ast = sp.render_tiles(s, "direct_lighting", 8)
    assert same_bits(before, mid) and same_bits(before, after) and same_bits(img, before)
    assert np.array_equal(counts(bst), counts(mst)) and np.array_equal(counts(bst), counts(ast))
    assert (bst.pipeline, bst.launches) == (ast.pipeline, ast.launches)
