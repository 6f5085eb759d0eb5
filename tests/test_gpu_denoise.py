"""The denoiser on the device (sp_denoiser_run, sp_denoise.hip) against the numpy
restatement of the rule (tests/_denoise.py, glibc's expf through the oracle): every output bit and
the count of taps, on synthetic buffers with planted specials, with each edge term alone, through
the three forms of the tile list, and on what render_tiles and Scene.features really write.  Then
that it denoises (a strict inequality against a 256-spp render) and the plumbing: guard words,
d_out == d_color, stream order with the render and the features, repeated runs, empty work."""
import numpy as np
import pytest
import torch

import simplepath_amd as sp
from tests import _denoise as dn, _lbvh_sets, _ray_query as rq

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 4  # words on either side of every device buffer
FILL = 0x5A5A5A5A
WORDS = {"color": 3, "albedo": 3, "normal": 3, "depth": 1, "coverage": 1, "out": 3}
# the sigmas of test_it_denoises, chosen on the CPU with the restatement on the oracle's 4-spp and
# 256-spp images of `extra` at 48 x 32: relL2 0.05689 against the noisy 0.06218
CHOSEN = dict(iterations=1, sigma_color=0.1, sigma_normal=0.3, sigma_depth=0.3, sigma_coverage=0.3)


def assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == F, (what, got.shape, want.shape)
    g, w = got.view(np.uint32).reshape(-1), want.view(np.uint32).reshape(-1)
    bad = np.flatnonzero(g != w)
    print(f"{what}: {bad.size} of {g.size} words differ")
    assert bad.size == 0, f"{what}: first {bad[:6]}: {got.reshape(-1)[bad[:6]]} != {want.reshape(-1)[bad[:6]]}"


def restated(width, height, ids, buffers, demodulate=True, **params):
    guides = {g: buffers.get(g) for g in dn.GUIDES}
    return dn.denoise(width, height, ids, buffers["color"], demodulate=demodulate, **guides, **dict(dn.DEFAULTS, **params))


# ---------------------------------------------------------------- 1. synthetic buffers
def test_planted_frame_every_bit_and_the_tap_count():
    """48 x 32, four levels: step 8 reaches 16 pixels, so taps cross several tiles and leave the image"""
    b = dn.synthetic(48, 32, 24)
    want, want_taps = restated(48, 32, None, b)
    with sp.Denoiser(48, 32) as den:
        guides = {g: b[g] for g in dn.GUIDES}
        got, st = den.run(b["color"], **guides, **dn.DEFAULTS, stats=True)
        assert st["launches"] == 1 + 1 + 4  # the first run builds the map; then prepare and four levels
        got2, st2 = den.run(b["color"], **guides, **dn.DEFAULTS, stats=True)
        assert st2["launches"] == 1 + 4
    assert_bits(got, want, "48x32 planted")
    assert got2.tobytes() == got.tobytes()  # two runs on one object
    assert st["pixels"] == st2["pixels"] == 48 * 32
    print(f"taps {st['taps']} (restatement {want_taps}) of {4 * 25 * 48 * 32}")
    assert st["taps"] == st2["taps"] == want_taps
    flat = got.reshape(-1, 3)
    nan_i, inf_i = (int(s) * 64 + int(l) for s, l in zip(*b["planted"]))
    assert np.isnan(flat[nan_i]).all() and np.isposinf(flat[inf_i]).all()  # the centre passes through
    assert np.isfinite(np.delete(flat, [nan_i, inf_i], axis=0)).all()      # and spreads to no neighbour


# ---------------------------------------------------------------- 2. each edge term alone, and all together
@pytest.mark.parametrize("which", dn.GUIDES[1:] + ("none", "all_without_demodulation", "all", "floors_and_eight_levels"))
def test_each_edge_term_on_a_clipped_frame(which):
    """20 x 12: 3 x 2 tiles, clipped in both axes"""
    b = dn.synthetic(20, 12, 6, seed=7)
    params, demodulate = {}, False
    if which in dn.GUIDES:
        given = {"color": b["color"], which: b[which]}
    elif which == "none":
        given = {"color": b["color"]}
    else:
        given = {k: b[k] for k in ("color",) + dn.GUIDES}
        demodulate = which != "all_without_demodulation"
        if which == "floors_and_eight_levels":
            params = dict(iterations=8, albedo_floor=0.25, depth_floor=2.5)
    want, want_taps = restated(20, 12, None, given, demodulate, **params)
    with sp.Denoiser(20, 12) as den:
        got, st = den.run(**given, **dict(dn.DEFAULTS, **params), demodulate=demodulate, stats=True)
    assert_bits(got, want, which)
    assert st["taps"] == want_taps and st["pixels"] == 20 * 12
    inside = dn.layout(20, 12, None)[2]
    assert not got.view(np.uint32)[~inside].any()  # lanes outside the image: +0


# ---------------------------------------------------------------- 3. tile lists
def device_buffers(n_tiles, names=tuple(WORDS)):
    return {k: torch.full((n_tiles * 64 * WORDS[k] + 2 * GUARD,), FILL, dtype=torch.int32, device="cuda:0") for k in names}


def fill(bufs, host):
    for k, v in host.items():
        if k in bufs:
            bufs[k][GUARD:-GUARD] = torch.from_numpy(np.ascontiguousarray(v, dtype=F).reshape(-1).view(np.int32).copy()).cuda()


def pointers(bufs, names):
    return {k + "_ptr": bufs[k].data_ptr() + 4 * GUARD for k in names}


def payload(buf, shape):
    return buf.cpu().numpy()[GUARD:-GUARD].view(F).reshape(shape)


def guards_intact(buf):
    a = buf.cpu().numpy()
    return bool((a[:GUARD] == FILL).all() and (a[-GUARD:] == FILL).all())


def test_a_permuted_subset_skips_the_taps_of_absent_tiles():
    subset = np.array([17, 2, 9, 23, 0, 10, 14], dtype=np.int32)  # of 6 x 4 tiles: listed tiles with absent neighbours
    b = dn.synthetic(48, 32, subset.size, seed=11)
    want, want_taps = restated(48, 32, subset, b)  # from the subset only, not from a full-frame filter
    with sp.Denoiser(48, 32, tile_ids=subset) as den:
        got, st = den.run(**{k: b[k] for k in ("color",) + dn.GUIDES}, **dn.DEFAULTS, stats=True)
    assert_bits(got, want, "subset")
    assert st["taps"] == want_taps and st["pixels"] == subset.size * 64


def test_a_device_list_with_an_id_outside_the_frame_and_a_repeat():
    ids = np.array([4, 1, 99, 4, -3, 0], dtype=np.int32)  # of 3 x 2 tiles; the two slots of tile 4 hold different data
    b = dn.synthetic(20, 12, ids.size, seed=12)
    want, want_taps = restated(20, 12, ids, b)
    d_ids = torch.from_numpy(ids).cuda()
    bufs = device_buffers(ids.size)
    fill(bufs, b)
    torch.cuda.synchronize()
    with sp.Denoiser(20, 12, d_tile_ids=d_ids.data_ptr(), num_tiles=ids.size) as den:
        st = den.run_device(**pointers(bufs, WORDS), **dn.DEFAULTS, stats=True)
        again = den.run_device(**pointers(bufs, WORDS), **dn.DEFAULTS, stats=True)
    got = payload(bufs["out"], (ids.size, 64, 3))
    assert_bits(got, want, "device list")
    assert st["taps"] == again["taps"] == want_taps
    assert not got[2].view(np.uint32).any() and not got[4].view(np.uint32).any()  # outside the frame: +0
    assert all(guards_intact(v) for v in bufs.values())


# ---------------------------------------------------------------- 4. the real pipeline
@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("denoise"))
    return {"mixed": _lbvh_sets.write_all(d)["mixed"][0], "extra": rq.write_extra_scene(d)}


def load(path, size):
    s = sp.Scene.from_file(path)
    s.set_resolution(*size)
    s.upload(device=0, bvh_mode=1)
    return s


@pytest.mark.parametrize("name,size", [("extra", (48, 32)), ("mixed", (20, 12))])
def test_render_features_denoise_match_the_restatement(paths, name, size):
    scene = load(paths[name], size)
    noisy, _ = sp.render_tiles(scene, "direct_lighting", 4)
    f = scene.features(4)
    with sp.Denoiser.for_scene(scene) as den:
        got, st = den.run(noisy, **f, **dn.DEFAULTS, stats=True)
    want, want_taps = dn.denoise(*size, None, noisy, **{g: f[g] for g in dn.GUIDES}, **dn.DEFAULTS)
    assert_bits(got, want, f"{name} {size}")
    assert st["taps"] == want_taps
    assert got.tobytes() != noisy.tobytes()


# ---------------------------------------------------------------- 5. it denoises
def test_it_denoises(paths):
    """relL2(denoised 4 spp, truth) < relL2(noisy 4 spp, truth), truth = 256 spp: strict, no margin.
    On the CPU (restatement on the oracle's images, sphere normals left zero): 0.05689 < 0.06218;
    on one MI355X: 0.05646 < 0.06217."""
    scene = load(paths["extra"], (48, 32))
    truth, _ = sp.render_tiles(scene, "direct_lighting", 256)
    noisy, _ = sp.render_tiles(scene, "direct_lighting", 4)
    with sp.Denoiser.for_scene(scene) as den:
        clean = den.run(noisy, **scene.features(4), **CHOSEN)
    e_noisy, e_clean = dn.relative_l2(noisy, truth), dn.relative_l2(clean, truth)
    print(f"relL2 against 256 spp: noisy 4 spp {e_noisy:.5f}, denoised 4 spp {e_clean:.5f}")
    assert e_clean < e_noisy


# ---------------------------------------------------------------- 6. plumbing
def test_guards_aliasing_and_the_host_form():
    b = dn.synthetic(48, 32, 24)
    host = {k: b[k] for k in ("color",) + dn.GUIDES}
    bufs = device_buffers(24)
    fill(bufs, host)
    torch.cuda.synchronize()
    with sp.Denoiser(48, 32) as den:
        want = den.run(**host, **dn.DEFAULTS)  # the host form
        assert den.run_device(**pointers(bufs, WORDS), **dn.DEFAULTS) is None  # only enqueued
        torch.cuda.synchronize()
        assert all(guards_intact(v) for v in bufs.values())
        for k in ("color",) + dn.GUIDES:  # the inputs are left as they were
            assert payload(bufs[k], (-1,)).tobytes() == np.ascontiguousarray(host[k]).tobytes(), k
        apart = payload(bufs["out"], (24, 64, 3))
        assert apart.tobytes() == want.tobytes()  # the host and the device form agree
        # d_out == d_color gives the bytes of the non-aliased call
        names = [k for k in WORDS if k != "out"]
        p = pointers(bufs, names)
        den.run_device(out_ptr=p["color_ptr"], **p, **dn.DEFAULTS, stats=True)
        assert payload(bufs["color"], (24, 64, 3)).tobytes() == apart.tobytes()
        assert all(guards_intact(v) for v in bufs.values())
        with pytest.raises(sp.SimplePathError) as e:  # any other overlap is refused, and changes nothing
            den.run_device(out_ptr=p["color_ptr"] + 4, **p, **dn.DEFAULTS)
        assert e.value.code == -3
        assert den.device_bytes == 24 * 64 * 48 + 24 * 4 + 16


def test_render_features_denoise_on_one_stream(paths):
    """enqueued on one non-default stream with no host wait in between = the synchronised sequence"""
    scene = load(paths["extra"], (48, 32))
    names = ("color", "albedo", "normal", "depth", "coverage", "out")
    ref = device_buffers(24, names)
    p = pointers(ref, names)
    feats = {k: p[k + "_ptr"] for k in dn.GUIDES}
    with sp.Denoiser.for_scene(scene) as den:
        sp.render_tiles_device(scene, "direct_lighting", 4, None, p["color_ptr"])
        torch.cuda.synchronize()
        scene.features_device(4, **{k + "_ptr": v for k, v in feats.items()}, stats=True)
        den.run_device(**p, **dn.DEFAULTS, stats=True)
        want = payload(ref["out"], (24, 64, 3)).copy()
    bufs = device_buffers(24, names)
    p = pointers(bufs, names)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with sp.Denoiser.for_scene(scene) as den:  # a fresh object: its first run builds its map on the stream too
        with torch.cuda.stream(stream):
            h = stream.cuda_stream
            assert sp.render_tiles_device(scene, "direct_lighting", 4, None, p["color_ptr"], h, stats=False) is None
            assert scene.features_device(4, **{k + "_ptr": p[k + "_ptr"] for k in dn.GUIDES}, stream=h) is None
            assert den.run_device(**p, **dn.DEFAULTS, stream=h) is None
            assert den.run_device(**p, **dn.DEFAULTS, stream=h) is None  # waits for the object's own previous run
        stream.synchronize()
    assert payload(bufs["out"], (24, 64, 3)).tobytes() == want.tobytes()
    assert all(guards_intact(v) for v in bufs.values())
    assert not np.isnan(want).any() and want.any()


def test_empty_work_and_the_scene_afterwards(paths):
    scene = load(paths["mixed"], (20, 12))
    one_shot, _ = sp.render_tiles(scene, "direct_lighting", 4)
    word = torch.full((64,), FILL, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    with sp.Progressive(scene, "direct_lighting") as prog:
        prog.render(2)
        with sp.Denoiser(20, 12, d_tile_ids=word.data_ptr(), num_tiles=0) as empty:
            st = empty.run_device(word.data_ptr(), word.data_ptr(), demodulate=False, stats=True)
            assert (st["launches"], st["pixels"], st["taps"]) == (0, 0, 0) and empty.device_bytes == 0
        with sp.Denoiser.for_scene(scene) as den:
            den.run(one_shot, **scene.features(4))
        torch.cuda.synchronize()
        assert (word.cpu().numpy() == FILL).all()
        tiles, _ = prog.render(2)  # the progress object and the scene are usable afterwards
        assert np.array_equal(tiles.view(np.uint32), one_shot.view(np.uint32))
    again, _ = sp.render_tiles(scene, "direct_lighting", 4)
    assert again.tobytes() == one_shot.tobytes()
