"""Deformations for the refit tests (test_refit_host.py, test_gpu_refit.py): each takes a scene's
vertices [nv, 3] and triangle indices [nt, 3] and returns new float32 positions of the same shape,
so the host restatement, the device and the oracle all get the same bits.

The per-triangle moves (jitter, permute, collapse_half) are for meshes whose triangles share no
vertex (tests/_lbvh_sets.py); shift, shrink, identity and bend move any mesh."""
import ctypes as C

import numpy as np

import simplepath_amd as sp

F = np.float32


def mesh_of(scene):
    """(vertices [nv, 3] float32, indices [nt, 3] int64): copies of the scene's host mesh"""
    d = scene.desc()
    nv, nt = d.info.num_vertices, d.info.num_triangles
    v = np.ctypeslib.as_array(d.vertices, shape=(nv, 3)).copy() if nv else np.zeros((0, 3), F)
    f = np.ctypeslib.as_array(d.indices, shape=(nt, 3)).astype(np.int64) if nt else np.zeros((0, 3), np.int64)
    return v.astype(F), f


def moved_scene(scene, vertices):
    """a new scene from the first one's description with other vertex positions (sp_scene_from_desc)"""
    d = scene.desc()
    v = np.ascontiguousarray(vertices, dtype=F)
    assert v.shape[0] == d.info.num_vertices
    d.vertices = v.ctypes.data_as(C.POINTER(C.c_float))
    return sp.Scene.from_desc(d)  # (copies every array before it returns)


def _unshared(v, f):
    assert f.size == 0 or np.unique(f).size == f.size, "per-triangle moves need triangles without shared vertices"


def identity(v, f):
    return v.copy()


def shift(v, f):
    return (v + np.array([0.37, -0.21, 0.11], dtype=F)).astype(F)


def shrink(v, f):
    # x and y by 2^-3: exact, and the wide nodes' grid exponents move by 3
    return (v * np.array([0.125, 0.125, 1.0], dtype=F)).astype(F)


def jitter(v, f, seed=5):
    """each triangle scaled about its centroid by a factor in [0.5, 1] and moved along z by up to 0.2:
    triangles that did not overlap as seen along z still do not"""
    _unshared(v, f)
    rng = np.random.default_rng(seed + f.shape[0])
    out = v.copy()
    if f.shape[0] == 0:
        return out
    tri = v[f]                                        # [nt, 3, 3]
    cen = tri.mean(axis=1, keepdims=True, dtype=F)
    k = rng.uniform(0.5, 1.0, (f.shape[0], 1, 1)).astype(F)
    dz = np.zeros((f.shape[0], 1, 3), dtype=F)
    dz[:, 0, 2] = rng.uniform(-0.2, 0.2, f.shape[0]).astype(F)
    out[f] = (cen + (tri - cen) * k + dz).astype(F)
    return out


def permute(v, f, seed=9):
    """triangle i takes the positions of triangle pi(i): the same surface under the worst topology"""
    _unshared(v, f)
    out = v.copy()
    if f.shape[0] == 0:
        return out
    pi = np.random.default_rng(seed + f.shape[0]).permutation(f.shape[0])
    out[f] = v[f[pi]]
    return out


def collapse_half(v, f):
    """every other triangle shrunk to its first vertex: zero-extent boxes (never rendered)"""
    _unshared(v, f)
    out = v.copy()
    if f.shape[0] == 0:
        return out
    half = f[::2]
    out[half[:, 1]] = v[half[:, 0]]
    out[half[:, 2]] = v[half[:, 0]]
    return out


def bend(v, f, amount=0.05):
    """a smooth bend for any mesh: x displaced by amount x the bounding box's x extent, as a parabola
    in y over the box (the tools' 5 % and 20 % bends)"""
    if v.shape[0] == 0:
        return v.copy()
    lo, hi = v.min(axis=0), v.max(axis=0)
    ext = np.maximum(hi - lo, F(1e-20))
    t = ((v[:, 1] - lo[1]) / ext[1]).astype(F)        # 0..1 along y
    out = v.copy()
    out[:, 0] = (v[:, 0] + F(amount) * ext[0] * (F(2.0) * t - F(1.0)) ** 2).astype(F)
    return out.astype(F)


MOVES = {"identity": identity, "shift": shift, "jitter": jitter, "shrink": shrink, "permute": permute,
         "collapse_half": collapse_half}
RENDERED = ("shift", "jitter", "shrink", "permute")   # collapse_half makes degenerate triangles: structural only

# the smallest sets at which a refit can go wrong: one leaf, one wide node, two wide levels at leaf 1
# (9), the wave (64, 65), the block (257), several blocks (1025), and spheres beside triangles
SETS = ("tri1", "tri2", "tri8", "tri9", "tri64", "tri65", "tri257", "tri1025", "mixed")
BUILDERS = ("host", "device")
LEAVES = (1, 4)
