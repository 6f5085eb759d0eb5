"""Constructed primitive sets for the device SAH builder tests (test_device_sah_host.py,
test_gpu_device_sah.py), beside the 22 sets of tests/_lbvh_sets.py.

Each set aims at one place where a parallel binned SAH build can go wrong:

grid16          256 congruent triangles on a 16 x 16 lattice in z = 0 (all coordinates dyadic): the x
                and the y sweep give exactly equal costs, so the axis-order rule decides, and equal
                costs at mirror bins test the bin-order rule.
two_clusters    3 + 300 triangles far apart: one child is a leaf at once, the other lives many levels.
dup_straddle    200 triangles, 50 centroids four times each.  Four copies cannot all lie more than 64
                slots apart within 200 slots (3 x 65 > 199), so the copies are 50 apart here, and
dup_straddle_wide  264 triangles, 66 centroids four times each, 66 slots apart: copies of one key sit
                in different waves.  Equal keys must keep slot order through every partition.
tri<n>          separated_triangles around the thresholds of sp_sah_build.hip (below).

Thresholds of the device builder: SMALL = 128, the largest range handed to one thread (129 is the
first size the level kernels split); BLOCK = 256 slots per workgroup of the level kernels, which
reduce in LDS when a workgroup lies inside one node and go to the node tables directly when it does
not: 255, 256 and 257 (in _lbvh_sets.SIZES) and 511, 512, 513 have a partial workgroup, only whole
ones, or one extra slot at the root; 2 * SMALL + 1 and + 3 give children on both sides of SMALL at
the second level; 1281 and 5000 take several levels with several open nodes each, whose boundaries
fall inside workgroups.  The tests also run with the hand-over size at 4 and 37 (SP_SAH_SMALL),
which sends every set through the level kernels down to nodes of a few slots, and at 1024, where
the nodes of the larger sets span several whole workgroups for more levels."""
import numpy as np

from tests import _lbvh_sets

SMALL, BLOCK = 128, 256
THRESHOLD_SIZES = (SMALL - 1, SMALL, SMALL + 1, 2 * SMALL + 3, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1, 5 * BLOCK + 1, 5000)
# (2 * SMALL + 1 = 257 is in _lbvh_sets.SIZES, as are BLOCK - 1 and BLOCK)
NEW = tuple(f"tri{n}" for n in THRESHOLD_SIZES) + ("grid16", "two_clusters", "dup_straddle", "dup_straddle_wide")

F = np.float32


def _soup(v):
    v = np.ascontiguousarray(v, dtype=F).reshape(-1, 3)
    return v, np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3)


def grid16():
    one = np.array([[-1, -1, 0], [1, -1, 0], [0, 1, 0]], dtype=F) / F(64.0)
    i, j = np.meshgrid(np.arange(16, dtype=F), np.arange(16, dtype=F), indexing="ij")
    cen = np.stack([(i.ravel() - F(7.5)) / F(8.0), (j.ravel() - F(7.5)) / F(8.0), np.zeros(256, dtype=F)], axis=1)
    return _soup(cen[:, None, :] + one[None, :, :])


def two_clusters():
    a, _ = _lbvh_sets.separated_triangles(3, seed=21)
    b, _ = _lbvh_sets.separated_triangles(300, seed=22)
    a = a * F(0.05) + np.array([-40.0, 0.5, 0.0], dtype=F)
    return _soup(np.concatenate([a, b * F(0.5)]))


def dup_straddle(distinct=50):
    v, _ = _lbvh_sets.separated_triangles(distinct, seed=31)
    return _soup(np.tile(v, (4, 1)))


def write_all(directory: str) -> dict:
    """name -> (scene path, bounded primitives expected or None): _lbvh_sets.write_all plus NEW"""
    out = _lbvh_sets.write_all(directory)
    for n in THRESHOLD_SIZES:
        out[f"tri{n}"] = (_lbvh_sets.write_set(directory, f"tri{n}", _lbvh_sets.separated_triangles(n)), n)
    out["grid16"] = (_lbvh_sets.write_set(directory, "grid16", grid16()), 256)
    out["two_clusters"] = (_lbvh_sets.write_set(directory, "two_clusters", two_clusters()), 303)
    out["dup_straddle"] = (_lbvh_sets.write_set(directory, "dup_straddle", dup_straddle(50)), 200)
    out["dup_straddle_wide"] = (_lbvh_sets.write_set(directory, "dup_straddle_wide", dup_straddle(66)), 264)
    return out
