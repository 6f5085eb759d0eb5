"""Constructed primitive sets for the BVH builder tests (test_device_build_host.py,
test_gpu_device_build.py): small PLY meshes and scenes around them, made once per session.

Each set aims at one place where a linear BVH build can go wrong: sizes around the wave (64), the
block (256) and a multi-block scan (1025); one Morton code for every primitive (the position
tie-break alone builds the tree); duplicated primitives; a centroid extent of zero on one or two
axes; spheres beside triangles; and the wedge strip, whose dynamic range puts most primitives
into one cell."""
import os

import numpy as np

from simplepath_amd import scenes

SIZES = (0, 1, 2, 3, 4, 5, 8, 9, 63, 64, 65, 255, 256, 257, 1025)


def separated_triangles(n: int, seed: int = 7):
    """n small triangles, one per cell of a grid over [-1, 1]^2 at random depths: no two share an
    edge or a vertex, and no two overlap as seen along z."""
    rng = np.random.default_rng(seed + n)
    side = max(1, int(np.ceil(np.sqrt(n))))
    cell = 2.0 / side
    k = rng.permutation(side * side)[:n]
    cx = -1.0 + (k % side + 0.5) * cell
    cy = -1.0 + (k // side + 0.5) * cell
    cz = rng.uniform(-0.3, 0.3, n)
    v = np.zeros((3 * n, 3), dtype=np.float32)
    for j, (dx, dy) in enumerate(((-0.35, -0.3), (0.35, -0.3), (0.0, 0.38))):
        v[j::3, 0] = cx + dx * cell * rng.uniform(0.6, 1.0, n)
        v[j::3, 1] = cy + dy * cell * rng.uniform(0.6, 1.0, n)
        v[j::3, 2] = cz + rng.uniform(-0.02, 0.02, n)
    return v, np.arange(3 * n, dtype=np.int32).reshape(-1, 3)


def identical_triangles(n: int = 37):
    one = np.array([[-0.6, -0.5, 0.0], [0.7, -0.4, 0.1], [0.0, 0.6, 0.05]], dtype=np.float32)
    return np.tile(one, (n, 1)), np.arange(3 * n, dtype=np.int32).reshape(-1, 3)


def half_duplicated(n: int = 64):
    v, _ = separated_triangles(n)
    v = np.concatenate([v, v[: 3 * (n // 2)]])
    return v, np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3)


def planar_centroids(n: int = 100):
    v, f = separated_triangles(n, seed=11)
    v[:, 2] = 0.0  # every vertex, so every centroid, at z = 0: a zero-extent axis
    return v, f


def collinear_centroids(n: int = 90):
    one = np.array([[0.0, -0.2, 0.0], [0.02, -0.2, 0.0], [0.0, 0.2, 0.0]], dtype=np.float32)
    v = np.tile(one, (n, 1))
    v[:, 0] += np.repeat(np.arange(n, dtype=np.float32) * np.float32(0.021) - np.float32(0.9), 3)
    return v, np.arange(3 * n, dtype=np.int32).reshape(-1, 3)


def scene_text(ply_rel, spheres=(), width=64, height=48) -> str:
    mesh = f'mesh {{\n    file: "{ply_rel}"\n    material: "set"\n}}\n' if ply_rel else ""
    balls = "".join(f'sphere {{\n    translate: {x} {y} {z}\n    scale: {r} {r} {r}\n    material: "ball"\n}}\n\n'
                    for x, y, z, r in spheres)
    return f"""version: 1

scene_parameters {{
    output_file_name: "set.pfm"
    width: {width}
    height: {height}
    max_depth: 3
}}

perspective_camera {{
    origin: 0.0 0.0 3.2
    look_at: 0.0 0.0 0.0
    fov: 45
}}

material_lambertian {{
    name: "set"
    diffuse: 0.8 0.6 0.3
}}

material_glossy {{
    name: "ball"
    diffuse: 0.3 0.7 0.4
    ior: 1.5
    roughness: 0.4
}}

material_lambertian {{
    name: "floor"
    diffuse: 0.4 0.4 0.5
}}

{mesh}
{balls}plane {{
    material: "floor"
    rotate: 1.0 0.0 0.0 90.0
    translate: 0.0 0.0 -0.6
}}

sphere_light {{
    translate: 0.4 0.6 2.5
    scale: 0.2 0.2 0.2
    radiance: 30.0 30.0 30.0
}}

environment_light {{
    radiance: 0.2 0.2 0.3
}}
"""


def write_set(directory: str, name: str, mesh=None, spheres=()) -> str:
    os.makedirs(os.path.join(directory, "ply_files"), exist_ok=True)
    rel = None
    if mesh is not None and mesh[1].shape[0] > 0:
        rel = os.path.join("ply_files", name + ".ply")
        scenes.write_ply(os.path.join(directory, rel), *mesh)
    path = os.path.join(directory, name + ".sp")
    with open(path, "w") as fh:
        fh.write(scene_text(rel, spheres))
    return path


def write_all(directory: str) -> dict:
    """name -> (scene path, bounded primitives expected; None where the loader decides: it drops
    the wedge strip's smallest triangles as degenerate)"""
    out = {}
    for n in SIZES:
        out[f"tri{n}"] = (write_set(directory, f"tri{n}", separated_triangles(n)), n)
    out["identical37"] = (write_set(directory, "identical37", identical_triangles(37)), 37)
    out["half_dup"] = (write_set(directory, "half_dup", half_duplicated(64)), 96)
    out["planar"] = (write_set(directory, "planar", planar_centroids(100)), 100)
    out["collinear"] = (write_set(directory, "collinear", collinear_centroids(90)), 90)
    balls = [(-0.8 + 0.2 * i, 0.5 * ((i % 3) - 1), 0.1 * (i % 4), 0.08) for i in range(9)]
    out["mixed"] = (write_set(directory, "mixed", separated_triangles(40), balls), 49)
    out["spheres_only"] = (write_set(directory, "spheres_only", None, balls[:5]), 5)
    out["wedge_strip"] = (scenes.write_wedge_strip_scene(directory), None)
    return out
