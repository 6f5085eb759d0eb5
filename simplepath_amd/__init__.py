"""simplepath_amd -- MI355X-native per-pixel integration path of kjeffery/SimplePath.

Host-side mirror of the reference's Scene / Integrator / TileScheduler interface
(base/Scene.h, Integrators/Integrator.h, base/TileScheduler.h, main.cpp:77-142) over the
C-ABI in include/simplepath_hip.h.  All integration runs in HIP kernels on the GPU; this module
only parses arguments, owns handles and moves buffers.

    scene = Scene.from_file("bunny.sp")          # sp::parse_file (base/FileParser.cpp:929)
    scene.upload(device=0)                       # BVH build + HBM residency
    sched = ColumnMajorTileScheduler(scene.width, scene.height)
    img, stats = render(scene, "direct_lighting", num_pixel_samples=256)   # main.cpp:109 render()
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _abi
from ._abi import INTEGRATORS, SimplePathError, check, lib

__all__ = [
    "Scene", "TileScheduler", "ColumnMajorTileScheduler", "RenderStats", "render", "render_tiles",
    "render_tiles_device", "tiles_to_image", "write_pfm", "string_to_integrator_type", "INTEGRATORS",
    "SimplePathError", "k_tile_dimension", "rsqrt_table", "set_rsqrt_table", "Progressive", "PIXEL_STATE_DTYPE", "PIXEL_NOISE_DTYPE", "AdaptiveResult",
    "RAY_DTYPE", "RAY_HIT_DTYPE", "make_rays", "camera_look_at", "render_views", "render_views_device",
    "RADIANCE_RAY_DTYPE", "make_radiance_rays", "pixel_seed", "FEATURE_IDS_DTYPE", "FEATURE_OUTPUTS",
    "Denoiser", "DENOISE_GUIDES",
]

k_tile_dimension = 8  # base/Tile.h:10


def string_to_integrator_type(s: str) -> int:
    """Integrators/Integrator.cpp:25 -- raises on unknown names like the reference."""
    out = C.c_int32()
    check(lib().sp_string_to_integrator(s.encode(), C.byref(out)))
    return out.value


# sp_ray / sp_ray_hit (include/simplepath_hip.h): the records of a ray query, 32 bytes each
RAY_DTYPE = np.dtype([("o", "<f4", (3,)), ("tmin", "<f4"), ("d", "<f4", (3,)), ("tmax", "<f4")])
RAY_HIT_DTYPE = np.dtype([("t", "<f4"), ("kind", "<i4"), ("index", "<i4"), ("material", "<i4"),
                          ("beta", "<f4"), ("gamma", "<f4"), ("reserved", "<u4", (2,))])
# sp_scene_features' d_ids: sample 0's hit as a ray query reports it, and the pixel's hit count |H|
FEATURE_IDS_DTYPE = np.dtype([("kind", "<i4"), ("index", "<i4"), ("material", "<i4"), ("hits", "<i4")])
# the five feature buffers: per pixel shape and dtype, in sp_feature_params order
FEATURE_OUTPUTS = {"ids": ((64,), FEATURE_IDS_DTYPE), "coverage": ((64,), np.float32), "depth": ((64,), np.float32),
                   "normal": ((64, 3), np.float32), "albedo": ((64, 3), np.float32)}
K_RAY_EPSILON = float(np.float32(0.001))      # RayLimits::m_t_min (math/Ray.h:17)
K_INFINITE = float(np.finfo(np.float32).max)  # RayLimits::m_t_max: k_infinite_distance


def make_rays(origins, directions, tmin=K_RAY_EPSILON, tmax=K_INFINITE) -> np.ndarray:
    """RAY_DTYPE records [n] from origins, directions [n, 3] and limits (scalars or [n])."""
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError("origins and directions must both be [n, 3]")
    rays = np.zeros(o.shape[0], dtype=RAY_DTYPE)
    rays["o"], rays["d"] = o, d
    rays["tmin"] = np.broadcast_to(np.asarray(tmin, dtype=np.float32), (o.shape[0],))
    rays["tmax"] = np.broadcast_to(np.asarray(tmax, dtype=np.float32), (o.shape[0],))
    return rays


# sp_radiance_ray (include/simplepath_hip.h): the record of a radiance query, 32 bytes
RADIANCE_RAY_DTYPE = np.dtype([("o", "<f4", (3,)), ("seed", "<u4"), ("d", "<f4", (3,)), ("reserved", "<u4")])


def pixel_seed(x, y):
    """main.cpp's integrator-sampler seed of pixel (x, y): ((x << 16) | y) ^ 0xb0ae9d99 as uint32
    (scalars give an int, arrays a uint32 array)."""
    s = ((np.asarray(x).astype(np.uint32) << np.uint32(16)) | np.asarray(y).astype(np.uint32)) ^ np.uint32(0xb0ae9d99)
    return int(s) if s.ndim == 0 else s


def make_radiance_rays(origins, directions, seeds) -> np.ndarray:
    """RADIANCE_RAY_DTYPE records [n] from origins, directions [n, 3] and sampler seeds (a scalar or
    [n], taken modulo 2^32).  Directions are used as given: normalise them."""
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError("origins and directions must both be [n, 3]")
    rays = np.zeros(o.shape[0], dtype=RADIANCE_RAY_DTYPE)
    rays["o"], rays["d"] = o, d
    rays["seed"] = np.broadcast_to((np.asarray(seeds).astype(np.int64) & 0xffffffff).astype(np.uint32), (o.shape[0],))
    return rays


@dataclass
class RenderStats:
    rays: int
    shadow_rays: int
    samples: int
    rng_draws: int
    kernel_ms: float
    pipeline: int = 0
    launches: int = 0
    primary_hits: int = 0
    stage_ms: tuple = (0.0, 0.0, 0.0, 0.0)
    parts: int = 1
    stack_depth: int = 0
    tail_tiles: int = 0   # megakernel: tiles rendered as tail chunks (ABI 6)
    tail_chunks: int = 0  # ... sample chunks per such tile


class Scene:
    """base/Scene.h:48 -- parsed scene, optionally resident in HBM."""

    def __init__(self, handle: C.c_void_p):
        self._h = handle
        self._device = None

    @classmethod
    def from_file(cls, path: str) -> "Scene":
        h = C.c_void_p()
        check(lib().sp_scene_load(path.encode(), C.byref(h)))
        return cls(h)

    @classmethod
    def from_string(cls, text: str, base_dir: str = ".") -> "Scene":
        h = C.c_void_p()
        check(lib().sp_scene_load_string(text.encode(), base_dir.encode(), C.byref(h)))
        return cls(h)

    @classmethod
    def from_desc(cls, desc: _abi.sp_scene_desc) -> "Scene":
        """Scene::Scene from an already-built, flattened scene (sp_scene_from_desc: copied)."""
        h = C.c_void_p()
        check(lib().sp_scene_from_desc(C.byref(desc), C.byref(h)))
        return cls(h)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _abi._lib is not None:
            _abi._lib.sp_scene_free(h)
            self._h = None

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def info(self) -> _abi.sp_scene_info:
        i = _abi.sp_scene_info()
        check(lib().sp_scene_get_info(self._h, C.byref(i)))
        return i

    def desc(self) -> _abi.sp_scene_desc:
        d = _abi.sp_scene_desc()
        check(lib().sp_scene_get_desc(self._h, C.byref(d)))
        return d

    @property
    def width(self) -> int:
        return self.info().image_width

    @property
    def height(self) -> int:
        return self.info().image_height

    @property
    def integrator_type(self) -> int:
        return self.info().integrator_type

    def set_resolution(self, width: int, height: int) -> None:
        check(lib().sp_scene_set_resolution(self._h, width, height))

    def set_camera(self, camera: _abi.sp_camera_desc) -> None:
        """Replace the camera (sp_scene_set_camera): a sp_camera_desc for the scene's image size, from
        camera_look_at() or made by hand.  On a resident scene nothing is uploaded or rebuilt -- the
        next render sees the new camera.  The transform then fixes the image size (set_resolution to
        another size raises SP_ERR_STATE), and progress objects made on the scene become invalid."""
        check(lib().sp_scene_set_camera(self._h, C.byref(camera)))

    @staticmethod
    def _upload_params(bvh_mode=0, stackless=False, stack_max_levels=0, wide_bvh=True, env_replay=False, sah_leaf=0,
                       binary_closest=False) -> _abi.sp_upload_params:
        p = _abi.sp_upload_params()
        p.bvh_mode = bvh_mode
        p.walk = _abi.SP_WALK_STACKLESS if stackless else _abi.SP_WALK_AUTO
        p.stack_max_levels = stack_max_levels
        p.no_wide_bvh = 0 if wide_bvh else 1
        p.binary_closest = 1 if binary_closest else 0
        p.env_replay = 1 if env_replay else 0
        p.sah_leaf = sah_leaf
        return p

    @staticmethod
    def _build_params(builder, finish="auto"):
        """sp_build_params_ex as the pointer the entry points take (struct_size tells it apart)"""
        b = _abi.sp_build_params_ex()
        b.struct_size = C.sizeof(_abi.sp_build_params_ex)
        b.builder = _abi.BUILDERS[builder] if isinstance(builder, str) else int(builder)
        b.finish = _abi.FINISHES[finish] if isinstance(finish, str) else int(finish)
        return C.cast(C.pointer(b), C.POINTER(_abi.sp_build_params))

    def upload(self, device: int = 0, bvh_mode: int = 0, stackless: bool = False, stack_max_levels: int = 0,
               wide_bvh: bool = True, env_replay: bool = False, sah_leaf: int = 0,
               binary_closest: bool = False, builder="auto", finish="auto") -> None:
        """bvh_mode 0 = SAH (throughput), 1 = the reference's median-split BVH (tie-exact order).
        The other options (sp_upload_params) change how the same image is computed, never the
        image: the parent-link walk, the LDS-stack depth budget, the image-light guide tables, the
        SAH leaf size.  On the SAH BVH, wide_bvh / binary_closest choose the 8-wide or binary walks,
        which can only differ in which of two primitives at exactly equal distance wins.
        builder "auto" | "host" | "device" | "device_sah" (sp_build_params): "device" builds a
        linear BVH on the GPU instead of the SAH one on the host -- a much shorter upload, a
        somewhat slower trace, and again the same image up to such ties.  "device_sah" builds the
        host's SAH tree on the GPU, byte for byte: the host build's images and trace rate after a
        short upload (bounds that are not finite are SP_ERR_UNSUPPORTED).
        finish "auto" | "host" | "device" (sp_build_params_ex): where the 8-wide collapse, the
        primitive records and the parent links are made from the binary tree.  Both make the same
        bytes; "auto" is "device" with a device builder and "host" otherwise."""
        p = self._upload_params(bvh_mode, stackless, stack_max_levels, wide_bvh, env_replay, sah_leaf, binary_closest)
        b = self._build_params(builder, finish)
        check(lib().sp_scene_upload_with(self._h, device, C.byref(p), b))
        self._device = device

    @staticmethod
    def _check_dict(c: _abi.sp_bvh_check) -> dict:
        d = {k: getattr(c, k) for k, _ in _abi.sp_bvh_check._fields_ if k not in ("struct_size", "reserved")}
        d["builder"] = {v: k for k, v in _abi.BUILDERS.items()}.get(c.builder, c.builder)
        return d

    def bvh_check(self) -> dict:
        """Structural check of the uploaded scene's binary geometry BVH, read back from the device
        (sp_scene_bvh_check): errors == 0 when every invariant holds; hash names the tree."""
        c = _abi.sp_bvh_check()
        c.struct_size = C.sizeof(_abi.sp_bvh_check)
        check(lib().sp_scene_bvh_check(self._h, C.byref(c)))
        return self._check_dict(c)

    def bvh_build_check(self, builder="auto", **upload_options) -> dict:
        """The same check on what upload(builder=..., **upload_options) would build, on the host
        alone (sp_scene_bvh_build_check); "device" and "device_sah" run the host restatement of that
        device builder."""
        p = self._upload_params(**upload_options)
        b = self._build_params(builder)
        c = _abi.sp_bvh_check()
        c.struct_size = C.sizeof(_abi.sp_bvh_check)
        check(lib().sp_scene_bvh_build_check(self._h, C.byref(p), b, C.byref(c)))
        return self._check_dict(c)

    @staticmethod
    def _wide_dict(c: _abi.sp_wide_check) -> dict:
        d = {k: getattr(c, k) for k, _ in _abi.sp_wide_check._fields_ if k not in ("struct_size", "reserved", "reserved2")}
        d["finish"] = {v: k for k, v in _abi.FINISHES.items()}.get(c.finish, c.finish)
        return d

    def wide_check(self) -> dict:
        """Structural check of the uploaded scene's 8-wide BVH and the hashes of every array the
        finish step made, read back from the device (sp_scene_wide_check)."""
        c = _abi.sp_wide_check()
        c.struct_size = C.sizeof(_abi.sp_wide_check)
        check(lib().sp_scene_wide_check(self._h, C.byref(c)))
        return self._wide_dict(c)

    def wide_build_check(self, builder="auto", finish="auto", **upload_options) -> dict:
        """The same on what upload(builder=..., finish=..., **upload_options) would make, on the
        host alone (sp_scene_wide_build_check); "device" runs the level-wise host restatement."""
        p = self._upload_params(**upload_options)
        b = self._build_params(builder, finish)
        c = _abi.sp_wide_check()
        c.struct_size = C.sizeof(_abi.sp_wide_check)
        check(lib().sp_scene_wide_build_check(self._h, C.byref(p), b, C.byref(c)))
        return self._wide_dict(c)

    @staticmethod
    def _mesh_update(vertices, normals=None):
        """sp_mesh_update over float32 copies of the arrays, which the caller keeps alive"""
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        if n is not None and n.shape != v.shape:
            raise ValueError("normals must have the shape of vertices")
        u = _abi.sp_mesh_update()
        u.struct_size = C.sizeof(_abi.sp_mesh_update)
        u.vertices = v.ctypes.data_as(C.POINTER(C.c_float))
        if n is not None:
            u.normals = n.ctypes.data_as(C.POINTER(C.c_float))
        u.num_vertices = v.shape[0]
        return u, (v, n)

    def update_mesh(self, vertices, normals=None, stats: bool = False):
        """Move the mesh (sp_scene_update_mesh): vertices [num_vertices, 3] in world space, as desc()
        holds them; normals optional.  The host mesh is overwritten in place; a scene resident with
        bvh_mode 0 is refitted on the device -- same trees, new boxes and records, no new upload --
        and progress objects made on it become invalid.  A scene resident with bvh_mode 1 refuses
        (SP_ERR_ARG): upload it again.  With stats=True returns a dict of sp_refit_stats (stage times
        in ms; the call then waits for the device after each stage), else None."""
        u, keep = self._mesh_update(vertices, normals)
        st = _abi.sp_refit_stats()
        st.struct_size = C.sizeof(_abi.sp_refit_stats)
        check(lib().sp_scene_update_mesh(self._h, C.byref(u), C.byref(st) if stats else None))
        del keep
        if not stats:
            return None
        return {k: getattr(st, k) for k, _ in _abi.sp_refit_stats._fields_ if k != "struct_size"}

    def refit_build_check(self, vertices, builder="auto", finish="auto", **upload_options):
        """Host only (sp_scene_refit_build_check): what upload(builder=..., finish=..., **upload_options)
        of the current mesh followed by update_mesh(vertices) leaves in device memory, made by the host
        restatement of the refit and checked against the moved mesh.  Returns (bvh_check dict,
        wide_check dict); the scene is not modified."""
        p = self._upload_params(**upload_options)
        b = self._build_params(builder, finish)
        u, keep = self._mesh_update(vertices)
        c = _abi.sp_bvh_check()
        c.struct_size = C.sizeof(_abi.sp_bvh_check)
        w = _abi.sp_wide_check()
        w.struct_size = C.sizeof(_abi.sp_wide_check)
        check(lib().sp_scene_refit_build_check(self._h, C.byref(p), b, C.byref(u), C.byref(c), C.byref(w)))
        del keep
        return self._check_dict(c), self._wide_dict(w)

    def set_materials(self, materials) -> None:
        """Replace every material (sp_scene_set_materials): a sequence of sp_material_desc, as many as
        the scene has (desc().materials).  On a resident scene the device array is rewritten -- no
        upload, no rebuild -- and progress objects made on the scene become invalid."""
        arr = (_abi.sp_material_desc * max(len(materials), 1))(*materials)
        check(lib().sp_scene_set_materials(self._h, arr, len(materials)))

    def set_lights(self, lights) -> None:
        """Replace the whole light list (sp_scene_set_lights): a sequence of sp_light_desc; count and
        kinds may change, an image light names an existing env image.  On a resident scene the light
        accelerator is rebuilt and the walk's stack sizes follow; geometry is not touched."""
        arr = (_abi.sp_light_desc * max(len(lights), 1))(*lights)
        check(lib().sp_scene_set_lights(self._h, arr, len(lights)))

    def set_env_image(self, image: int, pixels=None, device_ptr: int = 0, width: int = 0, height: int = 0,
                      max_radiance=None, light_to_world=None, stats: bool = False):
        """Replace env image `image`, or append one when image == desc().num_env_images
        (sp_scene_set_env_image).  pixels: [height, width, 3] float32 host array (already multiplied
        by the light's radiance), or device_ptr with width and height for the same layout on the
        device (e.g. a torch tensor's data_ptr()); neither keeps the current pixels.  max_radiance
        None keeps the current value; light_to_world None keeps the current rotation, else a 3x3
        array of the columns vx, vy, vz (rows of the array), whose inverse is computed here.  On a
        resident scene the tables are rebuilt on the device; a rotation alone rewrites only the
        record's matrices.  With stats=True returns a dict of sp_env_stats, else None."""
        d = self.desc()
        u = _abi.sp_env_update()
        u.struct_size = C.sizeof(_abi.sp_env_update)
        u.image = int(image)
        cur = d.env_images[image] if 0 <= image < d.num_env_images else None
        keep = None
        if pixels is not None:
            keep = np.ascontiguousarray(pixels, dtype=np.float32)
            if keep.ndim != 3 or keep.shape[2] != 3:
                raise ValueError("pixels must be [height, width, 3]")
            u.height, u.width = keep.shape[0], keep.shape[1]
            u.pixels = keep.ctypes.data_as(C.POINTER(C.c_float))
        else:
            u.width, u.height = int(width), int(height)
        if device_ptr:
            u.d_pixels = device_ptr
        if max_radiance is None:
            max_radiance = cur.max_radiance if cur is not None else np.finfo(np.float32).max
        u.max_radiance = float(np.float32(max_radiance))
        if light_to_world is None:
            if cur is not None:
                u.light_to_world, u.world_to_light = cur.light_to_world, cur.world_to_light
            else:
                light_to_world = np.eye(3)
        if light_to_world is not None:
            m = np.asarray(light_to_world, dtype=np.float64).reshape(3, 3)
            inv = np.linalg.inv(m.T).T  # rows are columns of the matrix: invert the matrix itself
            for dst, src in ((u.light_to_world, m), (u.world_to_light, inv)):
                for name, row in zip(("vx", "vy", "vz"), src):
                    setattr(dst, name, (C.c_float * 3)(*[float(np.float32(x)) for x in row]))
        st = _abi.sp_env_stats()
        st.struct_size = C.sizeof(_abi.sp_env_stats)
        check(lib().sp_scene_set_env_image(self._h, C.byref(u), C.byref(st) if stats else None))
        del keep
        if not stats:
            return None
        return {k: getattr(st, k) for k, _ in _abi.sp_env_stats._fields_ if k not in ("struct_size", "reserved", "reserved2")}

    @staticmethod
    def _env_dict(c: _abi.sp_env_check) -> dict:
        d = {k: getattr(c, k) for k, _ in _abi.sp_env_check._fields_ if k not in ("struct_size", "reserved", "hash")}
        d["builder"] = {v: k for k, v in _abi.ENV_BUILDERS.items()}.get(c.builder, c.builder)
        d["hashes"] = {name: int(c.hash[i]) for i, name in enumerate(_abi.ENV_TABLES)}
        return d

    def env_check(self, image: int = 0) -> dict:
        """The resident tables of env image `image` read back and compared, word for word, with what
        the host builder makes from the scene's current pixels (sp_scene_env_check): mismatches == 0
        when they are equal; hashes name each table; builder says who made the resident ones."""
        c = _abi.sp_env_check()
        c.struct_size = C.sizeof(_abi.sp_env_check)
        check(lib().sp_scene_env_check(self._h, image, C.byref(c)))
        return self._env_dict(c)

    def env_build_check(self, image: int = 0) -> dict:
        """The host half alone, no device (sp_scene_env_build_check): the hashes of the host builder's tables."""
        c = _abi.sp_env_check()
        c.struct_size = C.sizeof(_abi.sp_env_check)
        check(lib().sp_scene_env_build_check(self._h, image, C.byref(c)))
        return self._env_dict(c)

    def trace(self, origins, directions, tmin=K_RAY_EPSILON, tmax=K_INFINITE, mode="closest", normals: bool = False):
        """Ray queries on the resident scene from host arrays (sp_scene_trace_rays_host): the
        reference's Scene::intersect ("closest") and Scene::intersect_p ("any") for the caller's
        rays.  origins, directions: [n, 3]; tmin, tmax: scalars or [n] (the reference's RayLimits
        defaults).  Geometry only -- lights are not intersected; directions need not be unit
        vectors and t is in their units.
        "closest" returns a RAY_HIT_DTYPE array [n] (a miss: kind = index = material = -1, t = the
        ray's tmax), with normals=True also the shading normals [n, 3] float32 (zeros for a miss).
        "any" returns a bool array [n]: some primitive accepts the ray."""
        rays = make_rays(origins, directions, tmin, tmax)
        n = rays.shape[0]
        m = _abi.QUERY_MODES[mode] if isinstance(mode, str) else int(mode)
        if m == _abi.SP_QUERY_ANY:
            if normals:
                raise ValueError("an any-hit query has no normals")
            occ = np.zeros(max(n, 1), dtype=np.uint32)
            check(lib().sp_scene_trace_rays_host(self._h, m, C.c_void_p(rays.ctypes.data), n, None, None,
                                                 C.c_void_p(occ.ctypes.data), None))
            return occ[:n] != 0
        hits = np.zeros(max(n, 1), dtype=RAY_HIT_DTYPE)
        nrm = np.zeros((max(n, 1), 4), dtype=np.float32) if normals else None
        check(lib().sp_scene_trace_rays_host(self._h, m, C.c_void_p(rays.ctypes.data), n, C.c_void_p(hits.ctypes.data),
                                             C.c_void_p(nrm.ctypes.data) if normals else None, None, None))
        return (hits[:n], nrm[:n, :3].copy()) if normals else hits[:n]

    def trace_device(self, rays_ptr: int, n: int, hits_ptr: int = 0, normals_ptr: int = 0, occluded_ptr: int = 0,
                     mode="closest", stream=None, stats: bool = False):
        """Ray queries on device buffers (sp_scene_trace_rays), e.g. torch tensors' data_ptr():
        rays_ptr n RAY_DTYPE records (a [n, 8] float32 tensor: origin, tmin, direction, tmax);
        "closest" writes n RAY_HIT_DTYPE records to hits_ptr (a [n, 8] int32 tensor) and, when given,
        [n, 4] float32 normals to normals_ptr; "any" writes n uint32 words to occluded_ptr.  The three
        record buffers are 16-byte aligned (any torch allocation is).  With stats=False the query is
        only enqueued on `stream` (returns None); with stats=True the call waits and returns a dict of
        sp_ray_query_stats."""
        q = _abi.sp_ray_query()
        q.struct_size = C.sizeof(_abi.sp_ray_query)
        q.mode = _abi.QUERY_MODES[mode] if isinstance(mode, str) else int(mode)
        q.d_rays = rays_ptr or None
        q.num_rays = int(n)
        q.stream = stream
        q.d_hits = hits_ptr or None
        q.d_normals = normals_ptr or None
        q.d_occluded = occluded_ptr or None
        if not stats:
            check(lib().sp_scene_trace_rays(self._h, C.byref(q), None))
            return None
        st = _abi.sp_ray_query_stats()
        st.struct_size = C.sizeof(_abi.sp_ray_query_stats)
        check(lib().sp_scene_trace_rays(self._h, C.byref(q), C.byref(st)))
        return {k: getattr(st, k) for k, _ in _abi.sp_ray_query_stats._fields_ if k != "struct_size"}

    @staticmethod
    def _radiance_query(integrator, samples, n, rays_ptr=0, stream=None, waves_per_simd=0, per_lane_queries=False):
        if isinstance(integrator, str):
            integrator = string_to_integrator_type(integrator)
        q = _abi.sp_radiance_query()
        q.struct_size = C.sizeof(_abi.sp_radiance_query)
        q.integrator = int(integrator or 0)
        q.d_rays = rays_ptr or None
        q.num_rays = int(n)
        q.samples_per_ray = int(samples)
        q.waves_per_simd = int(waves_per_simd)
        q.flags = PER_LANE_QUERIES if per_lane_queries else 0
        q.stream = stream
        return q

    def radiance(self, origins, directions, seeds, integrator=None, samples: int = 1, **options):
        """Radiance along the caller's own rays on the resident scene, from host arrays
        (sp_scene_radiance_rays_host): the reference's Integrator::integrate for ray i = (origins[i],
        directions[i]) with a sampler seeded seeds[i], called `samples` times with the sampler running
        on, summed in call order and divided -- what main.cpp does for one pixel, whose seed is
        pixel_seed(x, y).  Directions are used as given (normalise them); lights are hit and sampled
        as in a render; a non-finite ray or a zero direction gives 0.  integrator None: the scene's.
        Returns ([n, 3] float32, RenderStats with the totals).  options: waves_per_simd,
        per_lane_queries (as render_tiles)."""
        rays = make_radiance_rays(origins, directions, seeds)
        n = rays.shape[0]
        q = self._radiance_query(integrator, samples, n, **options)
        out = np.zeros((max(n, 1), 3), dtype=np.float32)
        st = _abi.sp_render_stats()
        check(lib().sp_scene_radiance_rays_host(self._h, C.byref(q), C.c_void_p(rays.ctypes.data) if n else None,
                                                C.c_void_p(out.ctypes.data), C.byref(st)))
        return out[:n], _stats(st)

    def radiance_device(self, rays_ptr: int, n: int, out_ptr: int, integrator=None, samples: int = 1, stream=None,
                        stats: bool = True, **options):
        """radiance on device buffers (sp_scene_radiance_rays), e.g. torch tensors' data_ptr():
        rays_ptr n RADIANCE_RAY_DTYPE records (an [n, 8] float32 tensor: origin, seed, direction, 0,
        with columns 3 and 7 written through an int32 view; 16-byte aligned, as any torch allocation
        is), out_ptr n * 3 floats.  With stats=False the query is only enqueued on `stream` (returns
        None); with stats=True the call waits and returns RenderStats."""
        q = self._radiance_query(integrator, samples, n, rays_ptr, stream, **options)
        if not stats:
            check(lib().sp_scene_radiance_rays(self._h, C.byref(q), C.c_void_p(out_ptr), None))
            return None
        st = _abi.sp_render_stats()
        check(lib().sp_scene_radiance_rays(self._h, C.byref(q), C.c_void_p(out_ptr), C.byref(st)))
        return _stats(st)

    # ---- feature buffers on the render's own camera samples (SP_HAS_FEATURES)
    def _tile_args(self, p, tile_ids, d_tile_ids=0, num_tiles=0, camera=None, stream=None):
        """tile list, camera and stream of sp_camera_ray_params / sp_feature_params; returns what
        must stay alive for the call and the slot count"""
        keep = None
        n = (self.width + 7) // 8 * ((self.height + 7) // 8)
        if tile_ids is not None:
            keep = np.ascontiguousarray(tile_ids, dtype=np.int32)
            p.tile_ids = keep.ctypes.data_as(C.POINTER(C.c_int32))
            p.num_tiles = n = keep.size
        elif d_tile_ids:
            p.d_tile_ids = C.c_void_p(d_tile_ids)
            p.num_tiles = n = int(num_tiles)
        if camera is not None:
            p.camera = C.pointer(camera)
        p.stream = stream
        return keep, n

    @staticmethod
    def _feature_stats(call, *args, stats: bool):
        if not stats:
            check(call(*args, None))
            return None
        st = _abi.sp_feature_stats()
        st.struct_size = C.sizeof(_abi.sp_feature_stats)
        check(call(*args, C.byref(st)))
        return {k: getattr(st, k) for k, _ in _abi.sp_feature_stats._fields_ if k != "struct_size"}

    def _camera_ray_params(self, first_sample, num_samples, **tile_args):
        p = _abi.sp_camera_ray_params()
        p.struct_size = C.sizeof(_abi.sp_camera_ray_params)
        p.first_sample = int(first_sample)
        p.num_samples = int(num_samples)
        return (p,) + self._tile_args(p, **tile_args)

    def camera_rays(self, tile_ids=None, first_sample: int = 0, num_samples: int = 1, camera=None) -> np.ndarray:
        """The camera rays a render integrates (sp_scene_camera_rays_host): a RAY_DTYPE array
        [slots, num_samples, 64] whose record [slot, s, lane] is the ray of sample first_sample + s
        of that pixel (lane: the pixel's Morton index in its tile, as in the tile-packed image), with
        the integrators' limits.  Lanes outside the image are all-zero records, which trace()
        answers as a miss.  tile_ids None: every tile.  camera: a sp_camera_desc for this call only
        (the scene's camera is neither read nor changed)."""
        p, keep, n = self._camera_ray_params(first_sample, num_samples, tile_ids=tile_ids, camera=camera)
        rays = np.zeros((n, int(num_samples), 64), dtype=RAY_DTYPE)
        check(lib().sp_scene_camera_rays_host(self._h, C.byref(p), C.c_void_p(rays.ctypes.data) if rays.size else None, None))
        return rays

    def camera_rays_device(self, rays_ptr: int, tile_ids=None, first_sample: int = 0, num_samples: int = 1, camera=None,
                           stream=None, stats: bool = False, d_tile_ids: int = 0, num_tiles: int = 0):
        """camera_rays into a device buffer (sp_scene_camera_rays), e.g. a [slots, num_samples, 64, 8]
        float32 torch tensor's data_ptr() (16-byte aligned, as any torch allocation is).  tile_ids: a
        host list, or d_tile_ids / num_tiles a device list, or neither for every tile.  With
        stats=False the call is only enqueued on `stream` (returns None); with stats=True it waits and
        returns a dict of sp_feature_stats."""
        p, keep, n = self._camera_ray_params(first_sample, num_samples, tile_ids=tile_ids, d_tile_ids=d_tile_ids,
                                             num_tiles=num_tiles, camera=camera, stream=stream)
        return self._feature_stats(lib().sp_scene_camera_rays, self._h, C.byref(p), C.c_void_p(rays_ptr or None), stats=stats)

    def _feature_params(self, samples, tile_samples=None, d_tile_samples=0, **tile_args):
        p = _abi.sp_feature_params()
        p.struct_size = C.sizeof(_abi.sp_feature_params)
        p.samples_per_pixel = int(samples)
        keep, n = self._tile_args(p, **tile_args)
        counts = None
        if tile_samples is not None:
            counts = np.ascontiguousarray(tile_samples, dtype=np.uint32)
            if counts.shape != (n,):
                raise ValueError(f"tile_samples holds {counts.shape} counts for {n} tile slots")
            p.tile_samples = counts.ctypes.data_as(C.POINTER(C.c_uint32))
        elif d_tile_samples:
            p.d_tile_samples = C.c_void_p(d_tile_samples)
        return p, (keep, counts), n

    def features(self, samples: int, tile_ids=None, tile_samples=None, camera=None, outputs=FEATURE_OUTPUTS, stats: bool = False):
        """First-hit feature buffers on the render's own camera samples (sp_scene_features_host):
        per pixel, over its samples 0 .. n - 1 and the samples H among them that hit geometry
        (lights are not intersected), a dict of tile-packed arrays
          "ids"       [slots, 64] FEATURE_IDS_DTYPE: kind, index, material of sample 0's hit (-1: it
                      misses) and hits = |H|
          "coverage"  [slots, 64] float32: |H| / n
          "depth"     [slots, 64] float32: mean distance over H
          "normal"    [slots, 64, 3] float32: mean shading normal over H (not renormalised)
          "albedo"    [slots, 64, 3] float32: mean diffuse albedo over H (a clearcoat's base's)
        with +0 and (-1, -1, -1, 0) where nothing was hit.  n is `samples`, or tile_samples[slot] when
        given (Progressive.tile_samples() after adaptive rounds).  outputs: which of the five to
        compute.  camera: a sp_camera_desc for this call only.  tiles_to_image unpacks normal
        and albedo.  With stats=True returns (dict, dict of sp_feature_stats)."""
        outputs = tuple(outputs)
        if not outputs or any(o not in FEATURE_OUTPUTS for o in outputs):
            raise ValueError(f"outputs: some of {FEATURE_OUTPUTS}")
        p, keep, n = self._feature_params(samples, tile_samples, tile_ids=tile_ids, camera=camera)
        res = {}
        for name in outputs:
            shape, dtype = FEATURE_OUTPUTS[name]
            res[name] = np.zeros((max(n, 1),) + shape, dtype=dtype)
            setattr(p, "d_" + name, C.c_void_p(res[name].ctypes.data))
        st = self._feature_stats(lib().sp_scene_features_host, self._h, C.byref(p), stats=stats)
        res = {k: v[:n] for k, v in res.items()}
        return (res, st) if stats else res

    def features_device(self, samples: int, ids_ptr: int = 0, coverage_ptr: int = 0, depth_ptr: int = 0, normal_ptr: int = 0,
                        albedo_ptr: int = 0, tile_ids=None, tile_samples=None, camera=None, stream=None, stats: bool = False,
                        d_tile_ids: int = 0, num_tiles: int = 0, d_tile_samples: int = 0):
        """features into device buffers (sp_scene_features), e.g. torch tensors' data_ptr():
        ids_ptr [slots, 64, 4] int32, coverage_ptr and depth_ptr [slots, 64] float32, normal_ptr and
        albedo_ptr [slots, 64, 3] float32; any may be 0 (not computed), not all.  tile_samples: host
        counts, or d_tile_samples a device pointer to one uint32 per slot.  With stats=False the call is
        only enqueued on `stream` (returns None); host lists are copied before it returns."""
        p, keep, n = self._feature_params(samples, tile_samples, d_tile_samples, tile_ids=tile_ids, d_tile_ids=d_tile_ids,
                                          num_tiles=num_tiles, camera=camera, stream=stream)
        p.d_ids, p.d_coverage, p.d_depth = ids_ptr or None, coverage_ptr or None, depth_ptr or None
        p.d_normal, p.d_albedo = normal_ptr or None, albedo_ptr or None
        return self._feature_stats(lib().sp_scene_features, self._h, C.byref(p), stats=stats)

    def bvh_info(self):
        d, n, s = C.c_int32(), C.c_int64(), C.c_int64()
        check(lib().sp_scene_bvh_info(self._h, C.byref(d), C.byref(n), C.byref(s)))
        return {"depth": d.value, "nodes": n.value, "slots": s.value}

    def device_bytes(self) -> int:
        """HBM bytes of the uploaded scene (sp_scene_device_bytes)."""
        b = C.c_int64()
        check(lib().sp_scene_device_bytes(self._h, C.byref(b)))
        return b.value

    def bvh_build_info(self, bvh_mode: int = 0) -> dict:
        """Host-only BVH build statistics (no device): what upload(bvh_mode) would build."""
        i = _abi.sp_bvh_info()
        check(lib().sp_scene_bvh_build_info(self._h, bvh_mode, C.byref(i)))
        return {k: getattr(i, k) for k, _ in _abi.sp_bvh_info._fields_}


class TileScheduler:
    """base/TileScheduler.h:18 -- tiles of k_tile_dimension^2 pixels over the image extents."""

    def __init__(self, width: int, height: int):
        self.width, self.height = width, height
        self._counter = 0

    def get_num_tiles(self) -> int:
        n = C.c_int64()
        check(lib().sp_tile_count(self.width, self.height, C.byref(n)))
        return n.value

    def tile_origin(self, tile: int):
        x, y = C.c_int32(), C.c_int32()
        check(lib().sp_tile_origin(self.width, self.height, tile, C.byref(x), C.byref(y)))
        return x.value, y.value


class ColumnMajorTileScheduler(TileScheduler):
    """base/TileScheduler.h:59 -- tile index order x = i % tiles_x, y = i / tiles_x, pass clamp."""

    def __init__(self, width: int, height: int, pass_clamp: int = 1):
        super().__init__(width, height)
        self.pass_clamp = pass_clamp

    def get_next_tile(self) -> Optional[int]:
        n = self.get_num_tiles()
        c = self._counter
        self._counter += 1
        if c // n >= self.pass_clamp:
            return None
        return c % n

    def shard(self, rank: int, world: int) -> np.ndarray:
        """Tiles owned by `rank` of `world` (interleaved: balanced cost across ranks; shard.py)."""
        from .shard import shard_tiles
        return shard_tiles(self.get_num_tiles(), rank, world)


PIPELINES = {"auto": 0, "megakernel": 1, "wavefront": 2, "chunks": 3}
STAGE_TIMING = 4  # SP_RENDER_STAGE_TIMING
PER_LANE_QUERIES = 8  # SP_RENDER_PER_LANE_QUERIES (ABI 5)


def _params(integrator, spp, tile_ids: Optional[np.ndarray], stream=None, pipeline="auto",
            stage_timing=False, waves_per_simd=0, chunks_per_pixel=0, chunk_max_gb=0.0,
            tile_order_factor=0.0, per_lane_queries=False, tail_fraction=0.0) -> tuple:
    if isinstance(integrator, str):
        integrator = string_to_integrator_type(integrator)
    p = _abi.sp_render_params()
    p.integrator = int(integrator or 0)
    p.samples_per_pixel = int(spp)
    keep = None
    if tile_ids is not None:
        keep = np.ascontiguousarray(tile_ids, dtype=np.int32)
        p.tile_ids = keep.ctypes.data_as(C.POINTER(C.c_int32))
        p.num_tiles = keep.size
    p.stream = stream
    p.flags = ((PIPELINES[pipeline] if isinstance(pipeline, str) else int(pipeline)) | (STAGE_TIMING if stage_timing else 0)
               | (PER_LANE_QUERIES if per_lane_queries else 0))
    p.waves_per_simd = int(waves_per_simd)
    p.chunks_per_pixel = int(chunks_per_pixel)
    p.chunk_max_gb = float(chunk_max_gb)
    p.tile_order_factor = float(tile_order_factor)
    p.tail_fraction = float(tail_fraction)
    return p, keep


def _stats(s: _abi.sp_render_stats) -> RenderStats:
    return RenderStats(s.rays, s.shadow_rays, s.samples, s.rng_draws, s.kernel_ms, s.pipeline, s.launches,
                       s.primary_hits, tuple(s.stage_ms), s.parts, s.stack_depth, s.tail_tiles, s.tail_chunks)


def render_tiles(scene: Scene, integrator, num_pixel_samples: int, tile_ids: Optional[Sequence[int]] = None,
                 pipeline="auto", **options):
    """Render tiles on the GPU; returns (tile-packed radiance [n,64,3] float32, RenderStats).
    options: waves_per_simd, chunks_per_pixel, chunk_max_gb (sp_render_params, ABI 4),
    tile_order_factor (ABI 5: 0 automatic, > 0 forced with that factor, < 0 queue order),
    tail_fraction (ABI 6: megakernel tail chunks, 0 automatic, < 0 off, else the fraction of tiles),
    per_lane_queries (ABI 5: IterativeRRNEE without the merged query pass -- the comparison path)."""
    p, keep = _params(integrator, num_pixel_samples, None if tile_ids is None else np.asarray(tile_ids),
                      pipeline=pipeline, **options)
    n = keep.size if keep is not None else TileScheduler(scene.width, scene.height).get_num_tiles()
    out = np.zeros((max(n, 1), 64, 3), dtype=np.float32)
    st = _abi.sp_render_stats()
    check(lib().sp_render_tiles_host(scene.handle, C.byref(p), out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st)))
    return out[:n], _stats(st)


def render_tiles_device(scene: Scene, integrator, num_pixel_samples: int, tile_ids, out_ptr: int, stream=None,
                        pipeline="auto", stage_timing=False, stats=True, d_tile_ids: int = 0,
                        num_tiles: int = 0, **options):
    """Render into a caller-owned device buffer (e.g. a torch.cuda tensor's data_ptr()).
    tile_ids: host tile list (None: d_tile_ids, a device pointer to num_tiles int32 ids, or every
    tile).  With stats=False (and no stage timing) the render is only enqueued on `stream`: the
    call returns without waiting (returns None); a host tile list is copied before it returns."""
    p, keep = _params(integrator, num_pixel_samples, None if tile_ids is None else np.asarray(tile_ids), stream,
                      pipeline, stage_timing, **options)
    if d_tile_ids:
        p.d_tile_ids = C.c_void_p(d_tile_ids)
        p.num_tiles = int(num_tiles)
    if not stats:
        check(lib().sp_render_tiles(scene.handle, C.byref(p), C.c_void_p(out_ptr), None))
        return None
    st = _abi.sp_render_stats()
    check(lib().sp_render_tiles(scene.handle, C.byref(p), C.c_void_p(out_ptr), C.byref(st)))
    return _stats(st)


def camera_look_at(eye, look_at, up, fov_degrees: float, width: int, height: int) -> _abi.sp_camera_desc:
    """The parser's perspective_camera (origin, look_at, up, fov) for a width x height film, as a
    sp_camera_desc (sp_camera_look_at): host only, the parser's bits for equal attributes."""
    v = [(C.c_float * 3)(*[float(x) for x in a]) for a in (eye, look_at, up)]
    out = _abi.sp_camera_desc()
    check(lib().sp_camera_look_at(v[0], v[1], v[2], float(fov_degrees), int(width), int(height), C.byref(out)))
    return out


def _view_params(integrator, spp, cameras, tile_ids, d_cameras=0, d_tile_ids=0, num_tiles=0, num_views=0, stream=None,
                 waves_per_simd=0, per_lane_queries=False) -> tuple:
    if isinstance(integrator, str):
        integrator = string_to_integrator_type(integrator)
    p = _abi.sp_view_params()
    p.struct_size = C.sizeof(_abi.sp_view_params)
    p.integrator = int(integrator or 0)
    p.samples_per_pixel = int(spp)
    keep = [None, None]
    if cameras is not None:
        cams = list(cameras)
        keep[0] = (_abi.sp_camera_desc * max(len(cams), 1))(*cams)
        p.cameras = C.cast(keep[0], C.POINTER(_abi.sp_camera_desc))
        p.num_views = len(cams)
    else:
        p.d_cameras = d_cameras or None
        p.num_views = int(num_views)
    if tile_ids is not None:
        keep[1] = np.ascontiguousarray(np.asarray(tile_ids), dtype=np.int32)
        p.tile_ids = keep[1].ctypes.data_as(C.POINTER(C.c_int32))
        p.num_tiles = keep[1].size
    elif d_tile_ids:
        p.d_tile_ids = C.c_void_p(d_tile_ids)
        p.num_tiles = int(num_tiles)
    p.stream = stream
    p.waves_per_simd = int(waves_per_simd)
    p.flags = PER_LANE_QUERIES if per_lane_queries else 0
    return p, keep


def render_views(scene: Scene, integrator, num_pixel_samples: int, cameras, tile_ids: Optional[Sequence[int]] = None,
                 **options):
    """Many views of the resident scene in one launch (sp_render_views_host): cameras is a sequence of
    sp_camera_desc (camera_look_at(), scene.desc().camera, ...) for the scene's image size.  Returns
    (radiance [V, n, 64, 3] float32 -- view v is render_tiles' image after scene.set_camera(cameras[v]),
    bit for bit --, RenderStats with the totals over all views).  The scene's own camera is not used
    and not changed.  All views draw the same random numbers at the same pixel.
    options: waves_per_simd, per_lane_queries (as render_tiles)."""
    p, keep = _view_params(integrator, num_pixel_samples, cameras, tile_ids, **options)
    n = keep[1].size if keep[1] is not None else TileScheduler(scene.width, scene.height).get_num_tiles()
    v = max(int(p.num_views), 0)
    out = np.zeros((max(v * n, 1), 64, 3), dtype=np.float32)
    st = _abi.sp_render_stats()
    check(lib().sp_render_views_host(scene.handle, C.byref(p), out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st)))
    return out[:v * n].reshape(v, n, 64, 3), _stats(st)


def render_views_device(scene: Scene, integrator, num_pixel_samples: int, cameras, tile_ids, out_ptr: int,
                        d_cameras: int = 0, num_views: int = 0, stream=None, stats=True, d_tile_ids: int = 0,
                        num_tiles: int = 0, **options):
    """render_views into a caller-owned device buffer of V * n * 64 * 3 floats (e.g. a torch tensor's
    data_ptr()).  cameras: host sequence of sp_camera_desc, or None with d_cameras, a device pointer
    to num_views x 12 floats {vx, vy, vz, p} (a [V, 12] float32 tensor; 16-byte aligned).  tile_ids as
    render_tiles_device.  With stats=False the work is only enqueued on `stream` (returns None);
    host cameras and a host tile list are copied before the call returns."""
    p, keep = _view_params(integrator, num_pixel_samples, cameras, tile_ids, d_cameras, d_tile_ids, num_tiles, num_views,
                           stream, **options)
    if not stats:
        check(lib().sp_render_views(scene.handle, C.byref(p), C.c_void_p(out_ptr), None))
        return None
    st = _abi.sp_render_stats()
    check(lib().sp_render_views(scene.handle, C.byref(p), C.c_void_p(out_ptr), C.byref(st)))
    return _stats(st)


# sp_pixel_state (include/simplepath_hip.h): one pixel's carried state in a checkpoint
PIXEL_STATE_DTYPE = np.dtype([("mt", "<u8", (312,)), ("mt_pos", "<u8"), ("draws", "<u8"), ("sum", "<f4", (3,)),
                              ("reserved", "<u4")])


# sp_pixel_noise: one pixel's luminance statistics in an adaptive checkpoint
PIXEL_NOISE_DTYPE = np.dtype([("mean", "<f4"), ("m2", "<f4")])


@dataclass
class AdaptiveResult:
    """sp_adaptive_result: what one round did."""
    active_tiles: int    # tiles rendered in the round; 0: converged, the image was only resolved
    samples_total: int   # sum over pixels of samples done
    min_done: int
    max_done: int
    max_error: float     # over tiles, before the round


class Progressive:
    """Resumable render of one tile list (sp_progress): render(n) adds n samples per pixel, and the
    image after calls with n1, n2, ... samples is render_tiles' image at n1 + n2 + ... samples, bit
    for bit.  Holds 2520 bytes of device memory per pixel slot until close().  The scene must stay
    uploaded as it is: upload() with other options, set_resolution() or set_camera() invalidates the object.

        prog = Progressive(scene, "direct_lighting")
        while not good_enough(img):
            tiles, stats = prog.render(16)
            img = tiles_to_image(scene.width, scene.height, tiles)

    adaptive=True (sp_progress_create_adaptive; 8 more bytes per pixel slot) also keeps every pixel's
    luminance statistics and a sample count per tile: round() renders only the tiles whose error is
    still above a threshold, converge() repeats it until none is, and a tile that stopped at n samples
    holds render_tiles' image of that tile at n samples, bit for bit.

        prog = Progressive(scene, "direct_lighting", adaptive=True)
        tiles, rounds = prog.converge(threshold=0.02, min_samples=8, max_samples=256, step=16)
    """

    def __init__(self, scene: Scene, integrator=None, tile_ids: Optional[Sequence[int]] = None, waves_per_simd: int = 0,
                 tile_order_factor: float = 0.0, d_tile_ids: int = 0, num_tiles: int = 0, adaptive: bool = False):
        if isinstance(integrator, str):
            integrator = string_to_integrator_type(integrator)
        p = _abi.sp_progress_params()
        p.struct_size = C.sizeof(_abi.sp_progress_params)
        p.integrator = int(integrator or 0)
        keep = None
        if tile_ids is not None:
            keep = np.ascontiguousarray(np.asarray(tile_ids), dtype=np.int32)
            p.tile_ids = keep.ctypes.data_as(C.POINTER(C.c_int32))
            p.num_tiles = keep.size
        elif d_tile_ids:
            p.d_tile_ids = C.c_void_p(d_tile_ids)
            p.num_tiles = int(num_tiles)
        p.waves_per_simd = int(waves_per_simd)
        p.tile_order_factor = float(tile_order_factor)
        self._h = C.c_void_p()
        self._scene = scene  # the scene outlives the progress object
        self.adaptive = bool(adaptive)
        create = lib().sp_progress_create_adaptive if adaptive else lib().sp_progress_create
        check(create(scene.handle, C.byref(p), C.byref(self._h)))
        self.num_tiles = int(p.num_tiles) if (keep is not None or d_tile_ids) else \
            TileScheduler(scene.width, scene.height).get_num_tiles()

    def close(self) -> None:
        h = getattr(self, "_h", None)
        if h and _abi._lib is not None:
            _abi._lib.sp_progress_free(h)
        self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def samples(self) -> int:
        n = C.c_uint32()
        check(lib().sp_progress_samples(self._h, C.byref(n)))
        return n.value

    @property
    def device_bytes(self) -> int:
        b = C.c_int64()
        check(lib().sp_progress_device_bytes(self._h, C.byref(b)))
        return b.value

    def render(self, n: int, out_ptr: Optional[int] = None, stream=None, stats: bool = True):
        """Add n samples per pixel; returns (tile-packed radiance of all samples so far [tiles, 64, 3],
        RenderStats of this call).  out_ptr: a caller-owned device buffer of tiles * 64 * 3 floats
        (e.g. a torch tensor's data_ptr()); the call then returns (None, stats), and with stats=False
        it only enqueues the work on `stream` and returns (None, None).  Without out_ptr the image
        comes back in host memory (sp_progress_render_host; `stream` is not used)."""
        st = _abi.sp_render_stats() if stats else None
        if out_ptr is not None:
            check(lib().sp_progress_render(self._h, int(n), stream, C.c_void_p(out_ptr), C.byref(st) if stats else None))
            return None, (_stats(st) if stats else None)
        out = np.zeros((max(self.num_tiles, 1), 64, 3), dtype=np.float32)
        check(lib().sp_progress_render_host(self._h, int(n), out.ctypes.data_as(C.POINTER(C.c_float)),
                                            C.byref(st) if stats else None))
        return out[:self.num_tiles], (_stats(st) if stats else None)

    def export_state(self):
        """Checkpoint: (structured array of tiles * 64 PIXEL_STATE_DTYPE records, samples)."""
        arr = np.zeros(self.num_tiles * 64, dtype=PIXEL_STATE_DTYPE)
        n = C.c_uint32()
        check(lib().sp_progress_export(self._h, C.c_void_p(arr.ctypes.data), arr.size, C.byref(n)))
        return arr, n.value

    def import_state(self, arr: np.ndarray, samples: int) -> None:
        """Continue from a checkpoint export_state() wrote (same tile list, same scene file)."""
        a = np.ascontiguousarray(arr, dtype=PIXEL_STATE_DTYPE)
        check(lib().sp_progress_import(self._h, C.c_void_p(a.ctypes.data), a.size, int(samples)))


    # ---- adaptive objects (adaptive=True)

    @staticmethod
    def _adaptive_params(threshold, min_samples, max_samples, step, floor):
        p = _abi.sp_adaptive_params()
        p.struct_size = C.sizeof(_abi.sp_adaptive_params)
        p.threshold, p.floor = float(threshold), float(floor)
        p.min_samples, p.max_samples, p.step = int(min_samples), int(max_samples), int(step)
        return p

    def round(self, threshold: float, min_samples: int, max_samples: int, step: int, floor: float = 0.0,
              out_ptr: Optional[int] = None, stream=None, stats: bool = True, result: bool = True):
        """One round (sp_adaptive_round): tile errors, selection, `step` more samples on the tiles that
        are below min_samples or above `threshold` (never beyond max_samples), the others resolved.
        Returns (tile-packed image [tiles, 64, 3], RenderStats, AdaptiveResult).  out_ptr: a caller-owned
        device buffer; the image is then None, and with stats=False and result=False the round is only
        enqueued on `stream`.  floor: 0 = 0.01."""
        p = self._adaptive_params(threshold, min_samples, max_samples, step, floor)
        st = _abi.sp_render_stats() if stats else None
        rs = _abi.sp_adaptive_result() if result else None
        a_st, a_rs = (C.byref(st) if stats else None), (C.byref(rs) if result else None)
        out = None
        if out_ptr is not None:
            check(lib().sp_adaptive_round(self._h, C.byref(p), stream, C.c_void_p(out_ptr), a_st, a_rs))
        else:
            out = np.zeros((max(self.num_tiles, 1), 64, 3), dtype=np.float32)
            check(lib().sp_adaptive_round_host(self._h, C.byref(p), out.ctypes.data_as(C.POINTER(C.c_float)), a_st, a_rs))
            out = out[:self.num_tiles]
        res = AdaptiveResult(rs.active_tiles, rs.samples_total, rs.min_done, rs.max_done, rs.max_error) if result else None
        return out, (_stats(st) if stats else None), res

    def converge(self, threshold: float, min_samples: int, max_samples: int, step: int, floor: float = 0.0,
                 max_rounds: Optional[int] = None):
        """round() until no tile is active.  Returns (image, [(RenderStats, AdaptiveResult) per round]);
        the last round rendered nothing and resolved the whole image."""
        rounds = []
        while True:
            out, st, res = self.round(threshold, min_samples, max_samples, step, floor)
            rounds.append((st, res))
            if res.active_tiles == 0 or (max_rounds is not None and len(rounds) >= max_rounds):
                return out, rounds

    def tile_samples(self) -> np.ndarray:
        """Samples done, per tile slot (uint32)."""
        out = np.zeros(max(self.num_tiles, 1), dtype=np.uint32)
        check(lib().sp_adaptive_tile_samples(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size))
        return out[:self.num_tiles]

    def tile_errors(self, floor: float = 0.0) -> np.ndarray:
        """Tile error at the current state, per tile slot (float32; inf below 2 samples)."""
        out = np.zeros(max(self.num_tiles, 1), dtype=np.float32)
        check(lib().sp_adaptive_tile_errors(self._h, float(floor), out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out[:self.num_tiles]

    def export_noise(self):
        """The noise half of a checkpoint: (tiles * 64 PIXEL_NOISE_DTYPE records, per-tile counts)."""
        noise = np.zeros(self.num_tiles * 64, dtype=PIXEL_NOISE_DTYPE)
        counts = np.zeros(max(self.num_tiles, 1), dtype=np.uint32)
        check(lib().sp_adaptive_export(self._h, C.c_void_p(noise.ctypes.data), noise.size,
                                       counts.ctypes.data_as(C.POINTER(C.c_uint32)), counts.size))
        return noise, counts[:self.num_tiles]

    def import_noise(self, noise: np.ndarray, counts: np.ndarray) -> None:
        """After import_state(): the true per-tile counts and the statistics export_noise() wrote."""
        a = np.ascontiguousarray(noise, dtype=PIXEL_NOISE_DTYPE)
        c = np.ascontiguousarray(counts, dtype=np.uint32)
        keep = c if c.size else np.zeros(1, dtype=np.uint32)
        check(lib().sp_adaptive_import(self._h, C.c_void_p(a.ctypes.data), a.size,
                                       keep.ctypes.data_as(C.POINTER(C.c_uint32)), c.size))


# the denoiser's optional guide buffers: floats per pixel, in sp_denoise_params order
DENOISE_GUIDES = {"albedo": 3, "normal": 3, "depth": 1, "coverage": 1}


class Denoiser:
    """Edge-avoiding a-trous wavelet filter on tile-packed frames (sp_denoiser; the rule is in
    include/simplepath_hip.h): a 5x5 B3-spline kernel at steps 1, 2, 4, ... that colour, normal, depth
    and coverage differences stop at edges, with the albedo divided out before and multiplied back
    after.  Scene-free: it takes the frame size and the tile list a render used, and the buffers
    render_tiles and Scene.features write, as they are.

        with Denoiser.for_scene(scene) as dn:
            noisy, _ = render_tiles(scene, "direct_lighting", 8)
            clean = dn.run(noisy, **scene.features(8))
            img = tiles_to_image(scene.width, scene.height, clean)

    tile_ids: a host list (no repeats), or d_tile_ids / num_tiles a device list, or neither for every
    tile.  Holds 48 bytes of device memory per pixel slot from its first run until close()."""

    def __init__(self, width: int, height: int, tile_ids: Optional[Sequence[int]] = None, d_tile_ids: int = 0,
                 num_tiles: int = 0, device: int = 0):
        p = _abi.sp_denoiser_params()
        p.struct_size = C.sizeof(_abi.sp_denoiser_params)
        p.device, p.width, p.height = int(device), int(width), int(height)
        self.num_tiles = (int(width) + 7) // 8 * ((int(height) + 7) // 8)
        keep = None
        if tile_ids is not None:
            keep = np.ascontiguousarray(np.asarray(tile_ids), dtype=np.int32)
            p.tile_ids = keep.ctypes.data_as(C.POINTER(C.c_int32))
            p.num_tiles = self.num_tiles = keep.size
        elif d_tile_ids:
            p.d_tile_ids = C.c_void_p(d_tile_ids)
            p.num_tiles = self.num_tiles = int(num_tiles)
        self.width, self.height = int(width), int(height)
        self._h = C.c_void_p()
        check(lib().sp_denoiser_create(C.byref(p), C.byref(self._h)))

    @classmethod
    def for_scene(cls, scene: Scene, tile_ids: Optional[Sequence[int]] = None, device: int = 0) -> "Denoiser":
        """a denoiser for the scene's frame size"""
        return cls(scene.width, scene.height, tile_ids=tile_ids, device=device)

    def close(self) -> None:
        h = getattr(self, "_h", None)
        if h and _abi._lib is not None:
            _abi._lib.sp_denoiser_free(h)
        self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    @property
    def device_bytes(self) -> int:
        b = C.c_int64()
        check(lib().sp_denoiser_device_bytes(self._h, C.byref(b)))
        return b.value

    @staticmethod
    def _params(iterations, sigma_color, sigma_normal, sigma_depth, sigma_coverage, albedo_floor, depth_floor, demodulate,
                stream=None):
        p = _abi.sp_denoise_params()
        p.struct_size = C.sizeof(_abi.sp_denoise_params)
        p.iterations = int(iterations)
        p.flags = _abi.SP_DENOISE_DEMODULATE if demodulate else 0
        p.sigma_color, p.sigma_normal, p.sigma_depth = float(sigma_color), float(sigma_normal), float(sigma_depth)
        p.sigma_coverage, p.albedo_floor, p.depth_floor = float(sigma_coverage), float(albedo_floor), float(depth_floor)
        p.stream = stream
        return p

    @staticmethod
    def _stats(call, h, p, stats: bool):
        if not stats:
            check(call(h, C.byref(p), None))
            return None
        st = _abi.sp_denoise_stats()
        st.struct_size = C.sizeof(_abi.sp_denoise_stats)
        check(call(h, C.byref(p), C.byref(st)))
        return {k: getattr(st, k) for k in ("launches", "pixels", "taps", "kernel_ms")}

    def run(self, color, albedo=None, normal=None, depth=None, coverage=None, iterations: int = 5, sigma_color: float = 0.6,
            sigma_normal: float = 0.3, sigma_depth: float = 0.2, sigma_coverage: float = 0.4, albedo_floor: float = 0.0,
            depth_floor: float = 0.0, demodulate: bool = True, stats: bool = False, ids=None):
        """Denoise host arrays (sp_denoiser_run_host): color [slots, 64, 3] float32 as render_tiles
        returns it, and any of albedo, normal [slots, 64, 3], depth, coverage [slots, 64] as
        Scene.features returns them -- `**scene.features(n)` passes them all (its ids are not
        used).  A guide left out takes no part in the weights.  demodulate divides the albedo out
        before filtering and needs albedo and coverage (SimplePathError without them: pass False).
        Returns the tile-packed image [slots, 64, 3] (tiles_to_image unpacks it), with stats=True
        (image, dict of sp_denoise_stats)."""
        n = self.num_tiles
        given = {"color": color, "albedo": albedo, "normal": normal, "depth": depth, "coverage": coverage}
        p = self._params(iterations, sigma_color, sigma_normal, sigma_depth, sigma_coverage, albedo_floor, depth_floor,
                         demodulate)
        keep = {}
        for name, v in given.items():
            if v is None:
                continue
            ch = 3 if name == "color" else DENOISE_GUIDES[name]
            keep[name] = np.ascontiguousarray(v, dtype=np.float32)
            if keep[name].size != n * 64 * ch:
                raise ValueError(f"{name} holds {keep[name].shape} floats for {n} tile slots of 64 x {ch}")
            setattr(p, "d_" + name, C.c_void_p(keep[name].ctypes.data) if n else None)
        out = np.zeros((max(n, 1), 64, 3), dtype=np.float32)
        p.d_out = C.c_void_p(out.ctypes.data) if n else None
        st = self._stats(lib().sp_denoiser_run_host, self._h, p, stats)
        return (out[:n], st) if stats else out[:n]

    def run_device(self, color_ptr: int, out_ptr: int, albedo_ptr: int = 0, normal_ptr: int = 0, depth_ptr: int = 0,
                   coverage_ptr: int = 0, iterations: int = 5, sigma_color: float = 0.6, sigma_normal: float = 0.3,
                   sigma_depth: float = 0.2, sigma_coverage: float = 0.4, albedo_floor: float = 0.0, depth_floor: float = 0.0,
                   demodulate: bool = True, stream=None, stats: bool = False):
        """run on device buffers (sp_denoiser_run), e.g. torch tensors' data_ptr(): out_ptr may equal
        color_ptr.  With stats=False the call is only enqueued on `stream` (returns None), after the
        calls that were enqueued there before it: render, features and denoise on one stream need no
        host wait in between.  With stats=True it waits and returns a dict of sp_denoise_stats."""
        p = self._params(iterations, sigma_color, sigma_normal, sigma_depth, sigma_coverage, albedo_floor, depth_floor,
                         demodulate, stream)
        p.d_color, p.d_out = color_ptr or None, out_ptr or None
        p.d_albedo, p.d_normal, p.d_depth, p.d_coverage = albedo_ptr or None, normal_ptr or None, depth_ptr or None, coverage_ptr or None
        return self._stats(lib().sp_denoiser_run, self._h, p, stats)


def tiles_to_image(width: int, height: int, tiles: np.ndarray, tile_ids: Optional[np.ndarray] = None) -> np.ndarray:
    img = np.zeros((height, width, 3), dtype=np.float32)
    t = np.ascontiguousarray(tiles, dtype=np.float32)
    ids = None if tile_ids is None else np.ascontiguousarray(tile_ids, dtype=np.int32)
    check(lib().sp_tiles_to_image(width, height,
                                  None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                  0 if ids is None else ids.size,
                                  t.ctypes.data_as(C.POINTER(C.c_float)), img.ctypes.data_as(C.POINTER(C.c_float))))
    return img


def rsqrt_table() -> dict:
    """The RSQRTSS table scenes are built and rendered with (sp_rsqrt_table_get)."""
    bits, zero, den = C.c_int32(), C.c_uint32(), C.c_uint32()
    check(lib().sp_rsqrt_table_get(None, 0, C.byref(bits), C.byref(zero), C.byref(den)))
    entries = np.zeros(2 << bits.value, dtype=np.uint32)
    check(lib().sp_rsqrt_table_get(entries.ctypes.data_as(C.POINTER(C.c_uint32)), entries.size, None, None, None))
    return {"entries": entries, "bits": bits.value, "zero_result": zero.value, "denorm_result": den.value}


def set_rsqrt_table(table: Optional[dict]) -> None:
    """Emulate another CPU's RSQRTSS (a table from rsqrt_table() there); None: this host's."""
    if table is None:
        check(lib().sp_rsqrt_table_set(None, 0, 0, 0))
        return
    e = np.ascontiguousarray(table["entries"], dtype=np.uint32)
    if e.size != 2 << int(table["bits"]):
        raise ValueError("RSQRTSS table: entries must hold 2 << bits words")
    check(lib().sp_rsqrt_table_set(e.ctypes.data_as(C.POINTER(C.c_uint32)), int(table["bits"]),
                                   int(table["zero_result"]), int(table["denorm_result"])))


def write_pfm(path: str, image: np.ndarray) -> None:
    """Image/Image.cpp:40 write_pfm."""
    img = np.ascontiguousarray(image, dtype=np.float32)
    check(lib().sp_write_pfm(path.encode(), img.shape[1], img.shape[0], img.ctypes.data_as(C.POINTER(C.c_float))))


def render(scene: Scene, integrator=None, num_pixel_samples: int = 1):
    """main.cpp:109 render(): whole frame, returns (image HxWx3, RenderStats)."""
    tiles, st = render_tiles(scene, integrator or 0, num_pixel_samples)
    return tiles_to_image(scene.width, scene.height, tiles), st
