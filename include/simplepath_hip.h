/*
 * simplepath_hip.h -- C-ABI boundary of the MI355X-native SimplePath renderer.
 *
 * This is the drop-in boundary for the reference's per-pixel integration hot path
 * (kjeffery/SimplePath, main.cpp:77-107 `render_thread` driving
 * Integrators/Integrator.h:37 `Integrator::integrate` over
 * base/TileScheduler.h:29 `TileScheduler::get_next_tile`).  Every entry point takes
 * plain pointers and sizes; no C++ or torch types cross it.
 *
 * Entry points and the reference interface each one replaces:
 *
 *   sp_scene_load / sp_scene_load_string  base/FileParser.cpp:929 `sp::parse_file`
 *                                         + base/Scene.h:59 `Scene::Scene` (accelerators)
 *   sp_scene_from_desc                    base/Scene.h:59 `Scene::Scene` from an already-built
 *                                         scene (main.cpp:368-395 holds one)
 *   sp_scene_get_info                     base/Scene.h:90-96 (image_width, image_height,
 *                                         russian_roulette_depth, max_depth, integrator_type)
 *   sp_scene_get_desc                     the primitive / light / material / camera state
 *                                         held by base/Scene.h:99-105 (flattened, host memory)
 *   sp_scene_upload / sp_scene_upload_ex  (no reference counterpart: HBM residency; the
 *                                         Scene ctor's accelerator build, base/Scene.h:59)
 *   sp_scene_bvh_build_info               base/Scene.h:59 Scene ctor's BVHAccelerator build
 *                                         (shapes/BVHAccelerator.h:173), host only: statistics
 *   sp_scene_upload_with                  the same upload with the binary BVH built on the device
 *   sp_scene_bvh_check / _bvh_build_check (no counterpart: structural check of a built BVH)
 *   sp_scene_update_mesh                  (no counterpart: a moved mesh shown by refitting the resident BVHs)
 *   sp_scene_trace_rays / _host           base/Scene.h:74 `Scene::intersect` and base/Scene.h:79
 *                                         `Scene::intersect_p` for the caller's own rays
 *   sp_render_tiles                       main.cpp:77-107 `render_thread`: for each scheduled
 *                                         tile, for each pixel, num_pixel_samples x
 *                                         `integrator.integrate(camera.generate_ray(...))`,
 *                                         averaged -- executed by HIP kernels on the device
 *   sp_tiles_to_image                     main.cpp:100-102 `image(p.x, p.y) += ... /= spp`
 *                                         scatter of tile-packed radiance into the Image
 *   sp_tile_count                         base/TileScheduler.h:38-48 `get_num_tiles`
 *   sp_tile_origin                        base/TileScheduler.h:72-86 ColumnMajor tile order
 *   sp_string_to_integrator               Integrators/Integrator.cpp:25 `string_to_integrator_type`
 *
 * Error behaviour: every function returns SP_OK (0) or a negative SP_ERR_* code and
 * records a message retrievable with sp_last_error() (thread-local), mirroring the
 * reference's exceptions (ParsingException, std::runtime_error("Unknown integrator type")).
 */
#ifndef SIMPLEPATH_HIP_H
#define SIMPLEPATH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SP_ABI_VERSION 6

/* ---- status codes ------------------------------------------------------------- */
enum {
    SP_OK               = 0,
    SP_ERR_PARSE        = -1, /* sp::ParsingException                                 */
    SP_ERR_IO           = -2, /* unable to open file                                  */
    SP_ERR_ARG          = -3, /* invalid argument                                     */
    SP_ERR_HIP          = -4, /* HIP runtime failure / no device                      */
    SP_ERR_UNSUPPORTED  = -5, /* feature present in the reference but not on this path */
    SP_ERR_STATE        = -6  /* call order violated (e.g. render before upload)      */
};

/* ---- integrators: Integrators/Integrator.h:18 IntegratorType ---------------------- */
enum {
    SP_INTEGRATOR_NOT_SPECIFIED          = 0,
    SP_INTEGRATOR_MANDELBROT             = 1,
    SP_INTEGRATOR_BRUTE_FORCE            = 2,
    SP_INTEGRATOR_BRUTE_FORCE_ITERATIVE  = 3,
    SP_INTEGRATOR_BRUTE_FORCE_ITERATIVE_RR = 4,
    SP_INTEGRATOR_ITERATIVE_RRNEE        = 5,
    SP_INTEGRATOR_DIRECT_LIGHTING        = 6,
    SP_INTEGRATOR_WHITTED                = 7
};

/* ---- flattened scene (host memory, owned by the sp_scene) ------------------------- */

/* AffineSpace (math/AffineSpace.h:12): three columns + translation. */
typedef struct sp_affine {
    float vx[3], vy[3], vz[3], p[3];
} sp_affine;

/* LinearSpace3x3 (math/LinearSpace3x3.h:13): three columns. */
typedef struct sp_linear {
    float vx[3], vy[3], vz[3];
} sp_linear;

/* Material kinds produced by base/FileParser.cpp (materials/Material.h:808-829). */
enum {
    SP_MAT_LAMBERTIAN = 0, /* OneSampleMaterial{ LambertianBRDF }                             */
    SP_MAT_GLOSSY     = 1, /* OneSampleMaterial{ MicrofacetReflection(Beckmann), LambertianBRDF } */
    SP_MAT_CLEARCOAT  = 2  /* ClearcoatMaterial{ base }                                       */
};

typedef struct sp_material_desc {
    int32_t kind;
    int32_t base;               /* clearcoat: index of base material, else -1                 */
    float   lambert_albedo[3];  /* LambertianBRDF::m_albedo == albedo / pi (Material.h:317)   */
    float   microfacet_r[3];    /* MicrofacetReflection::m_r (white)                          */
    float   alpha_x, alpha_y;   /* BeckmannDistribution alphas (roughness_to_alpha, Material.h:231) */
    float   microfacet_ior;     /* MicrofacetReflection::m_ior                                */
    int32_t sample_visible_area;/* MicrofacetDistribution::m_sample_visible_area              */
    float   coat_ior;           /* ClearcoatMaterial::m_ior                                    */
    float   coat_color[3];      /* ClearcoatMaterial::m_specular_color                         */
} sp_material_desc;

/* Primitive kinds in Scene::m_accelerator_geometry order. */
enum { SP_PRIM_TRIANGLE = 0, SP_PRIM_SPHERE = 1, SP_PRIM_PLANE = 2 };

/* Sphere / Plane (shapes/Shape.h:42 TransformableShape). normal_to_world is
 * object_to_world.linear.inverse().transposed() -- what LinearSpace3x3::operator()(Normal3)
 * (math/LinearSpace3x3.h:163) recomputes on every call; here computed once with the same
 * arithmetic. */
typedef struct sp_xform_shape {
    sp_affine object_to_world;
    sp_affine world_to_object;
    sp_linear normal_to_world;
    int32_t   material;
    int32_t   kind; /* SP_PRIM_SPHERE or SP_PRIM_PLANE */
} sp_xform_shape;

/* Light kinds (Lights/Light.h). */
enum { SP_LIGHT_SPHERE = 0, SP_LIGHT_ENVIRONMENT = 1, SP_LIGHT_IMAGE_ENVIRONMENT = 2 };

typedef struct sp_light_desc {
    int32_t   kind;
    int32_t   image;           /* SP_LIGHT_IMAGE_ENVIRONMENT: index into sp_scene_desc.env_images, else -1 */
    float     radiance[3];
    sp_affine object_to_world; /* sphere light */
    sp_affine world_to_object;
    sp_linear normal_to_world;
} sp_light_desc;

/* Image-based environment light (Lights/Light.h:196 ImageBasedEnvironmentLight) as the parser
 * hands it to the light's constructor (base/FileParser.cpp:366-368): the PFM image (Image/
 * Image.cpp:78 read_pfm) already multiplied by `radiance`, before the constructor's
 * modify_image / create_distribution (those run at sp_scene_upload, and in the oracle). */
typedef struct sp_env_image {
    int32_t      width, height;
    const float* pixels;          /* img(x, y) = pixels[(y * width + x) * 3 + c]              */
    float        max_radiance;    /* std::numeric_limits<float>::max() when not given          */
    int32_t      reserved;
    sp_linear    light_to_world;  /* LinearTransformation: rotate/scale attributes             */
    sp_linear    world_to_light;  /* its inverse (Transformation::get_inverse)                  */
} sp_env_image;

/* PerspectiveCamera (Cameras/Camera.h:85): the transform built by create_transform. */
typedef struct sp_camera_desc {
    sp_affine transform;
    int32_t   film_width, film_height;
} sp_camera_desc;

typedef struct sp_scene_info {
    int32_t image_width, image_height;
    int32_t russian_roulette_depth, max_depth;
    int32_t integrator_type; /* SP_INTEGRATOR_* as parsed (0 = not specified)          */
    int32_t num_triangles, num_vertices, num_shapes, num_lights, num_materials;
    char    output_file_name[256];
} sp_scene_info;

typedef struct sp_scene_desc {
    sp_scene_info          info;
    sp_camera_desc         camera;
    /* mesh data: world-space (Mesh ctor pre-transforms, shapes/Triangle.h:25) */
    const float*           vertices;   /* num_vertices * 3                                   */
    const float*           normals;    /* num_vertices * 3 (transformed, not re-normalized)  */
    const uint32_t*        indices;    /* num_triangles * 3                                  */
    const int32_t*         tri_material;/* num_triangles                                     */
    const sp_xform_shape*  shapes;     /* num_shapes (spheres, planes)                       */
    /* Scene::m_geometry order before partitioning: (kind, index) pairs. kind = SP_PRIM_*;
     * index into triangles or shapes. */
    const int32_t*         prim_kind;
    const int32_t*         prim_index;
    int64_t                num_prims;
    const sp_light_desc*   lights;     /* Scene::m_lights order                              */
    const sp_material_desc* materials;
    const sp_env_image*    env_images; /* referenced by sp_light_desc.image (ABI 2)          */
    int32_t                num_env_images;
    int32_t                reserved;
} sp_scene_desc;

/* ---- render ------------------------------------------------------------------------ */

/* Zero-initialise (`sp_render_params p = {0};`): every field added in a later ABI means
 * "automatic" at 0.  Stream order: with stats == NULL, no SP_RENDER_STAGE_TIMING flag and the
 * tile list on the device (d_tile_ids) or absent, sp_render_tiles only enqueues work on `stream`
 * and returns -- two calls and a dependent kernel can be queued back to back with no host wait.
 * Requesting stats waits for the render (the counters are read back).  Calls on one scene share
 * its device scratch; they may come from several host threads and streams (the reference's
 * render() shares one Scene across threads, main.cpp:122-130): the scene serialises them, on the
 * host with a per-scene lock and on the device by making each call's stream wait for the previous
 * call's work (ABI 5).  A host tile list is copied before the call returns. */
typedef struct sp_render_params {
    int32_t        integrator;        /* SP_INTEGRATOR_*; 0 => scene's (DirectLighting if unset: main.cpp:387-392) */
    uint32_t       samples_per_pixel; /* main.cpp `--samples`                                    */
    const int32_t* tile_ids;          /* host array of tile indices (ColumnMajor order); NULL => d_tile_ids or all tiles */
    int64_t        num_tiles;         /* length of tile_ids / d_tile_ids (ignored when both are NULL) */
    void*          stream;            /* hipStream_t, NULL = default stream                      */
    int32_t        bvh_mode;          /* unused: the BVH is chosen at upload (kept for layout)     */
    int32_t        flags;             /* SP_PIPELINE_* (0 = automatic) | SP_RENDER_STAGE_TIMING   */
    /* ---- ABI 4 ---- */
    const int32_t* d_tile_ids;        /* DEVICE array of num_tiles tile indices, used when tile_ids is
                                         NULL: not copied or checked on the host (an id outside
                                         [0, tiles) -- negative ones included -- renders as zeros) */
    int32_t        waves_per_simd;    /* megakernel occupancy (__launch_bounds__ variant): 0 = automatic
                                         (DirectLighting 4, IterativeRRNEE 3, fewer if the LDS caps it);
                                         else DirectLighting 1-4, IterativeRRNEE 2-4               */
    int32_t        chunks_per_pixel;  /* sample-chunk pipeline: 0 = automatic (~120K (tile, chunk) items),
                                         else 1..samples_per_pixel                                 */
    float          chunk_max_gb;      /* sample-chunk buffer budget in GB: 0 = 96, never more than the
                                         device's free memory; AUTO falls back to the megakernel when
                                         the buffers do not fit                                    */
    /* ---- ABI 5 ---- */
    float          tile_order_factor; /* megakernel tile order (DirectLighting, IterativeRRNEE): 0 =
                                         automatic (a one-sample probe times every tile; tiles
                                         slower than 2x the mean go first, then 24 cost classes a
                                         quarter octave apart; from 6 tiles per wave and 128 spp --
                                         2.5 with tail chunks (ABI 6) --, IterativeRRNEE from 4 tiles
                                         per wave and 16 spp);
                                         > 0: with this factor whenever it can apply; < 0: queue
                                         order.  It cannot apply, and the frame renders in queue
                                         order whatever the factor, when the megakernel does not
                                         run (wavefront, sample chunks), when n_tiles is at most
                                         the persistent waves (each wave takes one tile), or for
                                         an integrator without a probe kernel (BruteForce*,
                                         Whitted, Mandelbrot).  A tile's estimate is its probe time
                                         blended with its queue neighbours' for a whole frame (the
                                         tiles left, right, above and below) or a host list with a
                                         constant stride k (a rank's interleaved shard: the tiles k
                                         columns left and right, and the tile below when k divides
                                         the tile columns); any other list uses each tile's own
                                         probe time.                                                  */
    /* ---- ABI 6 ---- */
    float          tail_fraction;     /* megakernel tail chunks (DirectLighting at 4 waves per SIMD, or
                                         3 without an image light, with the tile order):
                                         the most expensive tail_fraction x n_tiles tiles of the
                                         order are rendered as sample chunks at the end of the
                                         persistent queue, so the frame ends on short work items
                                         (identical image and counts).  0 = automatic: where it
                                         applies, waves / n_tiles clamped to [0.12, 0.4] (and AUTO
                                         then picks the megakernel with the order from 2.5 tiles per
                                         persistent wave and 128 spp -- the 2- and 3-GPU shards of a
                                         1080p frame -- or 4 tiles per wave and 64 spp);
                                         < 0 off, else (0, 1].                                      */
    int32_t        reserved;          /* must be 0                                                  */
} sp_render_params;

/* Device pipeline selection (sp_render_params.flags).  All produce identical images. */
enum {
    SP_PIPELINE_AUTO       = 0, /* by work size: megakernel, or sample chunks for DirectLighting
                                   below 24000 tiles when their buffers fit     */
    SP_PIPELINE_MEGAKERNEL = 1, /* one lane owns one pixel for all samples (sp_mega.hpp)        */
    SP_PIPELINE_WAVEFRONT  = 2, /* DirectLighting: per-sample primary/shade/shadow kernels with
                                   ballot/prefix-sum shadow-ray compaction (sp_wave.hip)         */
    SP_PIPELINE_SAMPLE_CHUNKS = 3, /* DirectLighting: each pixel's samples in parallel chunks
                                      (stream state snapshots; sp_chunk.hip)                      */
    SP_RENDER_STAGE_TIMING = 4, /* flag: HIP events between launches fill sp_render_stats.stage_ms
                                   (waits for the render)                                          */
    SP_RENDER_PER_LANE_QUERIES = 8 /* flag (ABI 5): IterativeRRNEE walks each ray on its own lane
                                   instead of dealing a bounce's MIS and next closest-hit walks
                                   over the wave (identical images; the comparison path)           */
};

/* Accelerator options of sp_scene_upload_ex (ABI 4).  Zero-initialise: 0 = automatic. */
enum { SP_WALK_AUTO = 0, SP_WALK_STACKLESS = 1 };
typedef struct sp_upload_params {
    int32_t bvh_mode;         /* 0 = SAH (fast), 1 = reference median-split order (tie-exact)       */
    int32_t walk;             /* SP_WALK_AUTO: per-wave LDS stack unless the BVH is deeper than
                                 stack_max_levels; SP_WALK_STACKLESS: parent links always         */
    int32_t stack_max_levels; /* 0 = 96                                                            */
    int32_t no_wide_bvh;      /* 1: all queries walk the binary BVH instead of the 8-wide one       */
    int32_t env_replay;       /* 1: image-light CDF lookups replay libstdc++ upper_bound step by step
                                 instead of the guide tables (identical results)                    */
    int32_t sah_leaf;         /* SAH leaf size 1-4: 0 = 4                                          */
    int32_t binary_closest;   /* 1: closest-hit queries keep the binary near-first walk (any-hit
                                 queries stay on the 8-wide BVH)                                    */
    int32_t reserved;         /* must be 0                                                          */
} sp_upload_params;

typedef struct sp_render_stats {
    uint64_t rays;            /* every ray cast: camera/extension + shadow + MIS rays            */
    uint64_t shadow_rays;     /* intersect_p queries                                              */
    uint64_t samples;         /* pixel samples (paths)                                            */
    uint64_t rng_draws;       /* IncoherentSampler draws                                          */
    float    kernel_ms;       /* HIP-event time of the render kernel(s)                           */
    int32_t  pipeline;        /* SP_PIPELINE_* that ran                                           */
    int32_t  launches;        /* kernel launches issued                                           */
    uint64_t primary_hits;    /* wavefront: camera rays that hit geometry (shading work items)     */
    float    stage_ms[4];     /* with SP_RENDER_STAGE_TIMING, wavefront: [init+resolve, primary,   */
                              /* shade, shadow] of part 0 summed over launches; megakernel: [0]   */
                              /* the render kernel, [1] the tile-order probe + partition           */
    int32_t  parts;           /* wavefront: concurrent parts (streams); part 0 holds ceil(tiles/2) */
    int32_t  stack_depth;     /* traversal-stack entries per lane the BVH walks needed (ABI 3)      */
    int32_t  tail_tiles;      /* megakernel: tiles rendered as tail chunks (ABI 6; 0: none)         */
    int32_t  tail_chunks;     /* ... and sample chunks per such tile                                */
} sp_render_stats;

/* BVH statistics (sp_scene_bvh_build_info).  depth = levels below the root of the binary BVH
 * (the reference's recursive BVHAccelerator walk, shapes/BVHAccelerator.h:62-77, nests this deep);
 * wide_depth = depth of the 8-wide any-hit BVH (SAH only, else 0); light_depth = the light
 * accelerator's; stack_depth = traversal-stack entries per lane a render needs. */
typedef struct sp_bvh_info {
    int32_t depth, wide_depth, light_depth, stack_depth;
    int64_t nodes, slots;
} sp_bvh_info;

/* ---- API ------------------------------------------------------------------------------ */
typedef struct sp_scene sp_scene;

const char* sp_version(void);
/* ABI 5: content hash (16 hex digits) of the sources, headers and flags the library was built from. */
const char* sp_build_id(void);
const char* sp_last_error(void);

int  sp_string_to_integrator(const char* name, int32_t* out);

int  sp_scene_load(const char* path, sp_scene** out);
int  sp_scene_load_string(const char* text, const char* base_dir, sp_scene** out);
/* Build a scene from a caller's flattened scene (a host that already parsed its scene, e.g.
 * the reference's main.cpp:368-395 sp::Scene): every array is copied and validated; nothing is
 * re-parsed.  Layout as sp_scene_get_desc returns it (world-space mesh, Scene::m_geometry order,
 * camera transform for film_width x film_height).  sp_scene_set_resolution can then not change
 * the image size (the camera transform fixes it). */
int  sp_scene_from_desc(const sp_scene_desc* desc, sp_scene** out);
void sp_scene_free(sp_scene* scene);
int  sp_scene_get_info(const sp_scene* scene, sp_scene_info* out);
/* Arrays in *out are owned by the scene: valid until sp_scene_free or sp_scene_set_resolution. */
int  sp_scene_get_desc(const sp_scene* scene, sp_scene_desc* out);
/* Override image size after load (camera rebuilt as FileParser would with these values). */
int  sp_scene_set_resolution(sp_scene* scene, int32_t width, int32_t height);

int  sp_tile_count(int32_t width, int32_t height, int64_t* out);
int  sp_tile_origin(int32_t width, int32_t height, int64_t tile, int32_t* x0, int32_t* y0);

/* Device side. */
int  sp_device_count(int32_t* out);
int  sp_scene_upload(sp_scene* scene, int32_t device, int32_t bvh_mode);
/* sp_scene_upload with explicit accelerator options (NULL = all automatic with bvh_mode 0).  A
 * scene already resident on `device` with the same effective options is not re-uploaded.  The
 * SP_STACKLESS / SP_STACK_MAX / SP_WIDE / SP_ENV_GUIDE / SP_SAH_LEAF environment variables
 * override fields left automatic (test hooks). */
int  sp_scene_upload_ex(sp_scene* scene, int32_t device, const sp_upload_params* params);
/* Render tiles into a DEVICE buffer laid out tile-packed: out[(slot*64 + morton)*3 + c],
 * slot = position of the tile in params->tile_ids (or the tile index itself when NULL).
 * Pixels of clipped border tiles that fall outside the image are written as 0. */
int  sp_render_tiles(sp_scene* scene, const sp_render_params* params, float* d_out,
                     sp_render_stats* stats);
/* Same as sp_render_tiles but allocates the device buffer itself and copies the tile-packed
 * radiance back into h_out (num_tiles * 64 * 3 floats). */
int  sp_render_tiles_host(sp_scene* scene, const sp_render_params* params, float* h_out,
                          sp_render_stats* stats);
/* BVH statistics of the uploaded scene (depth, node count, primitive slots). */
int  sp_scene_bvh_info(const sp_scene* scene, int32_t* depth, int64_t* nodes, int64_t* slots);
/* ABI 5: bytes the uploaded scene occupies in HBM (BVHs, primitive records, normals, materials,
 * lights, image-light tables, RSQRTSS table) -- what a frame streams at least once. */
int  sp_scene_device_bytes(const sp_scene* scene, int64_t* bytes);
/* Host only (no device needed): build the geometry BVH sp_scene_upload would build for bvh_mode
 * and report its statistics; nothing is uploaded. */
int  sp_scene_bvh_build_info(const sp_scene* scene, int32_t bvh_mode, sp_bvh_info* out);
/* Scatter tile-packed radiance (host memory) into a row-major width x height x 3 image. */
int  sp_tiles_to_image(int32_t width, int32_t height, const int32_t* tile_ids, int64_t num_tiles,
                       const float* tiles, float* image);
/* Write an image as PFM exactly as Image/Image.cpp:40 write_pfm does. */
int  sp_write_pfm(const char* path, int32_t width, int32_t height, const float* image);

/* ---- progressive renders ------------------------------------------------------------------
 * Render some samples, look at the image, render more: N calls of k samples give the image of one
 * sp_render_tiles call with N x k samples, bit for bit (every integrator, light kind and BVH mode).
 * A progress object keeps, per pixel slot of its tile list, what the reference's sample loop
 * carries from one sample to the next (main.cpp:94-102): the sampler state, image(p) before the
 * division, and the number of samples done (also the R2 index).  It owns that device memory
 * (2520 bytes per pixel slot; the device_bytes call reports it) until it is freed; nothing is kept
 * on the scene.  The scene must outlive the progress object, and a scene uploaded again with other
 * options or given another resolution invalidates it: every later call returns SP_ERR_STATE.
 * Calls run the megakernel, take the scene's lock and stream ordering like sp_render_tiles, and may
 * be mixed with it. */
#define SP_HAS_PROGRESS 1

typedef struct sp_progress sp_progress;

typedef struct sp_progress_params {     /* zero-initialise; struct_size = sizeof */
    uint32_t       struct_size;         /* a size the library does not know => SP_ERR_ARG             */
    int32_t        integrator;          /* as sp_render_params.integrator                              */
    const int32_t* tile_ids;            /* host list, copied; NULL => d_tile_ids or all tiles          */
    const int32_t* d_tile_ids;          /* device list, copied at creation                             */
    int64_t        num_tiles;
    int32_t        waves_per_simd;      /* as sp_render_params                                         */
    float          tile_order_factor;   /* as sp_render_params, without its samples threshold; the
                                           order is probed by the first call and kept                  */
    int32_t        reserved[2];         /* must be 0                                                   */
} sp_progress_params;

/* One pixel's carried state, host format (export / import).  mt / mt_pos are std::mt19937_64's own
 * _M_x / _M_p: streaming them into a std::mt19937_64 with operator>> continues the pixel's stream. */
typedef struct sp_pixel_state {
    uint64_t mt[312];
    uint64_t mt_pos;     /* 0..312 */
    uint64_t draws;      /* words drawn from the stream so far */
    float    sum[3];     /* image(p) before /= samples */
    uint32_t reserved;   /* 0 */
} sp_pixel_state;        /* 2528 bytes */

int  sp_progress_create(sp_scene* scene, const sp_progress_params* params, sp_progress** out);
void sp_progress_free(sp_progress* progress);
/* Adds more_samples (>= 1) to every pixel and writes the image of all samples so far, tile-packed as
 * sp_render_tiles does, into d_out (may be NULL: accumulate only).  Stream-ordered like
 * sp_render_tiles: with stats == NULL the call only enqueues work.  stats counts this call only. */
int  sp_progress_render(sp_progress* progress, uint32_t more_samples, void* stream, float* d_out,
                        sp_render_stats* stats);
/* The same with a device buffer of its own, copied back into h_out (num_tiles * 64 * 3 floats). */
int  sp_progress_render_host(sp_progress* progress, uint32_t more_samples, float* h_out, sp_render_stats* stats);
int  sp_progress_samples(const sp_progress* progress, uint32_t* out);
int  sp_progress_device_bytes(const sp_progress* progress, int64_t* out);
/* Checkpoint: num_tiles * 64 records, record slot * 64 + morton; capacity in records.  Pixels of
 * clipped border tiles outside the image export as zero records and are ignored on import.  Import
 * takes what export wrote, into a progress object of the same tile list on the same scene file
 * (another scene handle or process included); it checks mt_pos <= 312 and reserved == 0.  Both
 * wait for the object's queued renders. */
int  sp_progress_export(sp_progress* progress, sp_pixel_state* h_states, int64_t capacity, uint32_t* samples);
int  sp_progress_import(sp_progress* progress, const sp_pixel_state* h_states, int64_t count, uint32_t samples);

/* ---- adaptive sampling --------------------------------------------------------------------
 * An adaptive progress object also carries, per pixel, the running mean and sum of squared
 * deviations of its samples' luminance (the reference's RunningStats fed with relative_luminance),
 * and per tile the number of samples done: the sample count becomes a per-tile quantity.  A round
 * computes every tile's error, renders `step` more samples on the tiles that still need them and
 * resolves the others, so d_out always holds the whole current image.  A tile that stopped after n
 * samples holds the image of a one-shot render of that tile at n samples, bit for bit.
 *
 *   pixel error  e = sqrt((m2 / (n - 1)) / n) / (|mean| + floor),  +inf for n < 2 or a non-finite e
 *   tile error   E = max of e over the tile's pixels inside the image
 *   active       n < max_samples && (n < min_samples || !(E <= threshold)); gets min(step, max - n)
 *
 * 8 bytes per pixel slot and at most 16 per tile beyond a plain object's memory.  On an adaptive
 * object sp_progress_render still adds more_samples to every tile (from its own count) and updates
 * the statistics, sp_progress_samples returns the largest tile count, and sp_progress_export /
 * _import carry the sampler and the sums as before; sp_progress_import sets every tile's count to
 * `samples`.  A checkpoint is sp_progress_export + sp_adaptive_export, restored by
 * sp_progress_import followed by sp_adaptive_import (the true per-tile counts and the statistics).
 * The adaptive calls on a plain object return SP_ERR_STATE. */
#define SP_HAS_ADAPTIVE 1

int  sp_progress_create_adaptive(sp_scene* scene, const sp_progress_params* params, sp_progress** out);

typedef struct sp_adaptive_params {   /* zero-initialise; struct_size = sizeof */
    uint32_t struct_size;
    float    threshold;      /* >= 0, finite */
    uint32_t min_samples, max_samples, step;   /* step >= 1, min <= max, max >= 1 */
    float    floor;          /* 0 = 0.01 */
    uint32_t reserved[2];    /* must be 0 */
} sp_adaptive_params;

typedef struct sp_adaptive_result {
    int64_t  active_tiles;   /* tiles rendered in this round; 0 = converged, only the image was resolved */
    uint64_t samples_total;  /* sum over pixels of samples done */
    uint32_t min_done, max_done;
    float    max_error;      /* over tiles, before the round */
    uint32_t reserved;
} sp_adaptive_result;

/* one round: error -> select -> render step samples on the active tiles -> resolve the rest.
 * Stream-ordered: with stats == NULL and result == NULL the call only enqueues work (the active
 * list and its length stay on the device).  stats counts this round's rendering only. */
int  sp_adaptive_round(sp_progress* progress, const sp_adaptive_params* params, void* stream, float* d_out,
                       sp_render_stats* stats, sp_adaptive_result* result);
int  sp_adaptive_round_host(sp_progress* progress, const sp_adaptive_params* params, float* h_out,
                            sp_render_stats* stats, sp_adaptive_result* result);
/* Per tile slot: samples done, and the tile error at that state (floor 0 = 0.01).  capacity in
 * entries, >= num_tiles.  Both wait for the object's queued work. */
int  sp_adaptive_tile_samples(sp_progress* progress, uint32_t* h_out, int64_t capacity);
int  sp_adaptive_tile_errors(sp_progress* progress, float floor, float* h_out, int64_t capacity);
typedef struct sp_pixel_noise { float mean, m2; } sp_pixel_noise;
/* The noise half of a checkpoint: num_tiles * 64 records (record slot * 64 + morton, zero outside the
 * image) and num_tiles counts. */
int  sp_adaptive_export(sp_progress* progress, sp_pixel_noise* h_noise, int64_t capacity,
                        uint32_t* h_tile_samples, int64_t tiles);
int  sp_adaptive_import(sp_progress* progress, const sp_pixel_noise* h_noise, int64_t count,
                        const uint32_t* h_tile_samples, int64_t tiles);

/* ---- device BVH build ----------------------------------------------------------------------
 * An upload builds the geometry BVH on one host core (binned SAH, or the reference's median split).
 * sp_scene_upload_with can build it on the device instead: a linear BVH (Morton order, Karras 2012
 * ranges) that is ready in a fraction of the time and traces somewhat slower.  Everything after the
 * binary tree -- the 8-wide collapse, the primitive records, the stack or parent-link decision --
 * makes the same arrays for either builder, on the host or on the device (the device finish, below).
 * Images of a device-built scene differ from the SAH build's only
 * where two primitives are hit at exactly equal distance.  sp_scene_upload_ex(s, d, p) is
 * sp_scene_upload_with(s, d, p, NULL); NULL or SP_BUILDER_AUTO selects the host builders.  The
 * environment variable SP_DEVICE_BUILD=1 (a test hook like SP_WIDE) turns AUTO into DEVICE for
 * bvh_mode 0.  An explicit SP_BUILDER_DEVICE with bvh_mode 1 is SP_ERR_ARG: the reference order is a
 * host contract.  A device build that cannot allocate or sort returns SP_ERR_HIP; it never falls back
 * to the host.  The same scene uploaded with another builder is uploaded again.
 *
 * SP_BUILDER_DEVICE_SAH builds the host builder's binned SAH tree on the device: the same nodes and
 * the same primitive order byte for byte, so everything downstream -- both finishes, the refit, the
 * images, the trace rate -- is that of SP_BUILDER_HOST, at a fraction of the build time.  Large nodes
 * are split level by level, small ranges by one thread each.  It serves bvh_mode 0 only (bvh_mode 1:
 * SP_ERR_ARG); SP_FINISH_AUTO resolves to the device finish as for SP_BUILDER_DEVICE; a failed build
 * is SP_ERR_HIP, leaves no resident scene and never falls back to the host; 2^30 primitives or more
 * are SP_ERR_UNSUPPORTED, the host builder's limit.  A bound that is not finite (an infinite or NaN
 * vertex or transform: the scene loader does not refuse them) makes a NaN centroid, whose folds
 * depend on their order: the device SAH builder detects it in its first pass and returns
 * SP_ERR_UNSUPPORTED, leaving no resident scene; build such a scene with SP_BUILDER_HOST.
 * SP_DEVICE_BUILD=2 turns AUTO into DEVICE_SAH for bvh_mode 0 (1 keeps its meaning; an explicit
 * builder is never overridden; SP_SAH_SMALL=n sets the size of the ranges one thread builds, which
 * does not reach the tree).  HOST and DEVICE_SAH are different options although their bytes are
 * equal: changing between them uploads again.  The value 3 is not a builder and stays SP_ERR_ARG. */
#define SP_HAS_DEVICE_BUILD 1
#define SP_HAS_DEVICE_SAH 1

enum { SP_BUILDER_AUTO = 0, SP_BUILDER_HOST = 1, SP_BUILDER_DEVICE = 2, SP_BUILDER_DEVICE_SAH = 4 };
typedef struct sp_build_params {      /* zero-initialise; struct_size = sizeof */
    uint32_t struct_size;             /* a size the library does not know => SP_ERR_ARG */
    int32_t  builder;                 /* SP_BUILDER_* */
    int32_t  reserved[2];             /* must be 0 */
} sp_build_params;
int  sp_scene_upload_with(sp_scene* scene, int32_t device, const sp_upload_params* params, const sp_build_params* build);

/* Structural check of a binary geometry BVH.  errors counts the violations of: child indices in
 * range; every node reached from the root exactly once; leaf counts >= 1 and, for bvh_mode 0, at
 * most 7 and at most the leaf size of the options (the reference build makes a leaf of any size
 * where its split fails); the leaves' slot ranges partition [0, slots); prim_order is a
 * permutation; no child box or primitive bound lies outside its node's box on any axis (compared
 * with < and >, so an all-NaN bound does not count); depth agrees with a walk.  first_error_kind:
 * 1 child range, 2 reached twice, 3 unreachable, 4 leaf count, 5 slots, 6 prim_order, 7 box, 8 depth. */
typedef struct sp_bvh_check {         /* struct_size set by the caller */
    uint32_t struct_size;
    int32_t  builder;                 /* builder that made the tree: SP_BUILDER_HOST, _DEVICE or _DEVICE_SAH */
    int64_t  nodes, leaves, slots;
    int32_t  depth, max_leaf;         /* levels as sp_bvh_info.depth; largest leaf */
    int64_t  errors;                  /* 0 = every invariant holds */
    int32_t  first_error_kind, reserved;
    int64_t  first_error_node;
    uint64_t hash;                    /* FNV-1a 64 over the node array, then prim_order */
} sp_bvh_check;
/* Uploaded scene: copies the binary geometry BVH and the slot codes back from the device and checks them. */
int  sp_scene_bvh_check(sp_scene* scene, sp_bvh_check* out);
/* Host only, no device: builds what an upload with these options would build and checks it; builder
 * DEVICE or DEVICE_SAH runs the host restatement of that device algorithm, which makes the same tree
 * bit for bit (DEVICE_SAH: the level-wise form; bounds that are not finite are SP_ERR_UNSUPPORTED). */
int  sp_scene_bvh_build_check(const sp_scene* scene, const sp_upload_params* params, const sp_build_params* build,
                              sp_bvh_check* out);

/* ---- device finish -------------------------------------------------------------------------
 * After the binary tree an upload collapses it into the 8-wide BVH (wnodes, wslot_tri), packs the
 * primitive records (slot_tri, slot_code) and, for a stackless scene, links the parents.  The host
 * does this on one core; the device finish does it in kernels on the binary tree resident in device
 * memory, level by level, and writes the same bytes: every array equals the host's bit for bit, so
 * renders are identical.  SP_FINISH_AUTO is the device finish when the builder resolves to
 * SP_BUILDER_DEVICE or SP_BUILDER_DEVICE_SAH and the host finish otherwise, so a default upload is untouched.
 * SP_FINISH_DEVICE goes with either builder for bvh_mode 0; with bvh_mode 1 it is SP_ERR_ARG.  A
 * device finish that fails (allocation, more than 2^24 records or 64 levels, a leaf that does not
 * fit a meta byte, a failed quantisation) is SP_ERR_HIP and leaves no resident scene.  The
 * environment variable SP_DEVICE_FINISH=0|1 (a test hook like SP_DEVICE_BUILD) decides AUTO.  The
 * same scene uploaded with another finish is uploaded again.
 *
 * sp_build_params keeps its 16 bytes and its meaning.  sp_build_params_ex begins with the same
 * fields and adds the finish; pass it to sp_scene_upload_with and the check calls through a cast
 * -- struct_size tells the two apart. */
#define SP_HAS_DEVICE_FINISH 1

enum { SP_FINISH_AUTO = 0, SP_FINISH_HOST = 1, SP_FINISH_DEVICE = 2 };
typedef struct sp_build_params_ex {   /* zero-initialise; struct_size = sizeof */
    uint32_t struct_size;
    int32_t  builder;                 /* SP_BUILDER_* */
    int32_t  reserved[2];             /* must be 0 */
    int32_t  finish;                  /* SP_FINISH_* */
    int32_t  reserved2[3];            /* must be 0 */
} sp_build_params_ex;

/* Structural check of the 8-wide BVH and the records beside it.  errors counts the violations of:
 * an inner slot's child_base + s in range; every record reached from the root exactly once, the
 * others being holes (child slots no inner child took) that are all zero and named by no imask; an
 * occupied leaf slot's meta byte has a count of 1..7; the leaf ranges [leaf_base + offset, + count)
 * partition [0, slots); the wslot_tri codes are a permutation of slot_code; every child's decoded
 * box -- fma(q, step, origin) as the walk decodes it -- contains the exact union of all primitive
 * bounds beneath that child (compared with < and >, so a NaN bound does not count); depth agrees
 * with a walk; every occupied slot's lower quantised byte is <= its upper one on each axis and no
 * scale byte is 255.  first_error_kind: 1 child range, 2 reached twice, 3 unreachable, 4 hole, 5 meta
 * byte, 6 leaf ranges, 7 record codes, 8 box, 9 depth, 10 quantised bytes.  A scene without a wide tree (stackless,
 * no_wide_bvh, bvh_mode 1, no bounded primitive) reports records 0 and hash_nodes 0. */
typedef struct sp_wide_check {        /* struct_size set by the caller */
    uint32_t struct_size;
    int32_t  finish;                  /* SP_FINISH_HOST or _DEVICE that made the arrays */
    int64_t  records, holes, slots;
    int32_t  depth, reserved;
    int64_t  errors;
    int32_t  first_error_kind, reserved2;
    int64_t  first_error_node;
    uint64_t hash_nodes;              /* FNV-1a 64 over the wnodes words (0 when no wide tree) */
    uint64_t hash_records;            /* over slot_tri bytes, slot_code, then wslot_tri bytes */
    uint64_t hash_parents;            /* over parents (0 when not stackless) */
} sp_wide_check;
/* Uploaded scene: the arrays read back from the device. */
int  sp_scene_wide_check(sp_scene* scene, sp_wide_check* out);
/* Host only, no device: what an upload with these options would make; finish DEVICE runs the host
 * restatement of the device finish (the level-wise collapse), which makes the same arrays. */
int  sp_scene_wide_build_check(const sp_scene* scene, const sp_upload_params* params, const sp_build_params* build,
                               sp_wide_check* out);

/* ---- moving meshes: refit -----------------------------------------------------------------
 * A host that moves a mesh's vertices between frames need not upload again: sp_scene_update_mesh
 * writes the new positions into the scene and, when it is resident, refits every bounding box of
 * the resident trees bottom-up on the device.  The topology of the trees stays (what the SAH
 * builder chose for the first pose), nothing that stays is allocated, and the image is that of the
 * moved mesh: a tree's shape changes how fast a ray finds its hit, not which hit it finds (up to
 * the ties between primitives at exactly equal distance that any SAH-mode upload has).  After large
 * deformations the kept topology traces slower than a fresh build; when to build again is the
 * host's decision.
 *
 * What may change: vertex positions and, optionally, vertex normals.  Indices, materials, the
 * number and order of primitives, spheres, planes, lights and the camera stay.
 *
 * Validation comes first and changes nothing -- a refused call leaves the mesh and any residency
 * as they were -- in this order: null scene; struct sizes and reserved fields; null `vertices`;
 * num_vertices other than the scene's.  A scene without vertices takes num_vertices = 0 (vertices
 * may then be NULL) and the call does nothing.  Then:
 *   - the scene's host mesh is overwritten in place: pointers from an earlier sp_scene_get_desc
 *     stay valid and show the new values;
 *   - a scene that is not resident is done (refitted = 0): a later upload builds from the new mesh;
 *   - a scene resident with bvh_mode 1 is refused with SP_ERR_ARG before anything changes: the
 *     reference order is a contract about a tree built from the current positions.  Upload again;
 *   - a scene resident with bvh_mode 0 (either builder, either finish, any walk) is refitted in
 *     place: the call takes the scene's lock, waits for queued renders, rewrites the primitive
 *     records, the binary tree's boxes, the 8-wide tree's records and (when given) the normals,
 *     waits for the refit, and invalidates every progress object made on the scene (their samples
 *     belong to the old geometry: SP_ERR_STATE).  The tree's links, the light BVH, the walk, the
 *     stack sizing and sp_scene_device_bytes stay.  The next upload of the scene, with the resident
 *     options too, builds again from the current mesh.
 * A device failure (allocation, a box that cannot be quantised, a fit that did not complete) is
 * SP_ERR_HIP and leaves no resident scene, as after a failed upload; the host mesh is already the
 * new one, so uploading again is the recovery.  There is no fall-back.
 * The refitted arrays equal, byte for byte, those of the host restatement of the refit
 * (sp_scene_refit_build_check). */
#define SP_HAS_REFIT 1

typedef struct sp_mesh_update {      /* zero-initialise; struct_size = sizeof */
    uint32_t     struct_size;        /* a size the library does not know => SP_ERR_ARG */
    int32_t      reserved0;          /* must be 0 */
    const float* vertices;           /* HOST, num_vertices * 3, world space (as sp_scene_desc.vertices); required */
    const float* normals;            /* HOST, num_vertices * 3, or NULL: keep the current normals */
    int64_t      num_vertices;       /* must equal the scene's */
    int32_t      reserved[4];        /* must be 0 */
} sp_mesh_update;

typedef struct sp_refit_stats {      /* struct_size set by the caller */
    uint32_t struct_size;
    int32_t  refitted;               /* 0: host mesh only (scene not resident); 1: resident arrays refitted */
    int32_t  binary_passes, wide_passes;
    float    ms_copy, ms_pack, ms_binary, ms_wide, ms_total;   /* device stages; filled only when asked for */
    int64_t  scratch_bytes;          /* peak device scratch, all released before the call returns */
} sp_refit_stats;

/* stats may be NULL.  Passing stats (or setting SP_UPLOAD_TIMING) makes the call wait for the device
 * after each stage so that ms_* hold stage times. */
int  sp_scene_update_mesh(sp_scene* scene, const sp_mesh_update* update, sp_refit_stats* stats);

/* Host only, no device: build what an upload of the scene's CURRENT mesh with these options would
 * make, refit it to update->vertices with the host restatement of the device refit, and check the
 * result against the NEW bounds.  Either out pointer may be NULL.  The scene is not modified.
 * bvh_mode 1 is SP_ERR_ARG. */
int  sp_scene_refit_build_check(const sp_scene* scene, const sp_upload_params* params, const sp_build_params* build,
                                const sp_mesh_update* update, sp_bvh_check* bvh, sp_wide_check* wide);

/* ---- ray queries ---------------------------------------------------------------------------
 * sp_scene_trace_rays traces a caller's ray buffer against the resident scene: the reference's
 * Scene::intersect(ray, limits, isect) (base/Scene.h:74, SP_QUERY_CLOSEST) and
 * Scene::intersect_p(ray, limits) (base/Scene.h:79, SP_QUERY_ANY), which its integrators are only
 * clients of.  The walks are the render kernels' own, so a ray finds the hit an integrator's ray
 * would have found, bit for bit, whichever accelerator the upload chose.
 *
 * Geometry only: the query covers the geometry accelerator -- the unbounded shapes (planes) first,
 * then the BVH -- as Scene::intersect does.  Lights are not intersected (a sphere light is not in
 * the way of a query ray).  `d` need not be of unit length and `t` is in units of `d`.  The limits
 * are the reference's RayLimits: a hit needs tmin <= t <= tmax, so tmin > tmax misses.
 *
 * Closest hit: t is the smallest accepted distance; kind is SP_PRIM_*; index is the triangle's
 * index into sp_scene_desc.indices / 3 or the shape's index into sp_scene_desc.shapes; material is
 * the index into sp_scene_desc.materials; beta and gamma are the triangle's barycentrics (the hit
 * point is (1 - beta - gamma) v0 + beta v1 + gamma v2), 0 for the other kinds.  A miss is
 * kind = index = material = -1 with t = the bits of the ray's own tmax, zero barycentrics and an
 * all-zero normal.  Between primitives hit at exactly equal t the one reported is the one the walk
 * of this residency keeps -- the rule of the images: bvh_mode 1 keeps the reference's, the 8-wide
 * walk the lower wide slot, a device-built tree its own.  t itself does not depend on the walk.
 *
 * Normals: d_normals receives four floats per ray, the shading normal the integrators use (what the
 * reference's intersect_impl leaves in Intersection::m_normal: interpolated vertex normals for a
 * triangle, the transformed object-space normal for a sphere or plane; not flipped towards the
 * ray) and a 0.  Leaving it NULL skips that work and the RSQRTSS table a block would copy into LDS.
 *
 * Any hit: d_occluded[i] is 1 exactly when some primitive accepts the ray, else 0.
 *
 * Rays no integrator makes: a NaN limit, an origin or direction component that is NaN or infinite,
 * and a zero direction (which every primitive test rejects anyway) are answered as a miss without
 * a walk.  Every other ray is walked with its own limits: tmax = +inf is allowed (a hit at
 * t = +inf, which a denormal direction can produce, then counts), and so are rays parallel to an
 * axis -- a direction component of +0, -0 or a denormal, an origin exactly in a box plane of the
 * tree -- for which a box's entry distance comes out as NaN: such a box is entered, never skipped.
 *
 * Validation comes first and changes nothing, in this order: null scene or query; struct_size (the
 * query's, and that of stats when given) and reserved words; unknown mode; num_rays < 0; the
 * pointer rules of the mode -- a required pointer missing, a forbidden one given, d_rays / d_hits /
 * d_normals not 16-byte aligned or d_occluded not 4-byte aligned -- all SP_ERR_ARG; then a scene
 * that is not resident, SP_ERR_STATE.  num_rays == 0 succeeds and launches
 * nothing.  More than 2^39 - 256 rays in one call are SP_ERR_UNSUPPORTED (one block of 256 per
 * launch grid entry); a BVH whose stacks do not fit the LDS is SP_ERR_UNSUPPORTED as for a render.
 *
 * Ordering: the call is stream-ordered like sp_render_tiles.  It takes the scene's lock, makes
 * `stream` wait for the previous call on the scene and records the event the next call waits for.
 * With stats == NULL it only enqueues work: queries and renders can be queued back to back on one
 * stream and read after one synchronize.  With stats it waits and fills them (hits: closest-hit
 * records that are not a miss, or occluded rays; counted on the device only when asked for).
 * The buffers must stay valid until the work has run.
 *
 * Scene state: a query sees what is resident -- after sp_scene_update_mesh, the moved mesh.  It
 * does not invalidate progress objects and keeps nothing on the scene.
 *
 * sp_scene_trace_rays_host takes host arrays: it allocates device buffers, copies, traces, waits
 * and copies back, as sp_render_tiles_host does.  Which outputs it needs follows the mode as above
 * (h_hits for CLOSEST with h_normals optional, h_occluded for ANY); no alignment is asked of host
 * arrays. */
#define SP_HAS_RAY_QUERY 1

typedef struct sp_ray     { float o[3]; float tmin; float d[3]; float tmax; } sp_ray;      /* 32 bytes */
typedef struct sp_ray_hit { float t; int32_t kind; int32_t index; int32_t material;
                            float beta, gamma; uint32_t reserved[2]; } sp_ray_hit;          /* 32 bytes */
enum { SP_QUERY_CLOSEST = 0, SP_QUERY_ANY = 1 };
typedef struct sp_ray_query {          /* zero-initialise; struct_size = sizeof */
    uint32_t      struct_size;         /* a size the library does not know => SP_ERR_ARG */
    int32_t       mode;                /* SP_QUERY_* */
    const sp_ray* d_rays;              /* DEVICE, num_rays records, 16-byte aligned; required when num_rays > 0 */
    int64_t       num_rays;
    void*         stream;              /* hipStream_t, NULL = default stream */
    sp_ray_hit*   d_hits;              /* DEVICE, 16-byte aligned.  CLOSEST: required.  ANY: must be NULL */
    float*        d_normals;           /* DEVICE, 16-byte aligned.  CLOSEST, optional: 4 floats per ray
                                          (shading normal, 0).  ANY: must be NULL */
    uint32_t*     d_occluded;          /* DEVICE.  ANY: required, one word per ray, 1 or 0.  CLOSEST: must be NULL */
    int32_t       reserved[4];         /* must be 0 */
} sp_ray_query;
typedef struct sp_ray_query_stats {    /* struct_size set by the caller */
    uint32_t struct_size;
    int32_t  launches;                 /* kernel launches issued (0 for num_rays == 0) */
    uint64_t rays, hits;
    float    kernel_ms;                /* HIP-event time of the query kernel */
    int32_t  stack_depth;              /* LDS traversal-stack words per lane the walk of this mode used */
} sp_ray_query_stats;
int  sp_scene_trace_rays(sp_scene* scene, const sp_ray_query* query, sp_ray_query_stats* stats /* may be NULL */);
int  sp_scene_trace_rays_host(sp_scene* scene, int32_t mode, const sp_ray* h_rays, int64_t num_rays,
                              sp_ray_hit* h_hits, float* h_normals, uint32_t* h_occluded, sp_ray_query_stats* stats);

/* ---- camera edits ---------------------------------------------------------------------------
 * sp_camera_look_at builds the transform of a perspective camera on the host: what the parser's
 * perspective_camera block (origin, look_at, up, fov) gives for a film of width x height, with the
 * RSQRTSS table in effect (below) -- for equal attributes, the parser's bits.  It needs no scene and
 * no device.  SP_ERR_ARG: a null pointer, a non-finite input, a width or height outside 1..65535,
 * fov_degrees outside (0, 180).
 *
 * sp_scene_set_camera replaces the scene's camera.  Validation comes first and changes nothing, in
 * this order: null arguments; film_width or film_height other than the scene's image size; any
 * non-finite float -- all SP_ERR_ARG.  Then, under the scene's lock: the host camera is overwritten
 * and fixes the image size from now on, as after sp_scene_from_desc (sp_scene_set_resolution to
 * another size is SP_ERR_STATE; to the same size it succeeds and keeps the camera);
 * sp_scene_get_desc shows the new camera; and every progress object made on the scene becomes
 * invalid (SP_ERR_STATE), as after sp_scene_set_resolution.  On a resident scene only the twelve
 * floats every launch carries by value change: nothing is uploaded, rebuilt, refitted or waited
 * for, work already queued keeps the camera it was launched with, a moved mesh
 * (sp_scene_update_mesh) stays moved, and a later upload with the resident options still finds the
 * scene resident. */
#define SP_HAS_CAMERA_EDIT 1

int  sp_camera_look_at(const float eye[3], const float look_at[3], const float up[3],
                       float fov_degrees, int32_t width, int32_t height, sp_camera_desc* out);
int  sp_scene_set_camera(sp_scene* scene, const sp_camera_desc* camera);

/* ---- many views in one launch ---------------------------------------------------------------
 * sp_render_views renders num_views views of the resident scene -- one tile list, integrator and
 * sample count, one camera per view -- in ONE launch of the persistent megakernel, whose queue
 * holds num_views x num_tiles items.  For frames too small to fill the device (a 256 x 256 frame is
 * 1024 tiles; a 256-CU device keeps up to 4096 waves of one tile each) this replaces num_views
 * launches that each underfill it and each end in their own tail.
 *
 * View v is, bit for bit, the image sp_render_tiles gives for the same tiles, integrator and
 * samples after sp_scene_set_camera(cameras[v]) (SP_PIPELINE_MEGAKERNEL, tail chunks off).  The
 * pixel sampler and the integrator's sampler are seeded from the pixel position alone
 * (main.cpp:67-76): nothing of the view enters.  It follows that all views draw the SAME random
 * numbers at the same pixel -- their noise is correlated, as it is between the reference's own
 * renders of two cameras.  Averaging views does not average that noise away as independent
 * renders would; differences between nearby views are smoother for it.
 *
 * The scene's own camera is neither read nor changed, and progress objects stay valid.
 * Output: out[((v * num_tiles + slot) * 64 + morton) * 3 + c]; pixels of clipped border tiles
 * outside the image are 0, as for sp_render_tiles.  Stats are totals over all views: rays,
 * shadow_rays, samples and rng_draws are the sums of the single-view calls' counts, pipeline is
 * SP_PIPELINE_MEGAKERNEL and launches is 1.
 *
 * The views render in queue order: there is no tile-order probe and there are no tail chunks.
 * Prefer sp_render_views when a view has fewer tiles than the device keeps persistent waves: on one
 * MI355X (bunny, DirectLighting, 64 spp) 64 views of 256 x 256 took 146 ms against 397 ms for 64
 * sp_render_tiles calls queued back to back (1483 ms with SP_PIPELINE_MEGAKERNEL).  Prefer num_views
 * single sp_render_tiles calls for LARGE frames at sample counts where they order their queue and
 * cut tail chunks (from 128 spp): four 1920 x 1080 views at 256 spp took 896 ms in one launch and
 * 872 ms as four calls; at 64 spp both took 228 ms.  DESIGN.md section 27 has the figures.
 *
 * Ordering and locking as sp_render_tiles: the scene's lock; `stream` waits for the previous call
 * on the scene; with stats == NULL the call only enqueues.  Host cameras and a host tile list are
 * copied before the call returns; d_cameras and d_tile_ids must stay valid and unchanged until the
 * work has run.
 *
 * Validation comes first, in this order: null scene, params or output; struct_size and reserved
 * words; flags; num_views < 1; exactly one of cameras / d_cameras, d_cameras 16-byte aligned; a host
 * camera with another film size or a non-finite value; the tile-list rules of sp_render_tiles;
 * samples_per_pixel == 0 -- all SP_ERR_ARG; then a scene that is not resident, SP_ERR_STATE.  Then
 * the integrator as for sp_render_tiles; SP_INTEGRATOR_MANDELBROT is SP_ERR_UNSUPPORTED (it has no
 * camera), and so are more than INT32_MAX queue items (num_views x num_tiles). */
#define SP_HAS_VIEWS 1

typedef struct sp_view_params {        /* zero-initialise; struct_size = sizeof */
    uint32_t              struct_size;       /* a size the library does not know => SP_ERR_ARG */
    int32_t               integrator;        /* as sp_render_params */
    uint32_t              samples_per_pixel;
    int32_t               num_views;         /* >= 1 */
    const sp_camera_desc* cameras;           /* HOST, num_views; film size must be the scene's; or NULL */
    const float*          d_cameras;         /* DEVICE, num_views x 12 floats {vx, vy, vz, p}, 16-byte aligned;
                                                exactly one of cameras / d_cameras */
    const int32_t*        tile_ids;          /* as sp_render_params: host list, or */
    const int32_t*        d_tile_ids;        /* device list, or both NULL = every tile; shared by all views */
    int64_t               num_tiles;
    void*                 stream;
    int32_t               waves_per_simd;    /* as sp_render_params */
    int32_t               flags;             /* SP_RENDER_PER_LANE_QUERIES or 0; anything else SP_ERR_ARG */
    int32_t               reserved[4];       /* must be 0 */
} sp_view_params;
int  sp_render_views(sp_scene* scene, const sp_view_params* params, float* d_out, sp_render_stats* stats /* may be NULL */);
/* h_out: num_views * num_tiles * 64 * 3 floats in host memory; waits for the render */
int  sp_render_views_host(sp_scene* scene, const sp_view_params* params, float* h_out, sp_render_stats* stats);

/* ---- radiance queries -----------------------------------------------------------------------
 * sp_scene_radiance_rays runs an integrator along the caller's own rays on the resident scene: the
 * reference's Integrator::integrate(ray, scene, arena, sampler, pixel_coords)
 * (Integrators/Integrator.h:37), of which its pinhole camera is only one client (main.cpp:94-101).
 * A fisheye or equirectangular probe, an orthographic or thin-lens camera, bake points on a surface
 * or rays from a learned camera model get light here, where sp_scene_trace_rays gives hits.
 *
 * What record i means.  The library makes IncoherentSampler::create_new_sequence(Seed{seed}) -- the
 * mt19937_64 a render seeds per pixel, with `seed` taken as given --, calls the integrator
 * samples_per_ray times on the ray (o, d) with that one sampler running on, as main.cpp:94-101 does
 * for one pixel, sums the results in call order, divides by (float)samples_per_ray and writes
 * d_out[i * 3 + c].
 *
 * Direction: d is used as given.  The reference's cameras hand integrate a direction normalised by
 * sp::rsqrt and the materials take -d as wo: the caller normalises.
 * Position independence: a record's result does not depend on its position in the buffer or on its
 * neighbours.
 * Seeds: equal seeds on different rays give correlated noise.  main.cpp's seed for pixel (x, y) is
 * ((x << 16) | y) ^ 0xb0ae9d99.
 * Rays no integrator makes: a NaN or infinite component of o or d, or a zero d, gives radiance +0
 * without a walk or a draw; such a record counts no rays, samples or draws.  `reserved` of a
 * record is not checked (it lives in device memory).
 * Geometry and lights are a render's: unlike a ray query, lights are hit and sampled, because
 * integrate does that.  Equal-distance ties resolve as in a render of this residency.
 * Scene state: a query sees what is resident -- after sp_scene_update_mesh, the moved mesh.  It does
 * not read the camera: sp_scene_set_camera changes no bit of it.  It leaves progress objects valid
 * and keeps nothing on the scene beyond the scratch a render uses.
 *
 * One launch of a persistent kernel serves all rays: its waves take 64 consecutive records at a
 * time from a queue, because rays cost very differently.  That is the right call for many rays
 * (from a few thousand: one item per wave the device keeps resident) whatever their order or mix.
 * It is not the right call for a pinhole frame -- sp_render_tiles orders its tiles by cost, cuts
 * tail chunks and makes the camera rays itself -- nor for a handful of rays at many samples, which
 * keep one wave busy while the device idles: split such rays into records of fewer samples with
 * different seeds and average.  Records that are neighbours in the buffer share a wave: rays that
 * start and head alike (tile or Morton order of a probe) walk the tree together and run faster than
 * the same rays in random order.  On one MI355X (bunny at 1920 x 1080, DirectLighting, one ray per
 * pixel) two million rays in the render's tile order took about 2.4 ms at 1 sample and 65 ms at 64,
 * level with sp_render_tiles' megakernel for the same integrate calls; in row order 9-10 % more from
 * 16 samples (IterativeRRNEE: 2 %).  At one sample per ray about half of that is the fixed cost per record, mostly the
 * 312-word seeding of its generator.  DESIGN.md section 28 has the figures.
 *
 * Validation comes first and changes nothing, in this order: null scene, query or output;
 * struct_size and reserved words; flags other than SP_RENDER_PER_LANE_QUERIES; num_rays < 0; d_rays
 * missing when num_rays > 0, or not 16-byte aligned; samples_per_ray == 0; waves_per_simd out of the
 * integrator's range -- all SP_ERR_ARG; then a scene that is not resident, SP_ERR_STATE.  Then the
 * integrator resolves as for sp_render_tiles; SP_INTEGRATOR_MANDELBROT is SP_ERR_UNSUPPORTED (it
 * has no ray), and so are more than INT32_MAX queue items of 64 rays and a BVH too deep for the LDS
 * stacks, as for a render.  num_rays == 0 succeeds and launches nothing.
 *
 * Ordering and locking as sp_render_tiles: the scene's lock; `stream` waits for the previous call
 * on the scene; with stats == NULL the call only enqueues.  d_rays and d_out must stay valid until
 * the work has run.  Stats: rays, shadow_rays, samples and rng_draws are totals over the records,
 * pipeline is SP_PIPELINE_MEGAKERNEL and launches is 1.
 *
 * sp_scene_radiance_rays_host takes host arrays (query->d_rays is ignored; no alignment is asked of
 * h_rays): it allocates device buffers, copies, runs, waits and copies back. */
#define SP_HAS_RADIANCE_QUERY 1

typedef struct sp_radiance_ray { float o[3]; uint32_t seed; float d[3]; uint32_t reserved; } sp_radiance_ray; /* 32 bytes */

typedef struct sp_radiance_query {      /* zero-initialise; struct_size = sizeof */
    uint32_t               struct_size;       /* a size the library does not know => SP_ERR_ARG */
    int32_t                integrator;        /* as sp_render_params.integrator */
    const sp_radiance_ray* d_rays;            /* DEVICE, num_rays records, 16-byte aligned */
    int64_t                num_rays;
    uint32_t               samples_per_ray;   /* >= 1 */
    int32_t                waves_per_simd;    /* as sp_render_params */
    int32_t                flags;             /* SP_RENDER_PER_LANE_QUERIES or 0; anything else SP_ERR_ARG */
    int32_t                reserved0;         /* must be 0 */
    void*                  stream;            /* hipStream_t, NULL = default stream */
    int32_t                reserved[4];       /* must be 0 */
} sp_radiance_query;
/* d_out: DEVICE, num_rays * 3 floats */
int  sp_scene_radiance_rays(sp_scene* scene, const sp_radiance_query* query, float* d_out, sp_render_stats* stats /* may be NULL */);
/* h_rays, h_out: host arrays of num_rays records and num_rays * 3 floats; waits for the work */
int  sp_scene_radiance_rays_host(sp_scene* scene, const sp_radiance_query* query /* d_rays ignored */,
                                 const sp_radiance_ray* h_rays, float* h_out, sp_render_stats* stats /* may be NULL */);

/* ---- feature buffers on the render's own camera samples -------------------------------------
 * Two calls on a resident scene.  sp_scene_camera_rays exports the camera rays a render integrates;
 * sp_scene_features reduces first-hit features over them, per pixel, in the kernel that makes the
 * rays: the guide images a denoiser or compositor expects beside a Monte-Carlo frame (albedo,
 * shading normal, depth, coverage, ids), antialiased exactly as the frame is.
 *
 * The camera sample.  Sample i of pixel (x, y) is the reference's RSequenceSampler position
 * (main.cpp:67, math/Sampler.h:158) through PerspectiveCamera::generate_ray_impl
 * (Cameras/Camera.h:119): origin = the camera's p, direction normalised by sp::rsqrt.  It depends on
 * the pixel, the sample index and the camera only -- not on the integrator, the tile list or the
 * pipeline -- and is, bit for bit, the ray sp_render_tiles integrates for that sample.
 *
 * Tiles: the forms of sp_render_tiles -- a host list (checked, copied before return), a device
 * list (neither; an id outside the frame gives empty pixels), or both NULL for every tile.  One
 * lane owns one pixel, one wave one list slot; `lane` below is the pixel's Morton index in its tile,
 * as in the tile-packed image.
 *
 * Camera override: `camera`, when given, replaces the scene's camera for this call only.  It is
 * carried by value in the launch, as the views of sp_render_views are: the scene's camera is neither
 * read nor changed.  Its film size must be the scene's image size and its floats finite.
 *
 * sp_scene_camera_rays writes, for samples [first_sample, first_sample + num_samples), the record
 * d_rays[(slot * num_samples + s) * 64 + lane] = the ray of sample first_sample + s of that pixel,
 * with tmin = 0.001f and tmax = FLT_MAX (the integrators' RayLimits).  A lane outside the image
 * writes an all-zero record, which sp_scene_trace_rays answers as a miss without a walk.  The
 * records go to sp_scene_trace_rays as they are, and their o and d to sp_scene_radiance_rays.
 *
 * sp_scene_features: each pixel's lane loops over its samples i = 0 .. n - 1 and intersects the
 * camera ray of each with the geometry, by the render's own closest-hit walk with the integrators'
 * limits.  GEOMETRY ONLY, as a ray query: lights are not intersected, so a sphere light in front of
 * geometry is not in the buffers.  n is samples_per_pixel, or that slot's entry of tile_samples
 * (host, copied before return) / d_tile_samples (device) when one of them is given -- what
 * sp_adaptive_tile_samples returns after adaptive rounds.
 *
 * Let H be the samples that hit, in sample order.  All arithmetic is float32 without contraction;
 * a sum takes its first term as it is and adds the others in order.
 *   d_ids       4 x int32 per pixel: kind (SP_PRIM_*), index and material of SAMPLE 0's hit as a ray
 *               query reports them, or -1, -1, -1 when sample 0 misses; the fourth word is |H|
 *   d_coverage  1 float: (float)|H| / (float)n
 *   d_depth     1 float: (t_0 + t_1 + ...) over H / (float)|H|; directions are unit vectors, so t
 *               is the distance from the camera origin
 *   d_normal    3 floats: the sum over H of the shading normal (what sp_scene_trace_rays' d_normals
 *               holds) / (float)|H|; not renormalised
 *   d_albedo    3 floats: the sum over H of a(material) / (float)|H|, a(m)[c] =
 *               lambert_albedo[c] * 3.14159274f (sp_material_desc holds the albedo over pi); for
 *               SP_MAT_CLEARCOAT the lambert_albedo of its base material
 * |H| == 0, n == 0 or a pixel outside the image: every float is +0 and the ids are -1, -1, -1, 0.
 * Layout: tile-packed like the image, [slot][lane][channels].  Each of the five pointers is
 * optional, at least one must be given, and work that only an absent output needs is skipped (no
 * hit is finished when neither normal nor albedo is wanted).  Equal-distance ties resolve as in a
 * render of this residency; t does not depend on the walk.
 *
 * Validation comes first and changes nothing, in this order: null scene or params; struct_size (and
 * that of stats when given) and reserved words; num_tiles < 0 (and a sample range that ends past
 * 2^32); the tile-list rules of sp_render_tiles; both tile_samples and d_tile_samples; a camera with
 * another film size or a non-finite value; no output pointer; a device pointer that is misaligned
 * (16 bytes for d_rays and d_ids, 4 for the others) -- all SP_ERR_ARG; then a scene that is not
 * resident, SP_ERR_STATE.  num_tiles == 0 (and num_samples == 0 for the rays) succeeds and launches
 * nothing.  A BVH whose stacks do not fit the LDS is SP_ERR_UNSUPPORTED as for a render.
 *
 * Ordering and locking as sp_scene_trace_rays: the scene's lock; `stream` waits for the previous
 * call on the scene; with stats == NULL the call only enqueues.  Device lists and outputs must stay
 * valid until the work has run.  With stats the call waits and fills them.  The calls see what is
 * resident (a moved mesh, edited materials), leave progress objects valid and keep no memory on the
 * scene beyond the scratch a render uses.
 *
 * The _host forms take host arrays for the outputs (no alignment is asked of them): they allocate
 * device buffers, copy, run, wait and copy back.  The C++ header (simplepath_amd.hpp) needs no
 * wrapper for these calls: the structs are used as they are. */
#define SP_HAS_FEATURES 1

typedef struct sp_camera_ray_params {  /* zero-initialise; struct_size = sizeof */
    uint32_t              struct_size;       /* a size the library does not know => SP_ERR_ARG */
    uint32_t              first_sample;      /* the sample index of record s = 0 */
    uint32_t              num_samples;
    int32_t               reserved0;         /* must be 0 */
    const int32_t*        tile_ids;          /* as sp_render_params: host list, or */
    const int32_t*        d_tile_ids;        /* device list, or both NULL = every tile */
    int64_t               num_tiles;
    const sp_camera_desc* camera;            /* HOST, optional: this call's camera */
    void*                 stream;            /* hipStream_t, NULL = default stream */
    int32_t               reserved[4];       /* must be 0 */
} sp_camera_ray_params;                      /* 72 bytes */

typedef struct sp_feature_params {     /* zero-initialise; struct_size = sizeof */
    uint32_t              struct_size;       /* a size the library does not know => SP_ERR_ARG */
    uint32_t              samples_per_pixel; /* n of every slot, unless per-tile counts are given */
    const int32_t*        tile_ids;          /* as sp_render_params: host list, or */
    const int32_t*        d_tile_ids;        /* device list, or both NULL = every tile */
    int64_t               num_tiles;
    const uint32_t*       tile_samples;      /* HOST, one count per slot, or */
    const uint32_t*       d_tile_samples;    /* DEVICE, or both NULL = samples_per_pixel */
    const sp_camera_desc* camera;            /* HOST, optional: this call's camera */
    void*                 stream;            /* hipStream_t, NULL = default stream */
    int32_t*              d_ids;             /* DEVICE (the _host form: host), 16-byte aligned; 4 words per pixel */
    float*                d_coverage;        /* 1 float per pixel */
    float*                d_depth;           /* 1 float per pixel */
    float*                d_normal;          /* 3 floats per pixel */
    float*                d_albedo;          /* 3 floats per pixel */
    int32_t               reserved[4];       /* must be 0 */
} sp_feature_params;                         /* 120 bytes */

typedef struct sp_feature_stats {      /* struct_size set by the caller */
    uint32_t struct_size;
    int32_t  launches;                 /* kernel launches issued (0 when there was nothing to do) */
    uint64_t camera_rays;              /* features: rays walked (pixels inside the image x their n);
                                          camera rays: records written */
    uint64_t hits;                     /* features: the sum of |H| over the pixels; camera rays: 0 */
    float    kernel_ms;                /* HIP-event time of the kernel */
    int32_t  stack_depth;              /* LDS traversal-stack words per lane of the closest-hit walk */
} sp_feature_stats;                    /* 32 bytes */

/* d_rays: DEVICE, num_tiles * num_samples * 64 records, 16-byte aligned */
int  sp_scene_camera_rays(sp_scene* scene, const sp_camera_ray_params* params, sp_ray* d_rays, sp_feature_stats* stats /* may be NULL */);
int  sp_scene_camera_rays_host(sp_scene* scene, const sp_camera_ray_params* params, sp_ray* h_rays, sp_feature_stats* stats /* may be NULL */);
int  sp_scene_features(sp_scene* scene, const sp_feature_params* params, sp_feature_stats* stats /* may be NULL */);
/* the five output pointers are host arrays; waits for the work */
int  sp_scene_features_host(sp_scene* scene, const sp_feature_params* params, sp_feature_stats* stats /* may be NULL */);

/* ---- denoising: the edge-avoiding a-trous wavelet filter on tile-packed frames -------------------
 * A scene-free object: the filter is an image operator and reads nothing of a scene.  It consumes
 * what sp_render_tiles and sp_scene_features write -- tile-packed [slot][lane][channels], lane = the
 * pixel's Morton index in its 8x8 tile, tile id = ty * tiles_x + tx -- in place on the device, in
 * stream order.  A 5x5 B3-spline kernel is applied with steps 1, 2, 4, ...; colour, normal, depth
 * and coverage differences stop it at edges; the albedo is divided out before and multiplied back
 * after, so textures and material colour are not blurred.
 *
 * THE RULE.  All arithmetic is float32 with no contraction, in the operand order written.  p is a
 * pixel inside the image that belongs to a listed tile slot; its inputs are c_p[3] (colour), a_p[3]
 * (albedo), n_p[3] (normal), z_p (depth), k_p (coverage).
 *
 * Prepare.  With SP_DENOISE_DEMODULATE (needs d_albedo and d_coverage), per channel
 *     s = (k_p * a_p[ch]) + (1.0f - k_p)
 *     m_p[ch] = s > albedo_floor ? s : albedo_floor          (a NaN gives the floor)
 *     x0_p[ch] = c_p[ch] / m_p[ch]
 * without the flag x0_p = c_p and m is unused.
 *     g_p = 1.0f / (sigma_depth * (z_p > depth_floor ? z_p : depth_floor))
 *
 * Level i = 0 .. iterations - 1, constants computed once on the host in float32:
 *     step s = 1 << i;  sc = sigma_color * 2^-i (exact scaling);  inv_c = 1.0f / (sc * sc)
 *     inv_n = 1.0f / (sigma_normal * sigma_normal);  inv_k = 1.0f / (sigma_coverage * sigma_coverage)
 * Taps (dx, dy) in {-2..2}^2, dy the outer loop from -2, dx the inner loop from -2; the tap pixel is
 * q = (x + dx*s, y + dy*s).  A tap is skipped when q is outside the image or q's tile is not in the
 * list.  h = {1/16, 1/4, 3/8, 1/4, 1/16}, h2 = h[dx+2] * h[dy+2] (exact).  The four edge terms:
 *     d = x_q - x_p per channel;  ec = ((d0*d0 + d1*d1) + d2*d2) * inv_c
 *     d = n_q - n_p;              en = ((d0*d0 + d1*d1) + d2*d2) * inv_n
 *     dz = (z_q - z_p) * g_p;     ed = dz * dz
 *     dk = k_q - k_p;             ek = (dk * dk) * inv_k
 * A term whose guide pointer is NULL contributes +0 (every term is >= 0 or NaN, so the bits of the
 * sum are those of the sum without it).
 *     e = ((ec + en) + ed) + ek;   w = h2 * expf(-e)   (glibc's expf, bit for bit: lm_expf)
 * The tap counts only if w > 0 (NaN and 0 fail the comparison).  acc[ch] and W start at +0; for
 * each counted tap, in tap order, acc[ch] = acc[ch] + w * x_q[ch] and W = W + w.  Then
 *     x(i+1)_p[ch] = W > 0 ? acc[ch] / W : x(i)_p[ch]
 * Consequences: a NaN or infinite colour never spreads to its neighbours (its taps have e = NaN or
 * +inf, so w is NaN or 0), and a non-finite centre pixel passes through unchanged (none of its taps
 * counts, so W = 0).
 *
 * Finish.  out_p[ch] = x(L)_p[ch] * m_p[ch] with demodulation, x(L)_p[ch] without.  Lanes of a
 * listed tile that lie outside the image write +0.
 *
 * Parameters.  iterations 1 .. 8; sigma_color finite and > 0; sigma_normal, sigma_depth and
 * sigma_coverage finite and > 0 wherever their guide is given (not looked at otherwise);
 * albedo_floor and depth_floor finite and >= 0, 0 meaning 0.01f and 1e-3f (conventions, not
 * measurements).
 *
 * THE OBJECT.  sp_denoiser_create takes the device, the frame size and the tile list in the three
 * forms of sp_render_tiles: a host list (checked: an id out of range or a repeated id is SP_ERR_ARG;
 * copied before return), a device list, or neither for every tile.  It touches no device: the
 * object's memory -- two ping-pong planes of 16 bytes per pixel slot (x and z), a packed guide
 * record of 16 bytes per pixel slot (n and k), its own copy of the list, and the inverse map
 * slot_of_tile[tiles_x * tiles_y] (-1: absent) built by a small kernel -- is allocated and filled
 * by the object's first run, on that run's stream, ahead of its kernels.  A device list is read
 * then and not afterwards: it must hold the ids until the first run has executed.  In a device list
 * an id outside the frame makes that slot's outputs +0, and a repeated id is served to taps from
 * its lowest slot (atomicMin): every tap, the centre one included, reads q through the map, while
 * x_p, n_p, z_p, k_p are the slot's own; the result is deterministic.
 * sp_denoiser_device_bytes is what the object holds once it has run.
 *
 * sp_denoiser_run: d_color and d_out are required, [num_tiles][64][3] floats; d_albedo and d_normal
 * [num_tiles][64][3], d_depth and d_coverage [num_tiles][64], each optional.  d_out may equal
 * d_color; d_out may overlap no input in any other way.  The call is enqueued on `stream`.  It
 * waits only for the object's own previous run (the scratch is reused); ORDERING AGAINST THE CALLS
 * THAT PRODUCE THE INPUTS IS ORDINARY STREAM ORDER: enqueue sp_render_tiles, sp_scene_features and
 * this call on one stream, or order the streams with events.  Inputs and output must stay valid
 * until the work has run.  With stats == NULL the call only enqueues; with stats it waits and
 * fills them.  Launches: one prepare kernel, one per level, the finish fused into the last level
 * (the first run adds the map's).  sp_denoiser_run_host takes host arrays in the same fields (no
 * alignment is asked of them), allocates device buffers, copies, runs, waits and copies back.
 * Calls on one object run one at a time (the object's lock).
 *
 * Validation comes first and changes nothing, in this order: null arguments; struct_size values
 * (that of stats when given), reserved words and unknown flags; counts (width or height < 1, device
 * < 0, num_tiles < 0 or above 2^31 - 1) and the tile-list rules; iterations out of range, then a
 * sigma or a floor out of range; a missing d_color or d_out, then the demodulate flag without
 * d_albedo or d_coverage; a device pointer not 4-byte aligned, then a forbidden overlap -- all
 * SP_ERR_ARG with a message naming the field.  Only then device errors, SP_ERR_HIP.  num_tiles == 0
 * succeeds and launches nothing. */
#define SP_HAS_DENOISE 1
#define SP_DENOISE_DEMODULATE 1            /* sp_denoise_params.flags */
#define SP_DENOISE_MAX_ITERATIONS 8

typedef struct sp_denoiser sp_denoiser;

typedef struct sp_denoiser_params {    /* zero-initialise; struct_size = sizeof */
    uint32_t       struct_size;        /* a size the library does not know => SP_ERR_ARG */
    int32_t        device;
    int32_t        width, height;      /* the frame, in pixels */
    const int32_t* tile_ids;           /* as sp_render_params: host list, or */
    const int32_t* d_tile_ids;         /* device list, or both NULL = every tile */
    int64_t        num_tiles;
    int32_t        reserved[4];        /* must be 0 */
} sp_denoiser_params;                  /* 56 bytes */

typedef struct sp_denoise_params {     /* zero-initialise; struct_size = sizeof */
    uint32_t     struct_size;          /* a size the library does not know => SP_ERR_ARG */
    int32_t      iterations;           /* 1 .. SP_DENOISE_MAX_ITERATIONS */
    int32_t      flags;                /* SP_DENOISE_DEMODULATE or 0; anything else SP_ERR_ARG */
    int32_t      reserved0;            /* must be 0 */
    const float* d_color;              /* DEVICE (the _host form: host), 3 floats per pixel */
    const float* d_albedo;             /* 3 floats per pixel, optional */
    const float* d_normal;             /* 3 floats per pixel, optional */
    const float* d_depth;              /* 1 float per pixel, optional */
    const float* d_coverage;           /* 1 float per pixel, optional */
    float*       d_out;                /* 3 floats per pixel; may equal d_color */
    float        sigma_color, sigma_normal, sigma_depth, sigma_coverage;
    float        albedo_floor, depth_floor; /* 0: 0.01f and 1e-3f */
    void*        stream;               /* hipStream_t, NULL = default stream */
    int32_t      reserved[4];          /* must be 0 */
} sp_denoise_params;                   /* 112 bytes */

typedef struct sp_denoise_stats {      /* struct_size set by the caller */
    uint32_t struct_size;
    int32_t  launches;                 /* kernel launches issued (0 when there was nothing to do) */
    uint64_t pixels;                   /* pixels inside the image, over the listed slots */
    uint64_t taps;                     /* counted taps (w > 0), summed over levels and pixels */
    float    kernel_ms;                /* HIP-event time of the run's kernels */
    int32_t  reserved;
} sp_denoise_stats;                    /* 32 bytes */

int  sp_denoiser_create(const sp_denoiser_params* params, sp_denoiser** out);
void sp_denoiser_free(sp_denoiser* denoiser);
int  sp_denoiser_device_bytes(const sp_denoiser* denoiser, int64_t* out);
int  sp_denoiser_run(sp_denoiser* denoiser, const sp_denoise_params* params, sp_denoise_stats* stats /* may be NULL */);
/* the six buffer pointers are host arrays; waits for the work */
int  sp_denoiser_run_host(sp_denoiser* denoiser, const sp_denoise_params* params, sp_denoise_stats* stats /* may be NULL */);

/* ---- relighting: light, material and sky edits -------------------------------------------------
 * Three calls change what a look-dev session changes most, without a new upload: the materials,
 * the light list, and an image environment light (its pixels, its max_radiance, its rotation).  The
 * contract is refit's: an edited resident scene is, in every bit, what a fresh upload of the edited
 * descriptor would be.  The image light's tables (the constructor's clamped image, its
 * Distribution2D and the guide tables) are built on the device, byte for byte what the upload's
 * host builder makes (sp_scene_env_check).
 *
 * Common to all three, as for sp_scene_update_mesh: validation comes first and changes nothing;
 * the scene's host copy is then overwritten, so sp_scene_get_desc and a later upload see the edit;
 * a scene that is not resident is done at that point.  A resident scene takes the scene's lock,
 * waits for queued work, rewrites the device arrays, and invalidates every progress object made on
 * the scene (SP_ERR_STATE).  A device failure is SP_ERR_HIP and leaves no resident scene (the host
 * scene is already the edited one: upload again).  The geometry trees, the primitive records, the
 * RSQRTSS table and the camera are not touched.
 *
 * sp_scene_set_materials -- validation order: null scene; null `materials` with a nonzero count;
 * num_materials other than the scene's (triangles and shapes index the materials); each material
 * in turn: unknown kind, a clearcoat's base out of range; then a clearcoat whose base is a clearcoat
 * (SP_ERR_UNSUPPORTED, as at upload).  Pointers from an earlier sp_scene_get_desc are stale
 * afterwards (desc.materials is rebuilt).  The device side is one copy into the resident array.
 *
 * sp_scene_set_lights -- replaces the whole list; count and kinds may change.  Validation order:
 * null scene; num_lights < 0; null `lights` with a nonzero count; each light in turn: unknown kind,
 * an image light whose `image` names no env image of the scene.  Pointers from an earlier
 * sp_scene_get_desc are stale afterwards.  On a resident scene the light accelerator is built
 * again by the upload's own code (sphere lights partitioned from unbounded ones, the reference-order
 * light BVH, the slot table, parent links when stackless) into the scene's light blocks, and the walk
 * plan is recomputed from the new light depth: stack sizes and sp_bvh_info follow.  A light list so
 * deep that the walk would have to change between stack and parent links is SP_ERR_UNSUPPORTED
 * before anything changes (upload again).
 *
 * sp_scene_set_env_image -- replaces or appends one env image.  `image` is an existing index, or
 * num_env_images to append (so a scene loaded without a sky can get one; sp_scene_set_lights then
 * names it; removal is not offered).  At most one of `pixels` (host) and `d_pixels` (device) may be
 * given, in sp_env_image layout, already multiplied by the light's radiance; with either, width
 * and height are the new map's size.  With neither the current pixels are kept (width and height
 * must be 0 or the current size): when max_radiance is bit-equal to the current one only the two
 * matrices of the resident record change (rebuilt = 0: rotating the sky costs one small copy), else
 * the tables are rebuilt from the host's unclamped pixels.  Device pixels are copied back to the
 * host scene, which stays the truth.  Same dimensions: every table is rewritten in place and
 * sp_scene_device_bytes does not change (unless the map gains or loses its guide tables); other
 * dimensions: the map's blocks are released and allocated again.  Validation order: null scene or
 * update; struct sizes (the update's, and that of stats when given); reserved fields; `image`
 * outside [0, num_env_images]; both pixel pointers given; with pixels, width or height < 1 or above
 * 32767; without pixels, an append, or a size that is neither 0 nor the current one; all SP_ERR_ARG;
 * last, d_pixels on a scene that is not resident, SP_ERR_STATE.  Pointers from an earlier
 * sp_scene_get_desc are stale when the image count or an image's size changed.
 * sp_upload_params.env_replay of the resident upload still suppresses the guide tables. */
#define SP_HAS_RELIGHT 1

int  sp_scene_set_materials(sp_scene* scene, const sp_material_desc* materials, int32_t num_materials);
int  sp_scene_set_lights(sp_scene* scene, const sp_light_desc* lights, int32_t num_lights);

typedef struct sp_env_update {        /* zero-initialise; struct_size = sizeof */
    uint32_t     struct_size;         /* a size the library does not know => SP_ERR_ARG */
    int32_t      image;               /* an existing index, or num_env_images to append */
    int32_t      width, height;       /* the new map's size (with pixels); else 0 or the current size */
    const float* pixels;              /* HOST, width * height * 3, sp_env_image layout, or NULL */
    const void*  d_pixels;            /* DEVICE, the same layout, or NULL */
    float        max_radiance;        /* as sp_env_image */
    int32_t      reserved0;           /* must be 0 */
    sp_linear    light_to_world;      /* the light's rotation */
    sp_linear    world_to_light;      /* its inverse */
    int32_t      reserved[4];         /* must be 0 */
} sp_env_update;                      /* 128 bytes */

typedef struct sp_env_stats {         /* struct_size set by the caller */
    uint32_t struct_size;
    int32_t  rebuilt;                 /* 0: host scene only, or the matrices alone; 1: the resident tables were rebuilt */
    int32_t  guided;                  /* the rebuilt map's rows and marginal are ordered (no NaN): it can have guide tables */
    int32_t  reserved;
    float    ms_upload, ms_clamp, ms_func, ms_rows, ms_marginal, ms_guides, ms_total; /* device stages */
    int32_t  reserved2;
    int64_t  scratch_bytes;           /* peak device scratch, all released before the call returns */
} sp_env_stats;                       /* 56 bytes */

/* stats may be NULL.  Passing stats makes the call wait for the device after each stage so that
 * ms_* hold stage times. */
int  sp_scene_set_env_image(sp_scene* scene, const sp_env_update* update, sp_env_stats* stats);

/* The tables of one env image, in the order of sp_env_check.hash. */
enum { SP_ENV_RADIANCE = 0, SP_ENV_COND_FUNC = 1, SP_ENV_COND_CDF = 2, SP_ENV_COND_INT = 3, SP_ENV_MARG_FUNC = 4,
       SP_ENV_MARG_CDF = 5, SP_ENV_COND_GUIDE = 6, SP_ENV_MARG_GUIDE = 7, SP_ENV_SCALARS = 8, SP_ENV_TABLES = 8 };
enum { SP_ENV_BUILDER_HOST = 0, SP_ENV_BUILDER_DEVICE = 1 };

typedef struct sp_env_check {         /* struct_size set by the caller */
    uint32_t struct_size;
    int32_t  builder;                 /* SP_ENV_BUILDER_*: who made the tables that were hashed */
    int32_t  width, height, nu, nv;
    int32_t  guided;                  /* rows and marginal ordered */
    int32_t  cond_bits, marg_bits;
    uint32_t marg_int_bits;           /* the marginal's integral, as bits */
    int64_t  mismatches;              /* resident words that differ from the host builder's (0 for the build check) */
    int32_t  first_table;             /* SP_ENV_* of the first mismatch (SP_ENV_SCALARS: guided, bits or marg_int), -1: none */
    int32_t  reserved;
    int64_t  first_index;             /* its word index in that table, -1: none */
    uint64_t hash[10];                /* FNV-1a 64 per table (0: table absent); [8], [9] are 0 */
} sp_env_check;                       /* 144 bytes */

/* Reads the resident tables of env image `image` back, builds the host's from the scene's current
 * host pixels, and compares word for word (radiance as float4 words).  Guide tables the resident
 * scene does not hold (env_replay, or an unguided map) are not compared.  SP_ERR_STATE when the
 * scene is not resident; SP_ERR_ARG for an image out of range. */
int  sp_scene_env_check(sp_scene* scene, int32_t image, sp_env_check* out);
/* The host half alone, no device: the hashes of what the upload's host builder makes. */
int  sp_scene_env_build_check(const sp_scene* scene, int32_t image, sp_env_check* out);

/* RSQRTSS emulation table.  The reference normalises with RSQRTSS + one Newton step
 * (math/Math.h:205); RSQRTSS is a hardware table whose outputs differ between CPU vendors, so the
 * reference's images are those of the CPU it ran on.  By default scenes are built (host) and
 * rendered (device) with the table of this host's CPU, captured at start-up.  sp_rsqrt_table_set
 * installs another CPU's table -- e.g. the one recorded with a golden image made elsewhere -- for
 * every scene loaded and uploaded afterwards (entries == NULL: back to this host's table).
 * entries holds 2 << bits words: [exponent parity][leading mantissa bits]. */
int  sp_rsqrt_table_get(uint32_t* entries, int64_t capacity, int32_t* bits, uint32_t* zero_result,
                        uint32_t* denorm_result);
int  sp_rsqrt_table_set(const uint32_t* entries, int32_t bits, uint32_t zero_result, uint32_t denorm_result);

/* Numerics self-checks used by the tests (no GPU needed). */
int  sp_rsqrt_table_info(int32_t* mantissa_bits, int32_t* verified);
float sp_host_rsqrt_emulated(float x); /* table emulation of RSQRTSS, host-evaluated */

#ifdef __cplusplus
}
#endif
#endif /* SIMPLEPATH_HIP_H */
