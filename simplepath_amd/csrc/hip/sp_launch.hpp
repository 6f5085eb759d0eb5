// sp_launch.hpp -- the host-visible launch interface of the megakernel and its helper kernels:
// what sp_capi.hip calls, declared once.  The definitions (sp_mega.hip, sp_adaptive.hip) include
// it through sp_mega.hpp or directly; it needs the argument structs only, not the kernels' code.
#pragma once
#include "sp_device.hpp"

#include <hip/hip_runtime.h>

namespace spd {

// The persistent megakernel's families: a one-shot render (sp_render_kernel), a call on a progress
// object (sp_resume_kernel: needs ResumeArgs) and on an adaptive one (sp_adapt_kernel: AdaptArgs too),
// many views of the scene in one launch (sp_views_kernel: needs ViewArgs; no Mandelbrot), radiance
// along a caller's rays (sp_radiance_kernel, sp_radiance.hpp: needs RadianceArgs; no Mandelbrot;
// launched by launch_radiance below).
enum class MegaFamily { Render, Resume, Adapt, Views, Radiance };

// A family's kernel for an integrator.  variant = requested waves per SIMD of its
// __launch_bounds__ (DirectLighting 1..4, IterativeRRNEE 2..4; the others have one each).
const void* mega_kernel(MegaFamily family, int integ, int variant);
// The tail kernels.  variant 0: the sample chunks' fused form (sp_fused_kernel), 3 / 4: the tail
// kernel at 3 / 4 waves, -4: the tail kernel with an image light's replay (4 waves)
const void* tail_kernel(int variant);
// Resident blocks per CU of one of these kernels with lds_bytes of dynamic LDS (at least 1), and
// its static LDS (libm tables, the rho sink, IterativeRRNEE's served-estimate rows): the 160 KB
// guard and the LDS occupancy cap count it beside the dynamic part.
int    kernel_blocks_per_cu(const void* kernel, size_t lds_bytes);
size_t kernel_static_lds(const void* kernel);

// res / ad / vw: what the family needs (nullptr for the others)
hipError_t launch_mega(MegaFamily family, const Scene& sc, const RenderArgs& args, const ResumeArgs* res, const AdaptArgs* ad,
                       int integ, int variant, int blocks, size_t lds_bytes, hipStream_t stream, const ViewArgs* vw = nullptr);
hipError_t launch_tail(const Scene& sc, const RenderArgs& args, int variant, int blocks, size_t lds_bytes, hipStream_t stream);
// The radiance family (sp_radiance.hip): its kernel for an integrator (nullptr: Mandelbrot) and its
// launch; args.num_tiles = ceil(ra.num_rays / 64) queue items, args.spp = samples per ray.  A missing
// kernel is hipErrorInvalidDeviceFunction, never another kernel.
const void* radiance_kernel(int integ, int variant);
hipError_t  launch_radiance(const Scene& sc, const RenderArgs& args, const RadianceArgs& ra, int integ, int variant, int blocks,
                            size_t lds_bytes, hipStream_t stream);

// tile order: the one-sample probe of an integrator's megakernel, then the queue order
bool       has_probe(int integ);
hipError_t launch_probe(const Scene& sc, const RenderArgs& args, int integ, int variant, int blocks, size_t lds_bytes,
                        hipStream_t stream);
hipError_t launch_tile_order(float* tile_time, int64_t n_tiles, float factor, int tiles_x, int step, int32_t* order,
                             hipStream_t stream);

// adaptive rounds (sp_adaptive.hip): selection, list, resolve
hipError_t launch_adapt_select(const AdaptArgs& ad, const SelectArgs& sa, float* err, uint32_t* flag, hipStream_t stream);
hipError_t launch_adapt_compact(const AdaptArgs& ad, const int32_t* order, int64_t n_tiles, hipStream_t stream);
hipError_t launch_adapt_resolve(const ResumeArgs& res, const AdaptArgs& ad, bool skip_active, int64_t n_tiles, float* out,
                                hipStream_t stream);

} // namespace spd
