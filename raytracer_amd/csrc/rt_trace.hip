// rt_trace.hip -- the traversal kernels of the library and the small kernels around them, a translation unit of their own:
//   rt_trace_binary.inl   k_trace (the reference's walk: binary BVH, near child first), k_trace_monster
//   rt_wide_grid.inl      the exactness argument the 4-wide walks share (their format -- grid, node records, leaf gates, WideTuning -- is rt_wide_format.h,
//                         which every unit has through rt_device_core.h; the host builds the trees in rt_scene_prepare.h)
//   rt_wide_walk.h        the device parts the 4-wide walks share: slab test, hand-over lists, request ray, fold, interior step, mesh leaf (pair, gate, acceptance), finish, tallies
//   rt_trace_wide.inl     k_trace_wide (4-wide tree of a single-mesh scene; the rays it does not decide go through the reference's walk in the same launch)
//   rt_trace_packet.inl   k_trace_packet (the camera rays of a dense batch: one wave walks the 4-wide tree for an 8 x 8 pixel block, the node is uniform)
//   rt_beam_lists.inl     k_beam_lists_build (a still camera's per-tile leaf lists, which k_trace_packet scans in place of its walk; rt_beam_lists.h)
//   rt_trace_wide2.inl    k_trace_wide2 (4-wide top-level tree over 4-wide mesh trees)
//   rt_generate.inl       k_generate (camera rays, slot-per-pixel pipeline)
//   rt_post.inl           post-process, bloom, block errors, texture evaluation
//   rt_kat.inl            known-answer hooks (rtgpu_kat*)
//   rt_query.inl          batched ray queries around the walks above (rtgpu_trace_rays)
//   rt_denoise.inl        the a-trous filter (rtgpu_filter_atrous, rtgpu_denoise)
//   rt_temporal.inl       temporal accumulation (rtgpu_temporal_accumulate, rtgpu_denoise_temporal)
//   rt_raysource.inl      the primary-ray sources: k_generate fed from a table of rays (rtgpu_set_ray_source) or of rays with footprints and a thin lens
//                         (rtgpu_set_lens_source), the tables' checks, the camera's rays and footprints and a lens table's rays written out
// The host side (rt_runtime.hip) launches them through the declarations of rt_trace_kernels.h.
//
// Compile: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off
#define RT_DEVICE_KERNELS 1
#include "rt_trace_kernels.h"
#include "rt_vcm_state.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

using namespace rtd;

#include "rt_generate.inl"
#include "rt_trace_binary.inl"
#include "rt_wide_grid.inl"
#include "rt_wide_walk.h"
#include "rt_trace_wide.inl"
#include "rt_trace_packet.inl"
#include "rt_beam_lists.inl"
#include "rt_trace_wide2.inl"
#include "rt_kat.inl"
#include "rt_query.inl"
#include "rt_post.inl"

// the instantiations the host side launches
#define RT_X(S, C) template __global__ void RT_TRACE_ATTR(S) k_trace<S, C, false> RT_K_TRACE_ARGS;
RT_K_TRACE_INSTANCES(RT_X)
#undef RT_X
#define RT_X(S, D, L) template __global__ void RT_TRACE_ATTR(S) k_trace_wide<S, D, L> RT_K_TRACE_WIDE_ARGS;
RT_K_TRACE_WIDE_INSTANCES(RT_X)
#undef RT_X
#define RT_X(S) template __global__ void RT_TRACE_ATTR(S) k_trace_wide2<S> RT_K_TRACE_WIDE2_ARGS;
RT_K_TRACE_WIDE2_INSTANCES(RT_X)
#undef RT_X
// (last: the kernels above keep the places in the code object that they had before these existed)
#define RT_X(S) template __global__ void RT_TRACE_ATTR(S) k_trace<S, true, true> RT_K_TRACE_ARGS;
RT_K_TRACE_PER_RAY_INSTANCES(RT_X)
#undef RT_X

// (behind everything else, for the same reason)
#include "rt_denoise.inl"
#include "rt_temporal.inl"
#include "rt_raysource.inl"
