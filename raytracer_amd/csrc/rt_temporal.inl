// rt_temporal.inl -- kernels behind rtgpu_temporal_accumulate / rtgpu_denoise_temporal (include/rtgpu.h; host side: rt_runtime_temporal.inl).  Included by
// rt_trace.hip behind rt_denoise.inl, whose helpers it uses and whose -ffp-contract=off it shares: every a * b + c below is a rounded multiply and a rounded add.
// Temporal accumulation, the other half of SVGF: the world position of a pixel's first hit goes through the previous frame's worldToScreen, the previous
// frame's accumulated pair (A, B) and history length are fetched bilinearly from the four pixels around that point -- each tap tested against the pixel's own
// surface -- and blended with this frame's pair.  The definition stands in include/rtgpu.h; tests/temporal_ref.py is the same text in NumPy float32.
//
//   k_temporal_pack   planar history of a caller (the pure entries) -> the four 16-byte records per pixel the context keeps its own history in:
//                     {A.rgb, length}, {B.rgb, object id}, {N.xyz, valid}, {P.xyz, chain length (0.0f: first-hit guides)}
//   k_temporal        one lane per pixel, a wave = 64 consecutive x of one row.  The current planes are coalesced loads; a tap is four 16-byte gathers, no
//                     branch around it (a tap outside the frame loads the pixel's own address and is dropped by a select, as atrousTap does).  Neighbours
//                     share three of their four taps under coherent motion: the caches do what an LDS tile would.  It writes the planar outputs and,
//                     where asked, the records of the next frame's history and the remodulated image; every per-pixel operation exists once.
//   k_temporal<true>  the scene's objects moved between the two frames (rtgpu_update_objects): the pixel's object id selects an 80-byte record of the motion
//                     table -- one lane-indexed gather of five 16-byte loads; the table holds some hundred objects and neighbours share their object, so it
//                     is served from the caches, mostly as a broadcast -- whose matrix takes position and normal to where that surface point was in the
//                     previous frame.  Projection and the tap tests use the moved pair and the id the object had then; the stored history keeps this
//                     frame's own.  An unmoved object selects its own position and normal: the bits of k_temporal<false>.
//   k_temporal_moments<r>   history clipping: mean and gamma standard deviations of this frame's prepared colours over the (2r + 1)^2 window pixels on the pixel's
//                     own surface, from an LDS tile; two 16-byte records per pixel
//   k_temporal<., true>   the same kernel reading those records (coalesced): the reprojected A is clipped to mu +- g, B shifted along, the history length cut by how
//                     far A was pulled.  A compile-time variant: the two instantiations without it are what they were.
//   k_temporal<true, ., true>   a mesh was deformed between the two frames (rtgpu_temporal_accumulate_deform): three coalesced plane words more per pixel -- the
//                     triangle the first hit lies on and its barycentrics -- and, for lanes on a deformed object, one 36-byte gather (nine dwords: the record is
//                     4-byte aligned) of the triangle as it was when the history was stored.  v0 + u edge1 + v edge2 of that record, through the object's
//                     transform of then, is where the surface point was; the normal is not carried back.  A triangle id outside the record's range, or a range
//                     outside the array, starts the pixel before anything is read.  A compile-time variant of the moving kernels only: the four
//                     instantiations without it are what they were.
//   k_temporal_chain, k_temporal_moments_chain<r>   rtgpu_temporal_accumulate_chain: the same two bodies over chain guides (rt_temporal_body.inl and
//                     rt_temporal_moments_body.inl, each compiled a second time under RT_TEMPORAL_CHAIN) -- the virtual position is projected, the plane tolerance scales with the chain distance, a tap or a window pixel
//                     of another chain length is dropped; the chain length rides in the free lane of the {P.xyz, .} history record

__global__ void __launch_bounds__(RT_BLOCK) k_temporal_pack(const float* __restrict__ prevA, const float* __restrict__ prevB, const float* __restrict__ prevLength,
                                                            const float* __restrict__ prevDepth, const float* __restrict__ prevNormal, const float* __restrict__ prevPosition,
                                                            const uint32_t* __restrict__ prevObjectId, const uint32_t* __restrict__ prevChainLength, uint32_t pixels,
                                                            float4* __restrict__ recA, float4* __restrict__ recB, float4* __restrict__ recN, float4* __restrict__ recP)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pixels) return;
    const size_t n = pixels;
    const bool valid = (__float_as_uint(prevDepth[i]) & 0x7F800000u) != 0x7F800000u;
    recA[i] = make_float4(prevA[3 * (size_t)i], prevA[3 * (size_t)i + 1], prevA[3 * (size_t)i + 2], prevLength[i]);
    recB[i] = make_float4(prevB[3 * (size_t)i], prevB[3 * (size_t)i + 1], prevB[3 * (size_t)i + 2], __uint_as_float(prevObjectId ? prevObjectId[i] : 0u));
    recN[i] = make_float4(prevNormal[i], prevNormal[n + i], prevNormal[2 * n + i], valid ? 1.0f : 0.0f);
    recP[i] = make_float4(prevPosition[i], prevPosition[n + i], prevPosition[2 * n + i], __uint_as_float(prevChainLength ? prevChainLength[i] : 0u));   // (0.0f: first-hit guides)
}

// a history record in one 16-byte load (as atrousColour)
RT_DEV float4 temporalRecord(const float4* __restrict__ src, uint32_t q)
{
    const AtrousLanes lanes = *reinterpret_cast<const AtrousLanes*>(src + q);
    return make_float4(lanes.x, lanes.y, lanes.z, lanes.w);
}

// The colour statistics of history clipping ("Clipping the history", include/rtgpu.h): per pixel the mean and gamma standard deviations of the prepared colours
// over the window pixels that lie on the pixel's own surface.  A block stages its tile and a halo of kRadius into LDS as three 16-byte records -- {c.rgb, depth},
// {N.xyz, id bits}, {P.xyz, valid} -- with the prepare step done once per staged pixel; a record outside the frame is invalid, which is how its window pixel is
// skipped.  Each lane then walks its (2 kRadius + 1)^2 window row by row from LDS with no branch around a neighbour (selects, as atrousTap) and writes
// {mu.rgb, cnt} and {g.rgb, 0}.  Consecutive lanes read consecutive 16-byte records: no bank conflicts.  The window's columns are unrolled, its rows are not:
// with all 49 taps of radius 3 in one basic block the scheduler hoists every LDS load (218 VGPRs, two waves per SIMD) and the kernel takes twice as long
// (profiles/temporal_clip_resources.txt); a row at a time it holds 50 VGPRs, and the 25.5 KB tile lets six blocks -- six waves per SIMD -- share a CU.
// k_temporal_moments and k_temporal_moments_chain: ONE body (rt_temporal_moments_body.inl), compiled twice, as k_temporal's below.
#define RT_TEMPORAL_MOMENTS_KERNEL k_temporal_moments
#define RT_TEMPORAL_CHAIN 0
#include "rt_temporal_moments_body.inl"
#undef RT_TEMPORAL_MOMENTS_KERNEL
#undef RT_TEMPORAL_CHAIN
#define RT_TEMPORAL_MOMENTS_KERNEL k_temporal_moments_chain
#define RT_TEMPORAL_CHAIN 1
#include "rt_temporal_moments_body.inl"
#undef RT_TEMPORAL_MOMENTS_KERNEL
#undef RT_TEMPORAL_CHAIN
template __global__ void RT_TEMPORAL_MOMENTS_ATTR k_temporal_moments<1> RT_K_TEMPORAL_MOMENTS_ARGS;
template __global__ void RT_TEMPORAL_MOMENTS_ATTR k_temporal_moments<2> RT_K_TEMPORAL_MOMENTS_ARGS;
template __global__ void RT_TEMPORAL_MOMENTS_ATTR k_temporal_moments<3> RT_K_TEMPORAL_MOMENTS_ARGS;
template __global__ void RT_TEMPORAL_MOMENTS_ATTR k_temporal_moments_chain<1> RT_K_TEMPORAL_MOMENTS_CHAIN_ARGS;
template __global__ void RT_TEMPORAL_MOMENTS_ATTR k_temporal_moments_chain<2> RT_K_TEMPORAL_MOMENTS_CHAIN_ARGS;
template __global__ void RT_TEMPORAL_MOMENTS_ATTR k_temporal_moments_chain<3> RT_K_TEMPORAL_MOMENTS_CHAIN_ARGS;

// k_temporal and k_temporal_chain: ONE body (rt_temporal_body.inl), compiled twice, as k_shade's is.  The chain blocks are preprocessor blocks, so k_temporal
// is the token stream it was and its four instantiations are the code they were.  k_temporal alone has the third template argument (kDeform).
#define RT_TEMPORAL_KERNEL k_temporal
#define RT_TEMPORAL_CHAIN 0
#include "rt_temporal_body.inl"
#undef RT_TEMPORAL_KERNEL
#undef RT_TEMPORAL_CHAIN
#define RT_TEMPORAL_KERNEL k_temporal_chain
#define RT_TEMPORAL_CHAIN 1
#include "rt_temporal_body.inl"
#undef RT_TEMPORAL_KERNEL
#undef RT_TEMPORAL_CHAIN

template __global__ void RT_ATROUS_ATTR k_temporal<false, false, false>(const TemporalIn, const TemporalOut, uint32_t, uint32_t, const TemporalFrame);
template __global__ void RT_ATROUS_ATTR k_temporal<true, false, false>(const TemporalIn, const TemporalOut, uint32_t, uint32_t, const TemporalFrameMoving);
template __global__ void RT_ATROUS_ATTR k_temporal<false, true, false>(const TemporalIn, const TemporalOut, uint32_t, uint32_t, const TemporalFrameClip<TemporalFrame>);
template __global__ void RT_ATROUS_ATTR k_temporal<true, true, false>(const TemporalIn, const TemporalOut, uint32_t, uint32_t, const TemporalFrameClip<TemporalFrameMoving>);
template __global__ void RT_ATROUS_ATTR k_temporal<true, false, true>(const TemporalIn, const TemporalOut, uint32_t, uint32_t, const TemporalFrameDeform);
template __global__ void RT_ATROUS_ATTR k_temporal<true, true, true>(const TemporalIn, const TemporalOut, uint32_t, uint32_t, const TemporalFrameClip<TemporalFrameDeform>);
template __global__ void RT_ATROUS_ATTR k_temporal_chain<false, false>(const TemporalIn, const TemporalOut, uint32_t, uint32_t, const TemporalFrame, const TemporalChainPlanes);
template __global__ void RT_ATROUS_ATTR k_temporal_chain<true, false>(const TemporalIn, const TemporalOut, uint32_t, uint32_t, const TemporalFrameMoving, const TemporalChainPlanes);
template __global__ void RT_ATROUS_ATTR k_temporal_chain<false, true>(const TemporalIn, const TemporalOut, uint32_t, uint32_t, const TemporalFrameClip<TemporalFrame>, const TemporalChainPlanes);
template __global__ void RT_ATROUS_ATTR k_temporal_chain<true, true>(const TemporalIn, const TemporalOut, uint32_t, uint32_t, const TemporalFrameClip<TemporalFrameMoving>, const TemporalChainPlanes);
