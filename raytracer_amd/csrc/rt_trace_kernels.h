// rt_trace_kernels.h -- the kernels rt_trace.hip defines (traversal, camera rays, post-process, known-answer hooks), declared for the host side
// (rt_runtime.hip), and the argument structs both sides share.  rt_trace.hip includes it for the structs only (RT_DEVICE_KERNELS).
#pragma once
#include "rt_trace_common.h"
#include "rt_beam_lists.h"

// known-answer hooks (rt_kat.inl): function ids = the ids the fixtures of tests/golden/*.kat carry in their headers (tests/golden/README.md)
enum
{
    KAT_SIN_LANE = 1, KAT_SINCOS = 2, KAT_FASTLOG = 3, KAT_FASTACOS = 4, KAT_FASTATAN2 = 5,
    KAT_FLOAT_NORMAL2 = 6, KAT_HEMISPHERE_COS = 7, KAT_SPHERE = 8, KAT_CIRCLE = 9, KAT_ORTHO_BASIS = 10,
    KAT_FRESNEL_DIELECTRIC = 11, KAT_FRESNEL_METAL = 12, KAT_REFRACT3 = 13, KAT_REFLECT3 = 14,
    KAT_BOX_RAY = 20, KAT_BOX_RAY_TWOSIDED = 21, KAT_TRIANGLE_RAY = 22, KAT_MAKE_RAY = 23, KAT_TRANSFORM_RAY = 24,
    KAT_FAST_INVERSE = 25, KAT_TRANSFORM_SCALED = 26, KAT_FRAME_COMPOSE = 27,
    KAT_SHAPE_INTERSECT = 30, KAT_SHAPE_SAMPLE = 31, KAT_SHAPE_PDF = 32, KAT_SHAPE_EVAL = 33,
    KAT_LIGHT_ILLUMINATE = 40, KAT_LIGHT_RADIANCE = 41, KAT_LIGHT_EMIT = 42, KAT_LIGHT_ILLUMINATE_BIDIR = 43, KAT_LIGHT_RADIANCE_BIDIR = 44,
    KAT_BSDF_SAMPLE = 50, KAT_BSDF_EVALUATE = 51, KAT_BSDF_PDFS = 52,
    KAT_CAMERA_RAY = 60, KAT_CAMERA_FILM = 61, KAT_FILM_SPLAT = 62, KAT_PACKED_PHOTON = 63, KAT_HSV_TO_RGB = 64,
};
#define RT_KAT_MESH_STACK 64

struct PostScale { float c[3]; };
struct BlurPlan { uint32_t n, wl, wu; float m; };
struct BloomLevels { const float* level[5]; };
struct ErrorRow { uint32_t block, y; };

// The degenerate-ray rule of the ray queries (include/rtgpu.h): a non-finite origin, a direction whose squared length (dot3, the sum Ray() takes the
// root of) is 0 or not finite, or a maxDistance that is NaN or <= 0.  The host-side check of rtgpu_trace_rays and k_query_load (rt_query.inl) share it.
__host__ __device__ inline bool queryRayIsDegenerate(float ox, float oy, float oz, float maxDistance, float dx, float dy, float dz)
{
    const float lengthSq = (dx * dx + dy * dy) + (dz * dz + 0.0f);
    const bool originFinite = isfinite(ox) && isfinite(oy) && isfinite(oz);
    return !originFinite || !(lengthSq > 0.0f && lengthSq <= 3.402823466e+38f) || !(maxDistance > 0.0f);
}

// one list of the traversal kernels' instantiations: X(stack entries per lane, intersection counters) etc.
#define RT_TRACE_ATTR(kStack) __launch_bounds__(RT_BLOCK) __attribute__((amdgpu_waves_per_eu(kStack <= 24 ? 5 : 1)))
#define RT_K_TRACE_ARGS (const RtSceneDesc scene, const Paths paths, const uint32_t* __restrict__ queue, const uint32_t* __restrict__ queueCount, \
                         const uint32_t* __restrict__ shadowQueue, const uint32_t* __restrict__ shadowCount, uint32_t* __restrict__ cursor, unsigned long long* counters, const TravTuning tune)
#define RT_K_TRACE_WIDE_ARGS (const RtSceneDesc scene, const WideBvh bvh, const Paths paths, const uint32_t* __restrict__ queue, const uint32_t* __restrict__ queueCount, \
                              const uint32_t* __restrict__ shadowQueue, const uint32_t* __restrict__ shadowCount, uint32_t* __restrict__ cursor, unsigned long long* counters, const WideTuning tune)
#define RT_K_TRACE_WIDE2_ARGS (const RtSceneDesc scene, const WideScene wide, const Paths paths, const uint32_t* __restrict__ queue, const uint32_t* __restrict__ queueCount, \
                               const uint32_t* __restrict__ shadowQueue, const uint32_t* __restrict__ shadowCount, uint32_t* __restrict__ cursor, unsigned long long* counters, const WideTuning tune)
#define RT_K_TRACE_INSTANCES(X) X(24, false) X(24, true) X(32, false) X(32, true) X(64, false) X(64, true)
#define RT_K_TRACE_PER_RAY_INSTANCES(X) X(24) X(32) X(64)   // the counting walk that also stores every ray's own counts (TravTuning::rayCounts)
#define RT_K_TRACE_WIDE_INSTANCES(X) X(24, false, false) X(24, false, true) X(24, true, false)
#define RT_K_TRACE_WIDE2_INSTANCES(X) X(24)

// the a-trous filter (rt_denoise.inl): a block is RT_DENOISE_BLOCK_Y rows of 64 consecutive x, one wave per row; a level's constants
#define RT_DENOISE_BLOCK_X 64
#define RT_DENOISE_BLOCK_Y 4
struct AtrousLevel { int32_t step; float invN, invP, invC, varianceFloor; };   // (the variance-guided kernels: invC holds sigmaLum^2)
#define RT_ATROUS_ATTR __launch_bounds__(RT_DENOISE_BLOCK_X * RT_DENOISE_BLOCK_Y)
// the LDS-tiled variant for steps 1 and 2: a block is a tile of 8 rows x 32 columns (with its 2 * step halo: 30 KB of LDS at step 2)
#define RT_DENOISE_TILE_X 32
#define RT_DENOISE_TILE_Y 8
#define RT_ATROUS_TILED_ATTR __launch_bounds__(RT_DENOISE_TILE_X * RT_DENOISE_TILE_Y) __attribute__((amdgpu_waves_per_eu(1, 3)))   /* (at 4 waves per SIMD, 128 VGPRs, the compiler spills) */
#define RT_K_ATROUS_ARGS (const float4* __restrict__ recN, const float4* __restrict__ recP, const float4* __restrict__ src, float4* __restrict__ dst, \
                          const float* __restrict__ albedo, float* __restrict__ out, float* __restrict__ outVariance, uint32_t width, uint32_t height, const AtrousLevel level)

// temporal accumulation (rt_temporal.inl): k_atrous's block.  What k_temporal reads, what it writes (motion, image and the four records: where asked) and the
// call's constants (m: prevWorldToScreen)
struct TemporalIn { const float* color; const float* colorHalf; const float* depth; const float* normal; const float* position; const float* albedo; const uint32_t* objectId;
                    const float4* recA; const float4* recB; const float4* recN; const float4* recP; };   // (the records: the previous frame; NULL without history)
struct TemporalOut { float* a; float* b; float* length; float* motion; float* image; float4* recA; float4* recB; float4* recN; float4* recP; };
struct TemporalFrame { float colorScale, alphaMin, maxHistory, normalThreshold, planeTolerance, prevSampleOffset[2]; uint32_t useIds; float m[16]; };
// k_temporal<true>, moving objects: the frame's constants and the motion table -- five float4 per object, RtObjectMotion's 80 bytes: the rows of m, then
// {prevId, moved, 0, 0}.  The static instantiation takes TemporalFrame itself: its argument list is what it was before objects could move.
struct TemporalFrameMoving : TemporalFrame { const float4* objects; uint32_t numObjects; };
// k_temporal<., true>, history clipping: behind either frame the two planes of moment records k_temporal_moments wrote -- {mu.rgb, cnt} and {g.rgb, 0} --, the
// count a pixel needs to clip (RtTemporalClip::minCount, as a float: cnt is one) and the confidence plane (may be NULL).  The two instantiations without take the
// argument lists they took before there was a clip.
template <class Frame> struct TemporalFrameClip : Frame { const float4* momentMu; const float4* momentG; float* confidence; float minCount; };
// k_temporal<true, ., true>, deforming meshes (rtgpu_temporal_accumulate_deform): behind the moving frame this frame's triangle and barycentric planes and the
// triangle records the meshes had when the history was stored -- nine floats each, RtTriangle's 36 bytes.  A record of the motion table with moved ==
// RT_MOTION_DEFORMED names its mesh's range of them in its last two words.  The four instantiations without take the argument lists they took before.
struct TemporalFrameDeform : TemporalFrameMoving { const uint32_t* subObjectId; const float* barycentrics; const float* prevTriangles; uint32_t numPrevTriangles; };
template <bool kMoving, bool kClip = false, bool kDeform = false> struct TemporalFrameOf { typedef TemporalFrame type; };
template <> struct TemporalFrameOf<true, false, false> { typedef TemporalFrameMoving type; };
template <> struct TemporalFrameOf<true, false, true> { typedef TemporalFrameDeform type; };
template <bool kMoving, bool kDeform> struct TemporalFrameOf<kMoving, true, kDeform> { typedef TemporalFrameClip<typename TemporalFrameOf<kMoving, false, kDeform>::type> type; };
#define RT_K_TEMPORAL_ARGS (const TemporalIn in, const TemporalOut out, uint32_t width, uint32_t height, const typename TemporalFrameOf<kMoving, kClip, kDeform>::type frame)
// k_temporal_moments<kRadius> (history clipping): k_atrous_tiled's block of 8 rows x 32 columns with a halo of kRadius, three 16-byte records per staged pixel
// (at radius 3: 38 x 14 x 48 bytes = 25.5 KB of LDS); reads the current frame's planes of TemporalIn, writes the two moment records per pixel
struct TemporalMomentsFrame { float colorScale, normalThreshold, planeTolerance, gamma; };
#define RT_K_TEMPORAL_MOMENTS_ARGS (const TemporalIn in, uint32_t width, uint32_t height, const TemporalMomentsFrame frame, float4* __restrict__ outMu, float4* __restrict__ outG)
#define RT_TEMPORAL_MOMENTS_ATTR __launch_bounds__(RT_DENOISE_TILE_X * RT_DENOISE_TILE_Y)
// temporal accumulation over chain guides (rtgpu_temporal_accumulate_chain): k_temporal_chain and k_temporal_moments_chain are the second inclusions of
// rt_temporal_body.inl and rt_temporal_moments_body.inl, under RT_TEMPORAL_CHAIN 1, and take this frame's three chain planes behind the arguments of their
// siblings, which keep their own lists
struct TemporalChainPlanes { const float* virtualPosition; const uint32_t* chainLength; const float* chainDistance; };
#define RT_K_TEMPORAL_CHAIN_ARGS (const TemporalIn in, const TemporalOut out, uint32_t width, uint32_t height, const typename TemporalFrameOf<kMoving, kClip>::type frame, \
                                  const TemporalChainPlanes chain)
#define RT_K_TEMPORAL_MOMENTS_CHAIN_ARGS (const TemporalIn in, uint32_t width, uint32_t height, const TemporalMomentsFrame frame, float4* __restrict__ outMu, float4* __restrict__ outG, \
                                          const TemporalChainPlanes chain)

#ifndef RT_DEVICE_KERNELS
template <int kStack, bool kCount, bool kPerRay = false> __global__ void RT_TRACE_ATTR(kStack) k_trace RT_K_TRACE_ARGS;
template <int kStack, bool kDiag = false, bool kLocalExact = false> __global__ void RT_TRACE_ATTR(kStack) k_trace_wide RT_K_TRACE_WIDE_ARGS;
template <int kStack> __global__ void RT_TRACE_ATTR(kStack) k_trace_wide2 RT_K_TRACE_WIDE2_ARGS;
__global__ void __launch_bounds__(RT_BLOCK) k_trace_packet(const RtSceneDesc scene, const WideBvh bvh, const Paths paths, uint32_t* __restrict__ cursor, unsigned long long* counters, const WideTuning tune,
                                                           const BeamLists beam);
__global__ void __launch_bounds__(64) k_beam_lists_build(const WideBvh bvh, const uint32_t* __restrict__ slotPixel, uint32_t numSlots, const BeamCamera cam, uint32_t capacity,
                                                         BeamEntry* __restrict__ entries, uint32_t* __restrict__ counts);
__global__ void __launch_bounds__(RT_BLOCK) k_generate(const RtSceneDesc scene, const DevPass* __restrict__ passes, uint32_t slotsPerPass,
                                                       const Paths paths, const uint32_t* __restrict__ slotPixel, uint32_t numSlots,
                                                       uint32_t* __restrict__ queue, uint32_t* __restrict__ queueCount,
                                                       unsigned long long* counters);
__global__ void __launch_bounds__(RT_BLOCK) k_postprocess(const float* __restrict__ sum, uint32_t* __restrict__ front, uint32_t width, uint32_t height,
                                                          const RtPostprocessParams params, const PostScale colorScale);
__global__ void __launch_bounds__(64) k_kat_postprocess(const RtPostprocessParams* __restrict__ params, const PostScale* __restrict__ colorScales, const float* __restrict__ rgb,
                                                        uint32_t n, uint32_t* __restrict__ outBGR, float* __restrict__ outToneMapped);
__global__ void __launch_bounds__(RT_BLOCK) k_blur_lines(float* __restrict__ image, uint32_t width, uint32_t height, uint32_t vertical, const BlurPlan plan,
                                                         float* __restrict__ lineA, float* __restrict__ lineB);
__global__ void __launch_bounds__(RT_BLOCK) k_postprocess_bloom(const float* __restrict__ sum, const BloomLevels blurred, uint32_t* __restrict__ front, uint32_t width, uint32_t height,
                                                                const RtPostprocessParams params, const PostScale colorScale);
__global__ void __launch_bounds__(RT_BLOCK) k_block_error_rows(const float* __restrict__ sum, const float* __restrict__ secondary, uint32_t width,
                                                               const RtBlock* __restrict__ blocks, const ErrorRow* __restrict__ rows, uint32_t numRows,
                                                               float imageScalingFactor, float* __restrict__ rowErrors);
__global__ void __launch_bounds__(RT_BLOCK) k_block_error_total(const RtBlock* __restrict__ blocks, const uint32_t* __restrict__ firstRow, uint32_t numBlocks,
                                                                const float* __restrict__ rowErrors, uint32_t totalArea, float* __restrict__ outErrors);
__global__ void __launch_bounds__(RT_BLOCK) k_evaluate_textures(const RtSceneDesc scene, uint32_t count, const uint32_t* __restrict__ textureIndex,
                                                                const float* __restrict__ uv, float* __restrict__ out);
__global__ void __launch_bounds__(64) k_kat(const RtSceneDesc scene, uint32_t func, const float* __restrict__ in, uint32_t inStride, float* __restrict__ out,
                                            uint32_t outStride, uint32_t n);
__global__ void __launch_bounds__(64) k_kat_sampler(const uint16_t* __restrict__ blueNoise, const float* __restrict__ in, uint32_t inStride, float* __restrict__ out,
                                                    uint32_t count, uint32_t n);
__global__ void __launch_bounds__(64) k_kat_mesh(const RtSceneDesc scene, const float* __restrict__ rays, uint32_t n, uint32_t* __restrict__ out);
// ray queries (rt_query.inl)
__global__ void __launch_bounds__(RT_BLOCK) k_query_load(const float4* __restrict__ rays, uint32_t count, uint32_t mode, const Paths paths,
                                                         uint32_t* __restrict__ queue, uint32_t* __restrict__ queueCount, unsigned long long* counters);
__global__ void __launch_bounds__(RT_BLOCK) k_query_store(const RtSceneDesc scene, const float4* __restrict__ rays, uint32_t count, uint32_t mode, const Paths paths,
                                                          float4* __restrict__ hits, uint32_t* __restrict__ occluded);
__global__ void __launch_bounds__(RT_BLOCK) k_query_evaluate(const RtSceneDesc scene, const float4* __restrict__ rays, uint32_t count, const float4* __restrict__ hits,
                                                             float4* __restrict__ surfaces, unsigned long long* counters);
// a-trous filter (rt_denoise.inl)
__global__ void __launch_bounds__(RT_BLOCK) k_denoise_prepare(const float* __restrict__ color, const float* __restrict__ depth, const float* __restrict__ normal,
                                                              const float* __restrict__ position, const float* __restrict__ albedo, uint32_t pixels, float colorScale,
                                                              float4* __restrict__ recN, float4* __restrict__ recP, float4* __restrict__ recC);
__global__ void __launch_bounds__(RT_BLOCK) k_denoise_prepare_var(const float* __restrict__ color, const float* __restrict__ colorHalf, const float* __restrict__ depth,
                                                                  const float* __restrict__ normal, const float* __restrict__ position, const float* __restrict__ albedo,
                                                                  uint32_t pixels, float colorScale, float4* __restrict__ recN, float4* __restrict__ recP, float4* __restrict__ recC);
__global__ void __launch_bounds__(RT_BLOCK) k_denoise_prepare_accumulated(const float* __restrict__ color, const float* __restrict__ colorHalf, const float* __restrict__ depth,
                                                                          const float* __restrict__ normal, const float* __restrict__ position, uint32_t pixels,
                                                                          float4* __restrict__ recN, float4* __restrict__ recP, float4* __restrict__ recC);
template <bool kLast, bool kVar = false> __global__ void RT_ATROUS_ATTR k_atrous RT_K_ATROUS_ARGS;
template <bool kLast, int kStep, bool kVar = false> __global__ void RT_ATROUS_TILED_ATTR k_atrous_tiled RT_K_ATROUS_ARGS;
// temporal accumulation (rt_temporal.inl)
__global__ void __launch_bounds__(RT_BLOCK) k_temporal_pack(const float* __restrict__ prevA, const float* __restrict__ prevB, const float* __restrict__ prevLength,
                                                            const float* __restrict__ prevDepth, const float* __restrict__ prevNormal, const float* __restrict__ prevPosition,
                                                            const uint32_t* __restrict__ prevObjectId, const uint32_t* __restrict__ prevChainLength, uint32_t pixels,
                                                            float4* __restrict__ recA, float4* __restrict__ recB, float4* __restrict__ recN, float4* __restrict__ recP);
template <bool kMoving = false, bool kClip = false, bool kDeform = false> __global__ void RT_ATROUS_ATTR k_temporal RT_K_TEMPORAL_ARGS;
template <int kRadius> __global__ void RT_TEMPORAL_MOMENTS_ATTR k_temporal_moments RT_K_TEMPORAL_MOMENTS_ARGS;
template <bool kMoving = false, bool kClip = false> __global__ void RT_ATROUS_ATTR k_temporal_chain RT_K_TEMPORAL_CHAIN_ARGS;
template <int kRadius> __global__ void RT_TEMPORAL_MOMENTS_ATTR k_temporal_moments_chain RT_K_TEMPORAL_MOMENTS_CHAIN_ARGS;
// the ray source (rt_raysource.inl): k_generate's arguments and the table behind them; the table's check; the camera's rays in the table's layout
__global__ void __launch_bounds__(RT_BLOCK) k_generate_rays(const RtSceneDesc scene, const DevPass* __restrict__ passes, uint32_t slotsPerPass,
                                                            const Paths paths, const uint32_t* __restrict__ slotPixel, uint32_t numSlots,
                                                            uint32_t* __restrict__ queue, uint32_t* __restrict__ queueCount,
                                                            unsigned long long* counters, const float4* __restrict__ rays);
__global__ void __launch_bounds__(RT_BLOCK) k_ray_source_check(const float4* __restrict__ rays, uint32_t count, uint32_t* __restrict__ outDegenerate);
__global__ void __launch_bounds__(RT_BLOCK) k_camera_rays(const RtCamera camera, float sampleOffsetX, float sampleOffsetY, uint32_t width, uint32_t height, float4* __restrict__ out);
// the lens source (rt_raysource.inl): k_generate behind a table of lens rays; the table's check; the rays of a pass and the camera's footprints written out
__global__ void __launch_bounds__(RT_BLOCK) k_generate_lens(const RtSceneDesc scene, const DevPass* __restrict__ passes, uint32_t slotsPerPass,
                                                            const Paths paths, const uint32_t* __restrict__ slotPixel, uint32_t numSlots,
                                                            uint32_t* __restrict__ queue, uint32_t* __restrict__ queueCount,
                                                            unsigned long long* counters, const float4* __restrict__ table, uint32_t lens, uint32_t bokehShape);
__global__ void __launch_bounds__(RT_BLOCK) k_lens_source_check(const float4* __restrict__ table, uint32_t count, uint32_t lens, uint32_t* __restrict__ outRefused);
__global__ void __launch_bounds__(RT_BLOCK) k_lens_source_rays(const float4* __restrict__ table, uint32_t width, uint32_t height, float sx, float sy, uint32_t lens,
                                                               uint32_t bokehShape, uint32_t seed0, uint32_t seed1, uint32_t numDims, uint32_t blueNoiseLayers,
                                                               const uint16_t* __restrict__ blueNoise, unsigned long long rngKey0, unsigned long long rngKey1,
                                                               float4* __restrict__ out);
__global__ void __launch_bounds__(RT_BLOCK) k_camera_footprints(const RtCamera camera, float sampleOffsetX, float sampleOffsetY, uint32_t width, uint32_t height, float4* __restrict__ out);
__global__ void __launch_bounds__(RT_MONSTER_BLOCK) k_trace_monster(const RtSceneDesc scene, const Paths paths, const uint32_t* __restrict__ queue, const uint32_t* __restrict__ queueCount);
#endif
