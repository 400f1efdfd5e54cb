// rt_device_state.h -- device-side path state shared by the translation units of the library (rt_runtime.hip: host side; rt_trace.hip: traversal;
// rt_shade.hip: the shading kernels): the record arenas, per-pass constants, counter / sampler plumbing and the dense-arena helpers.
#pragma once
#include "rt_device_core.h"
#include <hip/hip_runtime.h>
#include <stdint.h>
using namespace rtd;

// =====================================================================================================
// Device-side data
// =====================================================================================================
// Path state lives in HBM as 16-byte RECORDS, one array per record kind (record-major, slot-minor): a lane moves a
// whole record with one dwordx4 access, a wave's accesses to consecutive slots coalesce into 1 KB, and a path
// vertex touches 7-9 arrays (and as many DRAM pages / TLB entries) instead of 34 scalar planes.
enum PathRecord : uint32_t
{
    R_ORIGIN,    // ray origin xyz BEFORE the 1e-3 offset | flags: depth (bits 0-7), lastSpecular << 8, (previous vertex's material + 1) << 9
                 // (dense arenas: also the origin of the vertex's any-hit rays -- the same point -- and, for a zombie, nothing else; shadowOriginRecord)
    R_DIR,       // ray direction xyz as passed to Ray()   | lastPdfW
    R_TP,        // throughput (4 lanes: RayColor::AlmostZero tests all four)
    R_RESULT,    // accumulated radiance rgb of this path  | pixel: x | y << 16
    R_HIT,       // objectId, subObjectId, distance, u
    R_SAMPLER,   // hit v | GenericSampler salt, generated | number of NEE requests pending for this vertex (dense arenas: | home index << 3, densePending)
    R_RNG,       // per-pixel xoroshiro128+ state (2 x 64 bit)
    R_SH_P,      // shading point xyz (shadow ray origin before the 1e-4 offset); the dense arenas do not use it (R_ORIGIN holds the same point)
    R_SH_TP,     // throughput at the vertex (the NEE fma uses it); dense arenas: written and read only while a request is pending
    R_NUM_BASE
};
// per NEE request two records, light-major: {direction xyz, tmax (< 0: no ray / occluded)}, {contribution rgb, -}.  Dense arenas (verdictRecord = 1):
// {direction xyz, tmax (< 0: no ray)}, {contribution rgb, < 0: no ray / occluded} -- the resolving vertex reads one record per request, not two
#define RT_SHADOW_RECORDS 2

struct Paths
{
    float4* base;       // (R_NUM_BASE + maxLights * RT_SHADOW_RECORDS) * capacity records
    uint32_t capacity;
    uint32_t maxLights; // NEE requests per vertex (1 for LightSamplingStrategy::Single)
    // Launch-uniform layout choices the shared any-hit walks follow.  The defaults are the first layout's (slot-per-pixel k_shade, the ray queries, VCM, the
    // recorder); the two dense arenas and k_tail's in-place arena use denseLayout().
    // ONE word for both (0: first layout, 1: dense): the walks have no scalar register to spare for a second one.
    uint32_t dense = 0u;
};
__host__ __device__ inline static Paths denseLayout(Paths p) { p.dense = 1u; return p; }
// the record whose xyz is the origin of the slot's any-hit rays: R_SH_P, or -- dense -- R_ORIGIN, which holds the same point
RT_DEV uint32_t shadowOriginRecord(const Paths& p) { return p.dense != 0u ? (uint32_t)R_ORIGIN : (uint32_t)R_SH_P; }
// which record of a request (pshadow's k) gets .w = -1 when its ray is occluded: the direction record, or -- dense -- the contribution record
RT_DEV uint32_t verdictRecord(const Paths& p) { return p.dense; }

RT_DEV float4& prec(const Paths& p, uint32_t record, uint32_t slot) { return p.base[(size_t)record * p.capacity + slot]; }
RT_DEV float4& pshadow(const Paths& p, uint32_t light, uint32_t k, uint32_t slot)
{
    return p.base[((size_t)R_NUM_BASE + (size_t)light * RT_SHADOW_RECORDS + k) * p.capacity + slot];
}
RT_DEV float4 f4(float x, float y, float z, float w) { float4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
// Path records are STREAMED: a bounce reads a record once and writes its successor once, gigabytes per launch, through the same 4 MB-per-XCD
// L2 that holds the scene's nodes, triangles and shading records.  Non-temporal accesses keep the stream from evicting the geometry.
#ifndef RT_STREAMING_HINTS
#define RT_STREAMING_HINTS 1
#endif
typedef float rt_float4v __attribute__((ext_vector_type(4)));
RT_DEV float4 ldStream(const float4& r)
{
#if RT_STREAMING_HINTS
    const rt_float4v v = __builtin_nontemporal_load(reinterpret_cast<const rt_float4v*>(&r));
    return f4(v.x, v.y, v.z, v.w);
#else
    return r;
#endif
}
RT_DEV void stStream(float4& r, const float4& v)
{
#if RT_STREAMING_HINTS
    const rt_float4v t = { v.x, v.y, v.z, v.w };
    __builtin_nontemporal_store(t, reinterpret_cast<rt_float4v*>(&r));
#else
    r = v;
#endif
}
RT_DEV float fbits(uint32_t u) { return __uint_as_float(u); }
RT_DEV uint32_t ubits(float f) { return __float_as_uint(f); }

struct DevPass
{
    RtCamera camera;
    const uint32_t* seed;
    uint32_t numDimensions;
    uint32_t blueNoiseLayers;
    float sampleOffset[2];
    uint32_t passIndex;
    uint32_t maxRayDepth;
    uint32_t minRussianRouletteDepth;
    uint32_t lightSamplingStrategy;
    float lightSamplingWeight[4];
    float bsdfSamplingWeight[4];
    uint64_t rngKey[2];
    uint32_t width, height;
};

#define RT_BLOCK 256

// per-block counter flush: LDS tally, then one 64-bit atomic per counter per block
RT_DEV void flushCounters(const Counters& c, unsigned long long* global)
{
    __shared__ uint32_t sC[RT_NUM_COUNTERS];
    if (threadIdx.x < RT_NUM_COUNTERS) sC[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RT_NUM_COUNTERS; ++k) if (c.c[k]) atomicAdd(&sC[k], c.c[k]);
    __syncthreads();
    if (threadIdx.x < RT_NUM_COUNTERS && sC[threadIdx.x]) atomicAdd(&global[threadIdx.x], (unsigned long long)sC[threadIdx.x]);
}
RT_DEV void zeroCounters(Counters& c) {
#pragma unroll
    for (int k = 0; k < RT_NUM_COUNTERS; ++k) c.c[k] = 0;
}

// a generator's pair of 64-bit words as the four lanes of a record (low word first), and back
RT_DEV float4 packPair(const uint64_t s[2])
{
    return f4(fbits((uint32_t)s[0]), fbits((uint32_t)(s[0] >> 32)), fbits((uint32_t)s[1]), fbits((uint32_t)(s[1] >> 32)));
}
RT_DEV void unpackPair(const float4& r, uint64_t s[2])
{
    s[0] = (uint64_t)ubits(r.x) | ((uint64_t)ubits(r.y) << 32);
    s[1] = (uint64_t)ubits(r.z) | ((uint64_t)ubits(r.w) << 32);
}

// GenericSampler + per-pixel RNG state of a path (R_SAMPLER.yz, R_RNG); `sampler` and `rng` are the records already loaded
RT_DEV void loadSampler(Sampler& s, uint32_t pix, const float4& sampler, const float4& rng, const DevPass& pass, const uint16_t* blueNoise)
{
    s.seed = pass.seed; s.numDims = pass.numDimensions; s.blueNoiseLayers = pass.blueNoiseLayers; s.blueNoise = blueNoise;
    s.bx = (pix & 0xFFFFu) & 127u; s.by = (pix >> 16) & 127u;
    s.salt = ubits(sampler.y); s.generated = ubits(sampler.z);
    unpackPair(rng, s.fallback.s);
}
RT_DEV void loadSampler(Sampler& s, const Paths& p, uint32_t slot, uint32_t pix, const float4& sampler, const DevPass& pass, const uint16_t* blueNoise)
{
    loadSampler(s, pix, sampler, prec(p, R_RNG, slot), pass, blueNoise);
}
// R_RNG: the four words of the per-pixel generator, as loadSampler reads them back
RT_DEV float4 packRng(const Sampler& s) { return packPair(s.fallback.s); }
RT_DEV void storeSampler(const Sampler& s, const Paths& p, uint32_t slot, float hitV, uint32_t pendingRequests)
{
    prec(p, R_SAMPLER, slot) = f4(hitV, fbits(s.salt), fbits(s.generated), fbits(pendingRequests));
    prec(p, R_RNG, slot) = packRng(s);
}
// the Hit a closest-hit walk left in R_HIT; its v rides in R_SAMPLER.x
RT_DEV Hit unpackHit(const float4& rHit, float v)
{
    Hit hit;
    hit.objectId = ubits(rHit.x); hit.subObjectId = ubits(rHit.y); hit.distance = rHit.z; hit.u = rHit.w; hit.v = v;
    return hit;
}

// ---- the generate kernels (k_generate*: rt_generate.inl, rt_dense.inl, rt_raysource.inl): one body around "the ray of this pixel" ----
// film coordinates of pixel (x, y) at a sample offset: invSize = VECTOR_ONE2 / FromIntegers(w, h, 1, 1); coords = (FromIntegers(x, realY) + sampleOffset) * invSize
// (the export kernels' -- k_camera_rays, k_camera_footprints; generatePaths writes the same three lines out: through this function one packed multiply of
// k_generate and of k_generate_dense comes out with its operands exchanged, and the two are held to the bytes they had)
RT_DEV V4 filmCoords(uint32_t x, uint32_t y, uint32_t width, uint32_t height, float sampleOffsetX, float sampleOffsetY)
{
    const uint32_t realY = height - 1u - y;
    const float invW = 1.0f / (float)(int32_t)width, invH = 1.0f / (float)(int32_t)height;
    return V4(((float)(int32_t)x + sampleOffsetX) * invW, ((float)(int32_t)realY + sampleOffsetY) * invH, 0.0f, 0.0f);
}
// Viewport::RenderTile's per-pixel prologue for every slot of a batch, the ray `rayOf(pass, pix, coords, sampler, origin, direction)` gives pixel pix
// (x | y << 16) -- it draws from the sampler, reset for the pixel, what the ray takes; `coords` are the pixel's film coordinates where RayOf::kFromFilm says
// the ray starts from the film, else zero -- and the records of a fresh path in the arena's layout:
//   slot per pixel (kDense false)   all of them, and the slot in `queue`
//   dense (kDense true)             origin and direction only, streamed: the five other records of a fresh path are functions of its slot, which bounce 0's
//                                   shade rebuilds (denseShadeVertex)
// (the grid-stride loop's ends are the kernel's to compute, RT_GRID_STRIDE: blockDim.x read in a device function compiles to another load, and k_generate and
// k_generate_dense are held to the code they had)
#define RT_GRID_STRIDE blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x
template <bool kDense, class RayOf>
RT_DEV void generatePaths(uint32_t firstSlot, uint32_t stride, const uint16_t* blueNoise, const DevPass* __restrict__ passes, uint32_t slotsPerPass, const Paths& paths, const uint32_t* __restrict__ slotPixel,
                          uint32_t numSlots, uint32_t* __restrict__ queue, RayOf rayOf)
{
    for (uint32_t slot = firstSlot; slot < numSlots; slot += stride)
    {
        // several passes ride in one batch: slot = passInBatch * slotsPerPass + pixelSlot
        const uint32_t passInBatch = slot / slotsPerPass;
        const DevPass& pass = passes[passInBatch];
        const uint32_t pix = slotPixel[slot - passInBatch * slotsPerPass];
        const uint32_t x = pix & 0xFFFFu, y = pix >> 16;
        V4 coords = zero4();
        if (RayOf::kFromFilm)   // (ahead of the sampler, where the camera kernels had it; a table's kernels keep their loads where they were)
        {
            const uint32_t realY = pass.height - 1u - y;
            const float invW = 1.0f / (float)(int32_t)pass.width, invH = 1.0f / (float)(int32_t)pass.height;
            coords = V4(((float)(int32_t)x + pass.sampleOffset[0]) * invW, ((float)(int32_t)realY + pass.sampleOffset[1]) * invH, 0.0f, 0.0f);
        }
        Sampler sampler;
        sampler.seed = pass.seed; sampler.numDims = pass.numDimensions; sampler.blueNoiseLayers = pass.blueNoiseLayers; sampler.blueNoise = blueNoise;
        sampler.resetPixel(x, y, pass.rngKey[0], pass.rngKey[1]);
        // Camera::GenerateRay up to (not including) the Ray constructor, which trace/shade re-run from origin+direction
        V4 origin, direction;
        rayOf(pass, pix, coords, sampler, origin, direction);
        if (kDense)
        {
            stStream(prec(paths, R_ORIGIN, slot), f4(origin.x, origin.y, origin.z, fbits(0x100u)));   // depth 0, lastSpecular = true (PathTracerMIS.h:29-34)
            stStream(prec(paths, R_DIR, slot), f4(direction.x, direction.y, direction.z, 1.0f));        // lastPdfW = 1
        }
        else
        {
            prec(paths, R_ORIGIN, slot) = f4(origin.x, origin.y, origin.z, fbits(0x100u));
            prec(paths, R_DIR, slot) = f4(direction.x, direction.y, direction.z, 1.0f);
            prec(paths, R_TP, slot) = f4(1.0f, 1.0f, 1.0f, 1.0f);
            prec(paths, R_RESULT, slot) = f4(0.0f, 0.0f, 0.0f, fbits(pix));
            storeSampler(sampler, paths, slot, 0.0f, 0u);
            queue[slot] = slot;
        }
    }
}
// the camera as `rayOf` (k_generate, k_generate_dense)
struct CameraRayOf
{
    static constexpr bool kFromFilm = true;
    __device__ __forceinline__ void operator()(const DevPass& pass, uint32_t, V4 coords, Sampler& sampler, V4& origin, V4& direction) const
    {
        cameraGenerateRayParts(pass.camera, coords, sampler, origin, direction);
    }
};
// block 0's epilogue, slot per pixel: every slot is queued
RT_DEV void generateQueueCount(uint32_t* __restrict__ queueCount, unsigned long long* counters, uint32_t numSlots)
{
    if (blockIdx.x == 0 && threadIdx.x == 0)
    {
        *queueCount = numSlots;
        atomicAdd(&counters[C_PRIMARY], (unsigned long long)numSlots);
    }
}

// The path's current ray exactly as the reference holds it: Ray(origin, direction) -- which normalises and
// computes invDir / originDivDir from the UN-offset origin -- and then origin += dir * 0.001f for
// secondary rays, leaving originDivDir stale (PathTracerMIS.cpp:392-393).
RT_DEV Ray makePathRay(const float4& origin, const float4& dir, uint32_t depth)
{
    Ray ray = makeRay(V4(origin.x, origin.y, origin.z, 0.0f), V4(dir.x, dir.y, dir.z, 0.0f));
    if (depth > 0) ray.origin = ray.origin + ray.dir * 0.001f;
    return ray;
}

// ---- dense path state (rt_dense.inl): an arena is RT_DENSE_SHARDS regions, region s holds its live paths upwards from s * shardCapacity ----
#define RT_DENSE_SHARDS 16u

struct DenseCounts
{
    const uint32_t* in;     // [0, 16): live paths per region of the arena being read; [16, 32): zombies per region
    uint32_t* out;          // the same for the arena being written (zeroed by the host)
    uint32_t shardCapacity;
    uint32_t* errorFlags;   // host-visible words of the context (RtgpuContext::deviceFlags): [0] != 0 = a region of the arena overflowed
    const uint32_t* primarySlotPixel;   // bounce 0 of a batch whose k_generate_dense stored origin and direction only: the slot -> pixel table; else null
    uint32_t stage;         // RT_STAGE_* bits: what this launch copies to LDS (the host decides: denseStageMask); 0: everything from memory
    uint32_t numPasses;     // passes of the batch (the seed rows a block stages)
};

// ---- launch-uniform tables of k_shade_dense in LDS (rt_dense.inl) ----
// A vertex reads its object, mesh, material and light records and the seed row of its pass from tables of a few hundred bytes that are the same for every lane
// of the launch; each such read was a trip to L2 of its own in the vertex's dependent chain.  A block copies them in front of its first vertex where they fit
// these capacities: the scene's tables as a group, and with them the seed rows where those fit too.
#define RT_STAGE_TABLES 1u    // scene.objects, meshes, materials, lights and globalLights
#define RT_STAGE_SEEDS  2u    // the seed rows of the batch's passes, numDimensions words each (rounded up to four); only together with RT_STAGE_TABLES
#define RT_STAGE_MAX_OBJECTS   8u
#define RT_STAGE_MAX_MESHES    8u
#define RT_STAGE_MAX_MATERIALS 32u
#define RT_STAGE_MAX_LIGHTS    8u
#define RT_STAGE_SEED_WORDS    2048u   // 8 KB: 24 passes of 64 dimensions take 6 KB
static_assert(sizeof(RtObject) % 16 == 0 && sizeof(RtMesh) % 16 == 0 && sizeof(RtMaterial) % 16 == 0 && sizeof(RtLight) % 16 == 0, "the staged tables are copied in 16-byte words");
__host__ __device__ __forceinline__ static uint32_t stageSeedRow(uint32_t numDims) { return (numDims + 3u) & ~3u; }   // words between two staged seed rows

// block 0's epilogue of the dense generate kernels: slot i = home i, so the regions of the first arena are simply filled one after the other
RT_DEV void generateShardCounts(uint32_t* __restrict__ counts, uint32_t shardCapacity, unsigned long long* counters, uint32_t numSlots)
{
    if (blockIdx.x == 0 && threadIdx.x < RT_DENSE_SHARDS)
    {
        const uint32_t first = threadIdx.x * shardCapacity;
        counts[threadIdx.x] = first >= numSlots ? 0u : (numSlots - first < shardCapacity ? numSlots - first : shardCapacity);
        if (threadIdx.x == 0) atomicAdd(&counters[C_PRIMARY], (unsigned long long)numSlots);
    }
}

// prefix sums of the 16 region counts into LDS (prefix[16] = total); all threads of the block call it
RT_DEV void denseLoadPrefix(const uint32_t* __restrict__ counts, uint32_t* sPrefix)
{
    if (threadIdx.x == 0)
    {
        uint32_t sum = 0;
        for (uint32_t s = 0; s < RT_DENSE_SHARDS; ++s) { sPrefix[s] = sum; sum += counts[s]; }
        sPrefix[RT_DENSE_SHARDS] = sum;
    }
}
RT_DEV uint32_t denseRegionOf(const uint32_t* sPrefix, uint32_t idx)
{
    uint32_t s = idx >= sPrefix[8] ? 8u : 0u;
    s += idx >= sPrefix[s + 4u] ? 4u : 0u;
    s += idx >= sPrefix[s + 2u] ? 2u : 0u;
    s += idx >= sPrefix[s + 1u] ? 1u : 0u;
    return s;
}
// slot of the idx-th live path
RT_DEV uint32_t denseLiveSlot(const uint32_t* sPrefix, uint32_t shardCapacity, uint32_t idx)
{
    const uint32_t s = denseRegionOf(sPrefix, idx);
    return s * shardCapacity + (idx - sPrefix[s]);
}
// The same prefix sums for the zombie counts (counts[16, 32)), by thread 64 while thread 0 sums the live ones; all threads of the block call it and
// synchronise afterwards.  Block 0 also checks the final counts of the launch before: it overfilled region s if the live paths growing up met the
// zombies growing down.
RT_DEV void denseLoadZombiePrefix(const uint32_t* counts, uint32_t shardCapacity, uint32_t* errorFlags, uint32_t* sZombiePrefix)
{
    if (threadIdx.x == 64)
    {
        uint32_t sum = 0;
        for (uint32_t s = 0; s < RT_DENSE_SHARDS; ++s)
        {
            sZombiePrefix[s] = sum; sum += counts[RT_DENSE_SHARDS + s];
            if (blockIdx.x == 0 && counts[s] + counts[RT_DENSE_SHARDS + s] > shardCapacity) errorFlags[0] = 1u;
        }
        sZombiePrefix[RT_DENSE_SHARDS] = sum;
    }
}
// slot of the idx-th vertex of a launch: the live paths first (region by region), then the zombies (from the top of their regions).  numLive is
// sLivePrefix[RT_DENSE_SHARDS], which both callers hold in a register: read from LDS again here, it moves the register allocation of the kernels
// the benchmark runs (k_shade_dense<1, false, false> 116 -> 115 VGPRs, k_tail<1, false> 84 -> 76 bytes of scratch).
RT_DEV uint32_t denseVertexSlot(const uint32_t* sLivePrefix, const uint32_t* sZombiePrefix, uint32_t numLive, uint32_t shardCapacity, uint32_t idx, bool& zombie)
{
    zombie = idx >= numLive;
    if (!zombie) return denseLiveSlot(sLivePrefix, shardCapacity, idx);
    const uint32_t z = idx - numLive, s = denseRegionOf(sZombiePrefix, z);
    return (s + 1u) * shardCapacity - 1u - (z - sZombiePrefix[s]);
}

#define RT_DENSE_MAX_LIGHTS 7u   // 256 vertices x 7 requests fit the block's append buffer between two flushes (k_shade_dense)
// R_SAMPLER.w of a dense arena: the pending-request count in the low bits, the path's home index (pass in batch * slotsPerPass + pixel slot) above
#define RT_DENSE_PENDING_BITS 3u
#define RT_DENSE_MAX_HOME (1u << (32u - RT_DENSE_PENDING_BITS))   // home indices of a batch stay below this (flushBatch bounds the batch)
static_assert(RT_DENSE_MAX_LIGHTS < (1u << RT_DENSE_PENDING_BITS), "the pending-request count of a dense vertex has RT_DENSE_PENDING_BITS bits");
RT_DEV uint32_t densePack(uint32_t home, uint32_t pending) { return (home << RT_DENSE_PENDING_BITS) | pending; }
RT_DEV uint32_t densePending(uint32_t packed) { return packed & ((1u << RT_DENSE_PENDING_BITS) - 1u); }
RT_DEV uint32_t denseHome(uint32_t packed) { return packed >> RT_DENSE_PENDING_BITS; }

// Occupancy the register allocator is held to per scene class: "lean + simple bitmaps" needs 135 VGPRs on its own and fits four waves per SIMD with
// 8-16 bytes of scratch (measured +4 % end to end on the textured Sponza-class scene); "lean + textures" 173 -> 168 = three waves (+8 %), "anything"
// 192 -> 168 = three waves (+1.5 %); the lean and the untextured classes keep what they get (forcing THEM further was slower,
// profiles/r03_shade_variants.txt).
#define RT_SHADE_MIN_WAVES(k, all) ((k) == 4 ? 4 : (((k) == 2 || ((k) == 0 && !(all))) ? 3 : 1))   // ("anything" under `All`: 216 VGPRs, left alone)

// ---- DebugRenderer (renderer name "Debug"): modes and the TriangleID colour (also a known-answer function of rt_kat.inl) ----
// DebugRenderer::RenderPixel after the primary ray's traversal (Core/Rendering/DebugRenderer.cpp:26-195, renderer "Debug"): one colour
// per pixel from the first hit.  mode = DebugRenderingMode (DebugRenderer.h:7-33; the four counter modes exist only under
// RT_ENABLE_INTERSECTION_COUNTERS, off in the reference).
enum { DBG_CAMERA_LIGHT = 0, DBG_TRIANGLE_ID, DBG_DEPTH, DBG_POSITION, DBG_NORMALS, DBG_TANGENTS, DBG_BITANGENTS, DBG_TEXCOORDS,
       DBG_BASE_COLOR, DBG_EMISSION, DBG_ROUGHNESS, DBG_METALNESS, DBG_IOR, DBG_NUM_MODES };
RT_DEV V4 hsvToRgb(float hue, float saturation, float value)   // Core/Color/ColorHelpers.h:133-156
{
    const int h_i = (int)(hue * 6.0f);
    const float f = hue * 6 - h_i;
    const float p = value * (1 - saturation);
    const float q = value * (1 - f * saturation);
    const float t = value * (1 - (1 - f) * saturation);
    if (h_i == 0) return V4(value, t, p, 0.0f);
    else if (h_i == 1) return V4(q, value, p, 0.0f);
    else if (h_i == 2) return V4(p, value, t, 0.0f);
    else if (h_i == 3) return V4(p, q, value, 0.0f);
    else if (h_i == 4) return V4(t, p, value, 0.0f);
    else if (h_i == 5) return V4(value, p, q, 0.0f);
    return zero4();
}
RT_DEV V4 debugTriangleIdColor(uint32_t objectId, uint32_t subObjectId)   // DebugRenderer.cpp:98-106
{
    const uint64_t hash = murmurFmix64((uint64_t)objectId | ((uint64_t)subObjectId << 32));
    const float hue = (float)(uint32_t)hash / (float)UINT32_MAX;
    const float saturation = 0.5f + 0.5f * (float)(uint32_t)(hash >> 32) / (float)UINT32_MAX;
    return hsvToRgb(hue, saturation, 1.0f);
}
