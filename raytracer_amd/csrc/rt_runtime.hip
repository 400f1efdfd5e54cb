// rt_runtime.hip -- the host side of the C-ABI of include/rtgpu.h: contexts, batch lanes, path-state arenas, scene upload, the launch
// sequences of the integrators.  The kernels live in rt_trace.hip (traversal, camera rays, post-process, known-answer hooks), rt_shade.hip
// (shading) and rt_tail.hip (the fused tail of a batch); this unit launches them through rt_trace_kernels.h / rt_shade_kernels.h.
//
// One pass (= one sample per owned pixel) is a fixed sequence of launches on the context's stream:
//
//   generate                               camera ray + sampler reset per path            (Viewport.cpp:305-331)
//   for depth = 0 .. maxRayDepth:
//       trace_closest                      two-level BVH closest hit                      (Scene.cpp:219)
//       shade                              miss / light hit / emission / NEE set-up / Russian roulette /
//                                          BSDF sample; compacts survivors into the next queue
//                                                                                         (PathTracerMIS.cpp:270-396)
//       trace_shadow                       any-hit occlusion of the NEE rays + accumulate (PathTracerMIS.cpp:81-119)
//   accumulate                             film sum (+ secondary sum on even passes)      (Film.cpp:25-39)
//
// Path state lives in HBM as structure-of-arrays indexed by path slot, so a wave reads 64 consecutive
// dwords per field; queues hold slot indices and are compacted with wave ballots (one atomic per wave).
// The two traversal kernels are PERSISTENT: a fixed grid of waves pulls rays from the queue through an atomic
// cursor and refills lanes whose ray has finished (rays of one wave take very different numbers of node
// steps), with the per-lane node stack in LDS.  NEE rays go through their own dense queue; their results are
// folded into the path radiance by the next kernel that touches the path (shade of the next bounce, or
// accumulate), which preserves the reference's accumulation order.
// Per-path arithmetic is kept in the reference's operation order (see rt_device_math.h), which makes the
// result independent of the wavefront schedule and reproducible against the CPU oracle.
//
//
// This file is the translation unit and keeps the contexts, the film and the small entry points; its parts: rt_runtime_context.h (RtgpuContext, BatchLane,
// staging copies, stream pool, HIP_TRY, LaunchTimer, free helpers), rt_knobs.h (every RTGPU_* environment variable), rt_multi.inl (multi-device contexts),
// rt_runtime_scene.inl (rtgpu_upload_scene, rtgpu_update_objects: the copies of what rt_scene_prepare.h checks and builds on the host), rt_runtime_render.inl (arena sizing, traversal launchers, batch submission), rt_runtime_vcm.inl (bidirectional
// integrator, Light Tracer), rt_runtime_kat.inl (known-answer hooks, rtgpu_evaluate_textures), rt_runtime_query.inl (batched ray queries), rt_runtime_paths.inl (path records),
// rt_runtime_aov.inl (AOVs), rt_runtime_denoise.inl (the a-trous filter, rtgpu_denoise, rtgpu_postprocess_from),
// rt_runtime_temporal.inl (temporal accumulation), rt_runtime_raysource.inl (the primary-ray sources: passes along a caller's table of rays, or of rays
// with footprints and a thin lens).
//
// Compile: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off
#include "rt_trace_common.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <string>
#include <unordered_map>
#include <vector>

using namespace rtd;

#include "rt_scene_prepare.h"
#include "rt_refit_keys.h"
#include "rt_trace_kernels.h"
#include "rt_shade_kernels.h"
#include "rt_tail_kernels.h"

#include "rt_runtime_context.h"
#include "rt_knobs.h"

static int flushPending(RtgpuContext* c);
static int vcmFlush(RtgpuContext* c);
static void freeVcm(RtgpuContext* c);
// Everything rtgpu_render_pass queued goes out: the bidirectional integrator's batch (rt_runtime_vcm.inl) and the PathTracerMIS batch.  Whatever replaces the film,
// the slot table or the scene calls this first, so that a queued pass renders the state it was queued in.
static int flushQueued(RtgpuContext* c)
{
    { const int r = vcmFlush(c); if (r) return r; }
    return flushPending(c);
}

#include "rt_multi.inl"

#define RTGPU_API extern "C" __attribute__((visibility("default")))

RTGPU_API const char* rtgpu_last_error(void) { return gLastError.c_str(); }
RTGPU_API uint32_t rtgpu_abi_version(void) { return RTGPU_ABI_VERSION; }

RTGPU_API int rtgpu_create(int deviceIndex, RtgpuContext** outCtx)
{
    if (!outCtx) return fail(RTGPU_ERR_INVALID_ARGUMENT, "outCtx is NULL");
    *outCtx = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(RTGPU_ERR_NO_DEVICE, "no HIP device available");
    if (deviceIndex < 0 || deviceIndex >= n) return fail(RTGPU_ERR_INVALID_ARGUMENT, "device index out of range");
    HIP_TRY(hipSetDevice(deviceIndex));
    RtgpuContext* c = new RtgpuContext();
    c->device = deviceIndex;
    memset(&c->sceneDev, 0, sizeof(c->sceneDev));
    memset(c->kernelMs, 0, sizeof(c->kernelMs)); memset(c->kernelLaunches, 0, sizeof(c->kernelLaunches));
    for (int i = 0; i < RT_SEED_RING; ++i) { c->seedEvents[i] = nullptr; c->seedEventUsed[i] = false; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, deviceIndex) == hipSuccess) c->numCUs = (uint32_t)prop.multiProcessorCount;
    {
        // six lanes (the most rtgpu_set_concurrency allows) plus scene, film and the bidirectional integrator's arenas must fit what is free now
        size_t freeBytes = 0, totalBytes = 0;
        if (hipMemGetInfo(&freeBytes, &totalBytes) == hipSuccess && freeBytes / 8u < c->laneBudgetBytes) c->laneBudgetBytes = freeBytes / 8u > ((size_t)64 << 20) ? freeBytes / 8u : ((size_t)64 << 20);
        // RTGPU_LANE_BUDGET_MB: the device memory ONE batch lane may take for its path-state arenas (a co-tenant's knob: four lanes of a full-HD frame reach
        // ~70 GB with the default; 4096 holds them to 16 GB at 5-pass batches).  Only ever lowers the budget; results do not depend on it (the batch a lane
        // holds shrinks, maxBatchFor / ensurePaths).
        const size_t asked = knobs::laneBudgetBytes();
        if (asked >= ((size_t)64 << 20) && asked < c->laneBudgetBytes) c->laneBudgetBytes = asked;
    }
    knobs::readContextKnobs(c);   // scheduling knobs (performance only; results do not depend on them)
    memset(&c->wide, 0, sizeof(c->wide));
    hipError_t e = hipSuccess;
    for (uint32_t i = 0; i < RT_MAX_LANES && e == hipSuccess; ++i)
    {
        e = acquireStream(c->device, &c->lanes[i].stream);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->lanes[i].accumulated, hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipMalloc((void**)&c->counters, 16 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(c->counters, 0, 16 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipHostMalloc((void**)&c->deviceFlags, 16 * sizeof(uint32_t), hipHostMallocMapped);
    if (e == hipSuccess) memset(c->deviceFlags, 0, 16 * sizeof(uint32_t));
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e == hipSuccess) e = hipMalloc((void**)&c->seedRingDev, (size_t)RT_SEED_RING * RTGPU_MAX_DIMENSIONS * sizeof(uint32_t));
    if (e == hipSuccess) e = hipHostMalloc((void**)&c->seedRingHost, (size_t)RT_SEED_RING * RTGPU_MAX_DIMENSIONS * sizeof(uint32_t), hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void**)&c->passRingDev, (size_t)RT_SEED_RING * sizeof(DevPass));
    if (e == hipSuccess) e = hipHostMalloc((void**)&c->passRingHost, (size_t)RT_SEED_RING * sizeof(DevPass), hipHostMallocDefault);
    for (int i = 0; i < RT_SEED_RING && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&c->seedEvents[i], hipEventDisableTiming);
    if (e != hipSuccess)
    {
        const std::string msg = std::string("context creation failed: ") + hipGetErrorString(e);
        rtgpu_destroy(c);
        return fail(RTGPU_ERR_DEVICE, msg);
    }
    *outCtx = c;
    return RTGPU_OK;
}

RTGPU_API int rtgpu_create_multi(const int* deviceIndices, uint32_t numDevices, RtgpuContext** outCtx)
{
    if (!outCtx) return fail(RTGPU_ERR_INVALID_ARGUMENT, "outCtx is NULL");
    *outCtx = nullptr;
    int visible = 0;
    if (hipGetDeviceCount(&visible) != hipSuccess || visible <= 0) return fail(RTGPU_ERR_NO_DEVICE, "no HIP device available");
    std::vector<int> devices;
    if (deviceIndices) devices.assign(deviceIndices, deviceIndices + numDevices);
    else for (int d = 0; d < (numDevices ? (int)numDevices : visible); ++d) devices.push_back(d);   // NULL: the first numDevices (0: all) visible ones
    if (devices.empty() || devices.size() > RTGPU_MAX_DEVICES) return fail(RTGPU_ERR_INVALID_ARGUMENT, "1..16 devices");
    for (int d : devices) if (d < 0 || d >= visible) return fail(RTGPU_ERR_INVALID_ARGUMENT, "device index out of range");
    RtgpuContext* c = nullptr;
    int r = rtgpu_create(devices[0], &c); if (r) return r;
    const uint32_t world = (uint32_t)devices.size();
    c->shard = { 0u, world };
    c->stagedGather = knobs::multiStaged();
    RtMultiInfo& info = c->multiInfo;
    info.numDevices = world; info.reasonDevice = -1; info.gatherReason = c->stagedGather ? 1u : 0u;
    for (uint32_t k = 0; k < world; ++k) { info.devices[k] = devices[k]; info.peerAccess[k] = devices[k] == devices[0] ? 1u : 0u; }
    for (uint32_t k = 1; k < world; ++k)
    {
        RtgpuContext* p = nullptr;
        r = rtgpu_create(devices[k], &p);
        if (r) { rtgpu_destroy(c); return r; }
        p->shard = { k, world }; p->isPeer = true;
        c->peers.push_back(p);
        if (devices[k] != devices[0] && !c->stagedGather)
        {
            // the gather kernel on device 0 reads the peers' sum buffers in place
            int can = 0;
            (void)hipSetDevice(devices[0]);
            if (hipDeviceCanAccessPeer(&can, devices[0], devices[k]) != hipSuccess || !can) { c->stagedGather = true; info.gatherReason = 2u; info.reasonDevice = devices[k]; }
            else
            {
                const hipError_t e = hipDeviceEnablePeerAccess(devices[k], 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { c->stagedGather = true; info.gatherReason = 3u; info.reasonDevice = devices[k]; info.reasonError = (int32_t)e; }
                else info.peerAccess[k] = 1u;
                (void)hipGetLastError();
            }
        }
    }
    (void)hipSetDevice(devices[0]);
    info.gatherMode = world == 1u ? RTGPU_GATHER_NONE : (c->stagedGather ? RTGPU_GATHER_STAGED_COPY : RTGPU_GATHER_PEER_KERNEL);
    if (knobs::verbose())
    {
        static const char* const why[] = { "", " (RTGPU_MULTI_STAGED=1)", " (hipDeviceCanAccessPeer: no)", " (hipDeviceEnablePeerAccess failed)" };
        fprintf(stderr, "[rtgpu] multi-device context: %u devices [", world);
        for (uint32_t k = 0; k < world; ++k) fprintf(stderr, "%s%d", k ? " " : "", devices[k]);
        fprintf(stderr, "], read-back gather = %s%s\n", world == 1u ? "none" : (c->stagedGather ? "hipMemcpyPeerAsync into staging buffers + kernel" : "kernel reading the peers' buffers in place (peer access)"),
                why[info.gatherReason < 4u ? info.gatherReason : 0u]);
    }
    *outCtx = c;
    return RTGPU_OK;
}

RTGPU_API int rtgpu_get_multi_info(RtgpuContext* c, RtMultiInfo* out)
{
    if (!c || !out) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = c->multiInfo;
    if (out->numDevices == 0u) { out->numDevices = 1u; out->devices[0] = c->device; out->peerAccess[0] = 1u; out->reasonDevice = -1; }   // a one-device context (rtgpu_create)
    return RTGPU_OK;
}

RTGPU_API int rtgpu_num_devices(RtgpuContext* c, uint32_t* outCount)
{
    if (!c || !outCount) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    *outCount = (uint32_t)c->peers.size() + 1u;
    return RTGPU_OK;
}

RTGPU_API void rtgpu_destroy(RtgpuContext* c)
{
    if (!c) return;
    for (RtgpuContext* p : c->peers) rtgpu_destroy(p);
    c->peers.clear();
    (void)hipSetDevice(c->device);
    (void)syncLanes(c);
    devFree(c->gatherStage);
    freeQuery(c);
    freeRecorder(c);
    freeAov(c);
    freeChain(c);
    freeDenoise(c);
    freeRaySource(c);
    freeScene(c); freeFilm(c);
    beamFreeRetired(c);
    devFree(c->beam.entries, c->beam.counts, c->beam.stats);
    if (c->beam.built) (void)hipEventDestroy(c->beam.built);
    for (uint32_t i = 0; i < RT_MAX_LANES; ++i)
    {
        freePaths(c->lanes[i]);
        if (i == 0) freeVcm(c);
        devFree(c->lanes[i].queueCounts, c->lanes[i].denseCounts);
        if (c->lanes[i].accumulated) (void)hipEventDestroy(c->lanes[i].accumulated);
    }
    devFree(c->counters, c->seedRingDev, c->passRingDev);
    if (c->deviceFlags) (void)hipHostFree(c->deviceFlags);
    if (c->seedRingHost) (void)hipHostFree(c->seedRingHost);
    if (c->passRingHost) (void)hipHostFree(c->passRingHost);
    for (int i = 0; i < RT_SEED_RING; ++i) if (c->seedEvents[i]) (void)hipEventDestroy(c->seedEvents[i]);
    if (c->refitOrder) (void)hipEventDestroy(c->refitOrder);
    for (auto& t : c->pendingTimed) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
    for (hipEvent_t e : c->eventPool) (void)hipEventDestroy(e);
    for (uint32_t i = 0; i < RT_MAX_LANES; ++i) if (c->lanes[i].stream) { (void)hipStreamSynchronize(c->lanes[i].stream); releaseStream(c->device, c->lanes[i].stream); }
    delete c;
}

#include "rt_runtime_scene.inl"

// slot -> pixel table: owned 64x64 tiles (tile % worldSize == rank), 8x8 blocks inside a tile, so that a
// wave covers an 8x8 pixel block (coherent primary rays)
static std::vector<uint32_t> buildSlotTable(uint32_t width, uint32_t height, RtgpuShard shard, const std::vector<uint8_t>& activeMask)
{
    std::vector<uint32_t> slots;
    slots.reserve((size_t)width * height / (shard.worldSize ? shard.worldSize : 1) + 4096);
    const uint32_t tilesX = (width + 63u) / 64u, tilesY = (height + 63u) / 64u;
    for (uint32_t ty = 0; ty < tilesY; ++ty)
        for (uint32_t tx = 0; tx < tilesX; ++tx)
        {
            const uint32_t tile = ty * tilesX + tx;
            if (shard.worldSize > 1 && tile % shard.worldSize != shard.rank) continue;
            for (uint32_t by = 0; by < 8; ++by)
                for (uint32_t bx = 0; bx < 8; ++bx)
                    for (uint32_t py = 0; py < 8; ++py)
                        for (uint32_t px = 0; px < 8; ++px)
                        {
                            const uint32_t x = tx * 64 + bx * 8 + px, y = ty * 64 + by * 8 + py;
                            if (x < width && y < height && (activeMask.empty() || activeMask[(size_t)y * width + x])) slots.push_back(x | (y << 16));
                        }
        }
    return slots;
}

// slot -> pixel table of the pixels this context renders: owned tiles, active blocks
static int rebuildSlots(RtgpuContext* c)
{
    devFree(c->slotPixel);
    beamInvalidate(c); beamFreeRetired(c);   // beam lists are per tile of the table that goes (like it, nothing in flight reads them here)
    const std::vector<uint32_t> slots = buildSlotTable(c->width, c->height, c->shard, c->activeMask);
    c->numSlots = (uint32_t)slots.size();
    // launches of a batch should stay large enough to fill 256 CUs: a 1/8 shard of a 1080p frame batches 16 passes
    // (measured on 1/8 of the Sponza-class frame: 0.57 -> 0.50 ms per pass), a full frame 8
    if (!c->passBatchFromEnv)
    {
        // (small frames / 1/8 shards of a full-HD frame: 20 passes per batch -- 16 -> 20: +3 % at the driver's 20 steps, profiles/r04_tail_sweep.txt)
        const uint32_t streamBase = knobs::passBatchBase(), smallBatch = knobs::smallFrameBatch();
        c->passBatch = c->numSlots != 0 && c->numSlots < 400000u ? (smallBatch ? smallBatch : 1u) : (streamBase ? streamBase : 1u);   // full frames: 5 -> 10 -> 20 -> 24 while streaming, one size per round of the lanes (flushBatch)
        // (very large frames: fewer passes per launch, an arena of 8 passes of an 8K frame would be 47 GB)
        while (c->passBatch > 1u && (size_t)c->numSlots * c->passBatch * ((size_t)R_NUM_BASE + RT_SHADOW_RECORDS) * sizeof(float4) > ((size_t)24 << 30)) c->passBatch /= 2u;
    }
    c->passBatchBase = c->passBatch;
    // four batch lanes: with the short re-trace launches behind k_trace_wide and streams that start with small batches, a fourth
    // concurrent launch sequence pays on full frames too (20 passes between read-backs: +4.6 %; 64 and 256 passes: unchanged)
    if (!c->lanesChosen) { c->numLanes = 4u; if (c->nextLane >= c->numLanes) c->nextLane = 0; }
    if (c->numSlots)
    {
        HIP_TRY(hipMalloc((void**)&c->slotPixel, slots.size() * sizeof(uint32_t)));
        HIP_TRY(rtMemcpy(c->slotPixel, slots.data(), slots.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    return RTGPU_OK;
}

static int rebuildFilm(RtgpuContext* c)
{
    waitDenoiseRead(c);
    freeFilm(c);
    if (c->width == 0 || c->height == 0) return RTGPU_OK;
    const size_t n = (size_t)c->width * c->height * 3;
    HIP_TRY(hipMalloc((void**)&c->sum, n * sizeof(float)));
    HIP_TRY(hipMalloc((void**)&c->secondary, n * sizeof(float)));
    HIP_TRY(hipMemset(c->sum, 0, n * sizeof(float)));
    HIP_TRY(hipMemset(c->secondary, 0, n * sizeof(float)));
    HIP_TRY(hipStreamSynchronize(nullptr));   // the batch lanes are non-blocking streams: they do not wait for the null stream's memsets
    c->activeMask.clear();   // a new film starts with the whole image active
    c->vcm.havePhotons = false;   // recorded per slot of the old film
    c->temporal.have = false;     // (and the history of rtgpu_denoise_temporal: another frame size, another film)
    return rebuildSlots(c);
}

RTGPU_API int rtgpu_resize(RtgpuContext* c, uint32_t width, uint32_t height)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (width == 0 || height == 0 || width > 65536u || height > 65536u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "Invalid viewport size");
    RT_FAN_OUT(c, rtgpu_resize(peer, width, height));
    HIP_TRY(hipSetDevice(c->device));
    { int fr = flushQueued(c); if (fr) return fr; }
    HIP_TRY(syncLanes(c));
    // a ray source is a frame's: the camera renders again, also when the size is the one the context has (an asynchronous AOV call may still read the table)
    // (both buffers are sized for the old frame: the one a refused table was copied into goes too)
    if (c->raySource.table || c->raySource.incoming) { waitQueries(c); dropRaySource(c); }
    c->width = width; c->height = height;
    return rebuildFilm(c);
}

RTGPU_API int rtgpu_set_shard(RtgpuContext* c, RtgpuShard shard)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (shard.worldSize == 0 || shard.rank >= shard.worldSize) return fail(RTGPU_ERR_INVALID_ARGUMENT, "invalid shard");
    if (!c->peers.empty() || c->isPeer) return fail(RTGPU_ERR_UNSUPPORTED, "a multi-device context shards the frame itself (rtgpu_create_multi)");
    HIP_TRY(hipSetDevice(c->device));
    { int fr = flushQueued(c); if (fr) return fr; }
    HIP_TRY(syncLanes(c));
    c->shard = shard;
    return rebuildFilm(c);
}

RTGPU_API int rtgpu_reset(RtgpuContext* c)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    RT_FAN_OUT(c, rtgpu_reset(peer));
    HIP_TRY(hipSetDevice(c->device));
    { int fr = flushQueued(c); if (fr) return fr; }
    HIP_TRY(syncLanes(c));
    waitDenoiseRead(c);
    if (c->sum)
    {
        const size_t n = (size_t)c->width * c->height * 3;
        HIP_TRY(hipMemset(c->sum, 0, n * sizeof(float)));
        HIP_TRY(hipMemset(c->secondary, 0, n * sizeof(float)));
    }
    HIP_TRY(hipMemset(c->counters, 0, 16 * sizeof(unsigned long long)));
    HIP_TRY(hipStreamSynchronize(nullptr));   // (see rebuildFilm)
    int r = resolveTimed(c); if (r) return r;
    memset(c->kernelMs, 0, sizeof(c->kernelMs)); memset(c->kernelLaunches, 0, sizeof(c->kernelLaunches));
    return RTGPU_OK;
}

#include "rt_runtime_render.inl"

#include "rt_runtime_vcm.inl"   // the bidirectional integrator's and the Light Tracer's launch sequences

static void defaultVcmParams(RtVcmParams& vp)
{
    memset(&vp, 0, sizeof(vp));
    vp.maxPathLength = 10; vp.useVertexConnection = 1; vp.useVertexMerging = 1;
    vp.initialMergingRadius = 0.02f; vp.minMergingRadius = 0.02f; vp.mergingRadiusMultiplier = 1.0f;
    for (int k = 0; k < 4; ++k) vp.bsdfSamplingWeight[k] = vp.lightSamplingWeight[k] = vp.vertexConnectingWeight[k] = vp.cameraConnectingWeight[k] = vp.vertexMergingWeight[k] = 1.0f;
}

RTGPU_API int rtgpu_set_integrator(RtgpuContext* c, uint32_t integrator, const RtVcmParams* vcm)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (integrator > RT_INTEGRATOR_LIGHT_TRACER) return fail(RTGPU_ERR_INVALID_ARGUMENT, "unknown integrator");
    if ((!c->peers.empty() || c->isPeer) && (integrator == RT_INTEGRATOR_VCM || integrator == RT_INTEGRATOR_LIGHT_TRACER))
        return fail(RTGPU_ERR_UNSUPPORTED, "VCM and the Light Tracer splat over the whole frame: they need a single-device context (rtgpu_create)");
    RT_FAN_OUT(c, rtgpu_set_integrator(peer, integrator, vcm));
    int r = rtgpu_synchronize(c); if (r) return r;
    RtVcmParams vp; defaultVcmParams(vp);
    if (vcm) vp = *vcm;
    if (integrator == RT_INTEGRATOR_VCM)
    {
        if (vp.maxPathLength < 1u || vp.maxPathLength > RT_VCM_MAX_PATH_LENGTH) return fail(RTGPU_ERR_INVALID_ARGUMENT, "maxPathLength must be 1..16");
        if (!(vp.initialMergingRadius >= vp.minMergingRadius) || !(vp.minMergingRadius > 0.0f)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "merging radii: initial >= min > 0 required");
        if (!(vp.mergingRadiusMultiplier > 0.0f && vp.mergingRadiusMultiplier <= 1.0f)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "mergingRadiusMultiplier must be in (0, 1]");
    }
    c->vcm.enabled = integrator == RT_INTEGRATOR_VCM;
    c->plainPathTracer = integrator == RT_INTEGRATOR_PATH_TRACER;
    c->lightTracer = integrator == RT_INTEGRATOR_LIGHT_TRACER;
    c->debugMode = integrator == RT_INTEGRATOR_DEBUG ? (c->debugMode >= 0 ? c->debugMode : (int)DBG_TRIANGLE_ID) : -1;   // DebugRenderer's default mode, DebugRenderer.cpp:16
    c->vcm.params = vp;
    c->vcm.havePhotons = false;
    return RTGPU_OK;
}

RTGPU_API int rtgpu_set_debug_rendering_mode(RtgpuContext* c, uint32_t mode)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (mode >= DBG_NUM_MODES) return fail(RTGPU_ERR_INVALID_ARGUMENT, "unknown DebugRenderingMode");
    if (c->debugMode < 0) return fail(RTGPU_ERR_NOT_READY, "the integrator is not RT_INTEGRATOR_DEBUG");
    RT_FAN_OUT(c, rtgpu_set_debug_rendering_mode(peer, mode));
    int r = rtgpu_synchronize(c); if (r) return r;
    c->debugMode = (int)mode;
    return RTGPU_OK;
}

RTGPU_API int rtgpu_vcm_num_photons(RtgpuContext* c, uint32_t* outCount)
{
    if (!c || !outCount) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    int r = rtgpu_synchronize(c); if (r) return r;
    *outCount = 0;
    if (!c->vcm.havePhotons || !c->vcm.arena.photonCount) return RTGPU_OK;
    std::vector<uint32_t> counts(c->numSlots);
    HIP_TRY(rtMemcpy(counts.data(), c->vcm.arena.photonCount + (size_t)c->vcm.lastPhotonPass * c->numSlots, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    unsigned long long total = 0; for (uint32_t n : counts) total += n;
    *outCount = (uint32_t)total;
    return RTGPU_OK;
}

// what a pass needs before it can be queued or recorded (rtgpu_render_pass, rtgpu_record_paths)
static int checkPass(const RtgpuContext* c, const RtPassParams* p)
{
    if (!c->sceneReady) return fail(RTGPU_ERR_NOT_READY, "rtgpu_upload_scene has not been called");
    if (!c->sum) return fail(RTGPU_ERR_NOT_READY, "rtgpu_resize has not been called");
    if (p->numDimensions > RTGPU_MAX_DIMENSIONS) return fail(RTGPU_ERR_INVALID_ARGUMENT, "numDimensions exceeds RTGPU_MAX_DIMENSIONS");
    if (p->numDimensions > 0 && !p->seed) return fail(RTGPU_ERR_INVALID_ARGUMENT, "seed is NULL");
    if (p->maxRayDepth >= 255u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "maxRayDepth must be < 255");
    if (!c->raySource.any() && p->camera.dofEnable && p->camera.bokehShape > 2u) return fail(RTGPU_ERR_UNSUPPORTED, "bokeh shapes: circle, hexagon, square (NGon is a TODO in the reference, texture-shaped bokeh is not implemented)");
    // (a lens source applies the pass's sample offset to its footprints: it is the one word of the caller's camera and offset that is read)
    if (c->raySource.kind == 2u && !(std::isfinite(p->sampleOffset[0]) && std::isfinite(p->sampleOffset[1])))
        return fail(RTGPU_ERR_INVALID_ARGUMENT, "sampleOffset is not finite (a lens source applies it to every ray's footprint)");
    return RTGPU_OK;
}
// the device's per-pass constants; `seed` is assigned where the pass is submitted
static void makeDevPass(const RtgpuContext* c, const RtPassParams* p, DevPass& pass)
{
    memset(&pass, 0, sizeof(pass));
    pass.camera = p->camera;
    pass.seed = nullptr;
    pass.numDimensions = p->numDimensions;
    pass.blueNoiseLayers = (c->sceneDev.blueNoise && p->useBlueNoise) ? 4u : 0u;   // GenericSampler.cpp:69-73
    pass.sampleOffset[0] = p->sampleOffset[0]; pass.sampleOffset[1] = p->sampleOffset[1];
    pass.passIndex = p->passIndex;
    pass.maxRayDepth = p->maxRayDepth;
    pass.minRussianRouletteDepth = p->minRussianRouletteDepth;
    pass.lightSamplingStrategy = p->lightSamplingStrategy;
    memcpy(pass.lightSamplingWeight, p->lightSamplingWeight, 16);
    memcpy(pass.bsdfSamplingWeight, p->bsdfSamplingWeight, 16);
    pass.rngKey[0] = p->rngKey[0]; pass.rngKey[1] = p->rngKey[1];
    pass.width = c->width; pass.height = c->height;
    // under a ray source the table is the camera: the pass carries one that draws nothing -- dense shading re-runs it at bounce 0 only to restore the
    // sampler (rt_dense.inl), which then stays as the table kernels left it -- and the caller's camera and sample offset are never read
    if (c->raySource.kind == 1u) { memset(&pass.camera, 0, sizeof(pass.camera)); pass.sampleOffset[0] = 0.0f; pass.sampleOffset[1] = 0.0f; }
    // under a lens source the pass keeps its sample offset (the lens kernels jitter by it) and carries a zeroed camera with the SOURCE's lens: the dense
    // re-run then takes the two draws the lens kernel took -- or none -- and discards its ray
    if (c->raySource.kind == 2u)
    {
        memset(&pass.camera, 0, sizeof(pass.camera));
        pass.camera.dofEnable = c->raySource.lens; pass.camera.bokehShape = c->raySource.bokehShape;
    }
}

RTGPU_API int rtgpu_render_pass(RtgpuContext* c, const RtPassParams* p)
{
    if (!c || !p) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    { const int r = checkPass(c, p); if (r) return r; }
    RT_FAN_OUT(c, rtgpu_render_pass(peer, p));   // asynchronous on every device: the shards render side by side
    HIP_TRY(hipSetDevice(c->device));
    waitDenoiseRead(c);
    if (c->numSlots == 0) return RTGPU_OK;   // this shard owns no pixels
    if (c->vcm.enabled) return vcmRenderPass(c, p);
    if (c->lightTracer) return lightTracerRenderPass(c, p);

    CtxPending pd;
    DevPass& pass = pd.pass;
    makeDevPass(c, p, pass);   // (its seed pointer is assigned when the batch is submitted)
    pd.seeds.assign(p->seed, p->seed + p->numDimensions);   // the caller's array may be reused right away

    // all passes of a batch share the structural parameters; a change submits what is queued first
    if (!c->pending.empty())
    {
        const DevPass& f = c->pending[0].pass;
        const bool same = f.numDimensions == pass.numDimensions && f.blueNoiseLayers == pass.blueNoiseLayers && f.maxRayDepth == pass.maxRayDepth &&
                          f.minRussianRouletteDepth == pass.minRussianRouletteDepth && f.lightSamplingStrategy == pass.lightSamplingStrategy &&
                          memcmp(f.lightSamplingWeight, pass.lightSamplingWeight, 16) == 0 && memcmp(f.bsdfSamplingWeight, pass.bsdfSamplingWeight, 16) == 0;
        if (!same) { int r = flushPending(c); if (r) return r; }
    }
    c->pending.push_back(std::move(pd));
    const uint32_t lightLimit = maxBatchFor(c, pass.lightSamplingStrategy == RT_LIGHT_SAMPLING_ALL ? c->numLights : 1u);
    if (c->pending.size() >= (c->passBatch < lightLimit ? c->passBatch : lightLimit)) return flushBatch(c, 0u);
    return RTGPU_OK;
}

RTGPU_API int rtgpu_synchronize(RtgpuContext* c)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    // every device's queued passes -- the first device's included -- are submitted before the first wait, so that the tails run side by side
    for (RtgpuContext* peer : c->peers) { HIP_TRY(hipSetDevice(peer->device)); int r = flushPending(peer); if (r) return r; }
    HIP_TRY(hipSetDevice(c->device));
    { int r = vcmFlush(c); if (r) return r; }
    { int r = flushPending(c); if (r) return r; }
    RT_FAN_OUT(c, rtgpu_synchronize(peer));
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(syncLanes(c));
    waitDenoiseRead(c);   // (the read-back calls gather the peers' tiles into the sum buffer next)
    c->batchesSinceSync = 0; c->batchesAtThisSize = 0;
    if (!c->passBatchFromEnv) c->passBatch = c->passBatchBase;
    if (c->deviceFlags && c->deviceFlags[0] != 0u)
    {
        c->deviceFlags[0] = 0u;
        return fail(RTGPU_ERR_DEVICE, "dense path state: a region of the arena overflowed (the frame since the last reset is invalid)");
    }
    return resolveTimed(c);
}

RTGPU_API int rtgpu_read_sum(RtgpuContext* c, float* sumRGB, float* secondaryRGB)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (!c->sum) return fail(RTGPU_ERR_NOT_READY, "rtgpu_resize has not been called");
    int r = rtgpu_synchronize(c); if (r) return r;
    r = gatherPeers(c); if (r) return r;
    const size_t bytes = (size_t)c->width * c->height * 3 * sizeof(float);
    if (sumRGB) HIP_TRY(rtMemcpy(sumRGB, c->sum, bytes, hipMemcpyDeviceToHost));
    if (secondaryRGB) HIP_TRY(rtMemcpy(secondaryRGB, c->secondary, bytes, hipMemcpyDeviceToHost));
    return RTGPU_OK;
}

// page-locked host memory for the read-back calls: hipMemcpy into registered memory runs at the PCIe link's rate
RTGPU_API int rtgpu_host_register(RtgpuContext* c, void* ptr, size_t bytes)
{
    if (!c || !ptr || !bytes) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    const hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterPortable);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(e == hipErrorNoDevice || e == hipErrorInvalidDevice ? RTGPU_ERR_NO_DEVICE : RTGPU_ERR_DEVICE, std::string("hipHostRegister: ") + hipGetErrorString(e)); }
    return RTGPU_OK;
}

RTGPU_API int rtgpu_host_unregister(RtgpuContext* c, void* ptr)
{
    if (!c || !ptr) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    const hipError_t e = hipHostUnregister(ptr);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(RTGPU_ERR_DEVICE, std::string("hipHostUnregister: ") + hipGetErrorString(e)); }
    return RTGPU_OK;
}

RTGPU_API int rtgpu_get_device_sum(RtgpuContext* c, void** sumDevice, void** secondaryDevice, size_t* numFloats)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (!c->sum) return fail(RTGPU_ERR_NOT_READY, "rtgpu_resize has not been called");
    int r = rtgpu_synchronize(c); if (r) return r;   // the pointers are handed out with every queued pass accumulated
    r = gatherPeers(c); if (r) return r;
    if (sumDevice) *sumDevice = c->sum;
    if (secondaryDevice) *secondaryDevice = c->secondary;
    if (numFloats) *numFloats = (size_t)c->width * c->height * 3;
    return RTGPU_OK;
}

RTGPU_API int rtgpu_get_counters(RtgpuContext* c, RtCounters* out)
{
    if (!c || !out) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    int r = rtgpu_synchronize(c); if (r) return r;
    unsigned long long host[16];
    HIP_TRY(rtMemcpy(host, c->counters, sizeof(host), hipMemcpyDeviceToHost));
    memset(out, 0, sizeof(*out));
    out->numRays = host[C_RAYS]; out->numShadowRays = host[C_SHADOW]; out->numShadowRaysHit = host[C_SHADOW_HIT];
    out->numPrimaryRays = host[C_PRIMARY]; out->numRayBoxTests = host[C_BOX]; out->numPassedRayBoxTests = host[C_BOX_PASS];
    out->numRayTriangleTests = host[C_TRI]; out->numPassedRayTriangleTests = host[C_TRI_PASS];
    out->numMeshHits = host[C_MESH_HITS]; out->numAnalyticHits = host[C_ANALYTIC_HITS];
    out->numShadowRayBoxTests = host[C_BOX_SHADOW]; out->numShadowRayTriangleTests = host[C_TRI_SHADOW];
    out->numRetracedRays = host[RT_COUNTER_RETRACED];
    out->_reserved[0] = host[RT_COUNTER_RETRACED + 1]; out->_reserved[1] = host[RT_COUNTER_RETRACED + 2]; out->_reserved[2] = host[RT_COUNTER_RETRACED + 3];   // diagnostics of the re-encoded walks: untrusted rays, stack overflows
    for (RtgpuContext* peer : c->peers)
    {
        RtCounters pc;
        r = rtgpu_get_counters(peer, &pc); if (r) return r;
        uint64_t* a = (uint64_t*)out; const uint64_t* b = (const uint64_t*)&pc;
        for (size_t i = 0; i < sizeof(RtCounters) / sizeof(uint64_t); ++i) a[i] += b[i];
    }
    HIP_TRY(hipSetDevice(c->device));
    return RTGPU_OK;
}

RTGPU_API int rtgpu_set_intersection_counters(RtgpuContext* c, int enable)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    RT_FAN_OUT(c, rtgpu_set_intersection_counters(peer, enable));
    int r = rtgpu_synchronize(c); if (r) return r;
    c->countIntersections = enable != 0;
    return RTGPU_OK;
}

static int checkBlocks(RtgpuContext* c, uint32_t numBlocks, const RtBlock* blocks)
{
    if (numBlocks && !blocks) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    for (uint32_t i = 0; i < numBlocks; ++i)
        if (blocks[i].minX >= blocks[i].maxX || blocks[i].minY >= blocks[i].maxY || blocks[i].maxX > c->width || blocks[i].maxY > c->height)
            return fail(RTGPU_ERR_INVALID_ARGUMENT, "block outside the viewport or empty");
    return RTGPU_OK;
}

RTGPU_API int rtgpu_compute_block_errors(RtgpuContext* c, uint32_t numPasses, uint32_t numBlocks, const RtBlock* blocks, float* outErrors)
{
    if (!c || (numBlocks && !outErrors)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!c->sum) return fail(RTGPU_ERR_NOT_READY, "rtgpu_resize has not been called");
    if (numPasses == 0) return fail(RTGPU_ERR_INVALID_ARGUMENT, "numPasses must be > 0");
    int r = checkBlocks(c, numBlocks, blocks); if (r) return r;
    if (numBlocks == 0) return RTGPU_OK;
    r = rtgpu_synchronize(c); if (r) return r;
    r = gatherPeers(c); if (r) return r;
    std::vector<ErrorRow> rows; std::vector<uint32_t> firstRow(numBlocks);
    for (uint32_t i = 0; i < numBlocks; ++i)
    {
        firstRow[i] = (uint32_t)rows.size();
        for (uint32_t y = blocks[i].minY; y < blocks[i].maxY; ++y) rows.push_back({ i, y });
    }
    RtBlock* dBlocks = nullptr; ErrorRow* dRows = nullptr; uint32_t* dFirst = nullptr; float* dRowErrors = nullptr; float* dOut = nullptr;
    hipError_t e = hipMalloc((void**)&dBlocks, numBlocks * sizeof(RtBlock));
    if (e == hipSuccess) e = hipMalloc((void**)&dRows, rows.size() * sizeof(ErrorRow));
    if (e == hipSuccess) e = hipMalloc((void**)&dFirst, numBlocks * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&dRowErrors, rows.size() * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&dOut, numBlocks * sizeof(float));
    if (e == hipSuccess) e = rtMemcpy(dBlocks, blocks, numBlocks * sizeof(RtBlock), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = rtMemcpy(dRows, rows.data(), rows.size() * sizeof(ErrorRow), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = rtMemcpy(dFirst, firstRow.data(), numBlocks * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess)
    {
        hipStream_t st = c->lanes[0].stream;
        const uint32_t numRows = (uint32_t)rows.size();
        hipLaunchKernelGGL(k_block_error_rows, dim3((numRows + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, st, c->sum, c->secondary, c->width, dBlocks, dRows, numRows,
                           1.0f / (float)numPasses, dRowErrors);
        hipLaunchKernelGGL(k_block_error_total, dim3((numBlocks + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, st, dBlocks, dFirst, numBlocks, dRowErrors, c->width * c->height, dOut);
        e = hipStreamSynchronize(st);
    }
    if (e == hipSuccess) e = rtMemcpy(outErrors, dOut, numBlocks * sizeof(float), hipMemcpyDeviceToHost);
    for (void* p : { (void*)dBlocks, (void*)dRows, (void*)dFirst, (void*)dRowErrors, (void*)dOut }) if (p) (void)hipFree(p);
    if (e != hipSuccess) return fail(RTGPU_ERR_DEVICE, std::string("rtgpu_compute_block_errors: ") + hipGetErrorString(e));
    return RTGPU_OK;
}

RTGPU_API int rtgpu_set_active_blocks(RtgpuContext* c, uint32_t numBlocks, const RtBlock* blocks)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (!c->sum) return fail(RTGPU_ERR_NOT_READY, "rtgpu_resize has not been called");
    int r = checkBlocks(c, numBlocks, blocks); if (r) return r;
    RT_FAN_OUT(c, rtgpu_set_active_blocks(peer, numBlocks, blocks));
    r = rtgpu_synchronize(c); if (r) return r;
    c->activeMask.clear();
    if (numBlocks)
    {
        c->activeMask.assign((size_t)c->width * c->height, 0);
        for (uint32_t i = 0; i < numBlocks; ++i)
            for (uint32_t y = blocks[i].minY; y < blocks[i].maxY; ++y)
                for (uint32_t x = blocks[i].minX; x < blocks[i].maxX; ++x)
                {
                    uint8_t& m = c->activeMask[(size_t)y * c->width + x];
                    if (m) return fail(RTGPU_ERR_INVALID_ARGUMENT, "active blocks overlap");
                    m = 1;
                }
    }
    return rebuildSlots(c);
}

// colorScale = colorFilter * 2^exposure on the host like the reference (Viewport.cpp:453)
static PostScale postScale(const RtPostprocessParams* p)
{
    const float exposureScale = powf(2.0f, p->exposure);
    return { { p->colorFilter[0] * exposureScale, p->colorFilter[1] * exposureScale, p->colorFilter[2] * exposureScale } };
}

// Bitmap::GaussianBlur(sigma, 8) on a width x height image: its window plan (Bitmap.cpp:935-946), or the refusal.  The reference's blur works on
// 4 columns at a time and on 4096-entry line buffers without bounds checks (Bitmap.cpp:925-931, :941, :978-990): sizes it would read or write
// out of bounds for are refused here
static int blurPlanFor(float sigma, uint32_t width, uint32_t height, BlurPlan* plan)
{
    if (width > 4096u || height > 4096u || (width % 4u) != 0u) return fail(RTGPU_ERR_UNSUPPORTED, "bloom: width must be a multiple of 4 and both sizes <= 4096 (Bitmap::GaussianBlur)");
    const uint32_t n = 8u;
    float wIdeal = sqrtf((12.0f * sigma * sigma / n) + 1.0f);
    uint32_t wl = (uint32_t)floorf(wIdeal);
    if (wl % 2u == 0u) wl--;
    const uint32_t wu = wl + 2u;
    const float mIdeal = (12.0f * sigma * sigma - n * wl * wl - 4.0f * n * wl - 3.0f * n) / (-4.0f * wl - 4.0f);
    plan->n = n; plan->wl = wl; plan->wu = wu; plan->m = roundf(mIdeal);
    if (width <= 2u * wu + 1u || height <= 2u * wu + 1u) return fail(RTGPU_ERR_UNSUPPORTED, "bloom: the image is not larger than the blur window (2 * wu + 1 pixels; 195 for the widest of a frame's five levels)");
    return RTGPU_OK;
}
// the blur itself, in place on a device image: rows, then columns.  lines: 2 * width * height * 3 floats of scratch
static void blurImage(hipStream_t stream, float* img, uint32_t width, uint32_t height, const BlurPlan& plan, float* lines)
{
    const size_t pixels = (size_t)width * height;
    hipLaunchKernelGGL(k_blur_lines, dim3((height * 3u + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, stream, img, width, height, 0u, plan, lines, lines + pixels * 3);
    hipLaunchKernelGGL(k_blur_lines, dim3((width * 3u + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, stream, img, width, height, 1u, plan, lines, lines + pixels * 3);
}

// rtgpu_postprocess (rgbHost == nullptr: the sum buffer) and rtgpu_postprocess_from (a caller's image of the context's size, rt_runtime_denoise.inl)
static int postprocessImage(RtgpuContext* c, const RtPostprocessParams* p, const float* rgbHost, uint32_t* frontBufferBGRA)
{
    if (!c->sum) return fail(RTGPU_ERR_NOT_READY, "rtgpu_resize has not been called");
    const bool bloom = p->bloomFactor > 0.0f;
    BlurPlan plans[5];
    if (bloom)
    {
        float blurSigma = 2.0f;   // Viewport.cpp:438-444
        for (int l = 0; l < 5; ++l)
        {
            const int pr = blurPlanFor(blurSigma, c->width, c->height, &plans[l]); if (pr) return pr;
            blurSigma *= 2.5f;
        }
    }
    if (p->tonemapper > RT_TONEMAPPER_ACES) return fail(RTGPU_ERR_INVALID_ARGUMENT, "unknown tonemapper");
    if (p->numPasses == 0) return fail(RTGPU_ERR_INVALID_ARGUMENT, "numPasses must be > 0");
    int r = rtgpu_synchronize(c); if (r) return r;
    if (!rgbHost) { r = gatherPeers(c); if (r) return r; }   // (a caller's image: the sum buffer is not read)
    const size_t pixels = (size_t)c->width * c->height;
    uint32_t* dFront = nullptr;
    float* dImage = nullptr;
    if (rgbHost)
    {
        HIP_TRY(hipMalloc((void**)&dImage, pixels * 3 * sizeof(float)));
        const hipError_t ce = rtMemcpy(dImage, rgbHost, pixels * 3 * sizeof(float), hipMemcpyHostToDevice);
        if (ce != hipSuccess) { devFree(dImage); return fail(RTGPU_ERR_DEVICE, std::string("rtgpu_postprocess_from: ") + hipGetErrorString(ce)); }
    }
    const float* image = rgbHost ? dImage : c->sum;
    { const hipError_t fe = hipMalloc((void**)&dFront, pixels * sizeof(uint32_t)); if (fe != hipSuccess) { devFree(dImage); HIP_TRY(fe); } }
    const PostScale scale = postScale(p);
    hipStream_t stream = c->lanes[0].stream;
    hipError_t e = hipSuccess;
    float* dBlur = nullptr; float* dLines = nullptr;
    if (!bloom) hipLaunchKernelGGL(k_postprocess, dim3((uint32_t)((pixels + RT_BLOCK - 1) / RT_BLOCK)), dim3(RT_BLOCK), 0, stream, image, dFront, c->width, c->height, *p, scale);
    else
    {
        // mBlurredImages[i] = GaussianBlur(copy of (i == 0 ? mSum : mBlurredImages[i - 1]), sigma_i, 8), Viewport.cpp:436-445
        e = hipMalloc((void**)&dBlur, pixels * 3 * sizeof(float) * 5);
        if (e == hipSuccess) e = hipMalloc((void**)&dLines, pixels * 3 * sizeof(float) * 2);
        BloomLevels levels;
        for (int l = 0; l < 5 && e == hipSuccess; ++l)
        {
            float* img = dBlur + (size_t)l * pixels * 3;
            levels.level[l] = img;
            e = hipMemcpyAsync(img, l == 0 ? image : dBlur + (size_t)(l - 1) * pixels * 3, pixels * 3 * sizeof(float), hipMemcpyDeviceToDevice, stream);
            if (e != hipSuccess) break;
            blurImage(stream, img, c->width, c->height, plans[l], dLines);
        }
        if (e == hipSuccess) hipLaunchKernelGGL(k_postprocess_bloom, dim3((uint32_t)((pixels + RT_BLOCK - 1) / RT_BLOCK)), dim3(RT_BLOCK), 0, stream, image, levels, dFront, c->width, c->height, *p, scale);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = rtMemcpy(frontBufferBGRA, dFront, pixels * sizeof(uint32_t), hipMemcpyDeviceToHost);
    devFree(dFront, dBlur, dLines, dImage);
    if (e != hipSuccess) return fail(RTGPU_ERR_DEVICE, std::string("rtgpu_postprocess: ") + hipGetErrorString(e));
    return RTGPU_OK;
}

RTGPU_API int rtgpu_postprocess(RtgpuContext* c, const RtPostprocessParams* p, uint32_t* frontBufferBGRA)
{
    if (!c || !p || !frontBufferBGRA) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    return postprocessImage(c, p, nullptr, frontBufferBGRA);
}

#include "rt_runtime_kat.inl"
#include "rt_runtime_query.inl"
#include "rt_runtime_paths.inl"
#include "rt_runtime_aov.inl"
#include "rt_runtime_denoise.inl"
#include "rt_runtime_temporal.inl"
#include "rt_runtime_refit.inl"   // rtgpu_update_mesh: a deformed mesh's tables refitted on the device
#include "rt_runtime_raysource.inl"   // rtgpu_set_ray_source, rtgpu_set_lens_source: primary rays from a table of the caller's

RTGPU_API int rtgpu_set_concurrency(RtgpuContext* c, uint32_t lanes)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (lanes < 1 || lanes > RT_MAX_LANES) return fail(RTGPU_ERR_INVALID_ARGUMENT, "lanes must be 1..6");
    RT_FAN_OUT(c, rtgpu_set_concurrency(peer, lanes));
    int r = rtgpu_synchronize(c); if (r) return r;
    c->numLanes = lanes; c->nextLane = 0; c->lanesChosen = true;
    return RTGPU_OK;
}

RTGPU_API int rtgpu_set_schedule(RtgpuContext* c, uint32_t knob, int32_t value)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (knob > RTGPU_SCHEDULE_LOCAL_RETRACE || value < -1 || (knob == RTGPU_SCHEDULE_LOCAL_RETRACE && value > 1) || value > 254) return fail(RTGPU_ERR_INVALID_ARGUMENT, "unknown knob or value out of range");
    RT_FAN_OUT(c, rtgpu_set_schedule(peer, knob, value));
    int r = rtgpu_synchronize(c); if (r) return r;
    if (knob == RTGPU_SCHEDULE_TAIL_BOUNCE) c->tailBounce = value; else c->localRetrace = value;
    return RTGPU_OK;
}

RTGPU_API int rtgpu_enable_timing(RtgpuContext* c, int enable)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    RT_FAN_OUT(c, rtgpu_enable_timing(peer, enable));
    int r = rtgpu_synchronize(c); if (r) return r;
    c->timing = enable != 0;
    return RTGPU_OK;
}

RTGPU_API int rtgpu_get_walk_info(RtgpuContext* c, RtWalkInfo* out)
{
    if (!c || !out) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    const uint32_t kernel = !useWide(c) ? RTGPU_WALK_BINARY : (c->wide.nodes ? RTGPU_WALK_WIDE : RTGPU_WALK_WIDE2);
    out->kernel = kernel; out->reserved = 0u;
    out->nodeBytes = c->walkNodeBytes[kernel]; out->leafBoxBytes = c->walkLeafBoxBytes[kernel]; out->triangleBytes = c->walkTriangleBytes;
    return RTGPU_OK;
}

// ---- beam lists (rt_beam_lists.h; the policy is beamListsFor, rt_runtime_render.inl) ----
RTGPU_API int rtgpu_set_beam_margin(RtgpuContext* c, float pixels)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (!(pixels >= 0.0f) || !(pixels <= 64.0f)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the beam margin is 0 .. 64 pixels");
    RT_FAN_OUT(c, rtgpu_set_beam_margin(peer, pixels));
    c->beam.margin = pixels;   // (part of the lists' key: the next still batch builds for it)
    return RTGPU_OK;
}

RTGPU_API int rtgpu_get_beam_list_info(RtgpuContext* c, RtBeamListInfo* out)
{
    if (!c || !out) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    { int fr = flushQueued(c); if (fr) return fr; }   // (a queued batch may build)
    const uint32_t retiredArrays = (uint32_t)c->beam.retired.size();   // before the lanes go idle, which frees them
    int r = rtgpu_synchronize(c); if (r) return r;
    const RtgpuContext::Beam& b = c->beam;
    unsigned long long stats[3] = { 0ull, 0ull, 0ull };
    if (b.stats) HIP_TRY(rtMemcpy(stats, b.stats, sizeof(stats), hipMemcpyDeviceToHost));
    out->allocations = b.allocations; out->retiredArrays = retiredArrays; out->reserved = 0u;
    out->builds = b.builds; out->packetsScanned = stats[0]; out->packetsWalkedOffset = stats[1]; out->packetsWalkedNoList = stats[2];
    out->valid = b.valid ? 1u : 0u; out->capacity = b.valid ? b.capacity : 0u; out->numTiles = b.valid ? b.numTiles : 0u; out->margin = b.valid ? b.builtMargin : b.margin;
    return RTGPU_OK;
}

RTGPU_API int rtgpu_read_beam_lists(RtgpuContext* c, int fromHost, uint32_t* counts, uint32_t* entries)
{
    if (!c || !counts || !entries) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    int r = rtgpu_synchronize(c); if (r) return r;
    const RtgpuContext::Beam& b = c->beam;
    if (!b.valid || !c->wide.nodes || c->updatable.objects.size() != 1u) return fail(RTGPU_ERR_NOT_READY, "no valid beam lists");
    if (!fromHost)
    {
        HIP_TRY(rtMemcpy(counts, b.counts, (size_t)b.numTiles * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(rtMemcpy(entries, b.entries, (size_t)b.numTiles * b.capacity * sizeof(BeamEntry), hipMemcpyDeviceToHost));
        return RTGPU_OK;
    }
    std::vector<float4> nodes((size_t)c->wide.numNodes * 4u), gate((size_t)(c->walkLeafBoxBytes[RTGPU_WALK_WIDE] / sizeof(float4)));
    std::vector<uint32_t> slots(c->numSlots);
    HIP_TRY(rtMemcpy(nodes.data(), c->wide.nodes, nodes.size() * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_TRY(rtMemcpy(gate.data(), c->wide.gate, gate.size() * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_TRY(rtMemcpy(slots.data(), c->slotPixel, slots.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    BeamCamera local;
    float lo[3], hi[3];
    beamTreeBounds(c->wide.base, c->wide.step, lo, hi);
    if (!beamCameraFor(b.camera, c->updatable.objects[0].invTransform, b.width, b.height, b.builtMargin, lo, hi, local)) return fail(RTGPU_ERR_NOT_READY, "no valid beam lists");
    const BeamListsHost h = buildBeamLists(nodes.data(), gate.data(), c->wide.base, c->wide.step, slots.data(), c->numSlots, local, b.capacity);
    memcpy(counts, h.counts.data(), h.counts.size() * sizeof(uint32_t));
    memcpy(entries, h.entries.data(), h.entries.size() * sizeof(BeamEntry));
    return RTGPU_OK;
}

RTGPU_API int rtgpu_get_update_info(RtgpuContext* c, RtUpdateInfo* out)
{
    if (!c || !out) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = c->updatable.info;
    out->walk = !useWide(c) ? RTGPU_WALK_BINARY : (c->wide.nodes ? RTGPU_WALK_WIDE : RTGPU_WALK_WIDE2);
    return RTGPU_OK;
}

RTGPU_API int rtgpu_get_kernel_times(RtgpuContext* c, double ms[RTGPU_NUM_KERNEL_CLASSES], uint64_t launches[RTGPU_NUM_KERNEL_CLASSES],
                                     const char* names[RTGPU_NUM_KERNEL_CLASSES])
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    int r = rtgpu_synchronize(c); if (r) return r;
    for (int i = 0; i < RTGPU_NUM_KERNEL_CLASSES; ++i)
    {
        if (ms) ms[i] = c->kernelMs[i];
        if (launches) launches[i] = c->kernelLaunches[i];
        if (names) names[i] = kKernelClassNames[i];
    }
    return RTGPU_OK;
}
