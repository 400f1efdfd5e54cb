// rt_runtime_query.inl -- batched ray queries, host side.  Included by rt_runtime.hip.

// ---- batched ray queries (include/rtgpu.h, rtgpu_trace_rays; kernels: rt_query.inl) ----------------------------------------------------------
// A chunk of rays goes through k_query_load -> the walk the context renders with -> k_query_store (-> k_query_evaluate), on the query's own arena.
#define RT_QUERY_CHUNK (1u << 22)   // rays per chunk: 4 M x 176 bytes of path records
enum { QC_QUEUE = 0, QC_CURSOR, QC_EXACT, QC_EXACT_SHADOW, QC_EXACT_CURSOR, QC_WORDS = 8 };

static int ensureQueryArena(RtgpuContext* c, uint32_t rays)
{
    RtgpuContext::Query& q = c->query;
    WalkArena& w = q.arena;
    if (!q.done) HIP_TRY(hipEventCreateWithFlags(&q.done, hipEventDisableTiming));
    if (!w.counts) HIP_TRY(hipMalloc((void**)&w.counts, QC_WORDS * sizeof(uint32_t)));
    if (!w.counters) HIP_TRY(hipMalloc((void**)&w.counters, 16 * sizeof(unsigned long long)));
    const uint32_t want = rays < RT_QUERY_CHUNK ? rays : RT_QUERY_CHUNK;   // (the arena grows up to the chunk)
    if (w.paths.base && w.paths.capacity >= want) return RTGPU_OK;
    freeQueryArena(c);   // (waits for the queries still using it)
    { const int r = growWalkArena(w, want); if (r) return r; }
    HIP_TRY(hipMalloc((void**)&q.stagedRays, (size_t)w.paths.capacity * sizeof(RtQueryRay)));
    HIP_TRY(hipMalloc((void**)&q.stagedHits, (size_t)w.paths.capacity * sizeof(RtQueryHit)));
    HIP_TRY(hipMalloc((void**)&q.stagedSurfaces, (size_t)w.paths.capacity * sizeof(RtQuerySurface)));
    HIP_TRY(hipMalloc((void**)&q.stagedOccluded, (size_t)w.paths.capacity * sizeof(uint32_t)));
    return RTGPU_OK;
}

// The walk over an arena of the library's own (ray queries, AOVs), whose queue holds closest-hit rays (`closest`) or any-hit requests.  `wide`: the render path's pair -- the 4-wide walk hands the rays it does not decide to the re-trace launch (which alone gives them a result); no
// block-local second walk and no k_trace_monster hand-over, neither changes a result.  Otherwise the reference's binary walk (k_trace), counting where the
// context counts or `rayCounts` (TravTuning::rayCounts: every closest-hit ray's own counts) is asked for.  Rays start where the caller put them: no offset.
static void launchArenaWalk(RtgpuContext* c, hipStream_t stream, const WalkArena& w, bool closest, bool wide, uint4* rayCounts)
{
    TraceStep s = { stream, w.counters, w.paths };
    if (closest) { s.queue = w.queue; s.queueCount = w.counts + QC_QUEUE; } else { s.shadowQueue = w.queue; s.shadowCount = w.counts + QC_QUEUE; }
    s.cursor = w.counts + QC_CURSOR;
    s.exactQueue = w.exactQueue; s.exactCount = w.counts + QC_EXACT; s.exactShadowQueue = w.exactShadowQueue; s.exactShadowCount = w.counts + QC_EXACT_SHADOW; s.exactCursor = w.counts + QC_EXACT_CURSOR;
    s.shadowOffset = 0.0f; s.mayTraceUndecidedRaysItself = false; s.rayCounts = rayCounts;
    launchTraceStep(c, s, wide);
}

// the launches of one chunk (n <= the arena's capacity), device pointers, on `stream`
static int launchQueryChunk(RtgpuContext* c, hipStream_t stream, uint32_t mode, const float4* rays, uint32_t n, float4* hits, float4* surfaces, uint32_t* occluded)
{
    RtgpuContext::Query& q = c->query;
    const WalkArena& w = q.arena;
    const bool closest = mode == RTGPU_TRACE_CLOSEST;
    const dim3 block(RT_BLOCK), grid((n + RT_BLOCK - 1u) / RT_BLOCK);
    HIP_TRY(hipMemsetAsync(w.counts, 0, QC_WORDS * sizeof(uint32_t), stream));
    hipLaunchKernelGGL(k_query_load, grid, block, 0, stream, rays, n, mode, w.paths, w.queue, w.counts + QC_QUEUE, w.counters);
    // Any-hit requests walk the reference's binary tree (k_trace) whatever the setting: the 4-wide walks' any-hit decision is exact for the rays the
    // integrators ask about (tmax = 0.999 x the light's distance: no triangle within an ulp of it), but a query's maxDistance may sit an ulp below a
    // hit, and there the conservative leaf gate of the 4-wide walks let 6 % of such rays report an occluder the reference's box test culls (DESIGN.md,
    // "Ray queries").
    launchArenaWalk(c, stream, w, closest, useWide(c) && closest, nullptr);
    hipLaunchKernelGGL(k_query_store, grid, block, 0, stream, c->sceneDev, rays, n, mode, w.paths, hits, occluded);
    if (surfaces) hipLaunchKernelGGL(k_query_evaluate, grid, block, 0, stream, c->sceneDev, rays, n, (const float4*)hits, surfaces, w.counters);
    HIP_TRY(hipGetLastError());
    return RTGPU_OK;
}

// argument rules shared by both entry points (count == 0 passes: the callers return at once)
static int checkQuery(RtgpuContext* c, uint32_t mode, const void* rays, uint32_t count, const void* hits, const void* surfaces, const void* occluded)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (mode != RTGPU_TRACE_CLOSEST && mode != RTGPU_TRACE_ANY) return fail(RTGPU_ERR_INVALID_ARGUMENT, "unknown ray query mode");
    if (mode == RTGPU_TRACE_ANY && (hits || surfaces)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "RTGPU_TRACE_ANY answers in `occluded` only: hits and surfaces must be NULL");
    if (mode == RTGPU_TRACE_CLOSEST && occluded) return fail(RTGPU_ERR_INVALID_ARGUMENT, "RTGPU_TRACE_CLOSEST answers in `hits` (and `surfaces`): occluded must be NULL");
    if (count == 0) return RTGPU_OK;
    if (!rays || (mode == RTGPU_TRACE_CLOSEST ? !hits : !occluded)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL ray or result buffer");
    if (!c->sceneReady) return fail(RTGPU_ERR_NOT_READY, "rtgpu_upload_scene has not been called");
    return RTGPU_OK;
}

// timing (rtgpu_enable_timing) measures the render passes: the query's launches stay out of the kernel classes
struct QueryUntimed
{
    RtgpuContext* c; bool was;
    explicit QueryUntimed(RtgpuContext* ctx) : c(ctx), was(ctx->timing) { c->timing = false; }
    ~QueryUntimed() { c->timing = was; }
};

RTGPU_API int rtgpu_trace_rays(RtgpuContext* c, uint32_t mode, const RtQueryRay* rays, uint32_t count, RtQueryHit* hits, RtQuerySurface* surfaces,
                               uint32_t* occluded, RtCounters* stats)
{
    int r = checkQuery(c, mode, rays, count, hits, surfaces, occluded); if (r) return r;
    if (count == 0) return RTGPU_OK;
    for (uint32_t i = 0; i < count; ++i)
    {
        const RtQueryRay& ray = rays[i];
        if (queryRayIsDegenerate(ray.origin[0], ray.origin[1], ray.origin[2], ray.maxDistance, ray.direction[0], ray.direction[1], ray.direction[2]))
            return fail(RTGPU_ERR_INVALID_ARGUMENT, "ray " + std::to_string(i) + " is degenerate (non-finite origin, zero or non-finite direction, or maxDistance not > 0)");
    }
    HIP_TRY(hipSetDevice(c->device));
    { int fr = vcmFlush(c); if (fr) return fr; }
    { int fr = flushPending(c); if (fr) return fr; }
    r = ensureQueryArena(c, count); if (r) return r;
    RtgpuContext::Query& q = c->query;
    const QueryUntimed untimed(c);
    hipStream_t stream = c->lanes[0].stream;
    HIP_TRY(hipStreamWaitEvent(stream, q.done, 0));
    HIP_TRY(hipMemsetAsync(q.arena.counters, 0, 16 * sizeof(unsigned long long), stream));
    const bool closest = mode == RTGPU_TRACE_CLOSEST;
    for (uint32_t first = 0; first < count; first += q.arena.paths.capacity)
    {
        const uint32_t n = count - first < q.arena.paths.capacity ? count - first : q.arena.paths.capacity;
        HIP_TRY(rtMemcpy(q.stagedRays, rays + first, (size_t)n * sizeof(RtQueryRay), hipMemcpyHostToDevice));
        r = launchQueryChunk(c, stream, mode, q.stagedRays, n, closest ? q.stagedHits : nullptr, surfaces ? q.stagedSurfaces : nullptr, closest ? nullptr : q.stagedOccluded);
        if (r) return r;
        HIP_TRY(hipStreamSynchronize(stream));
        if (closest) HIP_TRY(rtMemcpy(hits + first, q.stagedHits, (size_t)n * sizeof(RtQueryHit), hipMemcpyDeviceToHost));
        if (surfaces) HIP_TRY(rtMemcpy(surfaces + first, q.stagedSurfaces, (size_t)n * sizeof(RtQuerySurface), hipMemcpyDeviceToHost));
        if (!closest) HIP_TRY(rtMemcpy(occluded + first, q.stagedOccluded, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    HIP_TRY(hipEventRecord(q.done, stream));
    if (stats) HIP_TRY(rtMemcpy(stats, q.arena.counters, sizeof(RtCounters), hipMemcpyDeviceToHost));
    return RTGPU_OK;
}

RTGPU_API int rtgpu_trace_rays_async(RtgpuContext* c, uint32_t mode, const RtQueryRay* rays, uint32_t count, RtQueryHit* hits, RtQuerySurface* surfaces,
                                     uint32_t* occluded, RtCounters* stats, void* streamHandle)
{
    int r = checkQuery(c, mode, rays, count, hits, surfaces, occluded); if (r) return r;
    if (count == 0) return RTGPU_OK;
    if ((((uintptr_t)rays) | ((uintptr_t)hits) | ((uintptr_t)surfaces)) & 15u || ((uintptr_t)occluded & 3u) || ((uintptr_t)stats & 7u))
        return fail(RTGPU_ERR_INVALID_ARGUMENT, "rays, hits and surfaces must be 16-byte aligned device buffers (occluded 4, stats 8)");
    HIP_TRY(hipSetDevice(c->device));
    r = ensureQueryArena(c, count); if (r) return r;
    RtgpuContext::Query& q = c->query;
    const QueryUntimed untimed(c);
    hipStream_t stream = streamHandle ? (hipStream_t)streamHandle : c->lanes[0].stream;
    HIP_TRY(hipStreamWaitEvent(stream, q.done, 0));   // the arena is shared with the previous query, whatever its stream
    HIP_TRY(hipMemsetAsync(q.arena.counters, 0, 16 * sizeof(unsigned long long), stream));
    for (uint32_t first = 0; first < count; first += q.arena.paths.capacity)
    {
        const uint32_t n = count - first < q.arena.paths.capacity ? count - first : q.arena.paths.capacity;
        r = launchQueryChunk(c, stream, mode, (const float4*)(rays + first), n, hits ? (float4*)(hits + first) : nullptr, surfaces ? (float4*)(surfaces + first) : nullptr,
                             occluded ? occluded + first : nullptr);
        if (r) return r;
    }
    if (stats) HIP_TRY(hipMemcpyAsync(stats, q.arena.counters, sizeof(RtCounters), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipEventRecord(q.done, stream));
    return RTGPU_OK;
}
