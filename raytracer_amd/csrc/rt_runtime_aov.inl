// rt_runtime_aov.inl -- AOVs, host side.  Included by rt_runtime.hip.

// ---- AOVs (include/rtgpu.h, rtgpu_render_aovs; kernels: k_aov_pixels and k_aov_resolve, rt_aov.inl) -------------------------------------------
// A chunk of the frame's pixels, row-major, goes through k_aov_pixels -> k_generate -> a walk -> k_aov_resolve on the call's own arena.  The walk is the
// one the context renders with (the ray queries' pair: the 4-wide walk and its re-trace launch; launchArenaWalk), or -- when a cost plane is asked for -- the counting
// k_trace, the only walk that visits the reference's nodes in the reference's order, with TravTuning::rayCounts set.
static const uint32_t kAovChannels[RT_AOV_NUM_PLANES] = { 1, 3, 3, 3, 3, 2, 2, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1 };
#define RT_AOV_COST_PLANES ((1u << RT_AOV_BOX_TESTS) | (1u << RT_AOV_BOX_TESTS_PASSED) | (1u << RT_AOV_TRIANGLE_TESTS) | (1u << RT_AOV_TRIANGLE_TESTS_PASSED))
static const size_t kAovRingRecord = sizeof(DevPass) + (size_t)RTGPU_MAX_DIMENSIONS * sizeof(uint32_t);

static int ensureAovArena(RtgpuContext* c, uint32_t pixels, bool cost, size_t stagedWordsPerPixel)
{
    RtgpuContext::Aov& a = c->aov;
    WalkArena& w = a.arena;
    if (!a.done) HIP_TRY(hipEventCreateWithFlags(&a.done, hipEventDisableTiming));
    if (!w.counts) HIP_TRY(hipMalloc((void**)&w.counts, QC_WORDS * sizeof(uint32_t)));
    if (!w.counters) { HIP_TRY(hipMalloc((void**)&w.counters, 16 * sizeof(unsigned long long))); HIP_TRY(hipMemset(w.counters, 0, 16 * sizeof(unsigned long long))); }
    if (!a.passDev) HIP_TRY(hipMalloc((void**)&a.passDev, sizeof(DevPass)));
    if (!a.seedDev) HIP_TRY(hipMalloc((void**)&a.seedDev, (size_t)RTGPU_MAX_DIMENSIONS * sizeof(uint32_t)));
    if (!a.ringHost)
    {
        HIP_TRY(hipHostMalloc((void**)&a.ringHost, RtgpuContext::Aov::kRing * kAovRingRecord, hipHostMallocDefault));
        for (uint32_t i = 0; i < RtgpuContext::Aov::kRing; ++i) HIP_TRY(hipEventCreateWithFlags(&a.ringCopied[i], hipEventDisableTiming));
    }
    if (!w.paths.base || w.paths.capacity < pixels)
    {
        freeAovArena(c);   // (waits for the calls still using it)
        devFree(a.staged); a.stagedWords = 0;
        { const int r = growWalkArena(w, pixels); if (r) return r; }   // (`pixels` is a chunk at most)
        HIP_TRY(hipMalloc((void**)&a.slotPixel, (size_t)w.paths.capacity * sizeof(uint32_t)));
    }
    if (cost && !a.rayCounts) HIP_TRY(hipMalloc((void**)&a.rayCounts, (size_t)w.paths.capacity * sizeof(uint4)));
    const size_t stagedWords = stagedWordsPerPixel * w.paths.capacity;
    if (a.stagedWords < stagedWords)
    {
        if (a.done) HIP_TRY(hipEventSynchronize(a.done));
        devFree(a.staged); a.stagedWords = 0;
        HIP_TRY(hipMalloc((void**)&a.staged, stagedWords * sizeof(uint32_t)));
        a.stagedWords = stagedWords;
    }
    return RTGPU_OK;
}

// the launches of one chunk: pixels [firstPixel, firstPixel + n) of the frame (n <= the arena's capacity), on `stream`
static int launchAovChunk(RtgpuContext* c, hipStream_t stream, unsigned long long firstPixel, uint32_t n, uint32_t mask, const AovOutputs& out, size_t channelStride, size_t firstOut)
{
    RtgpuContext::Aov& a = c->aov;
    const WalkArena& w = a.arena;
    const bool cost = (mask & RT_AOV_COST_PLANES) != 0u;
    const dim3 block(RT_BLOCK), grid((n + RT_BLOCK - 1u) / RT_BLOCK);
    HIP_TRY(hipMemsetAsync(w.counts, 0, QC_WORDS * sizeof(uint32_t), stream));
    hipLaunchKernelGGL(k_aov_pixels, grid, block, 0, stream, a.slotPixel, n, firstPixel, c->width);
    // one pass, so a pass holds all `n` slots: slot / slotsPerPass = 0 for every slot
    launchGenerate(c, grid, stream, a.passDev, n, w.paths, a.slotPixel, n, w.queue, w.counts + QC_QUEUE, w.counters);   // (the camera's rays, or the ray source's)
    // a cost plane takes the counting binary walk; otherwise the walk the context renders with, as the ray queries take it (launchArenaWalk, rt_runtime_query.inl)
    launchArenaWalk(c, stream, w, true, useWide(c) && !cost, cost ? a.rayCounts : nullptr);
    const uint4* rayCounts = cost ? a.rayCounts : nullptr;
    if (c->leanScene == 1 || c->leanScene == 3) hipLaunchKernelGGL((k_aov_resolve<3>), grid, block, 0, stream, c->sceneDev, w.paths, n, mask, out, channelStride, firstOut, rayCounts);
    else hipLaunchKernelGGL((k_aov_resolve<0>), grid, block, 0, stream, c->sceneDev, w.paths, n, mask, out, channelStride, firstOut, rayCounts);
    HIP_TRY(hipGetLastError());
    return RTGPU_OK;
}

// argument rules shared by both entry points (numPlanes == 0 passes: the callers return at once); `mask`: bit = requested plane
static int checkAovs(RtgpuContext* c, const RtPassParams* p, const uint32_t* planes, uint32_t numPlanes, void* const* outputs, uint32_t& mask)
{
    mask = 0u;
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (numPlanes == 0) return RTGPU_OK;
    if (!p || !planes || !outputs) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    for (uint32_t k = 0; k < numPlanes; ++k)
    {
        if (planes[k] >= RT_AOV_NUM_PLANES) return fail(RTGPU_ERR_INVALID_ARGUMENT, "plane " + std::to_string(k) + ": unknown RtAovPlane " + std::to_string(planes[k]));
        if (mask & (1u << planes[k])) return fail(RTGPU_ERR_INVALID_ARGUMENT, "plane " + std::to_string(k) + ": RtAovPlane " + std::to_string(planes[k]) + " is requested twice");
        if (!outputs[k]) return fail(RTGPU_ERR_INVALID_ARGUMENT, "plane " + std::to_string(k) + ": NULL output buffer");
        mask |= 1u << planes[k];
    }
    return checkPass(c, p);
}

// the passes queued on the device the call answers on go out first -- with the context's timing as it is: they are passes, and their kernel times count
static int flushBeforeAovs(RtgpuContext* c)
{
    HIP_TRY(hipSetDevice(c->device));
    { int fr = vcmFlush(c); if (fr) return fr; }
    return flushPending(c);
}

// what both entry points do before their chunk loop: the arena fits, the pass's constants are on their way to the device (behind the previous call's
// last kernel, which still reads them).  `chunk`: the pixels of a chunk
static int beginAovs(RtgpuContext* c, const RtPassParams* p, hipStream_t stream, uint32_t mask, size_t stagedWordsPerPixel, uint32_t& chunk)
{
    const size_t pixels = (size_t)c->width * c->height;
    chunk = knobs::aovChunk();
    if (chunk > pixels) chunk = (uint32_t)pixels;
    int r = ensureAovArena(c, chunk, (mask & RT_AOV_COST_PLANES) != 0u, stagedWordsPerPixel); if (r) return r;
    RtgpuContext::Aov& a = c->aov;
    HIP_TRY(hipStreamWaitEvent(stream, a.done, 0));   // the arena is shared with the previous call, whatever its stream
    const uint32_t ring = a.ringCursor; a.ringCursor = (a.ringCursor + 1u) % RtgpuContext::Aov::kRing;
    HIP_TRY(hipEventSynchronize(a.ringCopied[ring]));   // (a fresh event is complete)
    char* record = a.ringHost + (size_t)ring * kAovRingRecord;
    DevPass pass;
    makeDevPass(c, p, pass);
    pass.seed = a.seedDev;
    memcpy(record, &pass, sizeof(pass));
    if (p->numDimensions) memcpy(record + sizeof(DevPass), p->seed, (size_t)p->numDimensions * sizeof(uint32_t));
    HIP_TRY(hipMemcpyAsync(a.passDev, record, sizeof(DevPass), hipMemcpyHostToDevice, stream));
    if (p->numDimensions) HIP_TRY(hipMemcpyAsync(a.seedDev, record + sizeof(DevPass), (size_t)p->numDimensions * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(a.ringCopied[ring], stream));
    return RTGPU_OK;
}

RTGPU_API int rtgpu_render_aovs(RtgpuContext* c, const RtPassParams* p, const uint32_t* planes, uint32_t numPlanes, void* const* outputs)
{
    uint32_t mask = 0u;
    int r = checkAovs(c, p, planes, numPlanes, outputs, mask); if (r) return r;
    if (numPlanes == 0) return RTGPU_OK;
    // a chunk's planes are staged channel-major on the device: channel `firstChannel[k] + ch` of the chunk at staged + that * capacity
    uint32_t firstChannel[RT_AOV_NUM_PLANES], channels = 0u;
    for (uint32_t k = 0; k < numPlanes; ++k) { firstChannel[k] = channels; channels += kAovChannels[planes[k]]; }
    r = flushBeforeAovs(c); if (r) return r;
    const QueryUntimed untimed(c);   // timing measures the render passes: the call's own launches stay out of the kernel classes
    hipStream_t stream = c->lanes[0].stream;
    uint32_t chunk = 0u;
    r = beginAovs(c, p, stream, mask, channels, chunk); if (r) return r;
    RtgpuContext::Aov& a = c->aov;
    const size_t pixels = (size_t)c->width * c->height, capacity = a.arena.paths.capacity;
    AovOutputs out;
    for (uint32_t id = 0; id < RT_AOV_NUM_PLANES; ++id) out.plane[id] = nullptr;
    for (uint32_t k = 0; k < numPlanes; ++k) out.plane[planes[k]] = a.staged + (size_t)firstChannel[k] * capacity;
    for (size_t first = 0; first < pixels; first += chunk)
    {
        const uint32_t n = pixels - first < chunk ? (uint32_t)(pixels - first) : chunk;
        r = launchAovChunk(c, stream, first, n, mask, out, capacity, 0u); if (r) return r;
        HIP_TRY(hipStreamSynchronize(stream));
        for (uint32_t k = 0; k < numPlanes; ++k)
            for (uint32_t ch = 0; ch < kAovChannels[planes[k]]; ++ch)
                HIP_TRY(rtMemcpy((uint32_t*)outputs[k] + (size_t)ch * pixels + first, a.staged + (size_t)(firstChannel[k] + ch) * capacity, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    HIP_TRY(hipEventRecord(a.done, stream));
    return RTGPU_OK;
}

RTGPU_API int rtgpu_render_aovs_async(RtgpuContext* c, const RtPassParams* p, const uint32_t* planes, uint32_t numPlanes, void* const* outputs, void* streamHandle)
{
    uint32_t mask = 0u;
    int r = checkAovs(c, p, planes, numPlanes, outputs, mask); if (r) return r;
    if (numPlanes == 0) return RTGPU_OK;
    for (uint32_t k = 0; k < numPlanes; ++k)
        if ((uintptr_t)outputs[k] & 15u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "plane " + std::to_string(k) + ": the output must be a 16-byte aligned device buffer");
    r = flushBeforeAovs(c); if (r) return r;
    const QueryUntimed untimed(c);
    hipStream_t stream = streamHandle ? (hipStream_t)streamHandle : c->lanes[0].stream;
    uint32_t chunk = 0u;
    r = beginAovs(c, p, stream, mask, 0u, chunk); if (r) return r;
    const size_t pixels = (size_t)c->width * c->height;
    AovOutputs out;
    for (uint32_t id = 0; id < RT_AOV_NUM_PLANES; ++id) out.plane[id] = nullptr;
    for (uint32_t k = 0; k < numPlanes; ++k) out.plane[planes[k]] = outputs[k];
    for (size_t first = 0; first < pixels; first += chunk)
    {
        const uint32_t n = pixels - first < chunk ? (uint32_t)(pixels - first) : chunk;
        r = launchAovChunk(c, stream, first, n, mask, out, pixels, first); if (r) return r;   // the planes are written in place
    }
    HIP_TRY(hipEventRecord(c->aov.done, stream));
    return RTGPU_OK;
}

// ---- guide chains (include/rtgpu.h, rtgpu_render_aovs_chain and rtgpu_render_aovs_virtual; kernels: k_shade_chain, rt_shade_body.inl, and k_aov_resolve_chain, rt_aov.inl) ----------------------
// The recorder's sequence (launchSlotBounces) over the chunking of the first-hit call: k_aov_pixels -> k_generate -> {trace with the walk the context renders with ->
// k_shade_chain} per bounce -> k_aov_resolve_chain, all on the call's stream with device-side queue counts.  The last bounce, min(maxChain, maxRayDepth), is traced
// and not shaded: every vertex at that depth stops, and a stop writes nothing.  So maxChain 0 launches what the first-hit call launches.
static const uint32_t kAovChainChannels[RT_AOV_VIRTUAL_NUM_PLANES - RT_AOV_NUM_PLANES] = { 1, 1, 3, 3 };   // RtAovChainPlane, then RtAovVirtualPlane
static uint32_t aovChainChannels(uint32_t plane) { return plane < RT_AOV_NUM_PLANES ? kAovChannels[plane] : kAovChainChannels[plane - RT_AOV_NUM_PLANES]; }

static int ensureChainArena(RtgpuContext* c, uint32_t pixels, uint32_t bounces, size_t stagedWordsPerPixel)
{
    RtgpuContext::Chain& a = c->chain;
    BatchLane& l = a.lane;
    if (!a.done) HIP_TRY(hipEventCreateWithFlags(&a.done, hipEventDisableTiming));
    if (!a.counters) { HIP_TRY(hipMalloc((void**)&a.counters, 16 * sizeof(unsigned long long))); HIP_TRY(hipMemset(a.counters, 0, 16 * sizeof(unsigned long long))); }
    if (!a.passDev) HIP_TRY(hipMalloc((void**)&a.passDev, sizeof(DevPass)));
    if (!a.seedDev) HIP_TRY(hipMalloc((void**)&a.seedDev, (size_t)RTGPU_MAX_DIMENSIONS * sizeof(uint32_t)));
    if (!a.ringHost)
    {
        HIP_TRY(hipHostMalloc((void**)&a.ringHost, RtgpuContext::Chain::kRing * kAovRingRecord, hipHostMallocDefault));
        for (uint32_t i = 0; i < RtgpuContext::Chain::kRing; ++i) HIP_TRY(hipEventCreateWithFlags(&a.ringCopied[i], hipEventDisableTiming));
    }
    if (!l.paths.base || l.paths.capacity < pixels)
    {
        freeChainArena(c);   // (waits for the calls still using it)
        devFree(a.staged); a.stagedWords = 0;
        uint32_t cap = 65536u;   // in powers of two from 64 K, as the first-hit call's arena (`pixels` is a chunk at most)
        while (cap < pixels) cap <<= 1;
        { const int r = allocLanePaths(l, cap, 1u); if (r) return r; }   // k_shade_chain writes no next-event request
        HIP_TRY(hipMalloc((void**)&a.slotPixel, (size_t)cap * sizeof(uint32_t)));
    }
    if (l.queueCountCapacity < bounces + 1u)
    {
        HIP_TRY(hipEventSynchronize(a.done));
        devFree(l.queueCounts);
        l.queueCountCapacity = bounces + 1u;
        HIP_TRY(hipMalloc((void**)&l.queueCounts, laneCountBytes(l)));
    }
    const size_t stagedWords = stagedWordsPerPixel * l.paths.capacity;
    if (a.stagedWords < stagedWords)
    {
        HIP_TRY(hipEventSynchronize(a.done));
        devFree(a.staged); a.stagedWords = 0;
        HIP_TRY(hipMalloc((void**)&a.staged, stagedWords * sizeof(uint32_t)));
        a.stagedWords = stagedWords;
    }
    return RTGPU_OK;
}

// the launches of one chunk: pixels [firstPixel, firstPixel + n) of the frame (n <= the arena's capacity), on `stream`; lastDepth = min(maxChain, maxRayDepth)
static int launchChainChunk(RtgpuContext* c, hipStream_t stream, unsigned long long firstPixel, uint32_t n, uint32_t maxChain, uint32_t lastDepth, uint32_t mask,
                            const AovChainOutputs& out, size_t channelStride, size_t firstOut)
{
    RtgpuContext::Chain& a = c->chain;
    BatchLane& l = a.lane;
    const LaneCounts counts(l);
    const dim3 block(RT_BLOCK), grid((n + RT_BLOCK - 1u) / RT_BLOCK);
    HIP_TRY(hipMemsetAsync(l.queueCounts, 0, laneCountBytes(l), stream));
    hipLaunchKernelGGL(k_aov_pixels, grid, block, 0, stream, a.slotPixel, n, firstPixel, c->width);
    // one pass, so a pass holds all `n` slots: slot / slotsPerPass = 0 for every slot
    launchGenerate(c, grid, stream, a.passDev, n, l.paths, a.slotPixel, n, l.queues[0], counts.pathCounts + 0, a.counters);
    launchSlotBounces(c, stream, a.counters, l, counts, lastDepth, lastDepth, false, [&](uint32_t depth)
    {
        if (depth == lastDepth) return;   // every vertex of the last bounce stops
        hipLaunchKernelGGL((k_shade_chain<false, false>), grid, block, 0, stream, c->sceneDev, a.passDev, n, l.paths, l.queues[depth & 1u], counts.pathCounts + depth,
                           l.queues[(depth + 1u) & 1u], counts.pathCounts + depth + 1, (uint32_t*)nullptr, (uint32_t*)nullptr, a.counters, maxChain);
    });
    if (c->leanScene == 1 || c->leanScene == 3) hipLaunchKernelGGL((k_aov_resolve_chain<3>), grid, block, 0, stream, c->sceneDev, l.paths, n, mask, out, channelStride, firstOut);
    else hipLaunchKernelGGL((k_aov_resolve_chain<0>), grid, block, 0, stream, c->sceneDev, l.paths, n, mask, out, channelStride, firstOut);
    HIP_TRY(hipGetLastError());
    return RTGPU_OK;
}

// argument rules shared by the entry points, in the order of checkAovs; `mask`: bit = requested plane (RtAovPlane, then RtAovChainPlane, then RtAovVirtualPlane);
// numKnown: RT_AOV_CHAIN_NUM_PLANES for the chain entries, RT_AOV_VIRTUAL_NUM_PLANES for rtgpu_render_aovs_virtual[_async]
static int checkAovsChain(RtgpuContext* c, const RtPassParams* p, const RtAovChain* chain, const uint32_t* planes, uint32_t numPlanes, void* const* outputs, uint32_t& mask,
                          uint32_t numKnown)
{
    mask = 0u;
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (!chain) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL chain");
    if (chain->maxChain > RT_AOV_CHAIN_MAX) return fail(RTGPU_ERR_INVALID_ARGUMENT, "maxChain must be 0..16");
    if (chain->flags != 0u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "RtAovChain::flags must be 0");
    if (numPlanes == 0) return RTGPU_OK;
    if (!p || !planes || !outputs) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    for (uint32_t k = 0; k < numPlanes; ++k)
    {
        if (planes[k] >= numKnown) return fail(RTGPU_ERR_INVALID_ARGUMENT, "plane " + std::to_string(k) + ": unknown plane " + std::to_string(planes[k]));
        if (planes[k] < RT_AOV_NUM_PLANES && ((1u << planes[k]) & RT_AOV_COST_PLANES))
            return fail(RTGPU_ERR_INVALID_ARGUMENT, "plane " + std::to_string(k) + ": the cost planes describe one traversal and have no chain form");
        if (mask & (1u << planes[k])) return fail(RTGPU_ERR_INVALID_ARGUMENT, "plane " + std::to_string(k) + ": plane " + std::to_string(planes[k]) + " is requested twice");
        if (!outputs[k]) return fail(RTGPU_ERR_INVALID_ARGUMENT, "plane " + std::to_string(k) + ": NULL output buffer");
        mask |= 1u << planes[k];
    }
    return checkPass(c, p);
}

// what both entry points do before their chunk loop (beginAovs' steps on the chain's own state)
static int beginAovsChain(RtgpuContext* c, const RtPassParams* p, hipStream_t stream, uint32_t lastDepth, size_t stagedWordsPerPixel, uint32_t& chunk)
{
    const size_t pixels = (size_t)c->width * c->height;
    chunk = knobs::aovChunk();
    if (chunk > pixels) chunk = (uint32_t)pixels;
    int r = ensureChainArena(c, chunk, lastDepth + 1u, stagedWordsPerPixel); if (r) return r;
    RtgpuContext::Chain& a = c->chain;
    HIP_TRY(hipStreamWaitEvent(stream, a.done, 0));   // the arena is shared with the previous call, whatever its stream
    const uint32_t ring = a.ringCursor; a.ringCursor = (a.ringCursor + 1u) % RtgpuContext::Chain::kRing;
    HIP_TRY(hipEventSynchronize(a.ringCopied[ring]));   // (a fresh event is complete)
    char* record = a.ringHost + (size_t)ring * kAovRingRecord;
    DevPass pass;
    makeDevPass(c, p, pass);
    pass.seed = a.seedDev;
    memcpy(record, &pass, sizeof(pass));
    if (p->numDimensions) memcpy(record + sizeof(DevPass), p->seed, (size_t)p->numDimensions * sizeof(uint32_t));
    HIP_TRY(hipMemcpyAsync(a.passDev, record, sizeof(DevPass), hipMemcpyHostToDevice, stream));
    if (p->numDimensions) HIP_TRY(hipMemcpyAsync(a.seedDev, record + sizeof(DevPass), (size_t)p->numDimensions * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(a.ringCopied[ring], stream));
    return RTGPU_OK;
}

// the host entries: rtgpu_render_aovs_chain and rtgpu_render_aovs_virtual, which knows one plane more
static int renderAovsChain(RtgpuContext* c, const RtPassParams* p, const RtAovChain* chain, const uint32_t* planes, uint32_t numPlanes, void* const* outputs, uint32_t numKnown)
{
    uint32_t mask = 0u;
    int r = checkAovsChain(c, p, chain, planes, numPlanes, outputs, mask, numKnown); if (r) return r;
    if (numPlanes == 0) return RTGPU_OK;
    uint32_t firstChannel[RT_AOV_VIRTUAL_NUM_PLANES], channels = 0u;
    for (uint32_t k = 0; k < numPlanes; ++k) { firstChannel[k] = channels; channels += aovChainChannels(planes[k]); }
    r = flushBeforeAovs(c); if (r) return r;
    const QueryUntimed untimed(c);   // timing measures the render passes
    hipStream_t stream = c->lanes[0].stream;
    const uint32_t lastDepth = chain->maxChain < p->maxRayDepth ? chain->maxChain : p->maxRayDepth;
    uint32_t chunk = 0u;
    r = beginAovsChain(c, p, stream, lastDepth, channels, chunk); if (r) return r;
    RtgpuContext::Chain& a = c->chain;
    const size_t pixels = (size_t)c->width * c->height, capacity = a.lane.paths.capacity;
    AovChainOutputs out;
    for (uint32_t id = 0; id < RT_AOV_VIRTUAL_NUM_PLANES; ++id) out.plane[id] = nullptr;
    for (uint32_t k = 0; k < numPlanes; ++k) out.plane[planes[k]] = a.staged + (size_t)firstChannel[k] * capacity;
    for (size_t first = 0; first < pixels; first += chunk)
    {
        const uint32_t n = pixels - first < chunk ? (uint32_t)(pixels - first) : chunk;
        r = launchChainChunk(c, stream, first, n, chain->maxChain, lastDepth, mask, out, capacity, 0u); if (r) return r;
        HIP_TRY(hipStreamSynchronize(stream));
        for (uint32_t k = 0; k < numPlanes; ++k)
            for (uint32_t ch = 0; ch < aovChainChannels(planes[k]); ++ch)
                HIP_TRY(rtMemcpy((uint32_t*)outputs[k] + (size_t)ch * pixels + first, a.staged + (size_t)(firstChannel[k] + ch) * capacity, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    HIP_TRY(hipEventRecord(a.done, stream));
    return RTGPU_OK;
}

RTGPU_API int rtgpu_render_aovs_chain(RtgpuContext* c, const RtPassParams* p, const RtAovChain* chain, const uint32_t* planes, uint32_t numPlanes, void* const* outputs)
{
    return renderAovsChain(c, p, chain, planes, numPlanes, outputs, RT_AOV_CHAIN_NUM_PLANES);
}

RTGPU_API int rtgpu_render_aovs_virtual(RtgpuContext* c, const RtPassParams* p, const RtAovChain* chain, const uint32_t* planes, uint32_t numPlanes, void* const* outputs)
{
    return renderAovsChain(c, p, chain, planes, numPlanes, outputs, RT_AOV_VIRTUAL_NUM_PLANES);
}

// the device entries
static int renderAovsChainAsync(RtgpuContext* c, const RtPassParams* p, const RtAovChain* chain, const uint32_t* planes, uint32_t numPlanes, void* const* outputs,
                                void* streamHandle, uint32_t numKnown)
{
    uint32_t mask = 0u;
    int r = checkAovsChain(c, p, chain, planes, numPlanes, outputs, mask, numKnown); if (r) return r;
    if (numPlanes == 0) return RTGPU_OK;
    for (uint32_t k = 0; k < numPlanes; ++k)
        if ((uintptr_t)outputs[k] & 15u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "plane " + std::to_string(k) + ": the output must be a 16-byte aligned device buffer");
    r = flushBeforeAovs(c); if (r) return r;
    const QueryUntimed untimed(c);
    hipStream_t stream = streamHandle ? (hipStream_t)streamHandle : c->lanes[0].stream;
    const uint32_t lastDepth = chain->maxChain < p->maxRayDepth ? chain->maxChain : p->maxRayDepth;
    uint32_t chunk = 0u;
    r = beginAovsChain(c, p, stream, lastDepth, 0u, chunk); if (r) return r;
    const size_t pixels = (size_t)c->width * c->height;
    AovChainOutputs out;
    for (uint32_t id = 0; id < RT_AOV_VIRTUAL_NUM_PLANES; ++id) out.plane[id] = nullptr;
    for (uint32_t k = 0; k < numPlanes; ++k) out.plane[planes[k]] = outputs[k];
    for (size_t first = 0; first < pixels; first += chunk)
    {
        const uint32_t n = pixels - first < chunk ? (uint32_t)(pixels - first) : chunk;
        r = launchChainChunk(c, stream, first, n, chain->maxChain, lastDepth, mask, out, pixels, first); if (r) return r;   // the planes are written in place
    }
    HIP_TRY(hipEventRecord(c->chain.done, stream));
    return RTGPU_OK;
}

RTGPU_API int rtgpu_render_aovs_chain_async(RtgpuContext* c, const RtPassParams* p, const RtAovChain* chain, const uint32_t* planes, uint32_t numPlanes, void* const* outputs,
                                            void* streamHandle)
{
    return renderAovsChainAsync(c, p, chain, planes, numPlanes, outputs, streamHandle, RT_AOV_CHAIN_NUM_PLANES);
}

RTGPU_API int rtgpu_render_aovs_virtual_async(RtgpuContext* c, const RtPassParams* p, const RtAovChain* chain, const uint32_t* planes, uint32_t numPlanes, void* const* outputs,
                                              void* streamHandle)
{
    return renderAovsChainAsync(c, p, chain, planes, numPlanes, outputs, streamHandle, RT_AOV_VIRTUAL_NUM_PLANES);
}

RTGPU_API int rtgpu_set_guide_chain(RtgpuContext* c, const RtAovChain* chain)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (chain && chain->maxChain > RT_AOV_CHAIN_MAX) return fail(RTGPU_ERR_INVALID_ARGUMENT, "maxChain must be 0..16");
    if (chain && chain->flags != 0u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "RtAovChain::flags must be 0");
    c->chain.guide = chain != nullptr;
    c->chain.guideMaxChain = chain ? chain->maxChain : 0u;
    return RTGPU_OK;
}
