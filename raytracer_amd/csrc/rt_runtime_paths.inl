// rt_runtime_paths.inl -- path records, host side.  Included by rt_runtime.hip.

// ---- path records (include/rtgpu.h, rtgpu_record_paths; kernels: k_shade_record and k_paths_finish, rt_shade.inl) --------------------------------
// The reference's PathDebugData hook.  A pixel's path depends on the pass and the pixel alone (per-pass seeds, a generator keyed by (rngKey, x, y)), so
// a recording is the slot-per-pixel pipeline (submitSlotBatch) over a slot -> pixel table of the caller's pixels: k_generate -> {trace -> k_shade_record}
// per bounce -> a last trace for the final next-event rays -> k_paths_finish.  Arena, queues, work counts, counters and pass constants are the recorder's own.
#define RT_RECORD_CHUNK (1u << 20)                    // slots per chunk at most ...
#define RT_RECORD_CHUNK_BYTES ((size_t)256 << 20)     // ... and as many as keep a chunk's records below this

static int ensureRecorder(RtgpuContext* c, uint32_t slots, uint32_t maxLights, uint32_t maxDepth, uint32_t recordStride)
{
    RtgpuContext::Recorder& rec = c->recorder;
    BatchLane& l = rec.lane;
    if (!rec.counters) HIP_TRY(hipMalloc((void**)&rec.counters, 16 * sizeof(unsigned long long)));
    if (!rec.passDev) HIP_TRY(hipMalloc((void**)&rec.passDev, sizeof(DevPass)));
    if (!rec.seedDev) HIP_TRY(hipMalloc((void**)&rec.seedDev, (size_t)RTGPU_MAX_DIMENSIONS * sizeof(uint32_t)));
    if (!l.paths.base || l.paths.capacity < slots || l.paths.maxLights < maxLights)
    {
        // grown in powers of two from 1 K slots, as the query arena is: a caller whose pixel lists grow slowly does not reallocate with every call
        uint32_t cap = 1024u;
        while (cap < slots) cap <<= 1;
        if (cap < l.paths.capacity) cap = l.paths.capacity;
        freePaths(l);
        devFree(rec.slotPixel, rec.infos);
        { const int r = allocLanePaths(l, cap, maxLights); if (r) return r; }
        HIP_TRY(hipMalloc((void**)&rec.slotPixel, (size_t)cap * sizeof(uint32_t)));
        HIP_TRY(hipMalloc((void**)&rec.infos, (size_t)cap * 2u * sizeof(float4)));
    }
    if (rec.recordCapacity < (size_t)slots * recordStride)
    {
        devFree(rec.records);
        rec.recordCapacity = 0;
        HIP_TRY(hipMalloc((void**)&rec.records, (size_t)slots * recordStride * sizeof(float4)));
        rec.recordCapacity = (size_t)slots * recordStride;
    }
    if (l.queueCountCapacity < maxDepth + 2u)
    {
        devFree(l.queueCounts);
        l.queueCountCapacity = maxDepth + 2u;
        HIP_TRY(hipMalloc((void**)&l.queueCounts, laneCountBytes(l)));
    }
    return RTGPU_OK;
}

// the launches of one chunk of `n` slots (rec.slotPixel holds their pixels), on `stream`: submitSlotBatch's bounces (launchSlotBounces) with the recording shade kernel
static int launchRecordChunk(RtgpuContext* c, hipStream_t stream, uint32_t n, uint32_t maxRayDepth, uint32_t recordStride)
{
    RtgpuContext::Recorder& rec = c->recorder;
    BatchLane& l = rec.lane;
    const LaneCounts counts(l);
    const dim3 block(RT_BLOCK), grid((n + RT_BLOCK - 1u) / RT_BLOCK);
    HIP_TRY(hipMemsetAsync(l.queueCounts, 0, laneCountBytes(l), stream));
    // one pass, so a pass holds all `n` slots: slot / slotsPerPass = 0 for every slot
    launchGenerate(c, grid, stream, rec.passDev, n, l.paths, rec.slotPixel, n, l.queues[0], counts.pathCounts + 0, rec.counters);   // (the camera's rays, or the ray source's)
    launchSlotBounces(c, stream, rec.counters, l, counts, maxRayDepth, maxRayDepth + 1u, c->numLights != 0, [&](uint32_t depth)
    {
        hipLaunchKernelGGL((k_shade_record<false, false>), grid, block, 0, stream, c->sceneDev, rec.passDev, n, l.paths, l.queues[depth & 1u], counts.pathCounts + depth,
                           l.queues[(depth + 1u) & 1u], counts.pathCounts + depth + 1, l.shadowQueues[depth & 1u], counts.shadowCounts + depth, rec.counters, rec.records, recordStride);
    });
    hipLaunchKernelGGL(k_paths_finish, grid, block, 0, stream, l.paths, n, rec.passDev, rec.records, recordStride, rec.infos, rec.counters);
    HIP_TRY(hipGetLastError());
    return RTGPU_OK;
}

RTGPU_API int rtgpu_record_paths(RtgpuContext* c, const RtPassParams* p, const uint32_t* pixelsXY, uint32_t numPixels, uint32_t maxVertices, RtPathVertex* vertices,
                                 RtPathInfo* infos)
{
    if (!c || !p) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    if (maxVertices == 0) return fail(RTGPU_ERR_INVALID_ARGUMENT, "maxVertices must be > 0");
    if (numPixels == 0) return RTGPU_OK;
    if (!pixelsXY || !vertices || !infos) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL pixel or result buffer");
    { const int r = checkPass(c, p); if (r) return r; }
    if (c->vcm.enabled || c->plainPathTracer || c->lightTracer || c->debugMode >= 0)
        return fail(RTGPU_ERR_UNSUPPORTED, "path records exist for RT_INTEGRATOR_PATH_TRACER_MIS only (the reference hooks PathDebugData into that renderer alone)");
    for (uint32_t i = 0; i < numPixels; ++i)
        if (pixelsXY[2u * i] >= c->width || pixelsXY[2u * i + 1u] >= c->height)
            return fail(RTGPU_ERR_INVALID_ARGUMENT, "pixel " + std::to_string(i) + " lies outside the frame");
    HIP_TRY(hipSetDevice(c->device));
    { int fr = vcmFlush(c); if (fr) return fr; }
    { int fr = flushPending(c); if (fr) return fr; }

    // a path has at most maxRayDepth + 1 vertices: the device buffer holds no more than that per slot, whatever the caller's capacity
    const uint32_t stored = maxVertices < p->maxRayDepth + 1u ? maxVertices : p->maxRayDepth + 1u;
    const uint32_t recordStride = 7u * stored + 1u;
    const uint32_t maxLights = p->lightSamplingStrategy == RT_LIGHT_SAMPLING_ALL && c->numLights ? c->numLights : 1u;
    size_t chunk = RT_RECORD_CHUNK_BYTES / ((size_t)recordStride * sizeof(float4));
    if (chunk > RT_RECORD_CHUNK) chunk = RT_RECORD_CHUNK;
    if (chunk > numPixels) chunk = numPixels;
    int r = ensureRecorder(c, (uint32_t)chunk, maxLights, p->maxRayDepth, recordStride); if (r) return r;
    RtgpuContext::Recorder& rec = c->recorder;
    const QueryUntimed untimed(c);   // timing measures the render passes
    hipStream_t stream = c->lanes[0].stream;

    DevPass pass;
    makeDevPass(c, p, pass);
    pass.seed = rec.seedDev;
    HIP_TRY(rtMemcpy(rec.seedDev, p->seed, (size_t)p->numDimensions * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(rtMemcpy(rec.passDev, &pass, sizeof(pass), hipMemcpyHostToDevice));

    std::vector<uint32_t> slotPixel(chunk);
    std::vector<float4> records(chunk * recordStride);
    std::vector<RtPathInfo> chunkInfos(chunk);
    for (uint32_t first = 0; first < numPixels; first += (uint32_t)chunk)
    {
        const uint32_t n = numPixels - first < chunk ? numPixels - first : (uint32_t)chunk;
        for (uint32_t i = 0; i < n; ++i) slotPixel[i] = pixelsXY[2u * (first + i)] | (pixelsXY[2u * (first + i) + 1u] << 16);   // (the film row flips in k_generate)
        HIP_TRY(rtMemcpy(rec.slotPixel, slotPixel.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
        r = launchRecordChunk(c, stream, n, p->maxRayDepth, recordStride); if (r) return r;
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(rtMemcpy(records.data(), rec.records, (size_t)n * recordStride * sizeof(float4), hipMemcpyDeviceToHost));
        HIP_TRY(rtMemcpy(chunkInfos.data(), rec.infos, (size_t)n * sizeof(RtPathInfo), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n; ++i)
        {
            // only the records the path has are written: the rest of the pixel's `maxVertices` stay as the caller left them
            const uint32_t have = chunkInfos[i].numVertices < stored ? chunkInfos[i].numVertices : stored;
            memcpy(vertices + (size_t)(first + i) * maxVertices, records.data() + (size_t)i * recordStride, (size_t)have * sizeof(RtPathVertex));
            infos[first + i] = chunkInfos[i];
        }
    }
    return RTGPU_OK;
}
