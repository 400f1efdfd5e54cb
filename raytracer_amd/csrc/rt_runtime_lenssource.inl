// rt_runtime_lenssource.inl -- the lens source, host side.  Included by rt_runtime.hip behind rt_runtime_raysource.inl, whose life cycle it shares.

// ---- the lens source (include/rtgpu.h, rtgpu_set_lens_source; kernels: rt_lenssource.inl) --------------------------------------------------------
// While RtgpuContext::raySource.lensTable is set, launchGenerate and submitDenseBatch (rt_runtime_render.inl) take k_generate_lens / k_generate_dense_lens,
// and makeDevPass keeps the pass's sample offset and hands the kernels a zeroed camera with the source's lens, so that dense shading's camera re-run takes
// the draws the lens took.  Setting a table is raySourceBegin's sequence (queued passes out, every reader waited for), then the copy into lensIncoming,
// k_lens_source_check, and the swap -- after which a plain table, if one was the source, retires.

static int lensSourceParams(const RtLensSourceParams* params)
{
    if (!params) return fail(RTGPU_ERR_INVALID_ARGUMENT, "params is NULL");
    if (params->lens > 1u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "RtLensSourceParams::lens is 0 or 1");
    if (params->bokehShape > 2u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "bokeh shapes: 0 circle, 1 hexagon, 2 square");
    return RTGPU_OK;
}

static int lensSourceBuffers(RtgpuContext* c, size_t entries)
{
    RtgpuContext::RaySource& s = c->raySource;
    if (!s.degenerate) HIP_TRY(hipMalloc((void**)&s.degenerate, sizeof(uint32_t)));
    if (!s.lensIncoming) HIP_TRY(hipMalloc((void**)&s.lensIncoming, entries * sizeof(RtLensRay)));   // (dropped with the frame's size: it holds this frame's entries)
    return RTGPU_OK;
}

// k_lens_source_check over raySource.lensIncoming on `stream`, read back; then the swap, or the refusal that leaves the source as it was
static int lensSourceCheckAndSwap(RtgpuContext* c, uint32_t entries, const RtLensSourceParams& params, hipStream_t stream)
{
    RtgpuContext::RaySource& s = c->raySource;
    HIP_TRY(hipMemsetAsync(s.degenerate, 0, sizeof(uint32_t), stream));
    const uint32_t wanted = (entries + RT_BLOCK - 1u) / RT_BLOCK, most = 4u * c->numCUs;
    hipLaunchKernelGGL(k_lens_source_check, dim3(wanted < most ? wanted : most), dim3(RT_BLOCK), 0, stream, s.lensIncoming, entries, params.lens, s.degenerate);
    HIP_TRY(hipGetLastError());
    uint32_t refused = 0u;
    HIP_TRY(hipMemcpyAsync(&refused, s.degenerate, sizeof(refused), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (refused != 0u)
        return fail(RTGPU_ERR_INVALID_ARGUMENT, std::to_string(refused) + " entries of the lens table are refused (an interpreted word that is not finite, a degenerate stored ray" +
                                                (params.lens ? ", a focalDistance that is not > 0)" : ")"));
    float4* const previous = s.lensTable;
    s.lensTable = s.lensIncoming; s.lensIncoming = previous;
    s.lens = params.lens; s.bokehShape = params.bokehShape;
    raySourceRetire(s.table, s.incoming);   // one context holds one source: a ray source ends here
    return RTGPU_OK;
}

RTGPU_API int rtgpu_set_lens_source(RtgpuContext* c, const RtLensRay* rays, uint64_t count, const RtLensSourceParams* params)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (!rays) return fail(RTGPU_ERR_INVALID_ARGUMENT, "rays is NULL (rtgpu_set_ray_source(ctx, NULL, 0) clears a source of either kind)");
    { const int r = lensSourceParams(params); if (r) return r; }
    // every device renders its own tiles from its own copy of the whole table; a refusal comes from the first peer, before any source has changed
    RT_FAN_OUT(c, rtgpu_set_lens_source(peer, rays, count, params));
    bool clear = false;
    int r = raySourceBegin(c, rays, count, clear); if (r) return r;
    r = lensSourceBuffers(c, (size_t)count); if (r) return r;
    HIP_TRY(rtMemcpy(c->raySource.lensIncoming, rays, (size_t)count * sizeof(RtLensRay), hipMemcpyHostToDevice));
    return lensSourceCheckAndSwap(c, (uint32_t)count, *params, c->lanes[0].stream);
}

RTGPU_API int rtgpu_set_lens_source_device(RtgpuContext* c, const RtLensRay* rays, uint64_t count, const RtLensSourceParams* params, void* streamHandle)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (!rays) return fail(RTGPU_ERR_INVALID_ARGUMENT, "rays is NULL (rtgpu_set_ray_source(ctx, NULL, 0) clears a source of either kind)");
    { const int r = lensSourceParams(params); if (r) return r; }
    if (!c->peers.empty() || c->isPeer) return fail(RTGPU_ERR_UNSUPPORTED, "rtgpu_set_lens_source_device takes a table of one device: a multi-device context takes rtgpu_set_lens_source");
    bool clear = false;
    int r = raySourceBegin(c, rays, count, clear); if (r) return r;
    r = callerDeviceArray(c, rays, (size_t)count * sizeof(RtLensRay), 3u, "rays", "128 bytes per pixel"); if (r) return r;
    r = lensSourceBuffers(c, (size_t)count); if (r) return r;
    RtgpuContext::RaySource& s = c->raySource;
    // the copy goes behind the stream that made the table
    const hipStream_t stream = c->lanes[0].stream;
    if (streamHandle && (hipStream_t)streamHandle != stream)
    {
        if (!s.order) HIP_TRY(hipEventCreateWithFlags(&s.order, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(s.order, (hipStream_t)streamHandle));
        HIP_TRY(hipStreamWaitEvent(stream, s.order, 0));
    }
    HIP_TRY(hipMemcpyAsync(s.lensIncoming, rays, (size_t)count * sizeof(RtLensRay), hipMemcpyDeviceToDevice, stream));
    return lensSourceCheckAndSwap(c, (uint32_t)count, *params, stream);   // (synchronises: the caller may overwrite or free the table on return)
}

RTGPU_API int rtgpu_get_ray_source_kind(RtgpuContext* c, uint32_t* outKind)
{
    if (!c || !outKind) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    *outKind = c->raySource.lensTable ? 2u : (c->raySource.table ? 1u : 0u);
    return RTGPU_OK;
}

// ---- the exports: a pass's rays under the lens source (k_lens_source_rays), the camera as a lens table (k_camera_footprints) --------------------------
// the device copy both synchronous entries read back from
static int lensExportBuffer(RtgpuContext* c, size_t bytes)
{
    RtgpuContext::RaySource& s = c->raySource;
    if (s.lensExportedBytes >= bytes) return RTGPU_OK;
    devFree(s.lensExported); s.lensExportedBytes = 0;
    HIP_TRY(hipMalloc((void**)&s.lensExported, bytes));
    s.lensExportedBytes = bytes;
    return RTGPU_OK;
}

static int checkLensSourceRays(const RtgpuContext* c, const RtPassParams* p, const void* out)
{
    if (!c || !p || !out) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!c->sum) return fail(RTGPU_ERR_NOT_READY, "rtgpu_resize has not been called");
    if (!c->raySource.lensTable) return fail(RTGPU_ERR_NOT_READY, "no lens source is set (rtgpu_set_lens_source)");
    if (p->numDimensions > RTGPU_MAX_DIMENSIONS) return fail(RTGPU_ERR_INVALID_ARGUMENT, "numDimensions exceeds RTGPU_MAX_DIMENSIONS");
    if (p->numDimensions > 0 && !p->seed) return fail(RTGPU_ERR_INVALID_ARGUMENT, "seed is NULL");
    if (!(std::isfinite(p->sampleOffset[0]) && std::isfinite(p->sampleOffset[1]))) return fail(RTGPU_ERR_INVALID_ARGUMENT, "sampleOffset is not finite");
    // (the lens draws of a pass are dithered by the scene's blue noise: without the scene they would be other draws than the pass's)
    if (c->raySource.lens && p->useBlueNoise && !c->sceneReady) return fail(RTGPU_ERR_NOT_READY, "rtgpu_upload_scene has not been called (the lens draws take the scene's blue noise)");
    return RTGPU_OK;
}
static int launchLensSourceRays(RtgpuContext* c, const RtPassParams* p, float4* out, hipStream_t stream)
{
    RtgpuContext::RaySource& s = c->raySource;
    const uint32_t entries = c->width * c->height;
    const uint32_t wanted = (entries + RT_BLOCK - 1u) / RT_BLOCK, most = 16u * c->numCUs;
    // the pass's sampler by value: the lens draws are its first two, so two words of the seed array are all the kernel can read
    const uint32_t numDims = p->numDimensions < 2u ? p->numDimensions : 2u;
    const uint32_t seed0 = numDims > 0u ? p->seed[0] : 0u, seed1 = numDims > 1u ? p->seed[1] : 0u;
    const uint32_t blueNoiseLayers = (c->sceneDev.blueNoise && p->useBlueNoise) ? 4u : 0u;   // (as makeDevPass)
    hipLaunchKernelGGL(k_lens_source_rays, dim3(wanted < most ? wanted : most), dim3(RT_BLOCK), 0, stream, s.lensTable, c->width, c->height, p->sampleOffset[0], p->sampleOffset[1],
                       s.lens, s.bokehShape, seed0, seed1, numDims, blueNoiseLayers, c->sceneDev.blueNoise, (unsigned long long)p->rngKey[0], (unsigned long long)p->rngKey[1], out);
    HIP_TRY(hipGetLastError());
    if (stream != c->lanes[0].stream)   // a set call, a resize or the context's end waits for this reader of the table (waitLensExport)
    {
        if (!s.lensRead) HIP_TRY(hipEventCreateWithFlags(&s.lensRead, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(s.lensRead, stream));
    }
    return RTGPU_OK;
}

RTGPU_API int rtgpu_read_lens_source_rays(RtgpuContext* c, const RtPassParams* p, RtPrimaryRay* out)
{
    int r = checkLensSourceRays(c, p, out); if (r) return r;
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t)c->width * c->height * sizeof(RtPrimaryRay);
    r = lensExportBuffer(c, bytes); if (r) return r;
    const hipStream_t stream = c->lanes[0].stream;
    r = launchLensSourceRays(c, p, c->raySource.lensExported, stream); if (r) return r;
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(rtMemcpy(out, c->raySource.lensExported, bytes, hipMemcpyDeviceToHost));
    return RTGPU_OK;
}

RTGPU_API int rtgpu_read_lens_source_rays_async(RtgpuContext* c, const RtPassParams* p, RtPrimaryRay* out, void* streamHandle)
{
    int r = checkLensSourceRays(c, p, out); if (r) return r;
    HIP_TRY(hipSetDevice(c->device));
    r = callerDeviceArray(c, out, (size_t)c->width * c->height * sizeof(RtPrimaryRay), 15u, "out", "32 bytes per pixel"); if (r) return r;
    return launchLensSourceRays(c, p, reinterpret_cast<float4*>(out), streamHandle ? (hipStream_t)streamHandle : c->lanes[0].stream);
}

static int checkCameraFootprints(const RtgpuContext* c, const RtPassParams* p, const void* out)
{
    if (!c || !p || !out) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!c->sum) return fail(RTGPU_ERR_NOT_READY, "rtgpu_resize has not been called");
    if ((uint64_t)c->width * c->height > 0x7FFFFFFFull) return fail(RTGPU_ERR_UNSUPPORTED, "a lens source holds fewer than 2^31 entries");
    if (p->camera.barrelDistortionVariableFactor != 0.0f)
        return fail(RTGPU_ERR_UNSUPPORTED, "a camera with a variable barrel factor draws its distortion per pixel and pass: a lens table cannot carry that draw");
    return RTGPU_OK;
}
static int launchCameraFootprints(RtgpuContext* c, const RtPassParams* p, float4* out, hipStream_t stream)
{
    const uint32_t entries = c->width * c->height;
    const uint32_t wanted = (entries + RT_BLOCK - 1u) / RT_BLOCK, most = 16u * c->numCUs;
    RtCamera pinhole = p->camera;
    pinhole.dofEnable = 0u;   // the stored ray is the pinhole's: the lens is the table's to apply (aperture and focalDistance travel in the entry)
    hipLaunchKernelGGL(k_camera_footprints, dim3(wanted < most ? wanted : most), dim3(RT_BLOCK), 0, stream, pinhole, p->sampleOffset[0], p->sampleOffset[1], c->width, c->height, out);
    HIP_TRY(hipGetLastError());
    return RTGPU_OK;
}

RTGPU_API int rtgpu_read_camera_footprints(RtgpuContext* c, const RtPassParams* p, RtLensRay* out)
{
    int r = checkCameraFootprints(c, p, out); if (r) return r;
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t)c->width * c->height * sizeof(RtLensRay);
    r = lensExportBuffer(c, bytes); if (r) return r;
    const hipStream_t stream = c->lanes[0].stream;
    r = launchCameraFootprints(c, p, c->raySource.lensExported, stream); if (r) return r;
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(rtMemcpy(out, c->raySource.lensExported, bytes, hipMemcpyDeviceToHost));
    return RTGPU_OK;
}

RTGPU_API int rtgpu_read_camera_footprints_async(RtgpuContext* c, const RtPassParams* p, RtLensRay* out, void* streamHandle)
{
    int r = checkCameraFootprints(c, p, out); if (r) return r;
    HIP_TRY(hipSetDevice(c->device));
    r = callerDeviceArray(c, out, (size_t)c->width * c->height * sizeof(RtLensRay), 15u, "out", "128 bytes per pixel"); if (r) return r;
    return launchCameraFootprints(c, p, reinterpret_cast<float4*>(out), streamHandle ? (hipStream_t)streamHandle : c->lanes[0].stream);
}
