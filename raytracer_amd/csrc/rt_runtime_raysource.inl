// rt_runtime_raysource.inl -- the primary-ray sources, host side.  Included by rt_runtime.hip.

// ---- the sources (include/rtgpu.h: rtgpu_set_ray_source, rtgpu_set_lens_source; kernels: rt_raysource.inl) -----------------------------------------------
// RtgpuContext::raySource.kind says where a pass's primary rays come from: 0 the camera, 1 a table of finished rays (RtPrimaryRay), 2 a table of lens rays
// (RtLensRay: footprints, jitter, a thin lens).  Under kind 1 and 2 every launch site of k_generate / k_generate_dense takes its table-fed counterpart
// (launchGenerate and submitDenseBatch, rt_runtime_render.inl; the AOV calls and the recorder through launchGenerate) and makeDevPass hands the kernels a
// zeroed camera: one that draws nothing under a plain table, one with the source's lens under a lens table, so that dense shading's camera re-run takes the
// draws the lens took.  Nothing else of a pass changes.  Setting a table of either kind is setSource: queued passes go out first, everything that could read
// the old table is waited for, the new one is copied into the context's second buffer, the kind's check kernel reads it once, and only a table it does not
// refuse changes places with the old one.

static dim3 sourceGrid(const RtgpuContext* c, uint32_t entries, uint32_t blocksPerCU)
{
    const uint32_t wanted = (entries + RT_BLOCK - 1u) / RT_BLOCK, most = blocksPerCU * c->numCUs;
    return dim3(wanted < most ? wanted : most);
}
static size_t sourceEntryBytes(uint32_t kind) { return kind == 2u ? sizeof(RtLensRay) : sizeof(RtPrimaryRay); }
static const char* sourceEntryUnit(size_t entryBytes) { return entryBytes == sizeof(RtLensRay) ? "128 bytes per pixel" : "32 bytes per pixel"; }

// `capacity` bytes at least in `buffer`, which holds nothing that is still needed
static int sourceBuffer(float4*& buffer, size_t& capacity, size_t bytes)
{
    if (capacity >= bytes) return RTGPU_OK;
    devFree(buffer); capacity = 0;
    HIP_TRY(hipMalloc((void**)&buffer, bytes));
    capacity = bytes;
    return RTGPU_OK;
}

// what every set entry checks and waits for before the copy; `clear`: the call clears the source and is done
static int raySourceBegin(RtgpuContext* c, const void* rays, uint64_t count, bool& clear)
{
    clear = false;
    if (!rays && count != 0u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "rays is NULL");
    if (rays && !c->sum) return fail(RTGPU_ERR_NOT_READY, "rtgpu_resize has not been called");
    if (rays && count != (uint64_t)c->width * c->height) return fail(RTGPU_ERR_INVALID_ARGUMENT, "a ray source has width * height entries");
    if (count > 0x7FFFFFFFull) return fail(RTGPU_ERR_UNSUPPORTED, "a ray source holds fewer than 2^31 entries");
    HIP_TRY(hipSetDevice(c->device));
    { int fr = flushQueued(c); if (fr) return fr; }   // the queued passes render the source they were queued under
    HIP_TRY(syncLanes(c));
    waitQueries(c);                                   // (AOV calls on a caller's stream read the table too)
    waitLensExport(c);                                // (and rtgpu_read_lens_source_rays_async reads a lens table)
    beamInvalidate(c);                                // (beam lists are the camera's: a source of either kind renders without them, and the camera after it builds anew)
    if (!rays) { dropRaySource(c); clear = true; }
    return RTGPU_OK;
}

// The four set entries behind their own argument checks: a table of `kind` (1 plain, 2 lens with `params`) in host memory, or -- `onDevice` -- in memory of the
// context's device, made on `streamHandle`.  A refused table leaves the source of whatever kind as it was; a caller who sets a table per pass (anti-aliasing)
// allocates twice, not per call.  Returns synchronised: the caller may overwrite or free the table.
static int setSource(RtgpuContext* c, uint32_t kind, const void* rays, uint64_t count, const RtLensSourceParams* params, bool onDevice, void* streamHandle)
{
    RtgpuContext::RaySource& s = c->raySource;
    const size_t bytes = (size_t)count * sourceEntryBytes(kind);
    bool clear = false;
    int r = raySourceBegin(c, rays, count, clear); if (r || clear) return r;
    if (onDevice) { r = callerDeviceArray(c, rays, bytes, 3u, "rays", sourceEntryUnit(sourceEntryBytes(kind))); if (r) return r; }
    if (!s.degenerate) HIP_TRY(hipMalloc((void**)&s.degenerate, sizeof(uint32_t)));
    r = sourceBuffer(s.incoming, s.incomingBytes, bytes); if (r) return r;   // (a refused table of before may lie there: nothing reads it)
    const hipStream_t stream = c->lanes[0].stream;
    if (!onDevice) HIP_TRY(rtMemcpy(s.incoming, rays, bytes, hipMemcpyHostToDevice));
    else
    {
        // the copy goes behind the stream that made the table
        if (streamHandle && (hipStream_t)streamHandle != stream)
        {
            if (!s.order) HIP_TRY(hipEventCreateWithFlags(&s.order, hipEventDisableTiming));
            HIP_TRY(hipEventRecord(s.order, (hipStream_t)streamHandle));
            HIP_TRY(hipStreamWaitEvent(stream, s.order, 0));
        }
        HIP_TRY(hipMemcpyAsync(s.incoming, rays, bytes, hipMemcpyDeviceToDevice, stream));
    }
    // the kind's check over `incoming`, read back (a block ends in one atomic on the same word: four blocks per CU, and the loop strides)
    HIP_TRY(hipMemsetAsync(s.degenerate, 0, sizeof(uint32_t), stream));
    const dim3 grid = sourceGrid(c, (uint32_t)count, 4u);
    if (kind == 2u) hipLaunchKernelGGL(k_lens_source_check, grid, dim3(RT_BLOCK), 0, stream, s.incoming, (uint32_t)count, params->lens, s.degenerate);
    else hipLaunchKernelGGL(k_ray_source_check, grid, dim3(RT_BLOCK), 0, stream, s.incoming, (uint32_t)count, s.degenerate);
    HIP_TRY(hipGetLastError());
    uint32_t refused = 0u;
    HIP_TRY(hipMemcpyAsync(&refused, s.degenerate, sizeof(refused), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (refused != 0u && kind == 2u)
        return fail(RTGPU_ERR_INVALID_ARGUMENT, std::to_string(refused) + " entries of the lens table are refused (an interpreted word that is not finite, a degenerate stored ray" +
                                                (params->lens ? ", a focalDistance that is not > 0)" : ")"));
    if (refused != 0u)
        return fail(RTGPU_ERR_INVALID_ARGUMENT, std::to_string(refused) + " entries of the table are degenerate rays (an origin or direction word that is not finite, a zero direction)");
    // the swap: one context holds one source, so a source of the other kind ends here and its table is the next call's `incoming`
    std::swap(s.table, s.incoming); std::swap(s.tableBytes, s.incomingBytes);
    s.kind = kind;
    if (kind == 2u) { s.lens = params->lens; s.bokehShape = params->bokehShape; }
    return RTGPU_OK;
}

RTGPU_API int rtgpu_set_ray_source(RtgpuContext* c, const RtPrimaryRay* rays, uint64_t count)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    // every device renders its own tiles from its own copy of the whole table; a refusal comes from the first peer, before any source has changed
    // (all of them check the same values)
    RT_FAN_OUT(c, rtgpu_set_ray_source(peer, rays, count));
    return setSource(c, 1u, rays, count, nullptr, false, nullptr);
}

RTGPU_API int rtgpu_set_ray_source_device(RtgpuContext* c, const RtPrimaryRay* rays, uint64_t count, void* streamHandle)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (!c->peers.empty() || c->isPeer) return fail(RTGPU_ERR_UNSUPPORTED, "rtgpu_set_ray_source_device takes a table of one device: a multi-device context takes rtgpu_set_ray_source");
    return setSource(c, 1u, rays, count, nullptr, true, streamHandle);
}

// what both lens entries refuse before anything else
static int lensSourceArguments(const RtgpuContext* c, const void* rays, const RtLensSourceParams* params)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (!rays) return fail(RTGPU_ERR_INVALID_ARGUMENT, "rays is NULL (rtgpu_set_ray_source(ctx, NULL, 0) clears a source of either kind)");
    if (!params) return fail(RTGPU_ERR_INVALID_ARGUMENT, "params is NULL");
    if (params->lens > 1u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "RtLensSourceParams::lens is 0 or 1");
    if (params->bokehShape > 2u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "bokeh shapes: 0 circle, 1 hexagon, 2 square");
    return RTGPU_OK;
}

RTGPU_API int rtgpu_set_lens_source(RtgpuContext* c, const RtLensRay* rays, uint64_t count, const RtLensSourceParams* params)
{
    { const int r = lensSourceArguments(c, rays, params); if (r) return r; }
    RT_FAN_OUT(c, rtgpu_set_lens_source(peer, rays, count, params));   // (as rtgpu_set_ray_source)
    return setSource(c, 2u, rays, count, params, false, nullptr);
}

RTGPU_API int rtgpu_set_lens_source_device(RtgpuContext* c, const RtLensRay* rays, uint64_t count, const RtLensSourceParams* params, void* streamHandle)
{
    { const int r = lensSourceArguments(c, rays, params); if (r) return r; }
    if (!c->peers.empty() || c->isPeer) return fail(RTGPU_ERR_UNSUPPORTED, "rtgpu_set_lens_source_device takes a table of one device: a multi-device context takes rtgpu_set_lens_source");
    return setSource(c, 2u, rays, count, params, true, streamHandle);
}

RTGPU_API int rtgpu_get_ray_source(RtgpuContext* c, uint64_t* outCount)
{
    if (!c || !outCount) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    *outCount = c->raySource.any() ? (uint64_t)c->width * c->height : 0u;   // (a source of either kind: rtgpu_get_ray_source_kind tells them apart)
    return RTGPU_OK;
}

RTGPU_API int rtgpu_get_ray_source_kind(RtgpuContext* c, uint32_t* outKind)
{
    if (!c || !outKind) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    *outKind = c->raySource.kind;
    return RTGPU_OK;
}

// ---- the exports: the camera's rays in the plain table's layout (rtgpu_read_camera_rays; k_camera_rays), a pass's rays under the lens source
// (rtgpu_read_lens_source_rays; k_lens_source_rays), the camera as a lens table (rtgpu_read_camera_footprints; k_camera_footprints) -------------------------
// An export is its check and its launch of width * height entries into `out` on `stream`; exportToHost and exportToDevice are the two ways out.
typedef int (*ExportLaunch)(RtgpuContext* c, const RtPassParams* p, float4* out, hipStream_t stream);

// the synchronous entries: into the context's device copy on lane 0, then to the caller's host memory
static int exportToHost(RtgpuContext* c, const RtPassParams* p, void* out, size_t entryBytes, ExportLaunch launch)
{
    HIP_TRY(hipSetDevice(c->device));
    RtgpuContext::RaySource& s = c->raySource;
    const size_t bytes = (size_t)c->width * c->height * entryBytes;
    int r = sourceBuffer(s.exported, s.exportedBytes, bytes); if (r) return r;
    const hipStream_t stream = c->lanes[0].stream;
    r = launch(c, p, s.exported, stream); if (r) return r;
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(rtMemcpy(out, s.exported, bytes, hipMemcpyDeviceToHost));
    return RTGPU_OK;
}
// the _async entries: into the caller's device array on the caller's stream
static int exportToDevice(RtgpuContext* c, const RtPassParams* p, void* out, size_t entryBytes, ExportLaunch launch, void* streamHandle)
{
    HIP_TRY(hipSetDevice(c->device));
    const int r = callerDeviceArray(c, out, (size_t)c->width * c->height * entryBytes, 15u, "out", sourceEntryUnit(entryBytes)); if (r) return r;
    return launch(c, p, reinterpret_cast<float4*>(out), streamHandle ? (hipStream_t)streamHandle : c->lanes[0].stream);
}

static int checkCameraRays(const RtgpuContext* c, const RtPassParams* p, const void* out)
{
    if (!c || !p || !out) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!c->sum) return fail(RTGPU_ERR_NOT_READY, "rtgpu_resize has not been called");
    if ((uint64_t)c->width * c->height > 0x7FFFFFFFull) return fail(RTGPU_ERR_UNSUPPORTED, "a ray source holds fewer than 2^31 entries");
    if (p->camera.dofEnable || p->camera.barrelDistortionVariableFactor != 0.0f)
        return fail(RTGPU_ERR_UNSUPPORTED, "a camera that draws from the sampler (depth of field, the variable barrel factor) has no table: a table cannot carry the draws");
    return RTGPU_OK;
}
static int launchCameraRays(RtgpuContext* c, const RtPassParams* p, float4* out, hipStream_t stream)
{
    hipLaunchKernelGGL(k_camera_rays, sourceGrid(c, c->width * c->height, 16u), dim3(RT_BLOCK), 0, stream, p->camera, p->sampleOffset[0], p->sampleOffset[1], c->width, c->height, out);
    HIP_TRY(hipGetLastError());
    return RTGPU_OK;
}

static int checkLensSourceRays(const RtgpuContext* c, const RtPassParams* p, const void* out)
{
    if (!c || !p || !out) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!c->sum) return fail(RTGPU_ERR_NOT_READY, "rtgpu_resize has not been called");
    if (c->raySource.kind != 2u) return fail(RTGPU_ERR_NOT_READY, "no lens source is set (rtgpu_set_lens_source)");
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
    // the pass's sampler by value: the lens draws are its first two, so two words of the seed array are all the kernel can read
    const uint32_t numDims = p->numDimensions < 2u ? p->numDimensions : 2u;
    const uint32_t seed0 = numDims > 0u ? p->seed[0] : 0u, seed1 = numDims > 1u ? p->seed[1] : 0u;
    const uint32_t blueNoiseLayers = (c->sceneDev.blueNoise && p->useBlueNoise) ? 4u : 0u;   // (as makeDevPass)
    hipLaunchKernelGGL(k_lens_source_rays, sourceGrid(c, c->width * c->height, 16u), dim3(RT_BLOCK), 0, stream, s.table, c->width, c->height, p->sampleOffset[0], p->sampleOffset[1],
                       s.lens, s.bokehShape, seed0, seed1, numDims, blueNoiseLayers, c->sceneDev.blueNoise, (unsigned long long)p->rngKey[0], (unsigned long long)p->rngKey[1], out);
    HIP_TRY(hipGetLastError());
    if (stream != c->lanes[0].stream)   // a set call, a resize or the context's end waits for this reader of the table (waitLensExport)
    {
        if (!s.lensRead) HIP_TRY(hipEventCreateWithFlags(&s.lensRead, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(s.lensRead, stream));
    }
    return RTGPU_OK;
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
    RtCamera pinhole = p->camera;
    pinhole.dofEnable = 0u;   // the stored ray is the pinhole's: the lens is the table's to apply (aperture and focalDistance travel in the entry)
    hipLaunchKernelGGL(k_camera_footprints, sourceGrid(c, c->width * c->height, 16u), dim3(RT_BLOCK), 0, stream, pinhole, p->sampleOffset[0], p->sampleOffset[1], c->width, c->height, out);
    HIP_TRY(hipGetLastError());
    return RTGPU_OK;
}

RTGPU_API int rtgpu_read_camera_rays(RtgpuContext* c, const RtPassParams* p, RtPrimaryRay* out)
{
    const int r = checkCameraRays(c, p, out);
    return r ? r : exportToHost(c, p, out, sizeof(RtPrimaryRay), launchCameraRays);
}
RTGPU_API int rtgpu_read_camera_rays_async(RtgpuContext* c, const RtPassParams* p, RtPrimaryRay* out, void* streamHandle)
{
    const int r = checkCameraRays(c, p, out);
    return r ? r : exportToDevice(c, p, out, sizeof(RtPrimaryRay), launchCameraRays, streamHandle);
}
RTGPU_API int rtgpu_read_lens_source_rays(RtgpuContext* c, const RtPassParams* p, RtPrimaryRay* out)
{
    const int r = checkLensSourceRays(c, p, out);
    return r ? r : exportToHost(c, p, out, sizeof(RtPrimaryRay), launchLensSourceRays);
}
RTGPU_API int rtgpu_read_lens_source_rays_async(RtgpuContext* c, const RtPassParams* p, RtPrimaryRay* out, void* streamHandle)
{
    const int r = checkLensSourceRays(c, p, out);
    return r ? r : exportToDevice(c, p, out, sizeof(RtPrimaryRay), launchLensSourceRays, streamHandle);
}
RTGPU_API int rtgpu_read_camera_footprints(RtgpuContext* c, const RtPassParams* p, RtLensRay* out)
{
    const int r = checkCameraFootprints(c, p, out);
    return r ? r : exportToHost(c, p, out, sizeof(RtLensRay), launchCameraFootprints);
}
RTGPU_API int rtgpu_read_camera_footprints_async(RtgpuContext* c, const RtPassParams* p, RtLensRay* out, void* streamHandle)
{
    const int r = checkCameraFootprints(c, p, out);
    return r ? r : exportToDevice(c, p, out, sizeof(RtLensRay), launchCameraFootprints, streamHandle);
}
