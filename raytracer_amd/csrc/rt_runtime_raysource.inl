// rt_runtime_raysource.inl -- the ray source, host side.  Included by rt_runtime.hip.

// ---- the ray source (include/rtgpu.h, rtgpu_set_ray_source; kernels: rt_raysource.inl) ----------------------------------------------------------
// While RtgpuContext::raySource.table is set, every launch site of k_generate / k_generate_dense takes its table-fed counterpart (launchGenerate and
// submitDenseBatch, rt_runtime_render.inl; the AOV calls and the recorder through launchGenerate) and makeDevPass hands the kernels a camera that draws
// nothing.  Nothing else of a pass changes.  Setting a table: queued passes go out first, everything that could read the old table is waited for, the new
// one is copied into the context's second buffer, k_ray_source_check reads it once, and only a table without a degenerate entry changes places with the
// old one.

static int raySourceBuffers(RtgpuContext* c, size_t entries)
{
    RtgpuContext::RaySource& s = c->raySource;
    if (!s.degenerate) HIP_TRY(hipMalloc((void**)&s.degenerate, sizeof(uint32_t)));
    if (!s.incoming) HIP_TRY(hipMalloc((void**)&s.incoming, entries * sizeof(RtPrimaryRay)));   // (dropped with the frame's size: it holds this frame's entries)
    return RTGPU_OK;
}

// The other kind's table after a set call succeeded (everything that read it has been waited for): it becomes that kind's spare buffer, or goes.
static void raySourceRetire(float4*& table, float4*& incoming)
{
    if (!table) return;
    if (!incoming) { incoming = table; table = nullptr; }
    else devFree(table);
}

// k_ray_source_check over raySource.incoming on `stream`, read back; then the swap, or the refusal that leaves the source as it was
static int raySourceCheckAndSwap(RtgpuContext* c, uint32_t entries, hipStream_t stream)
{
    RtgpuContext::RaySource& s = c->raySource;
    HIP_TRY(hipMemsetAsync(s.degenerate, 0, sizeof(uint32_t), stream));
    // (a block ends in one atomic on the same word: four blocks per CU, and the loop strides)
    const uint32_t wanted = (entries + RT_BLOCK - 1u) / RT_BLOCK, most = 4u * c->numCUs;
    hipLaunchKernelGGL(k_ray_source_check, dim3(wanted < most ? wanted : most), dim3(RT_BLOCK), 0, stream, s.incoming, entries, s.degenerate);
    HIP_TRY(hipGetLastError());
    uint32_t degenerate = 0u;
    HIP_TRY(hipMemcpyAsync(&degenerate, s.degenerate, sizeof(degenerate), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (degenerate != 0u)
        return fail(RTGPU_ERR_INVALID_ARGUMENT, std::to_string(degenerate) + " entries of the table are degenerate rays (an origin or direction word that is not finite, a zero direction)");
    float4* const previous = s.table;
    s.table = s.incoming; s.incoming = previous;
    raySourceRetire(s.lensTable, s.lensIncoming);   // one context holds one source: a lens source ends here
    return RTGPU_OK;
}

// what both entries check and wait for before the copy; `clear`: the call clears the source and is done
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
    if (!rays) { dropRaySource(c); clear = true; }
    return RTGPU_OK;
}

RTGPU_API int rtgpu_set_ray_source(RtgpuContext* c, const RtPrimaryRay* rays, uint64_t count)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    // every device renders its own tiles from its own copy of the whole table; a refusal comes from the first peer, before any source has changed
    // (all of them check the same values)
    RT_FAN_OUT(c, rtgpu_set_ray_source(peer, rays, count));
    bool clear = false;
    int r = raySourceBegin(c, rays, count, clear); if (r || clear) return r;
    r = raySourceBuffers(c, (size_t)count); if (r) return r;
    HIP_TRY(rtMemcpy(c->raySource.incoming, rays, (size_t)count * sizeof(RtPrimaryRay), hipMemcpyHostToDevice));
    return raySourceCheckAndSwap(c, (uint32_t)count, c->lanes[0].stream);
}

RTGPU_API int rtgpu_set_ray_source_device(RtgpuContext* c, const RtPrimaryRay* rays, uint64_t count, void* streamHandle)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (!c->peers.empty() || c->isPeer) return fail(RTGPU_ERR_UNSUPPORTED, "rtgpu_set_ray_source_device takes a table of one device: a multi-device context takes rtgpu_set_ray_source");
    bool clear = false;
    int r = raySourceBegin(c, rays, count, clear); if (r || clear) return r;
    r = callerDeviceArray(c, rays, (size_t)count * sizeof(RtPrimaryRay), 3u, "rays", "32 bytes per pixel"); if (r) return r;
    r = raySourceBuffers(c, (size_t)count); if (r) return r;
    RtgpuContext::RaySource& s = c->raySource;
    // the copy goes behind the stream that made the table
    const hipStream_t stream = c->lanes[0].stream;
    if (streamHandle && (hipStream_t)streamHandle != stream)
    {
        if (!s.order) HIP_TRY(hipEventCreateWithFlags(&s.order, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(s.order, (hipStream_t)streamHandle));
        HIP_TRY(hipStreamWaitEvent(stream, s.order, 0));
    }
    HIP_TRY(hipMemcpyAsync(s.incoming, rays, (size_t)count * sizeof(RtPrimaryRay), hipMemcpyDeviceToDevice, stream));
    return raySourceCheckAndSwap(c, (uint32_t)count, stream);   // (synchronises: the caller may overwrite or free the table on return)
}

RTGPU_API int rtgpu_get_ray_source(RtgpuContext* c, uint64_t* outCount)
{
    if (!c || !outCount) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    *outCount = c->raySource.any() ? (uint64_t)c->width * c->height : 0u;   // (a source of either kind: rtgpu_get_ray_source_kind tells them apart)
    return RTGPU_OK;
}

// ---- the camera's rays in the table's layout (rtgpu_read_camera_rays; k_camera_rays) -------------------------------------------------------------
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
    const uint32_t entries = c->width * c->height;
    const uint32_t wanted = (entries + RT_BLOCK - 1u) / RT_BLOCK, most = 16u * c->numCUs;
    hipLaunchKernelGGL(k_camera_rays, dim3(wanted < most ? wanted : most), dim3(RT_BLOCK), 0, stream, p->camera, p->sampleOffset[0], p->sampleOffset[1], c->width, c->height, out);
    HIP_TRY(hipGetLastError());
    return RTGPU_OK;
}

RTGPU_API int rtgpu_read_camera_rays(RtgpuContext* c, const RtPassParams* p, RtPrimaryRay* out)
{
    int r = checkCameraRays(c, p, out); if (r) return r;
    HIP_TRY(hipSetDevice(c->device));
    RtgpuContext::RaySource& s = c->raySource;
    const size_t entries = (size_t)c->width * c->height;
    if (s.exportedEntries < entries)
    {
        devFree(s.exported); s.exportedEntries = 0;
        HIP_TRY(hipMalloc((void**)&s.exported, entries * sizeof(RtPrimaryRay)));
        s.exportedEntries = entries;
    }
    const hipStream_t stream = c->lanes[0].stream;
    r = launchCameraRays(c, p, s.exported, stream); if (r) return r;
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(rtMemcpy(out, s.exported, entries * sizeof(RtPrimaryRay), hipMemcpyDeviceToHost));
    return RTGPU_OK;
}

RTGPU_API int rtgpu_read_camera_rays_async(RtgpuContext* c, const RtPassParams* p, RtPrimaryRay* out, void* streamHandle)
{
    int r = checkCameraRays(c, p, out); if (r) return r;
    HIP_TRY(hipSetDevice(c->device));
    r = callerDeviceArray(c, out, (size_t)c->width * c->height * sizeof(RtPrimaryRay), 15u, "out", "32 bytes per pixel"); if (r) return r;
    return launchCameraRays(c, p, reinterpret_cast<float4*>(out), streamHandle ? (hipStream_t)streamHandle : c->lanes[0].stream);
}
