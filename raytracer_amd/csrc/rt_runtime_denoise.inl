// rt_runtime_denoise.inl -- the a-trous filter, host side.  Included by rt_runtime.hip.

// ---- the a-trous filter (include/rtgpu.h, rtgpu_filter_atrous / rtgpu_denoise and their _var siblings; kernels: k_denoise_prepare, k_atrous and k_atrous_tiled, rt_denoise.inl) ------
// One call is k_denoise_prepare and one k_atrous / k_atrous_tiled launch per level on the call's stream, over the context's own scratch: four planes of 16-byte records per
// pixel (normal + valid, position, and the two colour buffers the levels ping-pong between).  The last level remodulates and writes the caller's float3 image.
#define RT_DENOISE_MAX_PIXELS ((size_t)16 << 20)

static int checkDenoiseParams(const RtDenoiseParams* p)
{
    if (p->iterations < 1u || p->iterations > 8u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "iterations must be 1..8");
    const float values[4] = { p->colorScale, p->sigmaColor, p->sigmaNormal, p->sigmaPlane };
    for (float v : values)
        if (!(v > 0.0f && v <= 3.402823466e+38f)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "colorScale and the three sigmas must be finite and > 0");
    return RTGPU_OK;
}

static int checkDenoiseVarParams(const RtDenoiseVarParams* p)
{
    if (p->iterations < 1u || p->iterations > 8u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "iterations must be 1..8");
    const float values[5] = { p->colorScale, p->sigmaLum, p->sigmaNormal, p->sigmaPlane, p->varianceFloor };
    for (float v : values)
        if (!(v > 0.0f && v <= 3.402823466e+38f)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "colorScale, the three sigmas and varianceFloor must be finite and > 0");
    return RTGPU_OK;
}

// what launchAtrous takes from either parameter block.  `variance`: the variance-guided filter (sigmaColor is then its sigmaLum)
struct AtrousPlan { uint32_t iterations, flags; float colorScale, sigmaColor, sigmaNormal, sigmaPlane, varianceFloor; bool variance; };
static AtrousPlan atrousPlan(const RtDenoiseParams* p) { return { p->iterations, p->flags, p->colorScale, p->sigmaColor, p->sigmaNormal, p->sigmaPlane, 0.0f, false }; }
static AtrousPlan atrousPlan(const RtDenoiseVarParams* p) { return { p->iterations, p->flags, p->colorScale, p->sigmaLum, p->sigmaNormal, p->sigmaPlane, p->varianceFloor, true }; }

static int checkFilterSize(uint32_t width, uint32_t height)
{
    if (width == 0 || height == 0) return fail(RTGPU_ERR_INVALID_ARGUMENT, "width and height must be > 0");
    if ((size_t)width * height > RT_DENOISE_MAX_PIXELS) return fail(RTGPU_ERR_UNSUPPORTED, "the a-trous filter takes at most 16 Mi pixels");
    return RTGPU_OK;
}

// `floats` of device memory for the entries that stage planes themselves
static int ensureDenoiseIo(RtgpuContext* c, size_t floats)
{
    RtgpuContext::Denoise& d = c->denoise;
    if (!d.done) HIP_TRY(hipEventCreateWithFlags(&d.done, hipEventDisableTiming));
    if (d.ioFloats >= floats) return RTGPU_OK;
    HIP_TRY(hipEventSynchronize(d.done));
    devFree(d.io); d.ioFloats = 0;
    HIP_TRY(hipMalloc((void**)&d.io, floats * sizeof(float)));
    d.ioFloats = floats;
    return RTGPU_OK;
}

// the record scratch for `pixels` pixels (four planes of 16-byte records), and the event every call on it is ordered by
static int ensureAtrousRecords(RtgpuContext* c, size_t pixels)
{
    RtgpuContext::Denoise& d = c->denoise;
    if (!d.done) HIP_TRY(hipEventCreateWithFlags(&d.done, hipEventDisableTiming));
    if (d.capacity >= pixels) return RTGPU_OK;
    HIP_TRY(hipEventSynchronize(d.done));   // (a fresh event is complete)
    devFree(d.records); d.capacity = 0;
    HIP_TRY(hipMalloc((void**)&d.records, 4u * pixels * sizeof(float4)));
    d.capacity = pixels;
    return RTGPU_OK;
}

// the launches of one call on `stream`; every pointer is device memory.  `colorIsSum`: the colour is the context's sum buffer (and colorHalf its secondary one), whose
// next writer waits for sumRead.  colorHalf and outVariance (may be NULL) belong to the variance-guided filter
static int launchAtrous(RtgpuContext* c, const AtrousPlan& plan, uint32_t width, uint32_t height, const float* color, const float* colorHalf, const float* depth, const float* normal,
                        const float* position, const float* albedo, float* out, float* outVariance, hipStream_t stream, bool colorIsSum)
{
    const AtrousPlan* const p = &plan;
    RtgpuContext::Denoise& d = c->denoise;
    const size_t pixels = (size_t)width * height;
    { int r = ensureAtrousRecords(c, pixels); if (r) return r; }
    HIP_TRY(hipStreamWaitEvent(stream, d.done, 0));   // the scratch is shared with the previous call, whatever its stream
    float4* const recN = d.records; float4* const recP = recN + d.capacity; float4* const buffers[2] = { recP + d.capacity, recP + 2u * d.capacity };
    if (!(p->flags & RT_DENOISE_DEMODULATE)) albedo = nullptr;
    const dim3 prepareGrid((uint32_t)((pixels + RT_BLOCK - 1u) / RT_BLOCK));
    if (p->variance && (p->flags & RT_DENOISE_INPUT_PREPARED)) hipLaunchKernelGGL(k_denoise_prepare_accumulated, prepareGrid, dim3(RT_BLOCK), 0, stream, color, colorHalf, depth, normal, position, (uint32_t)pixels, recN, recP, buffers[0]);
    else if (p->variance) hipLaunchKernelGGL(k_denoise_prepare_var, prepareGrid, dim3(RT_BLOCK), 0, stream, color, colorHalf, depth, normal, position, albedo, (uint32_t)pixels, p->colorScale, recN, recP, buffers[0]);
    else hipLaunchKernelGGL(k_denoise_prepare, prepareGrid, dim3(RT_BLOCK), 0, stream, color, depth, normal, position, albedo, (uint32_t)pixels, p->colorScale, recN, recP, buffers[0]);
    if (colorIsSum)
    {
        if (!d.sumRead) HIP_TRY(hipEventCreateWithFlags(&d.sumRead, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(d.sumRead, stream));
        d.sumReadPending = true;
    }
    // the host constants of the definition, in f32: 1 / sigma^2, the colour one four times larger per level (its sigma halves); the variance-guided filter has
    // sL2 = sigmaLum^2 in its place at every level
    const float invN = 1.0f / (p->sigmaNormal * p->sigmaNormal), invP = 1.0f / (p->sigmaPlane * p->sigmaPlane);
    float invC = p->variance ? p->sigmaColor * p->sigmaColor : 1.0f / (p->sigmaColor * p->sigmaColor);
    // blocks are numbered row by row along grid.x: at most 16 Mi pixels / 64 columns = 256 Ki rows of blocks, more than grid.y may hold
    const dim3 block(RT_DENOISE_BLOCK_X, RT_DENOISE_BLOCK_Y), grid(((width + RT_DENOISE_BLOCK_X - 1u) / RT_DENOISE_BLOCK_X) * ((height + RT_DENOISE_BLOCK_Y - 1u) / RT_DENOISE_BLOCK_Y));
    const dim3 tile(RT_DENOISE_TILE_X, RT_DENOISE_TILE_Y), tiles(((width + RT_DENOISE_TILE_X - 1u) / RT_DENOISE_TILE_X) * ((height + RT_DENOISE_TILE_Y - 1u) / RT_DENOISE_TILE_Y));
    const bool tiled = knobs::denoiseTiled();
    typedef void (*AtrousKernel) RT_K_ATROUS_ARGS;
    static const AtrousKernel tiledKernels[2][2][2] = { { { k_atrous_tiled<false, 1>, k_atrous_tiled<true, 1> }, { k_atrous_tiled<false, 2>, k_atrous_tiled<true, 2> } },
                                                        { { k_atrous_tiled<false, 1, true>, k_atrous_tiled<true, 1, true> }, { k_atrous_tiled<false, 2, true>, k_atrous_tiled<true, 2, true> } } };   // [variance][level][last]
    static const AtrousKernel directKernels[2][2] = { { k_atrous<false>, k_atrous<true> }, { k_atrous<false, true>, k_atrous<true, true> } };   // [variance][last]
    for (uint32_t s = 0; s < p->iterations; ++s)
    {
        const AtrousLevel level = { (int32_t)(1u << s), invN, invP, invC, p->varianceFloor };
        const bool last = s + 1u == p->iterations;
        const float4* const from = buffers[s & 1u]; float4* const to = last ? nullptr : buffers[(s + 1u) & 1u];
        const float* const levelAlbedo = last ? albedo : nullptr; float* const levelOut = last ? out : nullptr; float* const levelVariance = last ? outVariance : nullptr;
        // steps 1 and 2 from LDS tiles unless RTGPU_DENOISE_TILED=0 (a level takes 0.07 ms there against 0.11 ms at 1080p); wider steps gather from memory
        const bool fromTiles = tiled && s < 2u;
        const AtrousKernel kernel = fromTiles ? tiledKernels[p->variance ? 1 : 0][s][last ? 1 : 0] : directKernels[p->variance ? 1 : 0][last ? 1 : 0];
        hipLaunchKernelGGL(kernel, fromTiles ? tiles : grid, fromTiles ? tile : block, 0, stream, recN, recP, from, to, levelAlbedo, levelOut, levelVariance, width, height, level);
        if (!p->variance) invC = invC * 4.0f;
    }
    // `done` is recorded whatever the launches answered: the launches that went out use the scratch, and the next call orders itself behind this event
    const hipError_t launched = hipGetLastError();
    const hipError_t recorded = hipEventRecord(d.done, stream);
    HIP_TRY(launched);
    HIP_TRY(recorded);
    return RTGPU_OK;
}

static int checkFilter(RtgpuContext* c, const RtDenoiseParams* p, uint32_t width, uint32_t height, const void* color, const void* depth, const void* normal, const void* position,
                       const void* albedo, const void* out)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (!p || !color || !depth || !normal || !position || !out) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    if ((p->flags & RT_DENOISE_DEMODULATE) && !albedo) return fail(RTGPU_ERR_INVALID_ARGUMENT, "RT_DENOISE_DEMODULATE needs the albedo plane");
    int r = checkDenoiseParams(p); if (r) return r;
    return checkFilterSize(width, height);
}

RTGPU_API int rtgpu_filter_atrous(RtgpuContext* c, const RtDenoiseParams* p, uint32_t width, uint32_t height, const float* color, const float* depth, const float* normal,
                                  const float* position, const float* albedo, float* outRGB)
{
    int r = checkFilter(c, p, width, height, color, depth, normal, position, albedo, outRGB); if (r) return r;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)width * height;
    const bool demodulate = (p->flags & RT_DENOISE_DEMODULATE) != 0u;
    r = ensureDenoiseIo(c, 16u * n); if (r) return r;   // colour 3, depth 1, normal 3, position 3, albedo 3, the result 3
    hipStream_t stream = c->lanes[0].stream;
    HIP_TRY(hipEventSynchronize(c->denoise.done));   // the staging copies below are not ordered on a stream
    float* const dColor = c->denoise.io; float* const dDepth = dColor + 3u * n; float* const dNormal = dDepth + n; float* const dPosition = dNormal + 3u * n;
    float* const dAlbedo = dPosition + 3u * n; float* const dOut = dAlbedo + 3u * n;
    HIP_TRY(rtMemcpy(dColor, color, 3u * n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(rtMemcpy(dDepth, depth, n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(rtMemcpy(dNormal, normal, 3u * n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(rtMemcpy(dPosition, position, 3u * n * sizeof(float), hipMemcpyHostToDevice));
    if (demodulate) HIP_TRY(rtMemcpy(dAlbedo, albedo, 3u * n * sizeof(float), hipMemcpyHostToDevice));
    r = launchAtrous(c, atrousPlan(p), width, height, dColor, nullptr, dDepth, dNormal, dPosition, dAlbedo, dOut, nullptr, stream, false); if (r) return r;
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(rtMemcpy(outRGB, dOut, 3u * n * sizeof(float), hipMemcpyDeviceToHost));
    return RTGPU_OK;
}

RTGPU_API int rtgpu_filter_atrous_async(RtgpuContext* c, const RtDenoiseParams* p, uint32_t width, uint32_t height, const float* color, const float* depth, const float* normal,
                                        const float* position, const float* albedo, float* outRGB, void* streamHandle)
{
    int r = checkFilter(c, p, width, height, color, depth, normal, position, albedo, outRGB); if (r) return r;
    const size_t n = (size_t)width * height;
    const bool demodulate = (p->flags & RT_DENOISE_DEMODULATE) != 0u;
    const struct { const void* ptr; size_t floats; } inputs[5] = { { color, 3u * n }, { depth, n }, { normal, 3u * n }, { position, 3u * n }, { demodulate ? albedo : nullptr, 3u * n } };
    if ((uintptr_t)outRGB & 15u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the buffers must be 16-byte aligned device memory");
    for (const auto& in : inputs)
    {
        if (!in.ptr) continue;
        if ((uintptr_t)in.ptr & 15u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the buffers must be 16-byte aligned device memory");
        const uintptr_t a = (uintptr_t)in.ptr, b = (uintptr_t)outRGB;
        if (a < b + 3u * n * sizeof(float) && b < a + in.floats * sizeof(float)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the output overlaps an input");
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = streamHandle ? (hipStream_t)streamHandle : c->lanes[0].stream;
    return launchAtrous(c, atrousPlan(p), width, height, color, nullptr, depth, normal, position, albedo, outRGB, nullptr, stream, false);
}

// rtgpu_denoise / rtgpu_denoise_async and their _var siblings (pv in place of p; outVariance, optional, is memory of outRGB's kind): outHost or outDevice
static int denoiseFrame(RtgpuContext* c, const RtDenoiseParams* p, const RtDenoiseVarParams* pv, const RtPassParams* guideParams, float* outHost, float* outDevice, float* outVariance,
                        void* streamHandle)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if ((!p && !pv) || !guideParams || (!outHost && !outDevice)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    if (outDevice && (((uintptr_t)outDevice | (uintptr_t)outVariance) & 15u)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the output must be a 16-byte aligned device buffer");
    int r = pv ? checkDenoiseVarParams(pv) : checkDenoiseParams(p); if (r) return r;
    const AtrousPlan plan = pv ? atrousPlan(pv) : atrousPlan(p);
    if (!c->sceneReady) return fail(RTGPU_ERR_NOT_READY, "rtgpu_upload_scene has not been called");
    if (!c->sum) return fail(RTGPU_ERR_NOT_READY, "rtgpu_resize has not been called");
    r = checkPass(c, guideParams); if (r) return r;   // (before anything is submitted or allocated; rtgpu_render_aovs_async checks again)
    r = checkFilterSize(c->width, c->height); if (r) return r;
    // every queued pass is in the sum buffer, and a multi-device context's tiles are gathered on the first device, as for rtgpu_read_sum
    r = rtgpu_synchronize(c); if (r) return r;
    r = gatherPeers(c); if (r) return r;
    const size_t n = (size_t)c->width * c->height, plane = (n + 3u) & ~(size_t)3u;   // (planes start 16-byte aligned)
    if (outDevice && outVariance)
    {
        const uintptr_t a = (uintptr_t)outDevice, b = (uintptr_t)outVariance;
        if (a < b + n * sizeof(float) && b < a + 3u * n * sizeof(float)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "outVariance overlaps outRGB");
    }
    const bool demodulate = (plan.flags & RT_DENOISE_DEMODULATE) != 0u;
    r = ensureDenoiseIo(c, 10u * plane + (outHost ? (outVariance ? 3u * plane + n : 3u * n) : 0u)); if (r) return r;
    hipStream_t stream = streamHandle ? (hipStream_t)streamHandle : c->lanes[0].stream;
    HIP_TRY(hipStreamWaitEvent(stream, c->denoise.done, 0));   // the guide planes are shared with the previous call
    float* const dDepth = c->denoise.io; float* const dNormal = dDepth + plane; float* const dPosition = dNormal + 3u * plane; float* const dAlbedo = dPosition + 3u * plane;
    float* const out = outHost ? dAlbedo + 3u * plane : outDevice;
    float* const variance = outHost && outVariance ? out + 3u * plane : outVariance;
    // the guides: the first hits of the primary rays `guideParams` generates, through the AOV path (its arena, never a lane's)
    const uint32_t planes[4] = { RT_AOV_DEPTH, RT_AOV_NORMAL, RT_AOV_POSITION, RT_AOV_BASE_COLOR };
    void* const outputs[4] = { dDepth, dNormal, dPosition, dAlbedo };
    r = rtgpu_render_aovs_async(c, guideParams, planes, demodulate ? 4u : 3u, outputs, stream); if (r) return r;
    r = launchAtrous(c, plan, c->width, c->height, c->sum, pv ? c->secondary : nullptr, dDepth, dNormal, dPosition, dAlbedo, out, variance, stream, true); if (r) return r;
    if (outHost)
    {
        HIP_TRY(hipStreamSynchronize(stream));
        c->denoise.sumReadPending = false;
        HIP_TRY(rtMemcpy(outHost, out, 3u * n * sizeof(float), hipMemcpyDeviceToHost));
        if (outVariance) HIP_TRY(rtMemcpy(outVariance, variance, n * sizeof(float), hipMemcpyDeviceToHost));
    }
    return RTGPU_OK;
}

RTGPU_API int rtgpu_denoise(RtgpuContext* c, const RtDenoiseParams* p, const RtPassParams* guideParams, float* outRGB)
{
    return denoiseFrame(c, p, nullptr, guideParams, outRGB, nullptr, nullptr, nullptr);
}

RTGPU_API int rtgpu_denoise_async(RtgpuContext* c, const RtDenoiseParams* p, const RtPassParams* guideParams, float* outRGB, void* streamHandle)
{
    return denoiseFrame(c, p, nullptr, guideParams, nullptr, outRGB, nullptr, streamHandle);
}

// ---- the variance-guided filter (include/rtgpu.h, rtgpu_filter_atrous_var / rtgpu_denoise_var): the same launches with the kVar kernels ------------------------
static int checkFilterVar(RtgpuContext* c, const RtDenoiseVarParams* p, uint32_t width, uint32_t height, const void* color, const void* colorHalf, const void* depth, const void* normal,
                          const void* position, const void* albedo, const void* out)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (!p || !color || !colorHalf || !depth || !normal || !position || !out) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    if ((p->flags & RT_DENOISE_DEMODULATE) && !albedo) return fail(RTGPU_ERR_INVALID_ARGUMENT, "RT_DENOISE_DEMODULATE needs the albedo plane");
    int r = checkDenoiseVarParams(p); if (r) return r;
    return checkFilterSize(width, height);
}

RTGPU_API int rtgpu_filter_atrous_var(RtgpuContext* c, const RtDenoiseVarParams* p, uint32_t width, uint32_t height, const float* color, const float* colorHalf, const float* depth,
                                      const float* normal, const float* position, const float* albedo, float* outRGB, float* outVariance)
{
    int r = checkFilterVar(c, p, width, height, color, colorHalf, depth, normal, position, albedo, outRGB); if (r) return r;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)width * height;
    const bool demodulate = (p->flags & RT_DENOISE_DEMODULATE) != 0u;
    r = ensureDenoiseIo(c, 20u * n); if (r) return r;   // colour 3, half 3, depth 1, normal 3, position 3, albedo 3, the result 3, its variance 1
    hipStream_t stream = c->lanes[0].stream;
    HIP_TRY(hipEventSynchronize(c->denoise.done));   // the staging copies below are not ordered on a stream
    float* const dColor = c->denoise.io; float* const dHalf = dColor + 3u * n; float* const dDepth = dHalf + 3u * n; float* const dNormal = dDepth + n;
    float* const dPosition = dNormal + 3u * n; float* const dAlbedo = dPosition + 3u * n; float* const dOut = dAlbedo + 3u * n; float* const dVariance = dOut + 3u * n;
    HIP_TRY(rtMemcpy(dColor, color, 3u * n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(rtMemcpy(dHalf, colorHalf, 3u * n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(rtMemcpy(dDepth, depth, n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(rtMemcpy(dNormal, normal, 3u * n * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(rtMemcpy(dPosition, position, 3u * n * sizeof(float), hipMemcpyHostToDevice));
    if (demodulate) HIP_TRY(rtMemcpy(dAlbedo, albedo, 3u * n * sizeof(float), hipMemcpyHostToDevice));
    r = launchAtrous(c, atrousPlan(p), width, height, dColor, dHalf, dDepth, dNormal, dPosition, dAlbedo, dOut, outVariance ? dVariance : nullptr, stream, false); if (r) return r;
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(rtMemcpy(outRGB, dOut, 3u * n * sizeof(float), hipMemcpyDeviceToHost));
    if (outVariance) HIP_TRY(rtMemcpy(outVariance, dVariance, n * sizeof(float), hipMemcpyDeviceToHost));
    return RTGPU_OK;
}

RTGPU_API int rtgpu_filter_atrous_var_async(RtgpuContext* c, const RtDenoiseVarParams* p, uint32_t width, uint32_t height, const float* color, const float* colorHalf, const float* depth,
                                            const float* normal, const float* position, const float* albedo, float* outRGB, float* outVariance, void* streamHandle)
{
    int r = checkFilterVar(c, p, width, height, color, colorHalf, depth, normal, position, albedo, outRGB); if (r) return r;
    const size_t n = (size_t)width * height;
    const bool demodulate = (p->flags & RT_DENOISE_DEMODULATE) != 0u;
    // the inputs, then the outputs: each output against everything before it
    const struct { const void* ptr; size_t floats; } buffers[8] = { { color, 3u * n }, { colorHalf, 3u * n }, { depth, n }, { normal, 3u * n }, { position, 3u * n },
                                                                    { demodulate ? albedo : nullptr, 3u * n }, { outRGB, 3u * n }, { outVariance, n } };
    for (uint32_t o = 6u; o < 8u; ++o)
    {
        if (!buffers[o].ptr) continue;
        for (uint32_t i = 0; i <= o; ++i)
        {
            if (!buffers[i].ptr) continue;
            if ((uintptr_t)buffers[i].ptr & 15u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the buffers must be 16-byte aligned device memory");
            const uintptr_t a = (uintptr_t)buffers[i].ptr, b = (uintptr_t)buffers[o].ptr;
            if (i < o && a < b + buffers[o].floats * sizeof(float) && b < a + buffers[i].floats * sizeof(float))
                return fail(RTGPU_ERR_INVALID_ARGUMENT, "an output overlaps an input or the other output");
        }
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = streamHandle ? (hipStream_t)streamHandle : c->lanes[0].stream;
    return launchAtrous(c, atrousPlan(p), width, height, color, colorHalf, depth, normal, position, albedo, outRGB, outVariance, stream, false);
}

RTGPU_API int rtgpu_denoise_var(RtgpuContext* c, const RtDenoiseVarParams* p, const RtPassParams* guideParams, float* outRGB, float* outVariance)
{
    return denoiseFrame(c, nullptr, p, guideParams, outRGB, nullptr, outVariance, nullptr);
}

RTGPU_API int rtgpu_denoise_var_async(RtgpuContext* c, const RtDenoiseVarParams* p, const RtPassParams* guideParams, float* outRGB, float* outVariance, void* streamHandle)
{
    return denoiseFrame(c, nullptr, p, guideParams, nullptr, outRGB, outVariance, streamHandle);
}

RTGPU_API int rtgpu_postprocess_from(RtgpuContext* c, const RtPostprocessParams* p, const float* rgbHost, uint32_t* frontBufferBGRA)
{
    if (!c || !p || !rgbHost || !frontBufferBGRA) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    return postprocessImage(c, p, rgbHost, frontBufferBGRA);
}
