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

// Device scratch of the filter and of temporal accumulation: `buffer` holds perCount * capacity elements and grows to `count`, once the calls that use the old one
// are done.  Creates `done`, the event every call on the scratch is ordered by (a fresh event is complete)
template <class T> static int ensureScratch(RtgpuContext* c, T*& buffer, size_t& capacity, size_t count, size_t perCount = 1u)
{
    RtgpuContext::Denoise& d = c->denoise;
    if (!d.done) HIP_TRY(hipEventCreateWithFlags(&d.done, hipEventDisableTiming));
    if (capacity >= count) return RTGPU_OK;
    HIP_TRY(hipEventSynchronize(d.done));
    devFree(buffer); capacity = 0;
    HIP_TRY(hipMalloc((void**)&buffer, perCount * count * sizeof(T)));
    capacity = count;
    return RTGPU_OK;
}

// ---- a call's planes: the host entries stage them (stagePlanes, copyPlanesBack), the device entries check them (checkDevicePlanes) ------------------------------
// the planes of one call in the order of its arguments, every input before the first output.  A NULL plane is one the call does without
struct Plane { const void* ptr; uint32_t floatsPerPixel; bool output; };
struct PlaneTable
{
    Plane planes[25]; uint32_t count;
    bool has(uint32_t k) const { return planes[k].ptr != nullptr; }
    const float* in(uint32_t k) const { return (const float*)planes[k].ptr; }
    const uint32_t* ids(uint32_t k) const { return (const uint32_t*)planes[k].ptr; }
    float* out(uint32_t k) const { return (float*)const_cast<void*>(planes[k].ptr); }
};

// `device`: the planes of `host` laid into the context's io buffer, each plane of a buffer starting 16-byte aligned, the inputs copied up; `blob` (host memory in,
// its device copy out: the motion table, say) goes behind them
static int stagePlanes(RtgpuContext* c, const PlaneTable& host, size_t pixels, PlaneTable& device, const void** blob = nullptr, size_t blobBytes = 0u)
{
    const size_t stride = (pixels + 3u) & ~(size_t)3u;
    size_t floats = (blobBytes + sizeof(float) - 1u) / sizeof(float);
    for (uint32_t k = 0; k < host.count; ++k) if (host.has(k)) floats += host.planes[k].floatsPerPixel * stride;
    int r = ensureScratch(c, c->denoise.io, c->denoise.ioFloats, floats); if (r) return r;
    HIP_TRY(hipEventSynchronize(c->denoise.done));   // the staging copies below are not ordered on a stream
    device = host;
    float* cursor = c->denoise.io;
    for (uint32_t k = 0; k < host.count; ++k)
    {
        Plane& p = device.planes[k];
        if (!p.ptr) continue;
        if (!p.output) HIP_TRY(rtMemcpy(cursor, p.ptr, p.floatsPerPixel * pixels * sizeof(float), hipMemcpyHostToDevice));
        p.ptr = cursor;
        cursor += p.floatsPerPixel * stride;
    }
    if (blobBytes)
    {
        HIP_TRY(rtMemcpy(cursor, *blob, blobBytes, hipMemcpyHostToDevice));
        *blob = cursor;
    }
    return RTGPU_OK;
}

// the outputs of `device` (stagePlanes) back into those of `host`, once the stream is synchronized
static int copyPlanesBack(const PlaneTable& host, const PlaneTable& device, size_t pixels)
{
    for (uint32_t k = 0; k < host.count; ++k)
        if (host.has(k) && host.planes[k].output) HIP_TRY(rtMemcpy(host.out(k), device.planes[k].ptr, host.planes[k].floatsPerPixel * pixels * sizeof(float), hipMemcpyDeviceToHost));
    return RTGPU_OK;
}

// device planes: every one 16-byte aligned, each output against everything before it
static int checkDevicePlanes(const PlaneTable& b, size_t pixels)
{
    for (uint32_t o = 0; o < b.count; ++o)
    {
        const uintptr_t pb = (uintptr_t)b.planes[o].ptr;
        if (!pb) continue;
        if (pb & 15u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the buffers must be 16-byte aligned device memory");
        if (!b.planes[o].output) continue;
        for (uint32_t i = 0; i < o; ++i)
        {
            const uintptr_t pa = (uintptr_t)b.planes[i].ptr;
            if (pa && pa < pb + b.planes[o].floatsPerPixel * pixels * sizeof(float) && pb < pa + b.planes[i].floatsPerPixel * pixels * sizeof(float))
                return fail(RTGPU_ERR_INVALID_ARGUMENT, "an output overlaps an input or another output");
        }
    }
    return RTGPU_OK;
}

// the sum buffers were read on `stream`: whatever writes the film next waits for sumRead
static int markSumRead(RtgpuContext* c, hipStream_t stream)
{
    RtgpuContext::Denoise& d = c->denoise;
    if (!d.sumRead) HIP_TRY(hipEventCreateWithFlags(&d.sumRead, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(d.sumRead, stream));
    d.sumReadPending = true;
    return RTGPU_OK;
}

// behind the launches of a call: `done` is recorded whatever they answered -- those that went out use the scratch, and the next call orders itself behind this event
static int recordDone(RtgpuContext* c, hipStream_t stream)
{
    const hipError_t launched = hipGetLastError();
    const hipError_t recorded = hipEventRecord(c->denoise.done, stream);
    HIP_TRY(launched);
    HIP_TRY(recorded);
    return RTGPU_OK;
}

// the planes of the filter entries.  colorHalf and outVariance (may be NULL) belong to the variance-guided filter
enum { F_COLOR, F_HALF, F_DEPTH, F_NORMAL, F_POSITION, F_ALBEDO, F_OUT, F_VARIANCE };
static PlaneTable filterPlanes(const float* color, const float* colorHalf, const float* depth, const float* normal, const float* position, const float* albedo, float* out, float* outVariance)
{
    return { { { color, 3u, false }, { colorHalf, 3u, false }, { depth, 1u, false }, { normal, 3u, false }, { position, 3u, false }, { albedo, 3u, false }, { out, 3u, true },
               { outVariance, 1u, true } }, 8u };
}

// the launches of one call on `stream`; every plane is device memory.  `colorIsSum`: the colour is the context's sum buffer (and colorHalf its secondary one)
static int launchAtrous(RtgpuContext* c, const AtrousPlan& plan, uint32_t width, uint32_t height, const PlaneTable& b, hipStream_t stream, bool colorIsSum)
{
    const AtrousPlan* const p = &plan;
    RtgpuContext::Denoise& d = c->denoise;
    const size_t pixels = (size_t)width * height;
    int r = ensureScratch(c, d.records, d.capacity, pixels, 4u); if (r) return r;   // normals + valid, positions, two colour buffers
    HIP_TRY(hipStreamWaitEvent(stream, d.done, 0));   // the scratch is shared with the previous call, whatever its stream
    float4* const recN = d.records; float4* const recP = recN + d.capacity; float4* const buffers[2] = { recP + d.capacity, recP + 2u * d.capacity };
    const float* const color = b.in(F_COLOR); const float* const colorHalf = b.in(F_HALF); const float* const depth = b.in(F_DEPTH); const float* const normal = b.in(F_NORMAL);
    const float* const position = b.in(F_POSITION); const float* const albedo = (p->flags & RT_DENOISE_DEMODULATE) ? b.in(F_ALBEDO) : nullptr;
    float* const out = b.out(F_OUT); float* const outVariance = b.out(F_VARIANCE);
    const dim3 prepareGrid((uint32_t)((pixels + RT_BLOCK - 1u) / RT_BLOCK));
    if (p->variance && (p->flags & RT_DENOISE_INPUT_PREPARED)) hipLaunchKernelGGL(k_denoise_prepare_accumulated, prepareGrid, dim3(RT_BLOCK), 0, stream, color, colorHalf, depth, normal, position, (uint32_t)pixels, recN, recP, buffers[0]);
    else if (p->variance) hipLaunchKernelGGL(k_denoise_prepare_var, prepareGrid, dim3(RT_BLOCK), 0, stream, color, colorHalf, depth, normal, position, albedo, (uint32_t)pixels, p->colorScale, recN, recP, buffers[0]);
    else hipLaunchKernelGGL(k_denoise_prepare, prepareGrid, dim3(RT_BLOCK), 0, stream, color, depth, normal, position, albedo, (uint32_t)pixels, p->colorScale, recN, recP, buffers[0]);
    if (colorIsSum) { r = markSumRead(c, stream); if (r) return r; }
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
    return recordDone(c, stream);
}

// the pure entries: p or pv (the plain or the variance-guided filter, which needs colorHalf) over planes in device memory (onDevice), or in host memory, which is staged
static int filterImage(RtgpuContext* c, const RtDenoiseParams* p, const RtDenoiseVarParams* pv, uint32_t width, uint32_t height, PlaneTable b, bool onDevice, void* streamHandle)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if ((!p && !pv) || !b.has(F_COLOR) || (pv && !b.has(F_HALF)) || !b.has(F_DEPTH) || !b.has(F_NORMAL) || !b.has(F_POSITION) || !b.has(F_OUT))
        return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!((pv ? pv->flags : p->flags) & RT_DENOISE_DEMODULATE)) b.planes[F_ALBEDO].ptr = nullptr;   // (neither staged nor checked)
    else if (!b.has(F_ALBEDO)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "RT_DENOISE_DEMODULATE needs the albedo plane");
    int r = pv ? checkDenoiseVarParams(pv) : checkDenoiseParams(p); if (r) return r;
    r = checkFilterSize(width, height); if (r) return r;
    const size_t n = (size_t)width * height;
    if (onDevice) { r = checkDevicePlanes(b, n); if (r) return r; }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = streamHandle ? (hipStream_t)streamHandle : c->lanes[0].stream;
    PlaneTable device = b;
    if (!onDevice) { r = stagePlanes(c, b, n, device); if (r) return r; }
    r = launchAtrous(c, pv ? atrousPlan(pv) : atrousPlan(p), width, height, device, stream, false);
    if (r || onDevice) return r;
    HIP_TRY(hipStreamSynchronize(stream));
    return copyPlanesBack(b, device, n);
}

RTGPU_API int rtgpu_filter_atrous(RtgpuContext* c, const RtDenoiseParams* p, uint32_t width, uint32_t height, const float* color, const float* depth, const float* normal,
                                  const float* position, const float* albedo, float* outRGB)
{
    return filterImage(c, p, nullptr, width, height, filterPlanes(color, nullptr, depth, normal, position, albedo, outRGB, nullptr), false, nullptr);
}

RTGPU_API int rtgpu_filter_atrous_async(RtgpuContext* c, const RtDenoiseParams* p, uint32_t width, uint32_t height, const float* color, const float* depth, const float* normal,
                                        const float* position, const float* albedo, float* outRGB, void* streamHandle)
{
    return filterImage(c, p, nullptr, width, height, filterPlanes(color, nullptr, depth, normal, position, albedo, outRGB, nullptr), true, streamHandle);
}

// ---- one frame step: what the context-level calls (rtgpu_denoise, rtgpu_denoise_var, rtgpu_denoise_temporal and their _async siblings) do before and after their launches ----
// the call's stream and its planes in device memory, each `stride` floats per channel: the guides, `extra` (the caller's own planes), and the result -- the caller's
// device buffers, or io memory that finishFrame copies to outHost / varianceHost
struct FrameStep
{
    hipStream_t stream; size_t pixels, stride;
    float* depth; float* normal; float* position; float* albedo; uint32_t* id; float* extra; float* out; float* variance; float* outHost; float* varianceHost;
    uint32_t* chainLength; float* chainDistance; float* virtualPosition;   // (virtualChain only: the last five floats per pixel of `extra`)
    uint32_t* subObjectId; float* barycentrics;                            // (deformPlanes only: the last three floats per pixel of `extra`)
};

// The checks of a frame call behind those of its parameter blocks; then every queued pass is in the sum buffer, `stream` stands behind the previous call, and the first
// `guides` of depth, normal, position, base colour and object id are rendered on it: the first hits of the primary rays `guideParams` generates, through the AOV path
// (its arena, never a lane's) -- or, under rtgpu_set_guide_chain, the guide vertices of the paths it generates, through the chain call.  outHost or outDevice; outVariance (optional) is memory of the same kind, written with writesVariance only; outPlane (optional, beside
// outDevice only): one more device output of a float per pixel, held to the same rules.  virtualChain (rtgpu_denoise_temporal_chain; or NULL): the guides are rendered
// through rtgpu_render_aovs_virtual_async with this chain, whatever rtgpu_set_guide_chain says, and CHAIN_LENGTH, CHAIN_DISTANCE and VIRTUAL_POSITION beside them
// into the last five floats per pixel of the caller's `extra` planes.  deformPlanes (a temporal call that follows a deformed mesh; never beside a chain): SUB_OBJECT_ID
// and BARYCENTRICS are rendered beside the guides, into the last three floats per pixel of `extra`
static int beginFrame(RtgpuContext* c, const RtPassParams* guideParams, float* outHost, float* outDevice, float* outVariance, bool writesVariance, void* streamHandle,
                      uint32_t guides, uint32_t extraFloatsPerPixel, FrameStep& f, float* outPlane = nullptr, const RtAovChain* virtualChain = nullptr, bool deformPlanes = false)
{
    if (!guideParams || (!outHost && !outDevice)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    if (outDevice && (((uintptr_t)outDevice | (uintptr_t)outVariance | (uintptr_t)outPlane) & 15u)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the output must be a 16-byte aligned device buffer");
    if (!writesVariance) outVariance = nullptr;
    if (!c->sceneReady) return fail(RTGPU_ERR_NOT_READY, "rtgpu_upload_scene has not been called");
    if (!c->sum) return fail(RTGPU_ERR_NOT_READY, "rtgpu_resize has not been called");
    int r = checkPass(c, guideParams); if (r) return r;   // (before anything is submitted or allocated; rtgpu_render_aovs_async checks again)
    r = checkFilterSize(c->width, c->height); if (r) return r;
    const size_t n = (size_t)c->width * c->height, plane = (n + 3u) & ~(size_t)3u;   // (planes start 16-byte aligned)
    if (outDevice && outVariance)
    {
        const uintptr_t a = (uintptr_t)outDevice, b = (uintptr_t)outVariance;
        if (a < b + n * sizeof(float) && b < a + 3u * n * sizeof(float)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "outVariance overlaps outRGB");
    }
    if (outDevice && outPlane)
    {
        const uintptr_t a = (uintptr_t)outDevice, b = (uintptr_t)outVariance, p = (uintptr_t)outPlane;
        if ((p < a + 3u * n * sizeof(float) && a < p + n * sizeof(float)) || (b && p < b + n * sizeof(float) && b < p + n * sizeof(float)))
            return fail(RTGPU_ERR_INVALID_ARGUMENT, "an output overlaps another output");
    }
    // every queued pass is in the sum buffer, and a multi-device context's tiles are gathered on the first device, as for rtgpu_read_sum
    r = rtgpu_synchronize(c); if (r) return r;
    r = gatherPeers(c); if (r) return r;
    // guides: depth 1, normal 3, position 3, albedo 3, object id 1; the caller's planes; then the host entry's result
    r = ensureScratch(c, c->denoise.io, c->denoise.ioFloats, (11u + extraFloatsPerPixel) * plane + (outHost ? 3u * plane + (outVariance ? n : 0u) : 0u)); if (r) return r;
    f.stream = streamHandle ? (hipStream_t)streamHandle : c->lanes[0].stream;
    HIP_TRY(hipStreamWaitEvent(f.stream, c->denoise.done, 0));   // the io planes (and the temporal history) are shared with the previous call
    f.pixels = n; f.stride = plane;
    f.depth = c->denoise.io; f.normal = f.depth + plane; f.position = f.normal + 3u * plane; f.albedo = f.position + 3u * plane; f.id = (uint32_t*)(f.albedo + 3u * plane);
    f.extra = (float*)f.id + plane;
    f.outHost = outHost; f.varianceHost = outHost ? outVariance : nullptr;
    f.out = outHost ? f.extra + extraFloatsPerPixel * plane : outDevice;
    f.variance = f.varianceHost ? f.out + 3u * plane : outVariance;
    const uint32_t planes[5] = { RT_AOV_DEPTH, RT_AOV_NORMAL, RT_AOV_POSITION, RT_AOV_BASE_COLOR, RT_AOV_OBJECT_ID };
    void* const outputs[5] = { f.depth, f.normal, f.position, f.albedo, f.id };
    f.chainLength = nullptr; f.chainDistance = nullptr; f.virtualPosition = nullptr;
    f.subObjectId = nullptr; f.barycentrics = nullptr;
    if (virtualChain)
    {
        f.chainLength = (uint32_t*)(f.extra + (extraFloatsPerPixel - 5u) * plane); f.chainDistance = (float*)f.chainLength + plane; f.virtualPosition = f.chainDistance + plane;
        const uint32_t chainPlanes[8] = { RT_AOV_DEPTH, RT_AOV_NORMAL, RT_AOV_POSITION, RT_AOV_BASE_COLOR, RT_AOV_OBJECT_ID, RT_AOV_CHAIN_LENGTH, RT_AOV_CHAIN_DISTANCE, RT_AOV_VIRTUAL_POSITION };
        void* const chainOutputs[8] = { f.depth, f.normal, f.position, f.albedo, f.id, f.chainLength, f.chainDistance, f.virtualPosition };
        return rtgpu_render_aovs_virtual_async(c, guideParams, virtualChain, chainPlanes, 8u, chainOutputs, f.stream);
    }
    if (c->chain.guide)
    {
        // rtgpu_set_guide_chain: the same planes at the guide vertex of every pixel's path
        const RtAovChain chain = { c->chain.guideMaxChain, 0u, { 0u, 0u } };
        return rtgpu_render_aovs_chain_async(c, guideParams, &chain, planes, guides, outputs, f.stream);
    }
    if (deformPlanes)
    {
        f.subObjectId = (uint32_t*)(f.extra + (extraFloatsPerPixel - 3u) * plane); f.barycentrics = (float*)f.subObjectId + plane;
        const uint32_t deformAovs[7] = { RT_AOV_DEPTH, RT_AOV_NORMAL, RT_AOV_POSITION, RT_AOV_BASE_COLOR, RT_AOV_OBJECT_ID, RT_AOV_SUB_OBJECT_ID, RT_AOV_BARYCENTRICS };
        void* const deformOutputs[7] = { f.depth, f.normal, f.position, f.albedo, f.id, f.subObjectId, f.barycentrics };
        return rtgpu_render_aovs_async(c, guideParams, deformAovs, 7u, deformOutputs, f.stream);
    }
    return rtgpu_render_aovs_async(c, guideParams, planes, guides, outputs, f.stream);
}

// the host entry's epilogue: the stream has finished (with it the read of the sum buffers), and the result goes to the caller
static int finishFrame(RtgpuContext* c, const FrameStep& f)
{
    if (!f.outHost) return RTGPU_OK;
    HIP_TRY(hipStreamSynchronize(f.stream));
    c->denoise.sumReadPending = false;
    HIP_TRY(rtMemcpy(f.outHost, f.out, 3u * f.pixels * sizeof(float), hipMemcpyDeviceToHost));
    if (f.varianceHost) HIP_TRY(rtMemcpy(f.varianceHost, f.variance, f.pixels * sizeof(float), hipMemcpyDeviceToHost));
    return RTGPU_OK;
}

// rtgpu_denoise / rtgpu_denoise_async and their _var siblings (pv in place of p; outVariance, optional, is memory of outRGB's kind): outHost or outDevice
static int denoiseFrame(RtgpuContext* c, const RtDenoiseParams* p, const RtDenoiseVarParams* pv, const RtPassParams* guideParams, float* outHost, float* outDevice, float* outVariance,
                        void* streamHandle)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (!p && !pv) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    int r = pv ? checkDenoiseVarParams(pv) : checkDenoiseParams(p); if (r) return r;
    const AtrousPlan plan = pv ? atrousPlan(pv) : atrousPlan(p);
    FrameStep f;
    r = beginFrame(c, guideParams, outHost, outDevice, outVariance, true, streamHandle, (plan.flags & RT_DENOISE_DEMODULATE) ? 4u : 3u, 0u, f); if (r) return r;
    r = launchAtrous(c, plan, c->width, c->height, filterPlanes(c->sum, pv ? c->secondary : nullptr, f.depth, f.normal, f.position, f.albedo, f.out, f.variance), f.stream, true);
    return r ? r : finishFrame(c, f);
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
RTGPU_API int rtgpu_filter_atrous_var(RtgpuContext* c, const RtDenoiseVarParams* p, uint32_t width, uint32_t height, const float* color, const float* colorHalf, const float* depth,
                                      const float* normal, const float* position, const float* albedo, float* outRGB, float* outVariance)
{
    return filterImage(c, nullptr, p, width, height, filterPlanes(color, colorHalf, depth, normal, position, albedo, outRGB, outVariance), false, nullptr);
}

RTGPU_API int rtgpu_filter_atrous_var_async(RtgpuContext* c, const RtDenoiseVarParams* p, uint32_t width, uint32_t height, const float* color, const float* colorHalf, const float* depth,
                                            const float* normal, const float* position, const float* albedo, float* outRGB, float* outVariance, void* streamHandle)
{
    return filterImage(c, nullptr, p, width, height, filterPlanes(color, colorHalf, depth, normal, position, albedo, outRGB, outVariance), true, streamHandle);
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
