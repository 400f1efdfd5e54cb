// rt_runtime_temporal.inl -- temporal accumulation, host side.  Included by rt_runtime.hip behind rt_runtime_denoise.inl.

// ---- temporal accumulation (include/rtgpu.h, rtgpu_temporal_accumulate / rtgpu_denoise_temporal; kernels: k_temporal_pack and k_temporal, rt_temporal.inl) ------
// One call is one k_temporal launch on the call's stream.  The previous frame reaches it as four planes of 16-byte records: the context-level call keeps two sets
// of them (the previous frame's and the one being written, 128 bytes per pixel, RtgpuContext::Temporal), the pure entries pack the caller's planes into the
// a-trous filter's record scratch first (k_temporal_pack).  The calls share the filter's events: `done` orders them behind each other and behind the filter
// calls whatever their streams, `sumRead` stands behind the read of the sum buffers.

static int checkTemporalParams(const RtTemporalParams* t, bool withCamera)
{
    const float big = 3.402823466e+38f;
    if (!(t->colorScale > 0.0f && t->colorScale <= big)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "colorScale must be finite and > 0");
    if (!(t->alphaMin > 0.0f && t->alphaMin <= 1.0f)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "alphaMin must be in (0, 1]");
    if (!(t->maxHistory >= 1.0f && t->maxHistory <= big)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "maxHistory must be finite and >= 1");
    if (!(t->normalThreshold >= -1.0f && t->normalThreshold <= 1.0f)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "normalThreshold must be in [-1, 1]");
    if (!(t->planeTolerance > 0.0f && t->planeTolerance <= big)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "planeTolerance must be finite and > 0");
    if (withCamera)
    {
        for (float v : t->prevSampleOffset) if (!(fabsf(v) <= big)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "prevSampleOffset must be finite");
        for (float v : t->prevWorldToScreen) if (!(fabsf(v) <= big)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "prevWorldToScreen must be finite");
    }
    return RTGPU_OK;
}

static TemporalFrame temporalFrame(const RtTemporalParams* t, const float* worldToScreen, const float* sampleOffset, bool useIds)
{
    TemporalFrame f;
    f.colorScale = t->colorScale; f.alphaMin = t->alphaMin; f.maxHistory = t->maxHistory; f.normalThreshold = t->normalThreshold; f.planeTolerance = t->planeTolerance;
    f.prevSampleOffset[0] = sampleOffset[0]; f.prevSampleOffset[1] = sampleOffset[1];
    f.useIds = useIds ? 1u : 0u;
    for (int i = 0; i < 16; ++i) f.m[i] = worldToScreen[i];
    return f;
}

// motion: the device copy of an RtObjectMotion table (objects moved between the two frames: k_temporal<true>), or NULL: the static kernel, launched as ever
static void launchTemporalKernel(const TemporalIn& in, const TemporalOut& out, uint32_t width, uint32_t height, const TemporalFrame& frame, hipStream_t stream,
                                 const RtObjectMotion* motion = nullptr, uint32_t numObjects = 0u)
{
    const dim3 block(RT_DENOISE_BLOCK_X, RT_DENOISE_BLOCK_Y), grid(((width + RT_DENOISE_BLOCK_X - 1u) / RT_DENOISE_BLOCK_X) * ((height + RT_DENOISE_BLOCK_Y - 1u) / RT_DENOISE_BLOCK_Y));
    if (!motion) { hipLaunchKernelGGL(k_temporal<false>, grid, block, 0, stream, in, out, width, height, frame); return; }
    static_assert(sizeof(RtObjectMotion) == 5u * sizeof(float4), "k_temporal<true> reads a motion record as five float4");
    TemporalFrameMoving moving;
    static_cast<TemporalFrame&>(moving) = frame;
    moving.objects = reinterpret_cast<const float4*>(motion); moving.numObjects = numObjects;
    hipLaunchKernelGGL(k_temporal<true>, grid, block, 0, stream, in, out, width, height, moving);
}

// The motion table of rtgpu_denoise_temporal (include/rtgpu.h): then[o] = the id and transform current object o had when the history was stored.  Doubles, each dot
// product summed left to right, rounded to float once: products of two floats are exact in double, so this is NumPy's float64 result whatever the compiler contracts.
typedef RtgpuContext::Temporal::Then ObjectThen;
static void buildMotionTable(const std::vector<RtObject>& now, const std::vector<ObjectThen>& then, std::vector<RtObjectMotion>& table)
{
    table.resize(now.size());
    for (size_t o = 0; o < now.size(); ++o)
    {
        RtObjectMotion& r = table[o];
        memset(&r, 0, sizeof(r));
        r.prevId = then[o].id;
        r.moved = memcmp(now[o].transform, then[o].transform, sizeof(then[o].transform)) != 0 ? 1u : 0u;
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j)
            {
                double sum = (double)now[o].invTransform[4 * i] * (double)then[o].transform[j];
                for (int k = 1; k < 4; ++k) sum = sum + (double)now[o].invTransform[4 * i + k] * (double)then[o].transform[4 * k + j];
                r.m[4 * i + j] = (float)sum;
            }
    }
}

// the planes of the pure entries, as the caller passed them
struct TemporalPlanes
{
    const float* color; const float* colorHalf; const float* depth; const float* normal; const float* position; const float* albedo; const uint32_t* objectId;
    const float* prevA; const float* prevB; const float* prevLength; const float* prevDepth; const float* prevNormal; const float* prevPosition; const uint32_t* prevObjectId;
    float* outA; float* outB; float* outLength; float* outMotion;
};
static const uint32_t kTemporalBuffers = 18u, kTemporalFirstOutput = 14u;
// buffer k of the planes (the struct's order) and its floats per pixel
static const uint32_t kTemporalFloats[kTemporalBuffers] = { 3u, 3u, 1u, 3u, 3u, 3u, 1u, 3u, 3u, 1u, 1u, 3u, 3u, 1u, 3u, 3u, 1u, 2u };
static const void* temporalBuffer(const TemporalPlanes& b, uint32_t k)
{
    const void* const all[kTemporalBuffers] = { b.color, b.colorHalf, b.depth, b.normal, b.position, b.albedo, b.objectId, b.prevA, b.prevB, b.prevLength, b.prevDepth, b.prevNormal,
                                               b.prevPosition, b.prevObjectId, b.outA, b.outB, b.outLength, b.outMotion };
    return all[k];
}

// the motion table of the _moving entries (NULL, 0: the entries without)
struct TemporalMotion { const RtObjectMotion* objects; uint32_t numObjects; bool given; };
static const TemporalMotion kNoMotion = { nullptr, 0u, false };

static int checkTemporal(RtgpuContext* c, const RtTemporalParams* t, uint32_t width, uint32_t height, TemporalPlanes& b, bool& history, const TemporalMotion& motion = kNoMotion)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (motion.given && (!motion.objects || motion.numObjects == 0u)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the motion table is NULL or empty");
    if (motion.given && (!b.objectId || (b.prevA && !b.prevObjectId))) return fail(RTGPU_ERR_INVALID_ARGUMENT, "moving objects are followed by their ids: both id planes are required");
    if (!t || !b.color || !b.colorHalf || !b.depth || !b.normal || !b.position || !b.outA || !b.outB || !b.outLength) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    if (t->flags & RT_DENOISE_DEMODULATE) { if (!b.albedo) return fail(RTGPU_ERR_INVALID_ARGUMENT, "RT_DENOISE_DEMODULATE needs the albedo plane"); }
    else b.albedo = nullptr;
    const uint32_t given = (b.prevA ? 1u : 0u) + (b.prevB ? 1u : 0u) + (b.prevLength ? 1u : 0u) + (b.prevDepth ? 1u : 0u) + (b.prevNormal ? 1u : 0u) + (b.prevPosition ? 1u : 0u);
    if ((given != 0u && given != 6u) || (given == 0u && b.prevObjectId)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the previous frame's buffers must be given together or not at all");
    history = given == 6u;
    if (history && (b.objectId != nullptr) != (b.prevObjectId != nullptr)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the object test needs both id planes: give both or neither");
    int r = checkTemporalParams(t, true); if (r) return r;
    return checkFilterSize(width, height);
}

// the launches of a pure call on `stream`; every pointer is device memory
static int launchTemporal(RtgpuContext* c, const RtTemporalParams* t, uint32_t width, uint32_t height, const TemporalPlanes& b, bool history, hipStream_t stream,
                          const TemporalMotion& motion = kNoMotion)
{
    RtgpuContext::Denoise& d = c->denoise;
    const size_t pixels = (size_t)width * height;
    int r = ensureAtrousRecords(c, history ? pixels : 0u); if (r) return r;
    HIP_TRY(hipStreamWaitEvent(stream, d.done, 0));
    TemporalIn in = { b.color, b.colorHalf, b.depth, b.normal, b.position, b.albedo, b.objectId, nullptr, nullptr, nullptr, nullptr };
    if (history)
    {
        float4* const recA = d.records; float4* const recB = recA + d.capacity; float4* const recN = recB + d.capacity; float4* const recP = recN + d.capacity;
        hipLaunchKernelGGL(k_temporal_pack, dim3((uint32_t)((pixels + RT_BLOCK - 1u) / RT_BLOCK)), dim3(RT_BLOCK), 0, stream, b.prevA, b.prevB, b.prevLength, b.prevDepth, b.prevNormal,
                           b.prevPosition, b.prevObjectId, (uint32_t)pixels, recA, recB, recN, recP);
        in.recA = recA; in.recB = recB; in.recN = recN; in.recP = recP;
    }
    const TemporalOut out = { b.outA, b.outB, b.outLength, b.outMotion, nullptr, nullptr, nullptr, nullptr, nullptr };
    launchTemporalKernel(in, out, width, height, temporalFrame(t, t->prevWorldToScreen, t->prevSampleOffset, history && b.objectId && b.prevObjectId), stream,
                         history && motion.given ? motion.objects : nullptr, motion.numObjects);   // (without history every pixel starts: the table has nothing to say)
    const hipError_t launched = hipGetLastError();
    const hipError_t recorded = hipEventRecord(d.done, stream);   // (whatever the launches answered, as launchAtrous)
    HIP_TRY(launched);
    HIP_TRY(recorded);
    return RTGPU_OK;
}

// the host-pointer entries: every plane, and the motion table behind them, staged in the filter's second buffer
static int temporalAccumulateHost(RtgpuContext* c, const RtTemporalParams* t, uint32_t width, uint32_t height, TemporalPlanes host, const TemporalMotion& motion)
{
    bool history = false;
    int r = checkTemporal(c, t, width, height, host, history, motion); if (r) return r;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)width * height, plane = (n + 3u) & ~(size_t)3u;   // (planes start 16-byte aligned)
    const size_t tableFloats = motion.given ? (size_t)motion.numObjects * (sizeof(RtObjectMotion) / sizeof(float)) : 0u;
    r = ensureDenoiseIo(c, 41u * plane + tableFloats); if (r) return r;   // the floats per pixel of the 18 buffers
    hipStream_t stream = c->lanes[0].stream;
    HIP_TRY(hipEventSynchronize(c->denoise.done));   // the staging copies below are not ordered on a stream
    const void* staged[kTemporalBuffers];
    float* cursor = c->denoise.io;
    for (uint32_t k = 0; k < kTemporalBuffers; ++k)
    {
        const void* const source = temporalBuffer(host, k);
        staged[k] = source ? cursor : nullptr;
        if (source && k < kTemporalFirstOutput) HIP_TRY(rtMemcpy(cursor, source, kTemporalFloats[k] * n * sizeof(float), hipMemcpyHostToDevice));
        cursor += kTemporalFloats[k] * plane;
    }
    const TemporalPlanes device = { (const float*)staged[0], (const float*)staged[1], (const float*)staged[2], (const float*)staged[3], (const float*)staged[4], (const float*)staged[5],
                                    (const uint32_t*)staged[6], (const float*)staged[7], (const float*)staged[8], (const float*)staged[9], (const float*)staged[10],
                                    (const float*)staged[11], (const float*)staged[12], (const uint32_t*)staged[13], (float*)staged[14], (float*)staged[15], (float*)staged[16],
                                    (float*)staged[17] };
    TemporalMotion staged_motion = motion;
    if (motion.given)
    {
        HIP_TRY(rtMemcpy(cursor, motion.objects, tableFloats * sizeof(float), hipMemcpyHostToDevice));
        staged_motion.objects = reinterpret_cast<const RtObjectMotion*>(cursor);
    }
    r = launchTemporal(c, t, width, height, device, history, stream, staged_motion); if (r) return r;
    HIP_TRY(hipStreamSynchronize(stream));
    for (uint32_t k = kTemporalFirstOutput; k < kTemporalBuffers; ++k)
        if (staged[k]) HIP_TRY(rtMemcpy(const_cast<void*>(temporalBuffer(host, k)), staged[k], kTemporalFloats[k] * n * sizeof(float), hipMemcpyDeviceToHost));
    return RTGPU_OK;
}

RTGPU_API int rtgpu_temporal_accumulate(RtgpuContext* c, const RtTemporalParams* t, uint32_t width, uint32_t height, const float* color, const float* colorHalf, const float* depth,
                                        const float* normal, const float* position, const float* albedo, const uint32_t* objectId, const float* prevA, const float* prevB,
                                        const float* prevLength, const float* prevDepth, const float* prevNormal, const float* prevPosition, const uint32_t* prevObjectId,
                                        float* outA, float* outB, float* outLength, float* outMotion)
{
    const TemporalPlanes host = { color, colorHalf, depth, normal, position, albedo, objectId, prevA, prevB, prevLength, prevDepth, prevNormal, prevPosition, prevObjectId, outA, outB, outLength, outMotion };
    return temporalAccumulateHost(c, t, width, height, host, kNoMotion);
}

RTGPU_API int rtgpu_temporal_accumulate_moving(RtgpuContext* c, const RtTemporalParams* t, uint32_t width, uint32_t height, const float* color, const float* colorHalf, const float* depth,
                                               const float* normal, const float* position, const float* albedo, const uint32_t* objectId, const float* prevA, const float* prevB,
                                               const float* prevLength, const float* prevDepth, const float* prevNormal, const float* prevPosition, const uint32_t* prevObjectId,
                                               float* outA, float* outB, float* outLength, float* outMotion, const RtObjectMotion* objects, uint32_t numObjects)
{
    const TemporalPlanes host = { color, colorHalf, depth, normal, position, albedo, objectId, prevA, prevB, prevLength, prevDepth, prevNormal, prevPosition, prevObjectId, outA, outB, outLength, outMotion };
    const TemporalMotion motion = { objects, numObjects, true };
    return temporalAccumulateHost(c, t, width, height, host, motion);
}

// the device-pointer entries
static int temporalAccumulateDevice(RtgpuContext* c, const RtTemporalParams* t, uint32_t width, uint32_t height, TemporalPlanes b, const TemporalMotion& motion, void* streamHandle)
{
    bool history = false;
    int r = checkTemporal(c, t, width, height, b, history, motion); if (r) return r;
    if (motion.given && ((uintptr_t)motion.objects & 15u)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the motion table must be 16-byte aligned device memory");
    const size_t n = (size_t)width * height;
    // every buffer aligned; each output against everything before it
    for (uint32_t o = 0; o < kTemporalBuffers; ++o)
    {
        const uintptr_t pb = (uintptr_t)temporalBuffer(b, o);
        if (!pb) continue;
        if (pb & 15u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the buffers must be 16-byte aligned device memory");
        if (o < kTemporalFirstOutput) continue;
        for (uint32_t i = 0; i < o; ++i)
        {
            const uintptr_t pa = (uintptr_t)temporalBuffer(b, i);
            if (pa && pa < pb + kTemporalFloats[o] * n * sizeof(float) && pb < pa + kTemporalFloats[i] * n * sizeof(float))
                return fail(RTGPU_ERR_INVALID_ARGUMENT, "an output overlaps an input or another output");
        }
    }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = streamHandle ? (hipStream_t)streamHandle : c->lanes[0].stream;
    return launchTemporal(c, t, width, height, b, history, stream, motion);
}

RTGPU_API int rtgpu_temporal_accumulate_async(RtgpuContext* c, const RtTemporalParams* t, uint32_t width, uint32_t height, const float* color, const float* colorHalf,
                                              const float* depth, const float* normal, const float* position, const float* albedo, const uint32_t* objectId, const float* prevA,
                                              const float* prevB, const float* prevLength, const float* prevDepth, const float* prevNormal, const float* prevPosition,
                                              const uint32_t* prevObjectId, float* outA, float* outB, float* outLength, float* outMotion, void* streamHandle)
{
    const TemporalPlanes b = { color, colorHalf, depth, normal, position, albedo, objectId, prevA, prevB, prevLength, prevDepth, prevNormal, prevPosition, prevObjectId, outA, outB, outLength, outMotion };
    return temporalAccumulateDevice(c, t, width, height, b, kNoMotion, streamHandle);
}

RTGPU_API int rtgpu_temporal_accumulate_moving_async(RtgpuContext* c, const RtTemporalParams* t, uint32_t width, uint32_t height, const float* color, const float* colorHalf,
                                                     const float* depth, const float* normal, const float* position, const float* albedo, const uint32_t* objectId,
                                                     const float* prevA, const float* prevB, const float* prevLength, const float* prevDepth, const float* prevNormal,
                                                     const float* prevPosition, const uint32_t* prevObjectId, float* outA, float* outB, float* outLength, float* outMotion,
                                                     const RtObjectMotion* objects, uint32_t numObjects, void* streamHandle)
{
    const TemporalPlanes b = { color, colorHalf, depth, normal, position, albedo, objectId, prevA, prevB, prevLength, prevDepth, prevNormal, prevPosition, prevObjectId, outA, outB, outLength, outMotion };
    const TemporalMotion motion = { objects, numObjects, true };
    return temporalAccumulateDevice(c, t, width, height, b, motion, streamHandle);
}

RTGPU_API int rtgpu_temporal_reset(RtgpuContext* c)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    c->temporal.have = false;
    return RTGPU_OK;
}

// rtgpu_denoise_temporal / rtgpu_denoise_temporal_async: outHost or outDevice (outVariance is memory of the same kind, written with `v` only)
static int denoiseTemporalFrame(RtgpuContext* c, const RtTemporalParams* t, const RtDenoiseVarParams* v, const RtPassParams* guideParams, float* outHost, float* outDevice,
                                float* outVariance, void* streamHandle)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (!t || !guideParams || (!outHost && !outDevice)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    if (outDevice && (((uintptr_t)outDevice | (uintptr_t)outVariance) & 15u)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the output must be a 16-byte aligned device buffer");
    int r = checkTemporalParams(t, false); if (r) return r;
    if (v) { r = checkDenoiseVarParams(v); if (r) return r; }
    if (!c->sceneReady) return fail(RTGPU_ERR_NOT_READY, "rtgpu_upload_scene has not been called");
    if (!c->sum) return fail(RTGPU_ERR_NOT_READY, "rtgpu_resize has not been called");
    r = checkPass(c, guideParams); if (r) return r;
    r = checkFilterSize(c->width, c->height); if (r) return r;
    r = rtgpu_synchronize(c); if (r) return r;
    r = gatherPeers(c); if (r) return r;
    const size_t n = (size_t)c->width * c->height, plane = (n + 3u) & ~(size_t)3u;
    if (!v) outVariance = nullptr;
    if (outDevice && outVariance)
    {
        const uintptr_t a = (uintptr_t)outDevice, b = (uintptr_t)outVariance;
        if (a < b + n * sizeof(float) && b < a + 3u * n * sizeof(float)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "outVariance overlaps outRGB");
    }
    // guides: depth 1, normal 3, position 3, albedo 3, object id 1; the accumulated pair 3 + 3 and its length 1; then the host entry's result
    r = ensureDenoiseIo(c, 18u * plane + (outHost ? 3u * plane + n : 0u)); if (r) return r;
    RtgpuContext::Temporal& h = c->temporal;
    if (h.capacity < n)
    {
        HIP_TRY(hipEventSynchronize(c->denoise.done));
        devFree(h.records); h.capacity = 0; h.have = false;
        HIP_TRY(hipMalloc((void**)&h.records, 8u * n * sizeof(float4)));
        h.capacity = n;
    }
    hipStream_t stream = streamHandle ? (hipStream_t)streamHandle : c->lanes[0].stream;
    HIP_TRY(hipStreamWaitEvent(stream, c->denoise.done, 0));   // guide planes and history are shared with the previous call
    float* const dDepth = c->denoise.io; float* const dNormal = dDepth + plane; float* const dPosition = dNormal + 3u * plane; float* const dAlbedo = dPosition + 3u * plane;
    uint32_t* const dId = (uint32_t*)(dAlbedo + 3u * plane); float* const dA = (float*)dId + plane; float* const dB = dA + 3u * plane; float* const dLength = dB + 3u * plane;
    float* const out = outHost ? dLength + plane : outDevice;
    float* const variance = outHost && outVariance ? out + 3u * plane : outVariance;
    const uint32_t planes[5] = { RT_AOV_DEPTH, RT_AOV_NORMAL, RT_AOV_POSITION, RT_AOV_BASE_COLOR, RT_AOV_OBJECT_ID };
    void* const outputs[5] = { dDepth, dNormal, dPosition, dAlbedo, dId };
    r = rtgpu_render_aovs_async(c, guideParams, planes, 5u, outputs, stream); if (r) return r;
    float4* const from = h.records + (size_t)h.current * 4u * h.capacity; float4* const to = h.records + (size_t)(h.current ^ 1u) * 4u * h.capacity;
    TemporalIn in = { c->sum, c->secondary, dDepth, dNormal, dPosition, (t->flags & RT_DENOISE_DEMODULATE) ? dAlbedo : nullptr, dId, nullptr, nullptr, nullptr, nullptr };
    if (h.have) { in.recA = from; in.recB = from + h.capacity; in.recN = from + 2u * h.capacity; in.recP = from + 3u * h.capacity; }
    const TemporalOut res = { dA, dB, dLength, nullptr, v ? nullptr : out, to, to + h.capacity, to + 2u * h.capacity, to + 3u * h.capacity };
    const RtObjectMotion* motion = nullptr;
    const std::vector<RtObject>& objects = c->updatable.objects;
    if (h.have && h.movedSince && !objects.empty() && h.then.size() == objects.size())
    {
        // objects were updated since the history was stored: where each was then.  (The table is small and the copy is not ordered on a stream: the kernel
        // of the previous call may still read the last one.)
        std::vector<RtObjectMotion> table;
        buildMotionTable(objects, h.then, table);
        HIP_TRY(hipEventSynchronize(c->denoise.done));
        if (h.motionCapacity < table.size())
        {
            devFree(h.motion); h.motionCapacity = 0;
            HIP_TRY(hipMalloc((void**)&h.motion, table.size() * sizeof(RtObjectMotion)));
            h.motionCapacity = table.size();
        }
        HIP_TRY(rtMemcpy(h.motion, table.data(), table.size() * sizeof(RtObjectMotion), hipMemcpyHostToDevice));
        motion = h.motion;
    }
    launchTemporalKernel(in, res, c->width, c->height, temporalFrame(t, h.worldToScreen, h.sampleOffset, h.have), stream, motion, (uint32_t)objects.size());
    const hipError_t launched = hipGetLastError();
    const hipError_t recorded = hipEventRecord(c->denoise.done, stream);
    HIP_TRY(launched);
    HIP_TRY(recorded);
    RtgpuContext::Denoise& d = c->denoise;
    if (!d.sumRead) HIP_TRY(hipEventCreateWithFlags(&d.sumRead, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(d.sumRead, stream));
    d.sumReadPending = true;
    // this frame is the next call's history
    h.current ^= 1u; h.have = true;
    h.movedSince = false;
    h.then.resize(objects.size());
    for (size_t o = 0; o < objects.size(); ++o) { h.then[o].id = (uint32_t)o; memcpy(h.then[o].transform, objects[o].transform, sizeof(h.then[o].transform)); }
    memcpy(h.worldToScreen, guideParams->camera.worldToScreen, sizeof(h.worldToScreen));
    h.sampleOffset[0] = guideParams->sampleOffset[0]; h.sampleOffset[1] = guideParams->sampleOffset[1];
    if (v)
    {
        AtrousPlan plan = atrousPlan(v);
        plan.flags |= RT_DENOISE_INPUT_PREPARED; plan.colorScale = 1.0f;
        r = launchAtrous(c, plan, c->width, c->height, dA, dB, dDepth, dNormal, dPosition, dAlbedo, out, variance, stream, false); if (r) return r;
    }
    if (outHost)
    {
        HIP_TRY(hipStreamSynchronize(stream));
        d.sumReadPending = false;
        HIP_TRY(rtMemcpy(outHost, out, 3u * n * sizeof(float), hipMemcpyDeviceToHost));
        if (outVariance) HIP_TRY(rtMemcpy(outVariance, variance, n * sizeof(float), hipMemcpyDeviceToHost));
    }
    return RTGPU_OK;
}

RTGPU_API int rtgpu_denoise_temporal(RtgpuContext* c, const RtTemporalParams* t, const RtDenoiseVarParams* v, const RtPassParams* guideParams, float* outRGB, float* outVariance)
{
    return denoiseTemporalFrame(c, t, v, guideParams, outRGB, nullptr, outVariance, nullptr);
}

RTGPU_API int rtgpu_denoise_temporal_async(RtgpuContext* c, const RtTemporalParams* t, const RtDenoiseVarParams* v, const RtPassParams* guideParams, float* outRGB, float* outVariance,
                                           void* streamHandle)
{
    return denoiseTemporalFrame(c, t, v, guideParams, nullptr, outRGB, outVariance, streamHandle);
}
