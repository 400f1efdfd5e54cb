// rt_runtime_temporal.inl -- temporal accumulation, host side.  Included by rt_runtime.hip behind rt_runtime_denoise.inl.

// ---- temporal accumulation (include/rtgpu.h, rtgpu_temporal_accumulate / rtgpu_denoise_temporal; kernels: k_temporal_pack and k_temporal, rt_temporal.inl) ------
// One call is one k_temporal launch on the call's stream (a clipped call with a history: k_temporal_moments in front of it).  The previous frame reaches it as four planes of 16-byte records: the context-level call keeps two sets
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

// RtTemporalClip (history clipping): every field inside its stated range
static int checkTemporalClip(const RtTemporalClip* clip)
{
    if (clip->radius < 1u || clip->radius > 3u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "clip radius must be 1, 2 or 3");
    if (!(clip->gamma >= 0.0f && clip->gamma <= 1e6f)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "clip gamma must be finite and in [0, 1e6]");
    if (clip->minCount < 1u || clip->minCount > 49u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "clip minCount must be 1..49");
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

// history clipping of one launch: the clip, two planes of `capacity` moment records for k_temporal_moments to fill, and the confidence plane (may be NULL)
struct TemporalClipLaunch { const RtTemporalClip* clip; float4* moments; size_t capacity; float* confidence; };

// motion: the device copy of an RtObjectMotion table (objects moved between the two frames: k_temporal<true>), or NULL: the static kernel, launched as ever.
// clipped (or NULL): k_temporal_moments over this frame's planes first -- only with a history: without one nothing blends, and nothing is there to clip --, then
// the clipping variant of either kernel
// chain (or NULL): the planes are chain guides (rtgpu_temporal_accumulate_chain) -- the k_temporal_chain / k_temporal_moments_chain sibling of whichever kernel the
// call without would launch, with this frame's chain planes behind its arguments
// deform (or NULL; beside a motion table and never beside a chain): the table holds RT_MOTION_DEFORMED records -- k_temporal<true, ., true>, with this frame's
// triangle planes and the old triangle records behind the moving frame
struct TemporalDeformLaunch { const uint32_t* subObjectId; const float* barycentrics; const float* prevTriangles; uint32_t numPrevTriangles; };
static void launchTemporalKernel(const TemporalIn& in, const TemporalOut& out, uint32_t width, uint32_t height, const TemporalFrame& frame, hipStream_t stream,
                                 const RtObjectMotion* motion = nullptr, uint32_t numObjects = 0u, const TemporalClipLaunch* clipped = nullptr, const TemporalChainPlanes* chain = nullptr,
                                 const TemporalDeformLaunch* deform = nullptr)
{
    const dim3 block(RT_DENOISE_BLOCK_X, RT_DENOISE_BLOCK_Y), grid(((width + RT_DENOISE_BLOCK_X - 1u) / RT_DENOISE_BLOCK_X) * ((height + RT_DENOISE_BLOCK_Y - 1u) / RT_DENOISE_BLOCK_Y));
    if (!motion && !clipped)
    {
        if (chain) hipLaunchKernelGGL((k_temporal_chain<false, false>), grid, block, 0, stream, in, out, width, height, frame, *chain);
        else hipLaunchKernelGGL(k_temporal<false>, grid, block, 0, stream, in, out, width, height, frame);
        return;
    }
    static_assert(sizeof(RtObjectMotion) == 5u * sizeof(float4), "k_temporal<true> reads a motion record as five float4");
    TemporalFrameMoving moving;
    static_cast<TemporalFrame&>(moving) = frame;
    moving.objects = reinterpret_cast<const float4*>(motion); moving.numObjects = numObjects;
    static_assert(sizeof(RtTriangle) == 9u * sizeof(float), "k_temporal<true, ., true> reads a triangle record as nine floats");
    TemporalFrameDeform deforming;
    static_cast<TemporalFrameMoving&>(deforming) = moving;
    if (deform && motion) { deforming.subObjectId = deform->subObjectId; deforming.barycentrics = deform->barycentrics; deforming.prevTriangles = deform->prevTriangles; deforming.numPrevTriangles = deform->numPrevTriangles; }
    else deform = nullptr;
    if (!clipped)
    {
        if (deform) { hipLaunchKernelGGL((k_temporal<true, false, true>), grid, block, 0, stream, in, out, width, height, deforming); return; }
        if (chain) hipLaunchKernelGGL((k_temporal_chain<true, false>), grid, block, 0, stream, in, out, width, height, moving, *chain);
        else hipLaunchKernelGGL(k_temporal<true>, grid, block, 0, stream, in, out, width, height, moving);
        return;
    }
    float4* const mu = clipped->moments; float4* const g = mu + clipped->capacity;
    if (in.recA)
    {
        const dim3 tile(RT_DENOISE_TILE_X, RT_DENOISE_TILE_Y), tiles(((width + RT_DENOISE_TILE_X - 1u) / RT_DENOISE_TILE_X) * ((height + RT_DENOISE_TILE_Y - 1u) / RT_DENOISE_TILE_Y));
        const TemporalMomentsFrame moments = { frame.colorScale, frame.normalThreshold, frame.planeTolerance, clipped->clip->gamma };
        typedef void (*MomentsKernel) RT_K_TEMPORAL_MOMENTS_ARGS;
        static const MomentsKernel kernels[3] = { k_temporal_moments<1>, k_temporal_moments<2>, k_temporal_moments<3> };
        typedef void (*MomentsChainKernel) RT_K_TEMPORAL_MOMENTS_CHAIN_ARGS;
        static const MomentsChainKernel chainKernels[3] = { k_temporal_moments_chain<1>, k_temporal_moments_chain<2>, k_temporal_moments_chain<3> };
        if (chain) hipLaunchKernelGGL(chainKernels[clipped->clip->radius - 1u], tiles, tile, 0, stream, in, width, height, moments, mu, g, *chain);
        else hipLaunchKernelGGL(kernels[clipped->clip->radius - 1u], tiles, tile, 0, stream, in, width, height, moments, mu, g);
    }
    if (!motion)
    {
        TemporalFrameClip<TemporalFrame> f;
        static_cast<TemporalFrame&>(f) = frame;
        f.momentMu = mu; f.momentG = g; f.confidence = clipped->confidence; f.minCount = (float)clipped->clip->minCount;
        if (chain) hipLaunchKernelGGL((k_temporal_chain<false, true>), grid, block, 0, stream, in, out, width, height, f, *chain);
        else hipLaunchKernelGGL((k_temporal<false, true>), grid, block, 0, stream, in, out, width, height, f);
    }
    else if (deform)
    {
        TemporalFrameClip<TemporalFrameDeform> f;
        static_cast<TemporalFrameDeform&>(f) = deforming;
        f.momentMu = mu; f.momentG = g; f.confidence = clipped->confidence; f.minCount = (float)clipped->clip->minCount;
        hipLaunchKernelGGL((k_temporal<true, true, true>), grid, block, 0, stream, in, out, width, height, f);
    }
    else
    {
        TemporalFrameClip<TemporalFrameMoving> f;
        static_cast<TemporalFrameMoving&>(f) = moving;
        f.momentMu = mu; f.momentG = g; f.confidence = clipped->confidence; f.minCount = (float)clipped->clip->minCount;
        if (chain) hipLaunchKernelGGL((k_temporal_chain<true, true>), grid, block, 0, stream, in, out, width, height, f, *chain);
        else hipLaunchKernelGGL((k_temporal<true, true>), grid, block, 0, stream, in, out, width, height, f);
    }
}

// the moment records of a clipped call over `pixels` pixels: scratch of the clipped calls' own, ordered like the rest by denoise.done.  Without a history no
// moments are taken and none are read: nothing is allocated
static int temporalClipLaunch(RtgpuContext* c, const RtTemporalClip* clip, size_t pixels, bool history, float* confidence, TemporalClipLaunch& launch)
{
    RtgpuContext::Temporal& h = c->temporal;
    launch = { clip, nullptr, 0u, confidence };
    if (!history) return RTGPU_OK;
    int r = ensureScratch(c, h.moments, h.momentsCapacity, pixels, 2u); if (r) return r;
    launch.moments = h.moments; launch.capacity = h.momentsCapacity;
    return RTGPU_OK;
}

// The motion table of rtgpu_denoise_temporal (include/rtgpu.h): then[o] = the id and transform current object o had when the history was stored.  Doubles, each dot
// product summed left to right, rounded to float once: products of two floats are exact in double, so this is NumPy's float64 result whatever the compiler contracts.
// Deforming meshes (rtgpu_set_deform_tracking): an object whose mesh was deformed under a snapshot is no rigid record.  With `meshes` (the scene's mesh table: the
// call follows deformations) its record is RT_MOTION_DEFORMED -- m the words of the transform of then, _pad the mesh's range of the snapshot, which is laid
// out over the scene's triangle numbering --; without (rtgpu_denoise_temporal_chain) its pixels start, as those of a mesh deformed untracked do.
typedef RtgpuContext::Temporal::Then ObjectThen;
static void buildMotionTable(const std::vector<RtObject>& now, const std::vector<ObjectThen>& then, std::vector<RtObjectMotion>& table, const std::vector<RtMesh>* meshes = nullptr)
{
    table.resize(now.size());
    for (size_t o = 0; o < now.size(); ++o)
    {
        RtObjectMotion& r = table[o];
        memset(&r, 0, sizeof(r));
        r.prevId = then[o].id;
        if (then[o].deformed && meshes)
        {
            const RtMesh& mesh = (*meshes)[now[o].meshIndex];
            r.moved = RT_MOTION_DEFORMED;
            memcpy(r.m, then[o].transform, sizeof(r.m));
            r._pad[0] = mesh.firstTriangle; r._pad[1] = mesh.numTriangles;
            continue;
        }
        if (then[o].deformed) r.prevId = 0xFFFFFFFFu;
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

// the planes of the pure entries, in the order of their arguments
// (the four planes of RtTemporalChain and the two of RtTemporalDeform stand behind the other inputs: every input before the first output)
enum { T_COLOR, T_HALF, T_DEPTH, T_NORMAL, T_POSITION, T_ALBEDO, T_ID, T_PREV_A, T_PREV_B, T_PREV_LENGTH, T_PREV_DEPTH, T_PREV_NORMAL, T_PREV_POSITION, T_PREV_ID,
       T_VIRTUAL_POSITION, T_CHAIN_LENGTH, T_CHAIN_DISTANCE, T_PREV_CHAIN_LENGTH, T_SUB_OBJECT_ID, T_BARYCENTRICS, T_OUT_A, T_OUT_B, T_OUT_LENGTH, T_OUT_MOTION, T_OUT_CONFIDENCE };
static PlaneTable temporalPlanes(const float* color, const float* colorHalf, const float* depth, const float* normal, const float* position, const float* albedo, const uint32_t* objectId,
                                 const float* prevA, const float* prevB, const float* prevLength, const float* prevDepth, const float* prevNormal, const float* prevPosition,
                                 const uint32_t* prevObjectId, float* outA, float* outB, float* outLength, float* outMotion, float* outConfidence = nullptr,
                                 const RtTemporalChain* chain = nullptr, const RtTemporalDeform* deform = nullptr)
{
    return { { { color, 3u, false }, { colorHalf, 3u, false }, { depth, 1u, false }, { normal, 3u, false }, { position, 3u, false }, { albedo, 3u, false }, { objectId, 1u, false },
               { prevA, 3u, false }, { prevB, 3u, false }, { prevLength, 1u, false }, { prevDepth, 1u, false }, { prevNormal, 3u, false }, { prevPosition, 3u, false },
               { prevObjectId, 1u, false }, { chain ? chain->virtualPosition : nullptr, 3u, false }, { chain ? chain->chainLength : nullptr, 1u, false },
               { chain ? chain->chainDistance : nullptr, 1u, false }, { chain ? chain->prevChainLength : nullptr, 1u, false },
               { deform ? deform->subObjectId : nullptr, 1u, false }, { deform ? deform->barycentrics : nullptr, 2u, false },
               { outA, 3u, true }, { outB, 3u, true }, { outLength, 1u, true }, { outMotion, 2u, true }, { outConfidence, 1u, true } }, 25u };
}

// the motion table of the _moving entries (NULL, 0: the entries without)
struct TemporalMotion { const RtObjectMotion* objects; uint32_t numObjects; bool given; };
static const TemporalMotion kNoMotion = { nullptr, 0u, false };

static int checkTemporal(RtgpuContext* c, const RtTemporalParams* t, uint32_t width, uint32_t height, PlaneTable& b, bool& history, const TemporalMotion& motion)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (motion.given && (!motion.objects || motion.numObjects == 0u)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the motion table is NULL or empty");
    if (motion.given && (!b.has(T_ID) || (b.has(T_PREV_A) && !b.has(T_PREV_ID)))) return fail(RTGPU_ERR_INVALID_ARGUMENT, "moving objects are followed by their ids: both id planes are required");
    if (!t || !b.has(T_COLOR) || !b.has(T_HALF) || !b.has(T_DEPTH) || !b.has(T_NORMAL) || !b.has(T_POSITION) || !b.has(T_OUT_A) || !b.has(T_OUT_B) || !b.has(T_OUT_LENGTH))
        return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!(t->flags & RT_DENOISE_DEMODULATE)) b.planes[T_ALBEDO].ptr = nullptr;
    else if (!b.has(T_ALBEDO)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "RT_DENOISE_DEMODULATE needs the albedo plane");
    uint32_t given = 0u;
    for (uint32_t k = T_PREV_A; k <= T_PREV_POSITION; ++k) given += b.has(k) ? 1u : 0u;
    if ((given != 0u && given != 6u) || (given == 0u && b.has(T_PREV_ID))) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the previous frame's buffers must be given together or not at all");
    history = given == 6u;
    if (history && b.has(T_ID) != b.has(T_PREV_ID)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the object test needs both id planes: give both or neither");
    int r = checkTemporalParams(t, true); if (r) return r;
    return checkFilterSize(width, height);
}

// the launches of a pure call on `stream`; every plane is device memory
static int launchTemporal(RtgpuContext* c, const RtTemporalParams* t, uint32_t width, uint32_t height, const PlaneTable& b, bool history, hipStream_t stream, const TemporalMotion& motion,
                          const RtTemporalClip* clip, bool chained, const RtTemporalDeform* deform = nullptr, const float* prevTriangles = nullptr)
{
    RtgpuContext::Denoise& d = c->denoise;
    const size_t pixels = (size_t)width * height;
    int r = ensureScratch(c, d.records, d.capacity, history ? pixels : 0u, 4u); if (r) return r;   // (the filter's record scratch, and the event every call is ordered by)
    TemporalClipLaunch clipped;
    if (clip) { r = temporalClipLaunch(c, clip, pixels, history, b.out(T_OUT_CONFIDENCE), clipped); if (r) return r; }
    HIP_TRY(hipStreamWaitEvent(stream, d.done, 0));
    TemporalIn in = { b.in(T_COLOR), b.in(T_HALF), b.in(T_DEPTH), b.in(T_NORMAL), b.in(T_POSITION), b.in(T_ALBEDO), b.ids(T_ID), nullptr, nullptr, nullptr, nullptr };
    if (history)
    {
        float4* const recA = d.records; float4* const recB = recA + d.capacity; float4* const recN = recB + d.capacity; float4* const recP = recN + d.capacity;
        hipLaunchKernelGGL(k_temporal_pack, dim3((uint32_t)((pixels + RT_BLOCK - 1u) / RT_BLOCK)), dim3(RT_BLOCK), 0, stream, b.in(T_PREV_A), b.in(T_PREV_B), b.in(T_PREV_LENGTH),
                           b.in(T_PREV_DEPTH), b.in(T_PREV_NORMAL), b.in(T_PREV_POSITION), b.ids(T_PREV_ID), b.ids(T_PREV_CHAIN_LENGTH), (uint32_t)pixels, recA, recB, recN, recP);
        in.recA = recA; in.recB = recB; in.recN = recN; in.recP = recP;
    }
    const TemporalOut out = { b.out(T_OUT_A), b.out(T_OUT_B), b.out(T_OUT_LENGTH), b.out(T_OUT_MOTION), nullptr, nullptr, nullptr, nullptr, nullptr };
    const TemporalChainPlanes chain = { b.in(T_VIRTUAL_POSITION), b.ids(T_CHAIN_LENGTH), b.in(T_CHAIN_DISTANCE) };
    const TemporalDeformLaunch deforming = { b.ids(T_SUB_OBJECT_ID), b.in(T_BARYCENTRICS), prevTriangles, deform ? deform->numPrevTriangles : 0u };
    launchTemporalKernel(in, out, width, height, temporalFrame(t, t->prevWorldToScreen, t->prevSampleOffset, history && b.has(T_ID) && b.has(T_PREV_ID)), stream,
                         history && motion.given ? motion.objects : nullptr, motion.numObjects, clip ? &clipped : nullptr,   // (without history every pixel starts: the table has nothing to say)
                         chained ? &chain : nullptr, deform ? &deforming : nullptr);
    return recordDone(c, stream);
}

// the pure entries over planes (and a motion table) in device memory (onDevice), or in host memory: then staged, the table behind the planes
// (clipped: the _clip entries, which need `clip`)
// (chained: the _chain entries, whose table holds the planes of their RtTemporalChain -- `chain` itself is only tested for NULL -- and whose clip is optional)
// (deforming: the _deform entries, whose table holds the two planes of their RtTemporalDeform, whose clip is optional and whose motion table is required; the host
// entry reads the table -- a record's moved word and its triangle range -- and stages the triangle records behind it)
static int temporalAccumulate(RtgpuContext* c, const RtTemporalParams* t, uint32_t width, uint32_t height, PlaneTable b, TemporalMotion motion, bool onDevice, void* streamHandle,
                              bool clipped = false, const RtTemporalClip* clip = nullptr, bool chained = false, const RtTemporalChain* chain = nullptr,
                              bool deforming = false, const RtTemporalDeform* deform = nullptr)
{
    bool history = false;
    int r = checkTemporal(c, t, width, height, b, history, motion); if (r) return r;
    if (clipped || clip)
    {
        if (!clip) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL clip");
        r = checkTemporalClip(clip); if (r) return r;
    }
    if (!clip) b.planes[T_OUT_CONFIDENCE].ptr = nullptr;   // (not written: neither staged nor checked)
    if (chained)
    {
        if (!chain) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL chain");
        if (!b.has(T_VIRTUAL_POSITION) || !b.has(T_CHAIN_LENGTH) || !b.has(T_CHAIN_DISTANCE)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the chain's virtualPosition, chainLength and chainDistance planes are required");
        if (b.has(T_PREV_CHAIN_LENGTH) != history) return fail(RTGPU_ERR_INVALID_ARGUMENT, "prevChainLength goes with the previous frame's buffers: give it beside a history and only there");
    }
    if (deforming)
    {
        if (!deform) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL deform");
        if (!b.has(T_SUB_OBJECT_ID) || !b.has(T_BARYCENTRICS)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the deform's subObjectId and barycentrics planes are required");
        if (!deform->prevTriangles && deform->numPrevTriangles > 0u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "prevTriangles is NULL but numPrevTriangles is not zero");
        if (deform->_pad != 0u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "RtTemporalDeform::_pad must be 0");
        if (onDevice && ((uintptr_t)deform->prevTriangles & 3u)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "prevTriangles must be 4-byte aligned device memory");
        for (uint32_t o = 0; !onDevice && o < motion.numObjects; ++o)
        {
            const RtObjectMotion& record = motion.objects[o];
            if (record.moved > RT_MOTION_DEFORMED) return fail(RTGPU_ERR_INVALID_ARGUMENT, "RtObjectMotion::moved must be 0, 1 or RT_MOTION_DEFORMED");
            if (record.moved == RT_MOTION_DEFORMED && (uint64_t)record._pad[0] + record._pad[1] > deform->numPrevTriangles)
                return fail(RTGPU_ERR_INVALID_ARGUMENT, "a deformed record's triangle range lies outside prevTriangles");
        }
    }
    const size_t n = (size_t)width * height;
    if (onDevice && motion.given && ((uintptr_t)motion.objects & 15u)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the motion table must be 16-byte aligned device memory");
    if (onDevice) { r = checkDevicePlanes(b, n); if (r) return r; }
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = streamHandle ? (hipStream_t)streamHandle : c->lanes[0].stream;
    PlaneTable device = b;
    const void* table = motion.objects;
    const size_t tableBytes = motion.given ? motion.numObjects * sizeof(RtObjectMotion) : 0u, triangleBytes = deforming ? deform->numPrevTriangles * sizeof(RtTriangle) : 0u;
    const float* prevTriangles = deforming ? reinterpret_cast<const float*>(deform->prevTriangles) : nullptr;
    if (!onDevice && triangleBytes)
    {
        // (one blob: the motion table, a multiple of 16 bytes, then the triangle records)
        std::vector<uint8_t> blob(tableBytes + triangleBytes);
        memcpy(blob.data(), motion.objects, tableBytes);
        memcpy(blob.data() + tableBytes, deform->prevTriangles, triangleBytes);
        table = blob.data();
        r = stagePlanes(c, b, n, device, &table, blob.size()); if (r) return r;
        prevTriangles = reinterpret_cast<const float*>((const uint8_t*)table + tableBytes);
    }
    else if (!onDevice) { r = stagePlanes(c, b, n, device, &table, tableBytes); if (r) return r; }
    motion.objects = (const RtObjectMotion*)table;
    r = launchTemporal(c, t, width, height, device, history, stream, motion, clip, chained, deforming ? deform : nullptr, prevTriangles);
    if (r || onDevice) return r;
    HIP_TRY(hipStreamSynchronize(stream));
    return copyPlanesBack(b, device, n);
}

RTGPU_API int rtgpu_temporal_accumulate(RtgpuContext* c, const RtTemporalParams* t, uint32_t width, uint32_t height, const float* color, const float* colorHalf, const float* depth,
                                        const float* normal, const float* position, const float* albedo, const uint32_t* objectId, const float* prevA, const float* prevB,
                                        const float* prevLength, const float* prevDepth, const float* prevNormal, const float* prevPosition, const uint32_t* prevObjectId,
                                        float* outA, float* outB, float* outLength, float* outMotion)
{
    return temporalAccumulate(c, t, width, height, temporalPlanes(color, colorHalf, depth, normal, position, albedo, objectId, prevA, prevB, prevLength, prevDepth, prevNormal,
                                                                  prevPosition, prevObjectId, outA, outB, outLength, outMotion), kNoMotion, false, nullptr);
}

RTGPU_API int rtgpu_temporal_accumulate_moving(RtgpuContext* c, const RtTemporalParams* t, uint32_t width, uint32_t height, const float* color, const float* colorHalf, const float* depth,
                                               const float* normal, const float* position, const float* albedo, const uint32_t* objectId, const float* prevA, const float* prevB,
                                               const float* prevLength, const float* prevDepth, const float* prevNormal, const float* prevPosition, const uint32_t* prevObjectId,
                                               float* outA, float* outB, float* outLength, float* outMotion, const RtObjectMotion* objects, uint32_t numObjects)
{
    return temporalAccumulate(c, t, width, height, temporalPlanes(color, colorHalf, depth, normal, position, albedo, objectId, prevA, prevB, prevLength, prevDepth, prevNormal,
                                                                  prevPosition, prevObjectId, outA, outB, outLength, outMotion), { objects, numObjects, true }, false, nullptr);
}

RTGPU_API int rtgpu_temporal_accumulate_async(RtgpuContext* c, const RtTemporalParams* t, uint32_t width, uint32_t height, const float* color, const float* colorHalf,
                                              const float* depth, const float* normal, const float* position, const float* albedo, const uint32_t* objectId, const float* prevA,
                                              const float* prevB, const float* prevLength, const float* prevDepth, const float* prevNormal, const float* prevPosition,
                                              const uint32_t* prevObjectId, float* outA, float* outB, float* outLength, float* outMotion, void* streamHandle)
{
    return temporalAccumulate(c, t, width, height, temporalPlanes(color, colorHalf, depth, normal, position, albedo, objectId, prevA, prevB, prevLength, prevDepth, prevNormal,
                                                                  prevPosition, prevObjectId, outA, outB, outLength, outMotion), kNoMotion, true, streamHandle);
}

RTGPU_API int rtgpu_temporal_accumulate_moving_async(RtgpuContext* c, const RtTemporalParams* t, uint32_t width, uint32_t height, const float* color, const float* colorHalf,
                                                     const float* depth, const float* normal, const float* position, const float* albedo, const uint32_t* objectId,
                                                     const float* prevA, const float* prevB, const float* prevLength, const float* prevDepth, const float* prevNormal,
                                                     const float* prevPosition, const uint32_t* prevObjectId, float* outA, float* outB, float* outLength, float* outMotion,
                                                     const RtObjectMotion* objects, uint32_t numObjects, void* streamHandle)
{
    return temporalAccumulate(c, t, width, height, temporalPlanes(color, colorHalf, depth, normal, position, albedo, objectId, prevA, prevB, prevLength, prevDepth, prevNormal,
                                                                  prevPosition, prevObjectId, outA, outB, outLength, outMotion), { objects, numObjects, true }, true, streamHandle);
}

// the _clip entries: a table, or NULL and 0 -- then no object moved
static TemporalMotion clipMotion(const RtObjectMotion* objects, uint32_t numObjects) { return !objects && numObjects == 0u ? kNoMotion : TemporalMotion{ objects, numObjects, true }; }

RTGPU_API int rtgpu_temporal_accumulate_clip(RtgpuContext* c, const RtTemporalParams* t, uint32_t width, uint32_t height, const float* color, const float* colorHalf, const float* depth,
                                             const float* normal, const float* position, const float* albedo, const uint32_t* objectId, const float* prevA, const float* prevB,
                                             const float* prevLength, const float* prevDepth, const float* prevNormal, const float* prevPosition, const uint32_t* prevObjectId,
                                             float* outA, float* outB, float* outLength, float* outMotion, const RtObjectMotion* objects, uint32_t numObjects,
                                             const RtTemporalClip* clip, float* outConfidence)
{
    return temporalAccumulate(c, t, width, height, temporalPlanes(color, colorHalf, depth, normal, position, albedo, objectId, prevA, prevB, prevLength, prevDepth, prevNormal,
                                                                  prevPosition, prevObjectId, outA, outB, outLength, outMotion, outConfidence), clipMotion(objects, numObjects), false,
                              nullptr, true, clip);
}

RTGPU_API int rtgpu_temporal_accumulate_clip_async(RtgpuContext* c, const RtTemporalParams* t, uint32_t width, uint32_t height, const float* color, const float* colorHalf,
                                                   const float* depth, const float* normal, const float* position, const float* albedo, const uint32_t* objectId,
                                                   const float* prevA, const float* prevB, const float* prevLength, const float* prevDepth, const float* prevNormal,
                                                   const float* prevPosition, const uint32_t* prevObjectId, float* outA, float* outB, float* outLength, float* outMotion,
                                                   const RtObjectMotion* objects, uint32_t numObjects, const RtTemporalClip* clip, float* outConfidence, void* streamHandle)
{
    return temporalAccumulate(c, t, width, height, temporalPlanes(color, colorHalf, depth, normal, position, albedo, objectId, prevA, prevB, prevLength, prevDepth, prevNormal,
                                                                  prevPosition, prevObjectId, outA, outB, outLength, outMotion, outConfidence), clipMotion(objects, numObjects), true,
                              streamHandle, true, clip);
}

// the _chain entries: chain guides, an optional clip
RTGPU_API int rtgpu_temporal_accumulate_chain(RtgpuContext* c, const RtTemporalParams* t, uint32_t width, uint32_t height, const float* color, const float* colorHalf, const float* depth,
                                              const float* normal, const float* position, const float* albedo, const uint32_t* objectId, const float* prevA, const float* prevB,
                                              const float* prevLength, const float* prevDepth, const float* prevNormal, const float* prevPosition, const uint32_t* prevObjectId,
                                              float* outA, float* outB, float* outLength, float* outMotion, const RtObjectMotion* objects, uint32_t numObjects,
                                              const RtTemporalClip* clip, float* outConfidence, const RtTemporalChain* chain)
{
    return temporalAccumulate(c, t, width, height, temporalPlanes(color, colorHalf, depth, normal, position, albedo, objectId, prevA, prevB, prevLength, prevDepth, prevNormal,
                                                                  prevPosition, prevObjectId, outA, outB, outLength, outMotion, outConfidence, chain), clipMotion(objects, numObjects), false,
                              nullptr, false, clip, true, chain);
}

RTGPU_API int rtgpu_temporal_accumulate_chain_async(RtgpuContext* c, const RtTemporalParams* t, uint32_t width, uint32_t height, const float* color, const float* colorHalf,
                                                    const float* depth, const float* normal, const float* position, const float* albedo, const uint32_t* objectId,
                                                    const float* prevA, const float* prevB, const float* prevLength, const float* prevDepth, const float* prevNormal,
                                                    const float* prevPosition, const uint32_t* prevObjectId, float* outA, float* outB, float* outLength, float* outMotion,
                                                    const RtObjectMotion* objects, uint32_t numObjects, const RtTemporalClip* clip, float* outConfidence,
                                                    const RtTemporalChain* chain, void* streamHandle)
{
    return temporalAccumulate(c, t, width, height, temporalPlanes(color, colorHalf, depth, normal, position, albedo, objectId, prevA, prevB, prevLength, prevDepth, prevNormal,
                                                                  prevPosition, prevObjectId, outA, outB, outLength, outMotion, outConfidence, chain), clipMotion(objects, numObjects), true,
                              streamHandle, false, clip, true, chain);
}

// the _deform entries: a motion table that may hold RT_MOTION_DEFORMED records, the triangle planes and the old triangle records; an optional clip
RTGPU_API int rtgpu_temporal_accumulate_deform(RtgpuContext* c, const RtTemporalParams* t, uint32_t width, uint32_t height, const float* color, const float* colorHalf, const float* depth,
                                               const float* normal, const float* position, const float* albedo, const uint32_t* objectId, const float* prevA, const float* prevB,
                                               const float* prevLength, const float* prevDepth, const float* prevNormal, const float* prevPosition, const uint32_t* prevObjectId,
                                               float* outA, float* outB, float* outLength, float* outMotion, const RtObjectMotion* objects, uint32_t numObjects,
                                               const RtTemporalClip* clip, float* outConfidence, const RtTemporalDeform* deform)
{
    return temporalAccumulate(c, t, width, height, temporalPlanes(color, colorHalf, depth, normal, position, albedo, objectId, prevA, prevB, prevLength, prevDepth, prevNormal,
                                                                  prevPosition, prevObjectId, outA, outB, outLength, outMotion, outConfidence, nullptr, deform),
                              { objects, numObjects, true }, false, nullptr, false, clip, false, nullptr, true, deform);
}

RTGPU_API int rtgpu_temporal_accumulate_deform_async(RtgpuContext* c, const RtTemporalParams* t, uint32_t width, uint32_t height, const float* color, const float* colorHalf,
                                                     const float* depth, const float* normal, const float* position, const float* albedo, const uint32_t* objectId,
                                                     const float* prevA, const float* prevB, const float* prevLength, const float* prevDepth, const float* prevNormal,
                                                     const float* prevPosition, const uint32_t* prevObjectId, float* outA, float* outB, float* outLength, float* outMotion,
                                                     const RtObjectMotion* objects, uint32_t numObjects, const RtTemporalClip* clip, float* outConfidence,
                                                     const RtTemporalDeform* deform, void* streamHandle)
{
    return temporalAccumulate(c, t, width, height, temporalPlanes(color, colorHalf, depth, normal, position, albedo, objectId, prevA, prevB, prevLength, prevDepth, prevNormal,
                                                                  prevPosition, prevObjectId, outA, outB, outLength, outMotion, outConfidence, nullptr, deform),
                              { objects, numObjects, true }, true, streamHandle, false, clip, false, nullptr, true, deform);
}

// off by default; with it on, rtgpu_update_mesh keeps what rtgpu_denoise_temporal[_clip] needs to follow the mesh (rt_runtime_refit.inl)
RTGPU_API int rtgpu_set_deform_tracking(RtgpuContext* c, int enable)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    RT_FAN_OUT(c, rtgpu_set_deform_tracking(peer, enable));
    c->temporal.trackDeform = enable != 0;
    return RTGPU_OK;
}

RTGPU_API int rtgpu_temporal_reset(RtgpuContext* c)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    c->temporal.have = false;
    return RTGPU_OK;
}

// rtgpu_denoise_temporal / rtgpu_denoise_temporal_async: outHost or outDevice (outVariance is memory of the same kind, written with `v` only)
// clip (may be NULL: the call without) and outConfidence (optional, written with a clip only): memory of the result's kind
// chained: rtgpu_denoise_temporal_chain[_async], whose guides are the chain guides of `chain` (its own argument, never rtgpu_set_guide_chain's) with the virtual position
static int denoiseTemporalFrame(RtgpuContext* c, const RtTemporalParams* t, const RtDenoiseVarParams* v, const RtPassParams* guideParams, float* outHost, float* outDevice,
                                float* outVariance, void* streamHandle, const RtTemporalClip* clip = nullptr, float* outConfidence = nullptr, bool chained = false,
                                const RtAovChain* chain = nullptr)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (!t) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    int r = checkTemporalParams(t, false); if (r) return r;
    if (v) { r = checkDenoiseVarParams(v); if (r) return r; }
    if (clip) { r = checkTemporalClip(clip); if (r) return r; }
    if (c->raySource.any()) return fail(RTGPU_ERR_UNSUPPORTED, "temporal accumulation reprojects through the camera's worldToScreen, and a ray source has none: clear it, or call rtgpu_temporal_accumulate on planes of your own");
    // (before anything is submitted or the history touched) reprojecting a reflection needs the virtual motion of the mirrored point
    if (chained)
    {
        if (!chain) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL chain");
        if (chain->maxChain > RT_AOV_CHAIN_MAX) return fail(RTGPU_ERR_INVALID_ARGUMENT, "maxChain must be 0..16");
        if (chain->flags != 0u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "RtAovChain::flags must be 0");
    }
    else if (c->chain.guide) return fail(RTGPU_ERR_UNSUPPORTED, "temporal accumulation does not reproject through a guide chain: clear it with rtgpu_set_guide_chain(ctx, NULL), or call rtgpu_denoise_temporal_chain");
    if (!clip) outConfidence = nullptr;
    const bool stagesConfidence = outConfidence && outHost;
    // a mesh was deformed under a snapshot since the history was stored (rtgpu_set_deform_tracking), and this call will reach that history: it follows the
    // deformation, with two guide planes more.  (Decided here, before the planes are laid out, by what the lines below decide about the history.)
    const std::vector<RtObject>& objects = c->updatable.objects;
    bool follows = false;
    {
        const RtgpuContext::Temporal& h = c->temporal;
        if (!chained && h.have && !h.chained && h.capacity >= (size_t)c->width * c->height && h.movedSince && !objects.empty() && h.then.size() == objects.size() && c->updatable.deformSnapshot)
            for (const ObjectThen& then : h.then) follows = follows || then.deformed != 0u;
    }
    FrameStep f;
    // its own planes: the accumulated pair 3 + 3, its length 1 (and the host entry's confidence 1; behind them the chained call's chain planes 1 + 1 + 3)
    // (or the following call's triangle planes 1 + 2)
    r = beginFrame(c, guideParams, outHost, outDevice, outVariance, v != nullptr, streamHandle, 5u, (stagesConfidence ? 8u : 7u) + (chained ? 5u : 0u) + (follows ? 3u : 0u), f,
                   outDevice ? outConfidence : nullptr, chained ? chain : nullptr, follows); if (r) return r;
    float* const dA = f.extra; float* const dB = dA + 3u * f.stride; float* const dLength = dB + 3u * f.stride;
    float* const dConfidence = stagesConfidence ? dLength + f.stride : outConfidence;
    RtgpuContext::Temporal& h = c->temporal;
    if (h.capacity < f.pixels) h.have = false;
    if (!chained && h.chained) h.have = false;   // a history over chain guides holds chain lengths these entries never knew: to them it is no history, and they overwrite it
    r = ensureScratch(c, h.records, h.capacity, f.pixels, 8u); if (r) return r;   // two sets of four planes of records
    float4* const from = h.records + (size_t)h.current * 4u * h.capacity; float4* const to = h.records + (size_t)(h.current ^ 1u) * 4u * h.capacity;
    TemporalIn in = { c->sum, c->secondary, f.depth, f.normal, f.position, (t->flags & RT_DENOISE_DEMODULATE) ? f.albedo : nullptr, f.id, nullptr, nullptr, nullptr, nullptr };
    if (h.have) { in.recA = from; in.recB = from + h.capacity; in.recN = from + 2u * h.capacity; in.recP = from + 3u * h.capacity; }
    const TemporalOut res = { dA, dB, dLength, nullptr, v ? nullptr : f.out, to, to + h.capacity, to + 2u * h.capacity, to + 3u * h.capacity };
    const RtObjectMotion* motion = nullptr;
    if (h.have && h.movedSince && !objects.empty() && h.then.size() == objects.size())
    {
        // objects were updated since the history was stored: where each was then.  (The table is small and the copy is not ordered on a stream: the kernel
        // of the previous call may still read the last one.)
        std::vector<RtObjectMotion> table;
        buildMotionTable(objects, h.then, table, follows ? &c->updatable.meshTable : nullptr);
        HIP_TRY(hipEventSynchronize(c->denoise.done));
        r = ensureScratch(c, h.motion, h.motionCapacity, table.size()); if (r) return r;
        HIP_TRY(rtMemcpy(h.motion, table.data(), table.size() * sizeof(RtObjectMotion), hipMemcpyHostToDevice));
        motion = h.motion;
    }
    TemporalClipLaunch clipped;
    if (clip) { r = temporalClipLaunch(c, clip, f.pixels, h.have, dConfidence, clipped); if (r) return r; }
    const TemporalChainPlanes chainPlanes = { f.virtualPosition, f.chainLength, f.chainDistance };
    const TemporalDeformLaunch deforming = { f.subObjectId, f.barycentrics, reinterpret_cast<const float*>(c->updatable.deformSnapshot), c->sceneDev.numTriangles };
    launchTemporalKernel(in, res, c->width, c->height, temporalFrame(t, h.worldToScreen, h.sampleOffset, h.have), f.stream, motion, (uint32_t)objects.size(), clip ? &clipped : nullptr,
                         chained ? &chainPlanes : nullptr, follows && motion ? &deforming : nullptr);
    r = recordDone(c, f.stream); if (r) return r;
    r = markSumRead(c, f.stream); if (r) return r;
    // this frame is the next call's history
    h.current ^= 1u; h.have = true; h.chained = chained;
    h.movedSince = false;
    h.then.resize(objects.size());
    for (size_t o = 0; o < objects.size(); ++o) { h.then[o].id = (uint32_t)o; h.then[o].deformed = 0u; memcpy(h.then[o].transform, objects[o].transform, sizeof(h.then[o].transform)); }
    std::fill(c->updatable.deformState.begin(), c->updatable.deformState.end(), (uint8_t)0u);   // a new history: every snapshot shows a mesh of a frame it no longer holds
    memcpy(h.worldToScreen, guideParams->camera.worldToScreen, sizeof(h.worldToScreen));
    h.sampleOffset[0] = guideParams->sampleOffset[0]; h.sampleOffset[1] = guideParams->sampleOffset[1];
    if (v)
    {
        AtrousPlan plan = atrousPlan(v);
        plan.flags |= RT_DENOISE_INPUT_PREPARED; plan.colorScale = 1.0f;
        r = launchAtrous(c, plan, c->width, c->height, filterPlanes(dA, dB, f.depth, f.normal, f.position, f.albedo, f.out, f.variance), f.stream, false); if (r) return r;
    }
    r = finishFrame(c, f); if (r) return r;
    if (stagesConfidence) HIP_TRY(rtMemcpy(outConfidence, dConfidence, f.pixels * sizeof(float), hipMemcpyDeviceToHost));   // (behind finishFrame's wait for the stream)
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

RTGPU_API int rtgpu_denoise_temporal_clip(RtgpuContext* c, const RtTemporalParams* t, const RtDenoiseVarParams* v, const RtPassParams* guideParams, float* outRGB, float* outVariance,
                                          const RtTemporalClip* clip, float* outConfidence)
{
    return denoiseTemporalFrame(c, t, v, guideParams, outRGB, nullptr, outVariance, nullptr, clip, outConfidence);
}

RTGPU_API int rtgpu_denoise_temporal_clip_async(RtgpuContext* c, const RtTemporalParams* t, const RtDenoiseVarParams* v, const RtPassParams* guideParams, float* outRGB, float* outVariance,
                                                const RtTemporalClip* clip, float* outConfidence, void* streamHandle)
{
    return denoiseTemporalFrame(c, t, v, guideParams, nullptr, outRGB, outVariance, streamHandle, clip, outConfidence);
}

RTGPU_API int rtgpu_denoise_temporal_chain(RtgpuContext* c, const RtTemporalParams* t, const RtDenoiseVarParams* v, const RtPassParams* guideParams, const RtAovChain* chain, float* outRGB,
                                           float* outVariance, const RtTemporalClip* clip, float* outConfidence)
{
    return denoiseTemporalFrame(c, t, v, guideParams, outRGB, nullptr, outVariance, nullptr, clip, outConfidence, true, chain);
}

RTGPU_API int rtgpu_denoise_temporal_chain_async(RtgpuContext* c, const RtTemporalParams* t, const RtDenoiseVarParams* v, const RtPassParams* guideParams, const RtAovChain* chain,
                                                 float* outRGB, float* outVariance, const RtTemporalClip* clip, float* outConfidence, void* streamHandle)
{
    return denoiseTemporalFrame(c, t, v, guideParams, nullptr, outRGB, outVariance, streamHandle, clip, outConfidence, true, chain);
}
