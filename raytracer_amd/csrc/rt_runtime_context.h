// rt_runtime_context.h -- what every part of the host runtime shares: the staging copies, error reporting (HIP_TRY), the context and its batch lanes,
// the free helpers of their device memory, launch timing and the stream pool.  Included by rt_runtime.hip.
#pragma once
#include <mutex>

// =====================================================================================================
// Host side of the C-ABI
// =====================================================================================================
// Synchronous copies between HOST memory the caller owns and the device.  HIP would page-lock a large pageable range on the fly and keep the
// registration cached; the caller then frees the range (a std::vector of the host mirror, a numpy array) and a later allocation lands on the
// same addresses -- on some boxes of the pool the HSA runtime aborts the process a few dozen contexts later (no message; it went away with
// this).  So anything above 64 KB that is not page-locked already (hipHostMalloc / hipHostRegister: the viewport's sum bitmaps) travels
// through a page-locked staging buffer of the library, 8 MB at a time.
// one staging buffer (and its lock) per device: contexts on different devices copy side by side (rtgpu_create_multi).  8 MB of page-locked memory
// per device used, kept for the life of the process (freeing it from an exit handler would race the HIP runtime's own teardown)
struct Staging { std::mutex mutex; void* buffer = nullptr; };
static std::mutex gStagingTableMutex;
static std::unordered_map<int, Staging*> gStaging;
static const size_t kStagingBytes = (size_t)8 << 20;
static Staging* stagingOfCurrentDevice()
{
    int device = 0;
    (void)hipGetDevice(&device);
    std::lock_guard<std::mutex> lock(gStagingTableMutex);
    Staging*& s = gStaging[device];
    if (!s) s = new Staging();
    return s;
}
static bool hostRangeIsPageLocked(const void* p)
{
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // ordinary pageable memory: "invalid value"
    return attr.type == hipMemoryTypeHost;
}
static hipError_t rtMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind)
{
    if (bytes == 0) return hipSuccess;
    const bool h2d = kind == hipMemcpyHostToDevice, d2h = kind == hipMemcpyDeviceToHost;
    if ((!h2d && !d2h) || bytes <= ((size_t)64 << 10) || hostRangeIsPageLocked(h2d ? src : dst)) return hipMemcpy(dst, src, bytes, kind);
    Staging* const st = stagingOfCurrentDevice();
    std::lock_guard<std::mutex> lock(st->mutex);
    if (!st->buffer)
    {
        const hipError_t e = hipHostMalloc(&st->buffer, kStagingBytes, hipHostMallocPortable);
        if (e != hipSuccess) { st->buffer = nullptr; return e; }
    }
    for (size_t done = 0; done < bytes; done += kStagingBytes)
    {
        const size_t n = bytes - done < kStagingBytes ? bytes - done : kStagingBytes;
        if (h2d) memcpy(st->buffer, static_cast<const char*>(src) + done, n);
        const hipError_t e = h2d ? hipMemcpy(static_cast<char*>(dst) + done, st->buffer, n, kind) : hipMemcpy(st->buffer, static_cast<const char*>(src) + done, n, kind);
        if (e != hipSuccess) return e;
        if (d2h) memcpy(static_cast<char*>(dst) + done, st->buffer, n);
    }
    return hipSuccess;
}

static thread_local std::string gLastError;

static int fail(int code, const std::string& msg) { gLastError = msg; return code; }

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                           \
            return fail(_e == hipErrorOutOfMemory ? RTGPU_ERR_OUT_OF_MEMORY : RTGPU_ERR_DEVICE,          \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                             \
    } while (0)

enum KernelClass { KC_GENERATE = 0, KC_TRACE, KC_SHADE, KC_ACCUMULATE, KC_RETRACE, KC_TAIL, KC_COUNT };
static const char* const kKernelClassNames[RTGPU_NUM_KERNEL_CLASSES] = { "generate", "trace", "shade", "accumulate", "retrace", "tail", "", "" };

#define RT_SEED_RING 128

struct CtxPending { DevPass pass; std::vector<uint32_t> seeds; };
#define RT_VCM_MAX_BATCH 8

#define RT_MAX_LANES 6
struct BatchLane
{
    hipStream_t stream = nullptr;
    Paths paths = { nullptr, 0, 0 };
    uint32_t* queues[2] = { nullptr, nullptr };
    uint32_t* shadowQueues[2] = { nullptr, nullptr };   // capacity * maxLights NEE ray requests each, ping-pong per bounce
    uint32_t* exactQueue = nullptr;        // closest-hit rays / any-hit requests the 4-wide walks hand to the binary-tree kernel
    uint32_t* exactShadowQueue = nullptr;
    // dense path state (rt_dense.inl, LightSamplingStrategy::Single): the second arena of the ping-pong, the parked radiance of
    // finished paths, per bounce the live / zombie counts of the arena's regions (2 * RT_DENSE_SHARDS words per bounce)
    Paths paths2 = { nullptr, 0, 0 };
    float4* home = nullptr; size_t homeCapacity = 0;
    uint32_t* denseCounts = nullptr;
    // per-batch work counters, RT_LANE_COUNT_PLANES planes of (maxDepth + 2) uint32, zeroed once per batch (one word of each plane per bounce, so that no
    // reset ever races with a reader); LaneCounts names the planes
    uint32_t* queueCounts = nullptr;
    uint32_t queueCountCapacity = 0;
    hipEvent_t accumulated = nullptr;   // recorded after the lane's k_accumulate
};

// One trace step of a launch sequence, carried out by launchTraceStep (rt_runtime_render.inl); LaneCounts fills the first two groups for a bounce of a lane
struct TraceStep
{
    // the work: closest-hit rays and any-hit requests (either queue may be null) over `paths`, taken through `cursor`
    hipStream_t stream; unsigned long long* counters; Paths paths;
    const uint32_t* queue = nullptr; const uint32_t* queueCount = nullptr; const uint32_t* shadowQueue = nullptr; const uint32_t* shadowCount = nullptr; uint32_t* cursor = nullptr;
    // the hand-over of the 4-wide walks: what they leave to the re-trace launch, and its work cursor
    uint32_t* exactQueue = nullptr; uint32_t* exactCount = nullptr; uint32_t* exactShadowQueue = nullptr; uint32_t* exactShadowCount = nullptr; uint32_t* exactCursor = nullptr;
    // the call's policy
    float shadowOffset = 0.0001f;              // any-hit rays start this far along their direction (TravTuning::shadowOffset)
    const uint32_t* denseCounts = nullptr; uint32_t denseShardCapacity = 0u;   // dense path state: the closest-hit rays are the live paths of the arena's regions (no queue)
    bool mayTraceUndecidedRaysItself = true;   // a 4-wide walk may trace what it does not decide in its own blocks (launchTraceWide's policy decides whether it does)
    uint32_t bounce = 0u;                      // for the policies that depend on it (the block-local second walk, the packet walk of camera rays)
    uint4* rayCounts = nullptr;                // binary walk only: every closest-hit ray's own test counts (TravTuning::rayCounts); makes the walk a counting one
    BeamLists beam = {};                       // bounce 0 of a dense batch from a still camera: the lists k_trace_packet may scan (entries == nullptr: none)
};

// LaneCounts names the first six; eight are allocated and zeroed: 32 bytes per bounce are a multiple of 16 at any depth, which the runtime's memset fills with
// ONE kernel (the 24 bytes of six planes take a second fill kernel per batch at every odd maxDepth: the launch listings of tools/launch_order.py show it)
#define RT_LANE_COUNT_PLANES 8u
static size_t laneCountBytes(const BatchLane& l) { return (size_t)RT_LANE_COUNT_PLANES * l.queueCountCapacity * sizeof(uint32_t); }

// the planes of BatchLane::queueCounts in use, built once per flush; index each with the bounce
struct LaneCounts
{
    const BatchLane& lane;
    uint32_t* pathCounts; uint32_t* shadowCounts; uint32_t* cursors;              // path queues, next-event request queues, the traversal launches' work cursors
    uint32_t* exactCounts; uint32_t* exactShadowCounts; uint32_t* exactCursors;   // what the 4-wide walks hand to the re-trace launch, and its cursors
    explicit LaneCounts(const BatchLane& l)
        : lane(l), pathCounts(l.queueCounts), shadowCounts(l.queueCounts + 1 * l.queueCountCapacity), cursors(l.queueCounts + 2 * l.queueCountCapacity),
          exactCounts(l.queueCounts + 3 * l.queueCountCapacity), exactShadowCounts(l.queueCounts + 4 * l.queueCountCapacity),
          exactCursors(l.queueCounts + 5 * l.queueCountCapacity) {}
    // the work of bounce d: {closest-hit rays of bounce d, next-event requests of bounce d - 1}, whichever exist, and the bounce's work cursor
    void queuesOf(TraceStep& s, uint32_t d, bool haveClosest, bool haveShadow) const
    {
        s.queue = haveClosest ? lane.queues[d & 1u] : nullptr; s.queueCount = haveClosest ? pathCounts + d : nullptr;
        s.shadowQueue = haveShadow ? lane.shadowQueues[(d - 1u) & 1u] : nullptr; s.shadowCount = haveShadow ? shadowCounts + (d - 1u) : nullptr;
        s.cursor = cursors + d;
    }
    // the hand-over of bounce d
    void handOverOf(TraceStep& s, uint32_t d) const
    {
        s.exactQueue = lane.exactQueue; s.exactCount = exactCounts + d; s.exactShadowQueue = lane.exactShadowQueue; s.exactShadowCount = exactShadowCounts + d;
        s.exactCursor = exactCursors + d;
    }
};

// The arena of a walk over the library's own rays (ray queries, AOVs); `counts` and `counters` are allocated once by the owner and outlive a growth
struct WalkArena
{
    Paths paths = { nullptr, 0, 0 };          // maxLights = 1; capacity = the rays of one chunk
    uint32_t* queue = nullptr;                // the chunk's closest-hit rays or any-hit requests
    uint32_t* exactQueue = nullptr; uint32_t* exactShadowQueue = nullptr;   // what the 4-wide walks hand to the re-trace launch
    uint32_t* counts = nullptr;               // QC_WORDS work counts (QC_*, rt_runtime_query.inl)
    unsigned long long* counters = nullptr;   // 16 x u64, the layout of RtCounters
};

struct RtgpuContext
{
    int device = 0;
    uint32_t numCUs = 256;

    // scene (device copies); sceneDev holds DEVICE pointers
    RtSceneDesc sceneDev;
    std::vector<void*> sceneAllocs;
    bool sceneReady = false;
    uint32_t numLights = 0;
    // rtgpu_update_objects: host copies of what an update is checked against and permutes, and the room the upload left for a top level of another size
    struct Updatable
    {
        std::vector<RtObject> objects; std::vector<RtLight> lights;   // as they stand on the device
        std::vector<WideLevel> levels;                                // WideScene::levels as they stand on the device (empty: the scene has no two-level 4-wide trees)
        WideScene wide2 = {};                                         // the device arrays of those trees (RtgpuContext::wide2 is this, or empty while the top level could not be built)
        uint32_t maxMeshDepth = 0, topNodeCapacity = 0;               // deepest mesh tree; nodes the device's top-level array holds
        uint32_t topWideNodeCapacity = 0;                             // 4-wide nodes the top level's slab behind the mesh levels holds
        uint64_t meshNodeBytes = 0, meshGateBytes = 0;                // the mesh levels' share of walkNodeBytes / walkLeafBoxBytes[RTGPU_WALK_WIDE2]
        RtUpdateInfo info = {};                                       // rtgpu_get_update_info
        // rtgpu_update_mesh (rt_runtime_refit.inl): per mesh its plan and 4-wide level (rt_scene_prepare.h) and, from its first update on, the device copies
        // of its triangles' vertex indices (leaf order) and of the positions (rtgpu_update_mesh_device: of the normals and tangents it was given too); the device
        // arrays live in sceneAllocs and go with the scene
        struct Mesh
        {
            MeshRefitPlan plan; PreparedScene::MeshLevel level;
            RtVertexIndices* indices = nullptr; float* positions = nullptr; RtVertexShading* shading = nullptr; uint32_t* levelFirst = nullptr;
            float* normals = nullptr; float* tangents = nullptr;
        };
        std::vector<Mesh> meshes; std::vector<RtMesh> meshTable;
        std::vector<RtVertexIndices> vertexIndices;                   // the caller's, as uploaded: every update takes the new root box from them before it writes; a mesh's first update copies its share to the device
        const uint32_t* wide2SlotNode = nullptr; const uint32_t* wideSlotNode = nullptr;   // per 4-wide record the mesh node whose box it holds (PreparedScene), on the device
        // rtgpu_set_deform_tracking: the triangle records deformed meshes had when the temporal history was stored -- one device array over the scene's triangle
        // numbering, made with the first snapshot, in sceneAllocs -- and per mesh what happened since that history: 0 untouched, 1 its range of the array holds
        // its snapshot, 2 it was updated without one (its pixels start)
        RtTriangle* deformSnapshot = nullptr; std::vector<uint8_t> deformState;
        RefitCheckRecord* refitCheck = nullptr;                       // what k_refit_check found (rtgpu_update_mesh_device), in sceneAllocs
    } updatable;
    hipEvent_t refitOrder = nullptr;   // rtgpu_update_mesh_device: puts the refit's stream behind the caller's

    // film
    uint32_t width = 0, height = 0;
    RtgpuShard shard = { 0, 1 };
    // rtgpu_create_multi: the context the caller holds renders shard 0 and owns one more context per further device (shards 1..);
    // every call fans out, the read-back calls gather the peers' tiles into this context's sum buffers first (rt_multi.inl)
    std::vector<RtgpuContext*> peers;
    bool isPeer = false;
    bool stagedGather = false;         // no peer access between the devices (or RTGPU_MULTI_STAGED=1): hipMemcpyPeerAsync into staging buffers, then the gather
    float* gatherStage = nullptr; size_t gatherStageFloats = 0;
    bool axisParallelSun = false;      // the scene has a delta directional light along a coordinate plane / axis: its next-event rays fill the re-trace launches (full grid there)
    RtMultiInfo multiInfo = {};        // rtgpu_get_multi_info: which gather was chosen and why, its timings
    float* sum = nullptr;
    float* secondary = nullptr;
    uint32_t* slotPixel = nullptr;
    uint32_t numSlots = 0;
    std::vector<uint8_t> activeMask;   // adaptive rendering: 1 = pixel inside an active block; empty = whole image

    // Batch lanes.  Every batch of passes runs on ONE lane = its own stream, path-state arena, queues and work
    // counters; consecutive batches alternate lanes, so the drain of a persistent traversal launch (a handful of
    // rays with thousands of steps keep a few waves busy for milliseconds -- an axis-parallel NEE ray that grazes
    // a plane of box faces can take 30 000) overlaps with the next batch's kernels instead of idling the chip.
    // Only k_accumulate is ordered across lanes (an event): the film is summed in pass order.
    BatchLane lanes[RT_MAX_LANES];
    uint32_t numLanes = 4;
    bool lanesChosen = false;          // by RTGPU_LANES or rtgpu_set_concurrency; otherwise shards (< 1.1 M owned pixels) run 4 lanes
    uint32_t nextLane = 0;
    int lastAccumulateLane = -1;
    uint32_t traversalStackNeed = 0;   // deepest top-level + mesh stack the uploaded scene can produce
    WideBvh wide;                      // 4-wide collapse of the same tree (rt_trace_wide.inl); nodes == nullptr: none
    WideScene wide2;                   // two-level scenes: 4-wide top-level tree over 4-wide mesh trees (rt_trace_wide2.inl); nodes == nullptr: none
    bool wide2Allowed = true;          // RTGPU_WIDE2=0: two-level scenes keep the binary walk
    uint64_t walkNodeBytes[3] = { 0, 0, 0 }, walkLeafBoxBytes[3] = { 0, 0, 0 }, walkTriangleBytes = 0;   // rtgpu_get_walk_info, per RTGPU_WALK_* kernel
    bool wideAllowed = true;           // RTGPU_WIDE=0: single-mesh scenes walk the binary tree (k_trace) even with the intersection counters off
    bool denseAllowed = true;          // RTGPU_NO_DENSE=1: path state stays in the pixel's slot for the whole path (the first layout)
    TravTuning tune = { 28u, 32u, 0.0001f, nullptr, nullptr, RT_ABORT_CLOSEST_AFTER, nullptr, 0u };   // scheduling: measured plateau on MI355X (profiles/r01_tuning_sweep.txt)
    uint32_t travBlocksPerCU = 0;      // 0 = default
    int32_t tailBounce = -1;           // rtgpu_set_schedule: the bounce at which a dense batch hands over to k_tail (rt_tail.hip); 0 = never, -1 = policy
    int32_t localRetrace = -1;         // rtgpu_set_schedule: the 4-wide walks trace their undecided rays themselves; 0 / 1, -1 = policy
    int leanScene = 0;                 // the scene class of rt_device_core.h (kLean): 0 anything, 1 lean, 2 lean + textures, 3 anything without textures, 4 lean + simple bitmaps only
    bool countIntersections = false;   // box / triangle test counters: RT_ENABLE_INTERSECTION_COUNTERS of the reference, off by default like there (Core/Config.h:4);
                                       // rtgpu_set_intersection_counters, or RTGPU_INTERSECTION_COUNTERS=1 for the default of new contexts
    unsigned long long* counters = nullptr;   // 16 x u64
    uint32_t* deviceFlags = nullptr;          // page-locked, device-visible: kernels raise [0] when a region of a dense arena overflows; checked by every synchronising call

    // passes queued by rtgpu_render_pass and not yet submitted: up to passBatch of them ride through ONE launch
    // sequence (their paths are simply more slots), which amortises the per-launch tail of the persistent kernels
    std::vector<CtxPending> pending;
    uint32_t passBatch = 8;
    bool passBatchFromEnv = false;     // otherwise small frames / small shards (< 400 k owned pixels) batch 16 passes
    // A caller that streams passes (no read-back in between) gets larger batches: after every submitted batch of a full-size frame
    // the next one grows by 8 passes up to 24 (8 -> 2100, 16 -> 2125-2190, 24 -> 2195-2210 Msamples/s over 256 passes); any
    // synchronising call starts over at the base size, so a caller that renders few passes between read-backs keeps the small batches.
    uint32_t passBatchBase = 8;
    size_t laneBudgetBytes = (size_t)32 << 30;   // device memory one batch lane may take: 32 GB, less on a device that could not hold four such lanes
    uint32_t batchesAtThisSize = 0;    // full batches submitted at the current passBatch
    uint32_t batchesSinceSync = 0;     // batches submitted since the last synchronising call (their lanes are busy)
    DevPass* passRingDev = nullptr;
    DevPass* passRingHost = nullptr;    // pinned

    // per-pass seed ring
    uint32_t* seedRingDev = nullptr;
    uint32_t* seedRingHost = nullptr;   // pinned
    hipEvent_t seedEvents[RT_SEED_RING];
    bool seedEventUsed[RT_SEED_RING];
    uint32_t seedCursor = 0;

    bool plainPathTracer = false;      // RT_INTEGRATOR_PATH_TRACER: k_shade<false, true>
    bool lightTracer = false;          // RT_INTEGRATOR_LIGHT_TRACER: the light stage of rt_vcm.inl without MIS (k_lt_shade)
    int debugMode = -1;                // RT_INTEGRATOR_DEBUG: DebugRenderingMode, k_debug_shade after the primary rays' traversal
    // bidirectional integrator (rt_vcm.inl) on lane 0's stream.  Like PathTracerMIS passes, VCM passes ride through the launch
    // sequence in batches: the light stages of the batch first (pass j's photons are the merge set of pass j+1, so the hash grids
    // of passes 1.. are built between the stages), then the camera stages -- the same results as one pass at a time.
    struct Vcm
    {
        bool enabled = false;
        RtVcmParams params;
        float mergingRadiusVC = 0.0f, mergingRadiusVM = 0.0f;
        Paths lightPaths = { nullptr, 0, 0 }, cameraPaths = { nullptr, 0, 0 };
        VcmArena arena = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0 };
        uint32_t* mergeQueue = nullptr; uint32_t* connectQueue = nullptr;
        uint32_t* overflowQueue = nullptr;   // closest-hit rays k_trace hands to k_trace_monster
        uint32_t* exactQueue = nullptr; uint32_t* exactShadowQueue = nullptr;   // what the 4-wide walks hand to the binary-tree kernel (as BatchLane's)
        uint32_t traceSerial = 0;            // trace launches since the counters were zeroed: every launch has its own hand-over counters
        uint32_t* queues[4] = { nullptr, nullptr, nullptr, nullptr };          // light ping-pong, camera ping-pong
        uint32_t* shadowQueues[4] = { nullptr, nullptr, nullptr, nullptr };
        uint32_t* counts = nullptr;                                               // VCP_NUM_PLANES planes of RT_VCM_COUNT_PLANE words (VcmCountPlane, rt_runtime_vcm.inl)
        DevPass* passDev = nullptr; uint32_t* seedDev = nullptr;                 // RT_VCM_MAX_BATCH entries each
        VcmDev* devsDev = nullptr; HashGridView* gridsDev = nullptr;
        VcmPhotonGrid grids[RT_VCM_MAX_BATCH];                                    // merge set of pass j of the batch
        bool havePhotons = false;     // the arena holds the photons of the pass before the next one ...
        uint32_t lastPhotonPass = 0;  // ... in the storage of this pass of the last batch
        uint32_t requestsPerVertex = 0;
        uint32_t batch = 1, batchCapacity = 0;   // passes per launch sequence; what the arenas were sized for
        // passes queued by rtgpu_render_pass and not yet submitted
        struct Pending { RtPassParams params; std::vector<uint32_t> seeds; };
        std::vector<Pending> pending;
    } vcm;

    // batched ray queries (rtgpu_trace_rays): a path-state arena, queues, work counts and counters of their own -- never a lane's, never c->counters
    struct Query
    {
        WalkArena arena;
        float4* stagedRays = nullptr; float4* stagedHits = nullptr; float4* stagedSurfaces = nullptr; uint32_t* stagedOccluded = nullptr;   // rtgpu_trace_rays' device copies
        hipEvent_t done = nullptr;                // recorded behind every query: the next one (whatever its stream), a new arena and a new scene wait for it
    } query;

    // path records (rtgpu_record_paths): the slot-per-pixel pipeline over caller-chosen pixels, on an arena, queues, work counts, counters and per-pass
    // constants of its own -- never a lane's, never c->counters, never the seed ring
    struct Recorder
    {
        BatchLane lane;                           // arena, queues and work counts as a batch lane holds them (no second arena, no stream or event of its own)
        uint32_t* slotPixel = nullptr;            // slot -> pixel of the chunk being recorded
        float4* records = nullptr; size_t recordCapacity = 0;   // per slot: 7 float4 per stored vertex, then {numVertices, terminationReason} (rt_shade.inl)
        float4* infos = nullptr;                  // two per slot: RtPathInfo
        unsigned long long* counters = nullptr;   // 16 x u64
        DevPass* passDev = nullptr; uint32_t* seedDev = nullptr;   // the recorded pass
    } recorder;

    // AOVs (rtgpu_render_aovs): the first bounce of the slot-per-pixel pipeline over a chunk of the frame's pixels, on an arena, queues, work counts and counters
    // of its own -- never a lane's, never c->counters, never the seed ring
    struct Aov
    {
        WalkArena arena;                          // capacity = the pixels of one chunk; the queue is the chunk's primary rays (the identity); the counters are never read
        uint32_t* slotPixel = nullptr;            // slot -> pixel of the chunk (k_aov_pixels)
        uint4* rayCounts = nullptr;               // per slot what the counting walk counted for its ray (TravTuning::rayCounts); allocated with the first cost plane
        uint32_t* staged = nullptr; size_t stagedWords = 0;   // rtgpu_render_aovs' device copy of a chunk's planes
        DevPass* passDev = nullptr; uint32_t* seedDev = nullptr;   // the pass whose primary rays are traced
        // pass constants and seeds travel through a small ring of page-locked records: an asynchronous call returns before its copy has run
        static const uint32_t kRing = 4;
        char* ringHost = nullptr; hipEvent_t ringCopied[kRing] = { nullptr, nullptr, nullptr, nullptr }; uint32_t ringCursor = 0;
        hipEvent_t done = nullptr;                // recorded behind every call: the next one (whatever its stream) and a new arena wait for it
    } aov;

    // guide chains (rtgpu_render_aovs_chain): the slot-per-pixel bounce loop over a chunk of the frame's pixels with k_shade_chain, then k_aov_resolve_chain; arena,
    // queues, work counts, counters, pass constants and staging of its own -- never a lane's, the recorder's or the first-hit call's
    struct Chain
    {
        BatchLane lane;                           // arena (one request record pair per slot, never written), queues and work counts as a batch lane holds them
        uint32_t* slotPixel = nullptr;            // slot -> pixel of the chunk (k_aov_pixels)
        uint32_t* staged = nullptr; size_t stagedWords = 0;   // rtgpu_render_aovs_chain's device copy of a chunk's planes
        unsigned long long* counters = nullptr;   // 16 x u64, never read
        DevPass* passDev = nullptr; uint32_t* seedDev = nullptr;   // the pass whose paths are followed
        static const uint32_t kRing = 4;          // pass constants and seeds travel as the first-hit call's do (Aov::ringHost)
        char* ringHost = nullptr; hipEvent_t ringCopied[kRing] = { nullptr, nullptr, nullptr, nullptr }; uint32_t ringCursor = 0;
        hipEvent_t done = nullptr;                // recorded behind every call: the next one (whatever its stream), a new arena and a new scene wait for it
        bool guide = false; uint32_t guideMaxChain = 0;   // rtgpu_set_guide_chain: the frame step (beginFrame) renders its guides through the chain call
    } chain;

    // the a-trous filter (rtgpu_filter_atrous, rtgpu_denoise; rt_runtime_denoise.inl): scratch of its own, grown on use, freed with the context
    struct Denoise
    {
        float4* records = nullptr; size_t capacity = 0;   // four planes of `capacity` 16-byte records: normals + valid, positions, two colour buffers (64 bytes per pixel)
        float* io = nullptr; size_t ioFloats = 0;         // device copies of the host entries' inputs and output; rtgpu_denoise's guide planes
        hipEvent_t done = nullptr;                        // recorded behind every call: the next one (whatever its stream) and new scratch wait for it
        hipEvent_t sumRead = nullptr; bool sumReadPending = false;   // recorded behind the one kernel of rtgpu_denoise_async that reads the sum buffer (rtgpu_denoise_var_async: both sum buffers): whatever writes the film next waits for it
    } denoise;

    // temporal accumulation (rtgpu_denoise_temporal; rt_runtime_temporal.inl): the previous frame and the one being written, ordered by denoise.done
    struct Temporal
    {
        float4* records = nullptr; size_t capacity = 0;   // two sets of four planes of `capacity` 16-byte records: {A, length}, {B, id}, {N, valid}, {P, 0} (128 bytes per pixel)
        uint32_t current = 0; bool have = false;          // the set that holds the previous frame; false: no history (every pixel starts)
        bool chained = false;                             // that frame was written by rtgpu_denoise_temporal_chain: the free lane of {P, .} holds chain lengths
        float worldToScreen[16] = {}, sampleOffset[2] = {};   // of the pass that frame's guides were rendered with
        // moving objects: per CURRENT object the id and transform it had when the history was stored (rtgpu_update_objects carries them through its
        // permutations and raises movedSince); the device copy of the RtObjectMotion table built from them
        // (deformed: the object's mesh was deformed under a snapshot since then -- its id stays, and the call follows the deformation)
        struct Then { uint32_t id; float transform[16]; uint32_t deformed; };
        std::vector<Then> then; bool movedSince = false;
        bool trackDeform = false;                         // rtgpu_set_deform_tracking
        RtObjectMotion* motion = nullptr; size_t motionCapacity = 0;
        // history clipping: two planes of `momentsCapacity` 16-byte records, {mu.rgb, cnt} and {g.rgb, 0} (32 bytes per pixel), of the clipped calls, pure or not
        float4* moments = nullptr; size_t momentsCapacity = 0;
    } temporal;

    // where a pass's primary rays come from (rtgpu_set_ray_source, rtgpu_set_lens_source; rt_runtime_raysource.inl): the camera, or the table the generate
    // kernels read in its place.  One context holds one source.  `incoming` is the buffer the next table of either kind is copied into and checked in before
    // the two change places -- a refused table never becomes the source, and a caller who sets a table per pass (anti-aliasing) allocates twice, not per
    // call.  Both hold width * height entries and go with the film's size (rtgpu_resize).
    struct RaySource
    {
        uint32_t kind = 0u;                       // 0 the camera, 1 a plain table (RtPrimaryRay), 2 a lens table (RtLensRay): rtgpu_get_ray_source_kind's values
        float4* table = nullptr; size_t tableBytes = 0;         // null under kind 0
        float4* incoming = nullptr; size_t incomingBytes = 0;
        uint32_t* degenerate = nullptr;           // what the kind's check kernel counted
        float4* exported = nullptr; size_t exportedBytes = 0;   // the device copy the synchronous exports read back from (rtgpu_read_camera_rays, ...)
        hipEvent_t order = nullptr;               // the _device set entries: puts the copy behind the caller's stream
        uint32_t lens = 0u, bokehShape = 0u;      // RtLensSourceParams of a lens table
        hipEvent_t lensRead = nullptr;            // behind the last rtgpu_read_lens_source_rays_async on a caller's stream: it reads the lens table
        bool any() const { return kind != 0u; }   // a source of either kind: the camera is not read
    } raySource;

    // beam lists (rt_beam_lists.h; the policy: beamListsFor, rt_runtime_render.inl): a still camera's per-tile leaf lists, which k_trace_packet scans in place of
    // its walk.  They belong to ONE combination of camera, frame size, slot table (so shard and active blocks), geometry, margin and capacity: the first, the last
    // two and the size are compared by beamListsFor; whatever replaces one of the others calls beamInvalidate.  A launch in flight may read the arrays: while one
    // may (`inFlight`), a rebuild takes new arrays and retires these; retired arrays are freed wherever the lanes go idle (syncLanes: every synchronising call,
    // reset, upload, update, resize), and a caller who never synchronises holds at most RT_BEAM_MAX_RETIRED of them.  Behind idle lanes a rebuild of the same
    // size rewrites the arrays in place: an animation that deforms its mesh every frame, or a viewer that reads back between camera moves, allocates once.
    struct Beam
    {
        BeamEntry* entries = nullptr; uint32_t* counts = nullptr;
        uint32_t capacity = 0, numTiles = 0;
        bool valid = false;
        RtCamera camera = {}; uint32_t width = 0, height = 0; float builtMargin = 0.0f;   // what `entries` were built for
        hipEvent_t built = nullptr; int builtLane = -1; uint32_t lanesWaited = 0u;        // behind the build kernel; the lanes (bits) that wait for it already
        bool haveLast = false; RtCamera lastCamera = {};   // the camera of the previous batch: a build needs two batches from one camera
        float margin = 1.5f;                               // m in pixels: rtgpu_set_beam_margin (the host mirror sets 3 x antiAliasingSpread)
        unsigned long long* stats = nullptr;               // device, BeamLists::stats
        uint64_t builds = 0, allocations = 0;              // build launches; those of them that took new arrays (the others rewrote idle ones in place)
        bool inFlight = false;                             // a launch submitted since the lanes were last idle (syncLanes) may read `entries`
        std::vector<void*> retired;                        // at most RT_BEAM_MAX_RETIRED arrays: beamListsFor lets the lanes go idle before it retires more
    } beam;

    // timing
    bool timing = false;
    struct Timed { int kc; hipEvent_t a, b; };
    std::vector<Timed> pendingTimed;
    std::vector<hipEvent_t> eventPool;
    double kernelMs[RTGPU_NUM_KERNEL_CLASSES];
    uint64_t kernelLaunches[RTGPU_NUM_KERNEL_CLASSES];
};

// frees a device allocation (or several) and forgets it
template <class T> static void devFree(T*& p) { if (p) (void)hipFree(p); p = nullptr; }
template <class T, class... Rest> static void devFree(T*& p, Rest*&... rest) { devFree(p); devFree(rest...); }

static void freeScene(RtgpuContext* c)
{
    for (void* p : c->sceneAllocs) (void)hipFree(p);
    c->sceneAllocs.clear();
    memset(&c->sceneDev, 0, sizeof(c->sceneDev));
    c->sceneReady = false;
}

// the beam lists no longer describe what the next batch renders (scene, geometry, slot table, ray source): the next still camera builds anew
static void beamInvalidate(RtgpuContext* c) { c->beam.valid = false; c->beam.haveLast = false; }
// only where no launch is in flight (the callers have synchronised the lanes)
static void beamFreeRetired(RtgpuContext* c)
{
    for (void* p : c->beam.retired) (void)hipFree(p);
    c->beam.retired.clear();
}

static void freeFilm(RtgpuContext* c)
{
    beamInvalidate(c);   // the slot table goes
    devFree(c->sum, c->secondary, c->slotPixel);
    c->numSlots = 0;
}

static void freePaths(BatchLane& l)
{
    devFree(l.paths.base, l.queues[0], l.queues[1], l.shadowQueues[0], l.shadowQueues[1], l.exactQueue, l.exactShadowQueue, l.paths2.base, l.home);
    l.paths.capacity = 0; l.paths.maxLights = 0; l.paths2.capacity = 0; l.paths2.maxLights = 0; l.homeCapacity = 0;
}

static hipError_t syncLanes(RtgpuContext* c)
{
    hipError_t first = hipSuccess;
    for (uint32_t i = 0; i < RT_MAX_LANES; ++i)
        if (c->lanes[i].stream) { const hipError_t e = hipStreamSynchronize(c->lanes[i].stream); if (first == hipSuccess) first = e; }
    // every lane is idle: no launch reads beam-list arrays any more -- the retired ones go, and the ones in use may be rewritten in place (beamListsFor)
    if (first == hipSuccess) { beamFreeRetired(c); c->beam.inFlight = false; }
    return first;
}

static int resolveTimed(RtgpuContext* c)
{
    for (auto& t : c->pendingTimed)
    {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, t.a, t.b));
        c->kernelMs[t.kc] += ms;
        c->kernelLaunches[t.kc]++;
        c->eventPool.push_back(t.a); c->eventPool.push_back(t.b);
    }
    c->pendingTimed.clear();
    return RTGPU_OK;
}

static hipEvent_t acquireEvent(RtgpuContext* c)
{
    if (!c->eventPool.empty()) { hipEvent_t e = c->eventPool.back(); c->eventPool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

struct LaunchTimer
{
    RtgpuContext* c; hipStream_t stream; int kc; hipEvent_t a = nullptr, b = nullptr;
    LaunchTimer(RtgpuContext* ctx, hipStream_t st, int k) : c(ctx), stream(st), kc(k)
    {
        if (c->timing) { a = acquireEvent(c); b = acquireEvent(c); (void)hipEventRecord(a, stream); }
    }
    ~LaunchTimer()
    {
        if (c->timing) { (void)hipEventRecord(b, stream); c->pendingTimed.push_back({ kc, a, b }); }
    }
};

static void waitQueries(RtgpuContext* c)
{
    if (c->query.done) (void)hipEventSynchronize(c->query.done);
    if (c->aov.done) (void)hipEventSynchronize(c->aov.done);   // (an asynchronous AOV call walks the scene as a query does)
    if (c->chain.done) (void)hipEventSynchronize(c->chain.done);
}
// A freed walk arena for `want` rays, in powers of two from 64 K: a caller whose batches grow slowly does not reallocate with every call
static int growWalkArena(WalkArena& w, uint32_t want)
{
    uint32_t cap = 65536u;
    while (cap < want) cap <<= 1;
    HIP_TRY(hipMalloc((void**)&w.paths.base, ((size_t)R_NUM_BASE + RT_SHADOW_RECORDS) * cap * sizeof(float4)));
    HIP_TRY(hipMalloc((void**)&w.queue, (size_t)cap * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void**)&w.exactQueue, (size_t)cap * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void**)&w.exactShadowQueue, (size_t)cap * sizeof(uint32_t)));
    w.paths.capacity = cap; w.paths.maxLights = 1;
    return RTGPU_OK;
}
static void freeWalkArena(WalkArena& w) { devFree(w.paths.base, w.queue, w.exactQueue, w.exactShadowQueue); w.paths.capacity = 0; w.paths.maxLights = 0; }

static void freeQueryArena(RtgpuContext* c)
{
    RtgpuContext::Query& q = c->query;
    waitQueries(c);
    freeWalkArena(q.arena);
    devFree(q.stagedRays, q.stagedHits, q.stagedSurfaces, q.stagedOccluded);
}
static void freeQuery(RtgpuContext* c)
{
    RtgpuContext::Query& q = c->query;
    freeQueryArena(c);
    devFree(q.arena.counts, q.arena.counters);
    if (q.done) (void)hipEventDestroy(q.done);
    q.done = nullptr;
}

static void freeAovArena(RtgpuContext* c)
{
    RtgpuContext::Aov& a = c->aov;
    if (a.done) (void)hipEventSynchronize(a.done);
    freeWalkArena(a.arena);
    devFree(a.slotPixel, a.rayCounts);
}
static void freeAov(RtgpuContext* c)
{
    RtgpuContext::Aov& a = c->aov;
    freeAovArena(c);
    devFree(a.staged, a.arena.counts, a.arena.counters, a.passDev, a.seedDev);
    a.stagedWords = 0;
    if (a.ringHost) (void)hipHostFree(a.ringHost);
    a.ringHost = nullptr;
    for (uint32_t i = 0; i < RtgpuContext::Aov::kRing; ++i) { if (a.ringCopied[i]) (void)hipEventDestroy(a.ringCopied[i]); a.ringCopied[i] = nullptr; }
    if (a.done) (void)hipEventDestroy(a.done);
    a.done = nullptr;
}

static void freeChainArena(RtgpuContext* c)
{
    RtgpuContext::Chain& a = c->chain;
    if (a.done) (void)hipEventSynchronize(a.done);
    freePaths(a.lane);
    devFree(a.slotPixel);
}
static void freeChain(RtgpuContext* c)
{
    RtgpuContext::Chain& a = c->chain;
    freeChainArena(c);
    devFree(a.staged, a.lane.queueCounts, a.counters, a.passDev, a.seedDev);
    a.stagedWords = 0; a.lane.queueCountCapacity = 0;
    if (a.ringHost) (void)hipHostFree(a.ringHost);
    a.ringHost = nullptr;
    for (uint32_t i = 0; i < RtgpuContext::Chain::kRing; ++i) { if (a.ringCopied[i]) (void)hipEventDestroy(a.ringCopied[i]); a.ringCopied[i] = nullptr; }
    if (a.done) (void)hipEventDestroy(a.done);
    a.done = nullptr;
}

// before anything writes or frees the sum buffer: an rtgpu_denoise_async on a caller's stream may still be reading it
static void waitDenoiseRead(RtgpuContext* c)
{
    if (!c->denoise.sumReadPending) return;
    (void)hipEventSynchronize(c->denoise.sumRead);
    c->denoise.sumReadPending = false;
}
static void freeDenoise(RtgpuContext* c)
{
    RtgpuContext::Denoise& d = c->denoise;
    if (d.done) (void)hipEventSynchronize(d.done);
    devFree(d.records, d.io, c->temporal.records, c->temporal.motion, c->temporal.moments);
    d.capacity = 0; d.ioFloats = 0; c->temporal.capacity = 0; c->temporal.have = false; c->temporal.motionCapacity = 0; c->temporal.momentsCapacity = 0;
    if (d.done) (void)hipEventDestroy(d.done);
    if (d.sumRead) (void)hipEventDestroy(d.sumRead);
    d.done = nullptr; d.sumRead = nullptr; d.sumReadPending = false;
}

// A caller's device array of `bytes` bytes, before any kernel or copy reads or writes it (rtgpu_update_mesh_device, rtgpu_set_ray_source_device,
// rtgpu_read_camera_rays_async): aligned to alignMask + 1 bytes, device memory of the context's device, inside one allocation to its last byte.  `unit` names
// what the allocation must hold ("12 bytes per vertex").
static int callerDeviceArray(const RtgpuContext* c, const void* p, size_t bytes, uintptr_t alignMask, const char* name, const char* unit)
{
    const std::string what(name);
    if ((uintptr_t)p & alignMask) return fail(RTGPU_ERR_INVALID_ARGUMENT, what + " is not aligned to " + (alignMask == 3u ? std::string("a float") : std::to_string(alignMask + 1u) + " bytes"));
    hipPointerAttribute_t attributes;
    memset(&attributes, 0, sizeof(attributes));
    if (hipPointerGetAttributes(&attributes, p) != hipSuccess) { (void)hipGetLastError(); return fail(RTGPU_ERR_INVALID_ARGUMENT, what + " is not a device pointer"); }
    if (attributes.type != hipMemoryTypeDevice || attributes.device != c->device) return fail(RTGPU_ERR_INVALID_ARGUMENT, what + " is not memory of the context's device");
    hipDeviceptr_t base = nullptr; size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return fail(RTGPU_ERR_INVALID_ARGUMENT, what + " lies in no device allocation"); }
    const uintptr_t begin = (uintptr_t)base, at = (uintptr_t)p;
    if (at < begin || at - begin > size || size - (at - begin) < bytes) return fail(RTGPU_ERR_INVALID_ARGUMENT, what + ": its allocation ends before " + unit + " do");
    return RTGPU_OK;
}

// the ray source's tables (the caller has waited for whatever reads them): the camera renders again
static void waitLensExport(RtgpuContext* c) { if (c->raySource.lensRead) (void)hipEventSynchronize(c->raySource.lensRead); }
static void dropRaySource(RtgpuContext* c)
{
    RtgpuContext::RaySource& s = c->raySource;
    waitLensExport(c);
    devFree(s.table, s.incoming);
    s.kind = 0u; s.tableBytes = 0; s.incomingBytes = 0;
}
static void freeRaySource(RtgpuContext* c)
{
    RtgpuContext::RaySource& s = c->raySource;
    dropRaySource(c);
    devFree(s.degenerate, s.exported);
    s.exportedBytes = 0;
    if (s.order) (void)hipEventDestroy(s.order);
    s.order = nullptr;
    if (s.lensRead) (void)hipEventDestroy(s.lensRead);
    s.lensRead = nullptr;
}

static void freeRecorder(RtgpuContext* c)
{
    RtgpuContext::Recorder& rec = c->recorder;
    freePaths(rec.lane);
    devFree(rec.lane.queueCounts, rec.slotPixel, rec.records, rec.infos, rec.counters, rec.passDev, rec.seedDev);
    rec.lane.queueCountCapacity = 0; rec.recordCapacity = 0;
}

// Streams are recycled through a process-wide pool instead of being created and destroyed with every context: a test session (or an
// application that opens a renderer per frame size) goes through hundreds of contexts, and on some boxes of the pool the HSA runtime's
// event thread aborts the process after a few hundred stream (hardware queue) create / destroy cycles (no message; ROCm 7.0.2).  A context
// returns its idle streams at destruction, after it has synchronised them.
static std::mutex gStreamPoolMutex;
static std::unordered_map<int, std::vector<hipStream_t>> gStreamPool;   // device -> idle non-blocking streams
static hipError_t acquireStream(int device, hipStream_t* out)
{
    {
        std::lock_guard<std::mutex> lock(gStreamPoolMutex);
        auto& pool = gStreamPool[device];
        if (!pool.empty()) { *out = pool.back(); pool.pop_back(); return hipSuccess; }
    }
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}
static void releaseStream(int device, hipStream_t stream)
{
    std::lock_guard<std::mutex> lock(gStreamPoolMutex);
    gStreamPool[device].push_back(stream);
}
