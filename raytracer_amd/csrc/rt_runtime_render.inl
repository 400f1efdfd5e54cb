// rt_runtime_render.inl -- the PathTracerMIS launch sequence: arena sizing, the traversal launchers, the hand-over policies, the submission of a batch
// of passes on a lane.  Included by rt_runtime.hip.

// Streaming grows the batch 8 -> 16 -> 24 passes; frames beyond full HD stop earlier so that an arena stays below ~24 GB
// (176 bytes per slot with one NEE request per vertex: 4K frames reach 16 passes, 8K frames stay at 8 and below)
static uint32_t maxStreamingBatch(const RtgpuContext* c)
{
    const size_t perPass = (size_t)(c->numSlots ? c->numSlots : 1) * ((size_t)R_NUM_BASE + RT_SHADOW_RECORDS) * sizeof(float4);
    const uint32_t most = knobs::maxStreamBatch();   // tuning knob (a multiple of 8, at most 64)
    uint32_t batch = most < 8u ? 8u : (most > RT_SEED_RING / 2 ? RT_SEED_RING / 2 : most);
    while (batch > 8u && perPass * batch > ((size_t)24 << 30)) batch -= 8u;
    return batch;
}

// Device bytes one path slot costs a batch lane when a vertex can have `maxLights` next-event requests: the records of both arenas
// (the second one only exists with dense path state: up to RT_DENSE_MAX_LIGHTS requests per vertex), the parked radiance, the queues.  LightSamplingStrategy::All with many
// lights makes slots fat (64 lights: 2.2 KB), so the batch a lane can hold shrinks with it -- down to one pass.
static size_t bytesPerSlot(uint32_t maxLights)
{
    if (maxLights == 0) maxLights = 1;
    const size_t arena = ((size_t)R_NUM_BASE + (size_t)maxLights * RT_SHADOW_RECORDS) * sizeof(float4);
    return arena * (maxLights <= RT_DENSE_MAX_LIGHTS ? 2u : 1u) + sizeof(float4) + sizeof(uint32_t) * (3u + 3u * (size_t)maxLights);
}
static uint32_t maxBatchFor(const RtgpuContext* c, uint32_t maxLights)
{
    const size_t perPass = (size_t)(c->numSlots ? c->numSlots : 1) * bytesPerSlot(maxLights);
    const size_t batch = c->laneBudgetBytes / perPass;
    return batch < 1u ? 1u : (batch > RT_SEED_RING / 2 ? RT_SEED_RING / 2 : (uint32_t)batch);
}
// slots an arena is allocated for: the regions of dense path state need a margin each (a region's share of a launch is only
// roughly a sixteenth: blocks take turns)
static size_t arenaCapacityFor(size_t slots) { return (size_t)RT_DENSE_SHARDS * ((slots + RT_DENSE_SHARDS - 1u) / RT_DENSE_SHARDS + 65536u); }

// The seven buffers of a slot-per-pixel lane (freed before: freePaths) for `capacity` slots with `maxLights` next-event requests per vertex
static int allocLanePaths(BatchLane& l, size_t capacity, uint32_t maxLights)
{
    if ((unsigned long long)capacity * maxLights >= 0xFFFFFFFFull) return fail(RTGPU_ERR_UNSUPPORTED, "pixels x lights exceeds the NEE request index range");
    HIP_TRY(hipMalloc((void**)&l.paths.base, ((size_t)R_NUM_BASE + (size_t)maxLights * RT_SHADOW_RECORDS) * capacity * sizeof(float4)));
    for (int k = 0; k < 2; ++k) HIP_TRY(hipMalloc((void**)&l.queues[k], capacity * sizeof(uint32_t)));
    for (int k = 0; k < 2; ++k) HIP_TRY(hipMalloc((void**)&l.shadowQueues[k], capacity * maxLights * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void**)&l.exactQueue, capacity * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void**)&l.exactShadowQueue, capacity * maxLights * sizeof(uint32_t)));
    l.paths.capacity = (uint32_t)capacity; l.paths.maxLights = maxLights;
    return RTGPU_OK;
}

static int ensurePaths(RtgpuContext* c, BatchLane& l, uint32_t maxLights, uint32_t maxDepth)
{
    if (maxLights == 0) maxLights = 1;
    const bool wantDense = c->denseAllowed && maxLights <= RT_DENSE_MAX_LIGHTS;
    for (int attempt = 0; attempt < 2; ++attempt)
    {
        uint32_t maxBatch = (c->passBatchFromEnv || c->numSlots < 400000u) ? c->passBatch : maxStreamingBatch(c);   // the largest batch streaming can reach
        if (maxBatch > maxBatchFor(c, maxLights)) maxBatch = maxBatchFor(c, maxLights);
        const size_t wanted = (size_t)(c->numSlots ? c->numSlots : 1) * maxBatch;
        if (l.paths.base && l.paths.capacity >= arenaCapacityFor(wanted) && l.paths.maxLights >= maxLights && (!wantDense || (l.paths2.base && l.homeCapacity >= wanted))) break;
        HIP_TRY(hipStreamSynchronize(l.stream));
        freePaths(l);
        if (attempt == 0)
        {
            // The lane budget of rtgpu_create is a guess made before anything was allocated.  Contexts that share a device (several
            // renderers in one process, rtgpu_create_multi with a repeated index) see less: what is free NOW is shared by the lanes of
            // this context that still have to allocate, and the batch a lane may hold shrinks with it instead of a late out-of-memory.
            size_t freeBytes = 0, totalBytes = 0;
            if (hipMemGetInfo(&freeBytes, &totalBytes) == hipSuccess)
            {
                uint32_t lanesLeft = 0;
                for (uint32_t i = 0; i < c->numLanes; ++i) if (!c->lanes[i].paths.base) lanesLeft++;
                const size_t share = (size_t)((double)freeBytes * 0.9) / (lanesLeft ? lanesLeft : 1u);
                if (share < c->laneBudgetBytes)
                {
                    c->laneBudgetBytes = share;   // size the arenas again under the smaller budget
                    if (c->passBatch > maxBatchFor(c, maxLights)) c->passBatch = maxBatchFor(c, maxLights);
                    if (c->passBatchBase > c->passBatch) c->passBatchBase = c->passBatch;
                    continue;
                }
            }
        }
        const size_t cap = arenaCapacityFor(wanted);
        if (cap >= 0xFFFFFFFFull) return fail(RTGPU_ERR_UNSUPPORTED, "pixels x pass batch exceeds the slot index range");
        { const int r = allocLanePaths(l, cap, maxLights); if (r) return r; }
        if (wantDense)
        {
            HIP_TRY(hipMalloc((void**)&l.paths2.base, ((size_t)R_NUM_BASE + (size_t)maxLights * RT_SHADOW_RECORDS) * cap * sizeof(float4)));
            HIP_TRY(hipMalloc((void**)&l.home, wanted * sizeof(float4)));
            l.homeCapacity = wanted;
            l.paths2.capacity = (uint32_t)cap; l.paths2.maxLights = maxLights;
        }
        break;
    }
    if (l.queueCountCapacity < maxDepth + 2)
    {
        HIP_TRY(hipStreamSynchronize(l.stream));
        devFree(l.queueCounts, l.denseCounts);
        l.queueCountCapacity = maxDepth + 2;
        HIP_TRY(hipMalloc((void**)&l.queueCounts, laneCountBytes(l)));
        HIP_TRY(hipMalloc((void**)&l.denseCounts, (size_t)2 * RT_DENSE_SHARDS * (l.queueCountCapacity + 1u) * sizeof(uint32_t)));
    }
    return RTGPU_OK;
}

// LDS stack capacity of the binary walk in entries per lane: 24 (5 blocks per CU), 32 (4) or 64 (2); the scene's BVH depth decides
static uint32_t stackClassOf(const RtgpuContext* c) { return c->traversalStackNeed <= 24 ? 24u : (c->traversalStackNeed <= 32 ? 32u : 64u); }
// persistent traversal grids: enough resident waves to cover the latency of dependent node fetches; surplus blocks simply queue (there is no
// inter-block dependency, only the atomic cursor).  The 4-wide walks run on 24-entry stacks.
static uint32_t traversalBlocks(const RtgpuContext* c, uint32_t stackClass)
{
    return c->numCUs * (c->travBlocksPerCU ? c->travBlocksPerCU : (stackClass == 24u ? 5u : (stackClass == 32u ? 4u : 2u)));
}

// The reference's walk over the binary trees (k_trace) over the work of `s`: the one place that picks its instantiation.  The caller sets up `tune`, chooses the
// grid and times the launch; `counting`: with the box / triangle test counters (and, where tune.rayCounts is set, every ray's own counts).
static void launchTraceBinary(RtgpuContext* c, const TraceStep& s, dim3 grid, const TravTuning& tune, bool counting)
{
    const uint32_t stackClass = stackClassOf(c);
#define RT_LAUNCH_TRACE(S, C, R) hipLaunchKernelGGL((k_trace<S, C, R>), grid, dim3(RT_BLOCK), 0, s.stream, c->sceneDev, s.paths, s.queue, s.queueCount, s.shadowQueue, s.shadowCount, s.cursor, s.counters, tune)
#define RT_LAUNCH_TRACE_STACK(S) { if (counting && tune.rayCounts) RT_LAUNCH_TRACE(S, true, true); else if (counting) RT_LAUNCH_TRACE(S, true, false); else RT_LAUNCH_TRACE(S, false, false); }
    if (stackClass == 24u) RT_LAUNCH_TRACE_STACK(24) else if (stackClass == 32u) RT_LAUNCH_TRACE_STACK(32) else RT_LAUNCH_TRACE_STACK(64)
#undef RT_LAUNCH_TRACE_STACK
#undef RT_LAUNCH_TRACE
}

// The 4-wide tree: single-mesh scenes, intersection counters off (they belong to the reference's walk).  Stack: 24 entries per lane, a
// ray that would need more goes to the binary-tree kernel.
static bool useWide(const RtgpuContext* c) { return (c->wide.nodes != nullptr || (c->wide2.nodes != nullptr && c->wide2Allowed)) && c->wideAllowed && !c->countIntersections; }

static void launchTraceWide(RtgpuContext* c, const TraceStep& s)
{
    // A block traces the rays its walk does not decide itself (rt_trace_wide.inl) where launches are short: a 1/8 shard of a full-HD frame gains 10 %
    // (ten launches per batch less to wait for), a full frame loses 1.4 % (a block holds its slot of the CU while one wave walks; the separate launch
    // ran beside the other lanes' kernels) -- profiles/r04_local_exact_ab.txt; round 5: a 1/8 shard still gains 3 %, a 1/4 shard (518 k pixels) loses 2 %, halves 0
    // -- profiles/r05_shard_policy.txt.  So: small frames, unless rtgpu_set_schedule says otherwise.  Never on stacks deeper than the kernel's 24 entries (the
    // second walk runs on them), never where the caller forbids it (the bidirectional integrator: a degenerate closest-hit ray of a light path would hold a whole
    // block's slot of the CU for milliseconds, 16.5 -> 26 ms per pass, profiles/r04_vcm_wide_ab.txt; its separate launch holds one block per CU instead).
    const bool localExact = s.mayTraceUndecidedRaysItself && c->traversalStackNeed <= 24u && (c->localRetrace >= 0 ? c->localRetrace != 0 : c->numSlots < 400000u);
    const uint32_t chunkMin = knobs::wideChunkMin();   // tuning knob
    // drainAbortAfter, a test hook read per launch: a wave whose work queue ran dry N loop iterations ago hands the rays it still walks -- hits half found, written
    // through -- to the re-trace launch (the stack-overflow path, which the benchmark frame never takes).  As a schedule it moves time, it does not save any: what
    // k_trace_wide's drain loses (-5.6 % at N = 8) the re-trace launches gain (profiles/r05_drain_abort_ab.txt)
    // The work queue {closest-hit rays of bounce k, any-hit requests of bounce k - 1} is taken front to back: a launch ends with the drain of its last rays, so the
    // SHORT rays belong at the end, and under the far-first order of the interior step (rt_wide_walk.h) those are the any-hit rays: 9.9 interior visits against a
    // closest-hit ray's 17 (profiles/r06_claim_order_ab.txt: against the queue taken from its end, trace 47.5 -> 45.5 ms per 25 passes, +2 % on a 1/8 shard).
    WideTuning tune = { c->tune.refillMinIdle, c->tune.otherMinLanes, s.shadowOffset, s.exactQueue, s.exactCount, s.exactShadowQueue, s.exactShadowCount, s.denseCounts,
                        s.denseShardCapacity, chunkMin < 64u ? 64u : chunkMin, localExact ? 1u : 0u, knobs::wideDrainAbort() };
    const dim3 grid(traversalBlocks(c, 24u)), block(RT_BLOCK);
    LaunchTimer t(c, s.stream, KC_TRACE);
    if (c->wide.nodes == nullptr)
    {
        // a two-level scene (rt_trace_wide2.inl): held to five waves per SIMD (110 -> 96 VGPRs, 8 bytes of scratch: Cornell box trace -7 %, +2 % end to
        // end), 30 KB of LDS per block
        hipLaunchKernelGGL((k_trace_wide2<24>), grid, block, 0, s.stream, c->sceneDev, c->wide2, s.paths, s.queue, s.queueCount, s.shadowQueue, s.shadowCount, s.cursor, s.counters, tune);
        return;
    }
    const bool diag = knobs::wideDiag();       // walk statistics in the spare counters (tools/wide_diag.py)
    // the camera rays of a dense batch walk the tree as packets (rt_trace_packet.inl: a wave = an 8 x 8 pixel block, the node is uniform); RTGPU_PACKET=0: off
    const bool packets = knobs::packets();   // (read per launch: the tests switch it)
    if (packets && !diag && s.bounce == 0u && s.denseCounts != nullptr && s.shadowQueue == nullptr && s.queue == nullptr)
    {
        hipLaunchKernelGGL(k_trace_packet, dim3(c->numCUs * knobs::packetBlocksPerCU()), block, 0, s.stream, c->sceneDev, c->wide, s.paths, s.cursor, s.counters, tune, s.beam);
        return;
    }
    if (diag) tune.localExact = knobs::wideDiagMode();   // 2: stack-depth histogram instead of the visit counts (tools/wide_diag.py)
#define RT_LAUNCH_TRACE_WIDE(D, L) hipLaunchKernelGGL((k_trace_wide<24, D, L>), grid, block, 0, s.stream, c->sceneDev, c->wide, s.paths, s.queue, s.queueCount, s.shadowQueue, s.shadowCount, s.cursor, s.counters, tune)
    if (diag) RT_LAUNCH_TRACE_WIDE(true, false); else if (localExact) RT_LAUNCH_TRACE_WIDE(false, true); else RT_LAUNCH_TRACE_WIDE(false, false);
#undef RT_LAUNCH_TRACE_WIDE
}

// what a 4-wide walk handed over, as the work of a step of its own
static TraceStep handedOver(TraceStep s)
{
    s.queue = s.exactQueue; s.queueCount = s.exactCount; s.shadowQueue = s.exactShadowQueue; s.shadowCount = s.exactShadowCount; s.cursor = s.exactCursor;
    return s;
}

// The re-trace launch behind a 4-wide walk: the reference's own walk (k_trace) over the rays the walk handed over (0.1 % of a launch).  It keeps every ray
// it takes: since the axis-parallel prune (boxNearDegenerateAxes) made degenerate closest-hit rays short, no ray of the benchmark frame would go on to
// k_trace_monster, and an empty launch of that kernel behind every re-trace launch cost 2 % end to end under concurrency
// (profiles/r05_monsters_under_concurrency_ab.txt).  The cooperative walker serves the bidirectional integrator's launches (rt_runtime_vcm.inl).
// Its work is the hand-over of `s`.
static void launchRetrace(RtgpuContext* c, const TraceStep& s)
{
    TravTuning exactTune = c->tune;   // (no overflow queue: the launch hands nothing on)
    exactTune.denseCounts = nullptr; exactTune.denseShardCapacity = 0u;
    // a re-trace launch's queue is dry after the first claim and its duration is its longest ray: an any-hit ray that slides along a wall it started on (a sun in a
    // coordinate plane: the ray lies IN the wall's plane, Moeller-Trumbore never accepts the coplanar triangles) walks ~170 nodes = 250 us alone.  Idle lanes take its
    // deferred subtrees after RT_RETRACE_SPLIT_AFTER drain iterations instead of the 32 of a full launch.
    exactTune.splitAfter = knobs::retraceSplitAfter() ? knobs::retraceSplitAfter() : RT_RETRACE_SPLIT_AFTER;   // tuning knob
    LaunchTimer t(c, s.stream, KC_RETRACE);
    // one block per CU serves the usual few thousand requests; above 1024 requests per CU (exactTune.fullGridAbove = numCUs * 1024) the whole traversal grid works
    // (decided on the device from the counts)
    // (only where the scene can produce such queues -- a delta sun with an exactly-zero direction component, c->axisParallelSun: the 1024 extra blocks that read two
    //  counts and leave cost an ordinary scene ~0.5 % end to end, profiles/r05_retrace_grid_ab.txt; RTGPU_RETRACE_FULL_GRID=0 / 1 forces it)
    const int gridEnv = knobs::retraceFullGrid();
    const bool adaptiveGrid = gridEnv >= 0 ? gridEnv != 0 : c->axisParallelSun;
    exactTune.baseBlocks = adaptiveGrid ? c->numCUs : 0u; exactTune.fullGridAbove = c->numCUs * 256u * 4u;
    const dim3 retraceGrid(adaptiveGrid ? traversalBlocks(c, stackClassOf(c)) : c->numCUs);
    launchTraceBinary(c, handedOver(s), retraceGrid, exactTune, false);
}

// One trace step of a launch sequence.  `wide` (the render sequences: useWide(c)): the 4-wide tree serves the launch; what it does not trust goes through the
// binary-tree kernel right behind it (a small grid: few rays).  Otherwise the reference's binary walk on the full traversal grid, counting where the context
// counts or s.rayCounts is asked for.
static void launchTraceStep(RtgpuContext* c, const TraceStep& s, bool wide)
{
    if (wide) { launchTraceWide(c, s); launchRetrace(c, s); return; }
    TravTuning tune = c->tune; tune.shadowOffset = s.shadowOffset; tune.denseCounts = s.denseCounts; tune.denseShardCapacity = s.denseShardCapacity; tune.rayCounts = s.rayCounts;
    LaunchTimer t(c, s.stream, KC_TRACE);
    launchTraceBinary(c, s, dim3(traversalBlocks(c, stackClassOf(c))), tune, s.rayCounts != nullptr || c->countIntersections);
}

// The bounce at which a dense batch hands its remaining paths to k_tail (0: never).  rtgpu_set_schedule forces a bounce (0: off).
static uint32_t tailDepthFor(const RtgpuContext* c, uint32_t maxRayDepth, bool denseAll)
{
    if (c->tailBounce == 0 || denseAll || c->wide.nodes == nullptr || !useWide(c) || stackClassOf(c) != 24u || c->debugMode >= 0) return 0u;
    // Measured (profiles/r04_tail_sweep.txt, 20 passes): a 1/8 shard of the full-HD benchmark frame gains 6-8 % with the hand-over at bounce 4 or 5 (0.580 ->
    // 0.544 ms per pass, with 20-pass batches 0.575-0.606 -> 0.526-0.558; bounce 2: -20 %, 3: 0), a 1/4 shard +2 % at bounce 5 and +4 % at bounce 6 together with the block-local re-trace, halves and full frames lose 1-5 % at any bounce: the block-local
    // rounds pay a drain each and only beat the launch sequence where that is all floors.  So: small frames only.  Round 5 (faster traversal and re-trace launches,
    // profiles/r05_shard_policy.txt): bounce 6 beats 5 on the 1/8 shard too (0.499 -> 0.488 ms per pass), 4 loses everywhere, halves gain 0.6 % at 6 (left off).
    const uint32_t depth = c->tailBounce > 0 ? (uint32_t)c->tailBounce : (c->numSlots < 700000u ? 6u : 0u);
    return depth > maxRayDepth + 1u ? 0u : depth;
}

// Beam lists for the packet launch of a dense batch on lane `l` (rt_beam_lists.h; k_trace_packet's front end): `out.entries` stays null where the batch walks.
// Lists exist for: a single-mesh scene served by k_trace_wide on the 24-entry stack class, packets on, intersection counters off, a mesh object with a rigid
// transform, a pinhole camera (no depth of field, no barrel distortion: beamCameraFor) and no ray or lens source; every pass of the batch from ONE camera.
// Key: camera bytes, frame size, margin m, capacity -- compared here; slot table (so shard, active blocks), geometry, object transform, source: whoever
// replaces one calls beamInvalidate.
// Build trigger: a batch that finds the camera of the PREVIOUS batch unchanged and no valid lists builds them, on its lane's stream in front of its packet
// launch, followed by an event the other lanes wait for before their first packet launch that reads the lists.  A camera that moves every frame never pays for
// a build (tests/test_gpu_beam_lists.py holds builds at 0 for a camera that changes with every batch; tools/bench_temporal.py's frames turn the camera in the same
// way and are expected to build only in the tool's still reference render -- not measured); a frame that accumulates pays once, with its second batch.
// Break-even (profiles/beam_lists_kernel_stats_serial.txt, the full-HD benchmark frame): the build is 128 us once, a scanned pass saves about 57 us of the
// packet launch: paid back within 3 passes.
// Arrays a launch in flight may read are never rewritten or freed, and a context holds a bounded number of them (RtgpuContext::Beam).
static int beamListsFor(RtgpuContext* c, BatchLane& l, int laneIndex, const DevPass* passesHost, const DevPass* passesDev, uint32_t numPasses, BeamLists& out)
{
    RtgpuContext::Beam& b = c->beam;
    const bool served = knobs::beamLists() && knobs::packets() && !knobs::wideDiag() && c->wide.nodes != nullptr && useWide(c) && stackClassOf(c) == 24u &&
                        !c->raySource.any() && c->sceneDev.numObjects == 1u && c->updatable.objects.size() == 1u && c->numSlots != 0u;
    bool oneCamera = served;
    for (uint32_t i = 0; oneCamera && i < numPasses; ++i)
        oneCamera = memcmp(&passesHost[i].camera, &passesHost[0].camera, sizeof(RtCamera)) == 0 && passesHost[i].width == c->width && passesHost[i].height == c->height;
    if (!oneCamera) { b.haveLast = false; return RTGPU_OK; }
    const RtCamera& camera = passesHost[0].camera;
    const bool still = b.haveLast && memcmp(&b.lastCamera, &camera, sizeof(RtCamera)) == 0;
    b.lastCamera = camera; b.haveLast = true;
    const uint32_t capacity = knobs::beamListCap();
    const bool keyed = b.valid && memcmp(&b.camera, &camera, sizeof(RtCamera)) == 0 && b.width == c->width && b.height == c->height && b.builtMargin == b.margin && b.capacity == capacity;
    if (!keyed)
    {
        b.valid = false;
        if (!still) return RTGPU_OK;
        BeamCamera local;
        float lo[3], hi[3];
        beamTreeBounds(c->wide.base, c->wide.step, lo, hi);
        if (!beamCameraFor(camera, c->updatable.objects[0].invTransform, c->width, c->height, b.margin, lo, hi, local)) return RTGPU_OK;
        const uint32_t numTiles = (c->numSlots + 63u) / 64u;
        // where the arrays come from: behind idle lanes the ones the context has are rewritten in place (same size) or freed; while a launch may read them
        // they are retired and new ones taken -- after the lanes went idle (syncLanes frees what is retired) if that would exceed RT_BEAM_MAX_RETIRED
        if (b.inFlight && b.entries && b.retired.size() + 2u > RT_BEAM_MAX_RETIRED) HIP_TRY(syncLanes(c));
        if (b.inFlight)
        {
            if (b.entries) b.retired.push_back(b.entries);
            if (b.counts) b.retired.push_back(b.counts);
            b.entries = nullptr; b.counts = nullptr;
        }
        else if (b.entries && (b.numTiles != numTiles || b.capacity != capacity)) devFree(b.entries, b.counts);
        if (!b.entries || !b.counts)
        {
            devFree(b.entries, b.counts);
            HIP_TRY(hipMalloc((void**)&b.entries, (size_t)numTiles * capacity * sizeof(BeamEntry)));
            HIP_TRY(hipMalloc((void**)&b.counts, (size_t)numTiles * sizeof(uint32_t)));
            b.allocations++;
        }
        if (!b.stats)
        {
            HIP_TRY(hipMalloc((void**)&b.stats, 3 * sizeof(unsigned long long)));
            HIP_TRY(hipMemsetAsync(b.stats, 0, 3 * sizeof(unsigned long long), l.stream));
        }
        if (!b.built) HIP_TRY(hipEventCreateWithFlags(&b.built, hipEventDisableTiming));
        hipLaunchKernelGGL(k_beam_lists_build, dim3(numTiles), dim3(64), 0, l.stream, c->wide, c->slotPixel, c->numSlots, local, capacity, b.entries, b.counts);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(b.built, l.stream));
        b.capacity = capacity; b.numTiles = numTiles; b.camera = camera; b.width = c->width; b.height = c->height; b.builtMargin = b.margin;
        b.builtLane = laneIndex; b.lanesWaited = 1u << laneIndex; b.valid = true; b.builds++;
    }
    else if (!(b.lanesWaited & (1u << laneIndex)))
    {
        HIP_TRY(hipStreamWaitEvent(l.stream, b.built, 0));
        b.lanesWaited |= 1u << laneIndex;
    }
    b.inFlight = true;
    out.entries = b.entries; out.counts = b.counts; out.capacity = b.capacity; out.slotsPerPass = c->numSlots; out.margin = b.builtMargin; out.passes = passesDev; out.stats = b.stats;
    return RTGPU_OK;
}

// The scene-class ladders of the shading kernels and of the fused tail (rt_shade_kernels.h, rt_tail_kernels.h): kLean class, plain path tracer, all lights
#define RT_LAUNCH_SHADE_DENSE_STAGE(L, P, A, S) hipLaunchKernelGGL((k_shade_dense<L, P, A, S>), grid, block, 0, l.stream, c->sceneDev, passesDev, c->numSlots, in, out, dc, \
                                                              l.shadowQueues[depth & 1u], counts.shadowCounts + depth, l.home, c->counters)
#define RT_LAUNCH_SHADE_DENSE(L, P, A) do { if (stage & RT_STAGE_SEEDS) RT_LAUNCH_SHADE_DENSE_STAGE(L, P, A, 2); else if (stage & RT_STAGE_TABLES) RT_LAUNCH_SHADE_DENSE_STAGE(L, P, A, 1); \
                                         else RT_LAUNCH_SHADE_DENSE_STAGE(L, P, A, 0); } while (0)
#define RT_LAUNCH_TAIL(L, P) hipLaunchKernelGGL((k_tail<L, P>), tailGrid, block, 0, l.stream, c->sceneDev, c->wide, passesDev, c->numSlots, in, args, l.home, c->counters)

// What a launch of k_shade_dense reads from LDS copies (RT_STAGE_*, rt_device_state.h): the scene's small tables where every one of them fits its capacity,
// and then the batch's seed rows where they fit theirs; decided per launch from the scene's counts and the batch -- nothing is cached, so scene updates and
// uploads need no extra work.  RTGPU_SHADE_STAGE=0: nothing.
static uint32_t denseStageMask(const RtgpuContext* c, uint32_t numPasses, uint32_t numDimensions)
{
    if (!knobs::shadeStage()) return 0u;   // (read per launch: the tests switch it)
    const RtSceneDesc& d = c->sceneDev;
    if (d.numObjects > RT_STAGE_MAX_OBJECTS || d.numMeshes > RT_STAGE_MAX_MESHES || d.numMaterials > RT_STAGE_MAX_MATERIALS || d.numLights > RT_STAGE_MAX_LIGHTS ||
        d.numGlobalLights > RT_STAGE_MAX_LIGHTS) return 0u;
    return (size_t)numPasses * stageSeedRow(numDimensions) <= RT_STAGE_SEED_WORDS ? RT_STAGE_TABLES | RT_STAGE_SEEDS : RT_STAGE_TABLES;
}

// The bounces of a batch with DENSE path state (rt_dense.inl): one next-event request per vertex (LightSamplingStrategy::Single, or none: "Path Tracer"),
// or one per light under LightSamplingStrategy::All with a handful of lights (the benchmark scene has two): `denseAll`
static int submitDenseBatch(RtgpuContext* c, BatchLane& l, const LaneCounts& counts, const DevPass* passesDev, uint32_t totalSlots, uint32_t maxRayDepth, bool denseAll, dim3 grid, uint32_t numDimensions,
                            const BeamLists& beam)
{
    const dim3 block(RT_BLOCK);
    const uint32_t numPasses = totalSlots / (c->numSlots ? c->numSlots : 1u), stage = denseStageMask(c, numPasses, numDimensions);
    const uint32_t shardCapacity = (totalSlots + RT_DENSE_SHARDS - 1u) / RT_DENSE_SHARDS + 65536u;
    const uint32_t plane = 2u * RT_DENSE_SHARDS;
    // a fresh path's records: only origin and direction are stored, bounce 0's shade rebuilds the rest from the slot (rt_dense.inl)
    // (the tail kernel never sees bounce 0 -- tailDepthFor returns >= 1 -- and the traversal kernels read origin and direction only)
    HIP_TRY(hipMemsetAsync(l.denseCounts, 0, (size_t)plane * (l.queueCountCapacity + 1u) * sizeof(uint32_t), l.stream));
    {
        LaunchTimer t(c, l.stream, KC_GENERATE);
        if (c->raySource.kind == 2u)
            hipLaunchKernelGGL(k_generate_dense_lens, grid, block, 0, l.stream, c->sceneDev, passesDev, c->numSlots, l.paths, c->slotPixel, totalSlots, shardCapacity, l.denseCounts, c->counters, c->raySource.table, c->raySource.lens, c->raySource.bokehShape);
        else if (c->raySource.kind == 1u)
            hipLaunchKernelGGL(k_generate_dense_rays, grid, block, 0, l.stream, c->sceneDev, passesDev, c->numSlots, l.paths, c->slotPixel, totalSlots, shardCapacity, l.denseCounts, c->counters, c->raySource.table);
        else hipLaunchKernelGGL(k_generate_dense, grid, block, 0, l.stream, c->sceneDev, passesDev, c->numSlots, l.paths, c->slotPixel, totalSlots, shardCapacity, l.denseCounts, c->counters);
    }
    const bool haveNee = c->numLights != 0 && !c->plainPathTracer;
    // The fused tail (rt_tail.hip): from bounce `tailDepth` on, one persistent launch takes the batch's remaining paths to their end.  Single-mesh
    // scenes behind the 4-wide walk, one next-event request per vertex.
    const uint32_t tailDepth = tailDepthFor(c, maxRayDepth, denseAll);
    for (uint32_t depth = 0; depth <= maxRayDepth + 1u; ++depth)
    {
        // (the dense record layout: any-hit origins in R_ORIGIN, verdicts in the contribution record -- rt_device_state.h)
        const Paths in = denseLayout((depth & 1u) ? l.paths2 : l.paths);
        const Paths out = denseLayout((depth & 1u) ? l.paths : l.paths2);
        if (tailDepth != 0u && depth == tailDepth)
        {
            const TailArgs args = { l.denseCounts + (size_t)plane * depth, shardCapacity, counts.cursors + depth, c->tune.refillMinIdle, c->tune.otherMinLanes, c->deviceFlags };
            uint32_t tailBlocks = (totalSlots + RT_TAIL_PATHS - 1u) / RT_TAIL_PATHS;   // never more blocks than chunks of the whole batch
            if (tailBlocks > c->numCUs * knobs::tailBlocksPerCU()) tailBlocks = c->numCUs * knobs::tailBlocksPerCU();   // tuning knob
            const dim3 tailGrid(tailBlocks ? tailBlocks : 1u);
            LaunchTimer t(c, l.stream, KC_TAIL);
            if (c->plainPathTracer) RT_LAUNCH_TAIL(0, true);
            else if (c->leanScene == 1) RT_LAUNCH_TAIL(1, false); else if (c->leanScene == 2) RT_LAUNCH_TAIL(2, false);
            else if (c->leanScene == 3) RT_LAUNCH_TAIL(3, false); else if (c->leanScene == 4) RT_LAUNCH_TAIL(4, false); else RT_LAUNCH_TAIL(0, false);
            break;
        }
        const bool haveClosest = depth <= maxRayDepth, haveShadow = depth > 0 && haveNee;
        if (haveClosest || haveShadow)
        {
            TraceStep s = { l.stream, c->counters, in };
            counts.queuesOf(s, depth, false, haveShadow);   // (the closest-hit rays are the arena's live paths: no queue)
            counts.handOverOf(s, depth);
            s.denseCounts = haveClosest ? l.denseCounts + (size_t)plane * depth : nullptr; s.denseShardCapacity = shardCapacity; s.bounce = depth;
            if (depth == 0u) s.beam = beam;
            launchTraceStep(c, s, useWide(c));
        }
        // bounce `depth`: shades the live paths; folds the visibility results of the previous bounce's zombies in (the last round does only that)
        const DenseCounts dc = { l.denseCounts + (size_t)plane * depth, l.denseCounts + (size_t)plane * (depth + 1u), shardCapacity, c->deviceFlags,
                                 depth == 0u ? c->slotPixel : nullptr, stage, numPasses };
        LaunchTimer t(c, l.stream, KC_SHADE);
        if (c->plainPathTracer) RT_LAUNCH_SHADE_DENSE(0, true, false);
        else if (denseAll) { if (c->leanScene == 1) RT_LAUNCH_SHADE_DENSE(1, false, true); else if (c->leanScene == 2) RT_LAUNCH_SHADE_DENSE(2, false, true); else if (c->leanScene == 4) RT_LAUNCH_SHADE_DENSE(4, false, true); else RT_LAUNCH_SHADE_DENSE(0, false, true); }
        else if (c->leanScene == 1) RT_LAUNCH_SHADE_DENSE(1, false, false); else if (c->leanScene == 2) RT_LAUNCH_SHADE_DENSE(2, false, false);
        else if (c->leanScene == 3) RT_LAUNCH_SHADE_DENSE(3, false, false); else if (c->leanScene == 4) RT_LAUNCH_SHADE_DENSE(4, false, false); else RT_LAUNCH_SHADE_DENSE(0, false, false);
    }
    return RTGPU_OK;
}
#undef RT_LAUNCH_SHADE_DENSE
#undef RT_LAUNCH_SHADE_DENSE_STAGE
#undef RT_LAUNCH_TAIL

// The bounces of a slot-per-pixel sequence on lane `l` (a batch lane or the recorder's), after its k_generate.  Bounce k: trace {closest-hit rays of bounce k,
// next-event rays of bounce k - 1} -> shade(k); one last trace for the next-event rays of the final bounce.
template <class Shade>
static void launchSlotBounces(RtgpuContext* c, hipStream_t stream, unsigned long long* counters, const BatchLane& l, const LaneCounts& counts, uint32_t maxRayDepth, uint32_t lastDepth,
                              bool haveNee, Shade shade)
{
    for (uint32_t depth = 0; depth <= lastDepth; ++depth)
    {
        const bool haveClosest = depth <= maxRayDepth, haveShadow = depth > 0 && haveNee;
        if (haveClosest || haveShadow)
        {
            TraceStep s = { stream, counters, l.paths };
            counts.queuesOf(s, depth, haveClosest, haveShadow);
            counts.handOverOf(s, depth);
            launchTraceStep(c, s, useWide(c));
        }
        if (haveClosest) shade(depth);
    }
}

// k_generate of a slot-per-pixel sequence (a batch lane's, the recorder's, the AOV calls'): from the camera, or from the ray source where one is set
static void launchGenerate(RtgpuContext* c, dim3 grid, hipStream_t stream, const DevPass* passesDev, uint32_t slotsPerPass, const Paths& paths, const uint32_t* slotPixel,
                           uint32_t totalSlots, uint32_t* queue, uint32_t* queueCount, unsigned long long* counters)
{
    if (c->raySource.kind == 2u)
        hipLaunchKernelGGL(k_generate_lens, grid, dim3(RT_BLOCK), 0, stream, c->sceneDev, passesDev, slotsPerPass, paths, slotPixel, totalSlots, queue, queueCount, counters, c->raySource.table, c->raySource.lens, c->raySource.bokehShape);
    else if (c->raySource.kind == 1u)
        hipLaunchKernelGGL(k_generate_rays, grid, dim3(RT_BLOCK), 0, stream, c->sceneDev, passesDev, slotsPerPass, paths, slotPixel, totalSlots, queue, queueCount, counters, c->raySource.table);
    else hipLaunchKernelGGL(k_generate, grid, dim3(RT_BLOCK), 0, stream, c->sceneDev, passesDev, slotsPerPass, paths, slotPixel, totalSlots, queue, queueCount, counters);
}

#define RT_LAUNCH_SHADE(...) hipLaunchKernelGGL((k_shade<__VA_ARGS__>), grid, block, 0, l.stream, c->sceneDev, passesDev, c->numSlots, l.paths, l.queues[depth & 1u], counts.pathCounts + depth, \
                                             l.queues[(depth + 1u) & 1u], counts.pathCounts + depth + 1, l.shadowQueues[depth & 1u], counts.shadowCounts + depth, c->counters)

// The bounces of a batch whose path state stays in the pixel's slot (the first layout: many lights per vertex, the debug renderer, RTGPU_NO_DENSE=1)
static void submitSlotBatch(RtgpuContext* c, BatchLane& l, const LaneCounts& counts, const DevPass* passesDev, uint32_t totalSlots, uint32_t maxRayDepth, dim3 grid)
{
    const dim3 block(RT_BLOCK);
    {
        LaunchTimer t(c, l.stream, KC_GENERATE);
        launchGenerate(c, grid, l.stream, passesDev, c->numSlots, l.paths, c->slotPixel, totalSlots, l.queues[0], counts.pathCounts + 0, c->counters);
    }
    launchSlotBounces(c, l.stream, c->counters, l, counts, maxRayDepth, c->debugMode >= 0 ? 0u : maxRayDepth + 1u, c->numLights != 0 && !c->plainPathTracer, [&](uint32_t depth)
    {
        LaunchTimer t(c, l.stream, KC_SHADE);
        if (c->debugMode >= 0)
            hipLaunchKernelGGL(k_debug_shade, grid, block, 0, l.stream, c->sceneDev, l.paths, l.queues[0], counts.pathCounts + 0, (uint32_t)c->debugMode, c->counters);
        else if (c->plainPathTracer) RT_LAUNCH_SHADE(false, true);
        else if (c->leanScene == 1) RT_LAUNCH_SHADE(true); else RT_LAUNCH_SHADE(false);
    });
}
#undef RT_LAUNCH_SHADE

// Submits the queued passes as one batch: generate -> {trace -> shade} per bounce -> trace -> accumulate.
static int flushBatch(RtgpuContext* c, uint32_t maxPasses)
{
    if (c->pending.empty()) return RTGPU_OK;
    HIP_TRY(hipSetDevice(c->device));
    uint32_t numPasses = maxPasses && maxPasses < c->pending.size() ? maxPasses : (uint32_t)c->pending.size();
    const DevPass& first = c->pending[0].pass;
    const uint32_t maxLights = first.lightSamplingStrategy == RT_LIGHT_SAMPLING_ALL ? c->numLights : 1u;
    BatchLane& l = c->lanes[c->nextLane];
    const int laneIndex = (int)c->nextLane;
    c->nextLane = (c->nextLane + 1u) % c->numLanes;
    // all lanes get their arenas with the first batch: a 3 GB hipMalloc costs tens of milliseconds
    int r = RTGPU_OK;
    for (uint32_t i = 0; i < c->numLanes && r == RTGPU_OK; ++i) r = ensurePaths(c, c->lanes[i], maxLights, first.maxRayDepth);
    if (r) { c->pending.clear(); return r; }
    // The arenas may have been sized under a budget that shrank at allocation (several contexts on one device, little free memory): the batch
    // is what the lane's allocation holds, the rest stays queued for the next flush.
    {
        const size_t perPass = c->numSlots ? c->numSlots : 1u;
        // (dense path state: a path's home index shares a word with its pending-request count, rt_device_state.h -- whatever the lane budget allowed)
        while (numPasses > 1u && (arenaCapacityFor(perPass * numPasses) > l.paths.capacity || (l.paths2.base && (perPass * numPasses > l.homeCapacity || perPass * numPasses > RT_DENSE_MAX_HOME)))) --numPasses;
        if (arenaCapacityFor(perPass * numPasses) > l.paths.capacity || (l.paths2.base && perPass * numPasses > l.homeCapacity))
        {
            c->pending.clear();
            return fail(RTGPU_ERR_OUT_OF_MEMORY, "a batch lane's path-state arena does not hold one pass of this frame");
        }
        if (l.paths2.base && perPass * numPasses > RT_DENSE_MAX_HOME)
        {
            c->pending.clear();
            return fail(RTGPU_ERR_UNSUPPORTED, "one pass of this frame exceeds the home index range of dense path state");
        }
    }

    // contiguous ring slots for the batch (seeds + pass constants); wait until their previous users have finished
    if (c->seedCursor + numPasses > RT_SEED_RING) c->seedCursor = 0;
    const uint32_t firstSlot = c->seedCursor; c->seedCursor = (c->seedCursor + numPasses) % RT_SEED_RING;
    for (uint32_t i = 0; i < numPasses; ++i)
    {
        const uint32_t slot = firstSlot + i;
        if (c->seedEventUsed[slot]) HIP_TRY(hipEventSynchronize(c->seedEvents[slot]));
        uint32_t* seedHost = c->seedRingHost + (size_t)slot * RTGPU_MAX_DIMENSIONS;
        uint32_t* seedDev = c->seedRingDev + (size_t)slot * RTGPU_MAX_DIMENSIONS;
        CtxPending& pd = c->pending[i];
        if (!pd.seeds.empty()) memcpy(seedHost, pd.seeds.data(), pd.seeds.size() * sizeof(uint32_t));
        pd.pass.seed = seedDev;
        c->passRingHost[slot] = pd.pass;
    }
    // the batch's ring slots are contiguous: ONE copy for the seeds of all its passes and one for their constants (a copy per pass in front of a 20-pass
    // batch of a small frame was 0.25 ms of stream time before the first kernel, profiles/r04_timeline_serial_shard8.txt)
    HIP_TRY(hipMemcpyAsync(c->seedRingDev + (size_t)firstSlot * RTGPU_MAX_DIMENSIONS, c->seedRingHost + (size_t)firstSlot * RTGPU_MAX_DIMENSIONS,
                           (size_t)numPasses * RTGPU_MAX_DIMENSIONS * sizeof(uint32_t), hipMemcpyHostToDevice, l.stream));
    HIP_TRY(hipMemcpyAsync(c->passRingDev + firstSlot, c->passRingHost + firstSlot, numPasses * sizeof(DevPass), hipMemcpyHostToDevice, l.stream));
    const DevPass* passesDev = c->passRingDev + firstSlot;

    const uint32_t totalSlots = c->numSlots * numPasses;
    const uint32_t maxBlocks = c->numCUs * knobs::shadeBlocksPerCU();   // tuning knob
    const uint32_t blocksNeeded = (totalSlots + RT_BLOCK - 1) / RT_BLOCK;
    const uint32_t pixelBlocks = (c->numSlots + RT_BLOCK - 1) / RT_BLOCK;
    const dim3 grid(blocksNeeded < maxBlocks ? blocksNeeded : maxBlocks), pixelGrid(pixelBlocks < maxBlocks ? pixelBlocks : maxBlocks), block(RT_BLOCK);
    const LaneCounts counts(l);

    HIP_TRY(hipMemsetAsync(l.queueCounts, 0, laneCountBytes(l), l.stream));
    const bool dense = c->denseAllowed && c->debugMode < 0 && maxLights <= RT_DENSE_MAX_LIGHTS && l.paths2.base != nullptr;
    const bool denseAll = dense && first.lightSamplingStrategy == RT_LIGHT_SAMPLING_ALL && !c->plainPathTracer;
    if (dense)
    {
        BeamLists beam = {};
        r = beamListsFor(c, l, laneIndex, c->passRingHost + firstSlot, passesDev, numPasses, beam); if (r) return r;
        r = submitDenseBatch(c, l, counts, passesDev, totalSlots, first.maxRayDepth, denseAll, grid, first.numDimensions, beam); if (r) return r;
    }
    else submitSlotBatch(c, l, counts, passesDev, totalSlots, first.maxRayDepth, grid);

    // the film is summed in pass order: this batch's accumulate runs after the previous batch's
    if (c->lastAccumulateLane >= 0 && c->lastAccumulateLane != laneIndex) HIP_TRY(hipStreamWaitEvent(l.stream, c->lanes[c->lastAccumulateLane].accumulated, 0));
    {
        LaunchTimer t(c, l.stream, KC_ACCUMULATE);
        if (dense) hipLaunchKernelGGL(k_accumulate_home, pixelGrid, block, 0, l.stream, l.home, c->slotPixel, c->numSlots, numPasses, c->sum, c->secondary, c->width, passesDev);
        else hipLaunchKernelGGL(k_accumulate, pixelGrid, block, 0, l.stream, l.paths, c->numSlots, numPasses, c->sum, c->secondary, c->width, passesDev, c->counters);
    }
    HIP_TRY(hipEventRecord(l.accumulated, l.stream));
    c->lastAccumulateLane = laneIndex;
    c->pending.erase(c->pending.begin(), c->pending.begin() + numPasses);
    c->batchesSinceSync++;
    // a stream starts with small batches (a caller that renders 4 or 8 passes and reads back gets two or three overlapping launch
    // sequences instead of one: +7 %) and grows while the caller keeps streaming
    if (!c->passBatchFromEnv && c->numSlots >= 400000u && numPasses == c->passBatch && ++c->batchesAtThisSize >= c->numLanes)
    {
        // every lane has one batch of this size in flight: the next round of the lanes carries twice as many passes
        uint32_t next = c->passBatch * 2u;
        if (next > maxStreamingBatch(c)) next = maxStreamingBatch(c);
        if (next > c->passBatch) { c->passBatch = next; c->batchesAtThisSize = 0; }
    }
    HIP_TRY(hipGetLastError());
    for (uint32_t i = 0; i < numPasses; ++i)
    {
        HIP_TRY(hipEventRecord(c->seedEvents[firstSlot + i], l.stream));
        c->seedEventUsed[firstSlot + i] = true;
    }
    return RTGPU_OK;
}

// Submits everything that is queued.  What is left when the caller stops streaming (a synchronising call, a parameter change) goes out
// as one batch per free lane instead of one batch: the launch sequences of the parts overlap, which hides the tails of their persistent
// launches (20 passes between read-backs: 8 + 12 -> 8 + 6 + 6 on three lanes).  Results do not depend on the split.
static int flushPending(RtgpuContext* c)
{
    if (c->pending.empty()) return RTGPU_OK;
    uint32_t parts = 1;
    if (c->numSlots >= 400000u && !c->passBatchFromEnv && !c->vcm.enabled)
    {
        const uint32_t lanesFree = c->batchesSinceSync ? c->numLanes - 1u : c->numLanes;
        parts = (uint32_t)c->pending.size() / 2u;
        if (parts > lanesFree) parts = lanesFree;
        if (parts < 1u) parts = 1u;
    }
    const uint32_t each = ((uint32_t)c->pending.size() + parts - 1u) / parts;
    while (!c->pending.empty()) { const int r = flushBatch(c, each); if (r) return r; }
    return RTGPU_OK;
}
