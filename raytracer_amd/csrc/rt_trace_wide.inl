// rt_trace_wide.inl -- traversal of single-mesh scenes over a 4-WIDE tree collapsed from the reference's binary tree (same SAH splits,
// same leaves), one ray per lane.  Device only; included by rt_trace.hip and rt_tail.hip after rt_wide_grid.inl, whose exactness argument it
// shares; the device parts it has in common with the other 4-wide walks (slab test, hand-over lists, request ray, fold, interior step, mesh leaf, finish, tallies) are
// rt_wide_walk.h.  The tree's format (WideBvh, node records, gates) is rt_wide_format.h; the host builds it in rt_scene_prepare.h (buildQuantBvh, buildWideBvh).
//
// Why.  k_trace waits ~0.8 us per dependent node fetch with 20 waves per CU to hide it: the walk is a chain of ~29 round
// trips per ray.  Two earlier attempts changed what a round trip moves -- half the bytes (k_trace_quant: no gain, the conversions ate
// it), a quad of lanes per ray (1.7x slower, instruction bound) -- not how many there are.  A 4-wide node shortens the chain to 17: one
// round trip fetches four children (64 bytes: four of k_trace_quant's 16-byte records), i.e. two levels of the binary tree at once, and
// the per-step overhead (stack, loop, scheduling ballots) is paid half as often.
// What came of it (profiles/r02_wide_*): the kernel is no longer latency-bound but ISSUE-bound -- vector ALU busy 90 % at 57 % lane
// utilisation -- so what counts is instructions per visit (137 after the permute / pair-sort step below, 161 before): 164.5 -> 147 ms
// per 69 passes of the benchmark against k_trace.  Variants that add live state (a leaf set aside, shared any-hit rays in the drain phase,
// fat leaves, one gate per ray, deferred children in slot order, one-wave blocks) spilled on the 96-VGPR cliff or lost otherwise; their
// measurements are in profiles/r02_wide_diag.txt and DESIGN 4, their code is in the history (round 2), not here.
//
// Exactness: the argument of rt_wide_grid.inl word for word (conservative boxes visit a superset of the reference's leaves in another order;
// a leaf's triangles count only behind the leaf's exact box; runner-up within tol, zero direction components, far origins -> the
// binary-tree kernel decides), plus one more hand-over: a ray whose stack would overflow.

#define RT_WIDE_STACK 16           // stack entries per lane of the 4-wide walk
#define RT_WIDE_PARK 6u            // words per lane behind the stack (traceWideLoop's `park`)
#define RT_WIDE_LOCAL_EXACT 256u   // per block and kind: ~40 x what a block of the benchmark hands over per launch

// The walk as a device function (k_trace_wide below; k_tail, rt_tail.hip, runs it over a block's own queues in LDS: `queue`, `shadowQueue`,
// the counts and `cursor` are generic pointers, `sharingWaves` = the waves that claim from `cursor`).
template <int kStack, bool kDiag = false>
RT_DEV void traceWideLoop(const RtSceneDesc& scene, const WideBvh& bvh, const Paths& paths, const uint32_t* queue, const uint32_t* queueCount,
                          const uint32_t* shadowQueue, const uint32_t* shadowCount, uint32_t* cursor, unsigned long long* counters, const WideTuning& tune,
                          const WideLocal& handOver, uint32_t* sStack, uint32_t* sDensePrefix, uint32_t sharingWaves)
{
    uint32_t* const stack = sStack + threadIdx.x;   // entry e at stack[e * RT_BLOCK]: bank = lane, conflict free at any depth
    // Behind the stack's kStack entries: RT_WIDE_PARK words per lane that only the leaf phase reads -- the local ray's invDir and originDivDir, which the
    // exact box test of a leaf needs (round 5: rebuilding them there cost three IEEE divisions, ~100 of the leaf phase's 320 instructions, every time
    // some lane of the wave had a triangle hit to confirm)
    float* const park = reinterpret_cast<float*>(sStack + kStack * RT_BLOCK) + threadIdx.x;
    if (tune.denseCounts) { denseLoadPrefix(tune.denseCounts, sDensePrefix); __syncthreads(); }
    const uint32_t numClosest = tune.denseCounts ? sDensePrefix[RT_DENSE_SHARDS] : (queueCount ? *queueCount : 0u);
    const uint32_t count = numClosest + (shadowCount ? *shadowCount : 0u);
    // the mesh object's inverse transform is fetched per refill through the constant address space (scalar loads of a uniform address): sixteen scalar registers
    // less across the whole loop, whose header spilled a dozen of them into vector lanes every iteration
    typedef const __attribute__((address_space(4))) float* ConstF;
    const ConstF invTransformWords = (ConstF)(uintptr_t)scene.objects[0].invTransform;
    const RtTriangle* const tris = scene.triangles + scene.meshes[scene.objects[0].meshIndex].firstTriangle;
    const float inf = __uint_as_float(0x7f800000u);

    // per-lane ray state
    float ox = 0, oy = 0, oz = 0, dx = 0, dy = 0, dz = 0;     // local ray (triangle tests, leaf gate)
    float ax = 0, ay = 0, az = 0, bx = 0, by = 0, bz = 0;     // folded slab constants: t(q) = fma(q, a, b)
    float best = 0, second = 0, tol = 0;
    uint32_t cur = RT_QUANT_DONE, sp = 0, slot = 0, light = 0;
    bool have = false, shadow = false, occluded = false, exhausted = false, overflow = false;
    // tallies per WAVE (ballots at wave-uniform points of the loop: scalar registers; as per-lane counters they were four of the 96 vector registers)
    uint32_t numRetraced = 0, numShadowRays = 0, numUntrusted = 0, numOverflow = 0;
    uint32_t diagVisits = 0, diagSlots = 0, diagLeaves = 0;   // kDiag: interior visits, lane slots of the interior loop (64 per wave step), leaf visits
    uint32_t diagGates = 0, diagHitWrites = 0;                // kDiag, RTGPU_WIDE_DIAG=3: exact-box fetches and hit records written through, per lane and launch (the walk's byte model, bench.py)
    uint32_t diagMaxSp = 0, diagDeep[3] = { 0u, 0u, 0u };     // kDiag, RTGPU_WIDE_DIAG=2: rays whose stack held more than 9 / 13 / 17 entries (what a 12 / 16 / 20-entry stack would hand over)

    uint32_t chunkSize = count / (sharingWaves * 4u);
    chunkSize = chunkSize < tune.chunkMin ? tune.chunkMin : (chunkSize > 1024u ? 1024u : chunkSize);
    WaveChunk chunk = { 0u, 0u };

    // kDiag: wave clock per phase (0 refill, 1 interior loop, 2 leaf / finish) and the number of times each ran
    unsigned long long diagClock[3] = { 0ull, 0ull, 0ull }, diagPrev = kDiag ? (unsigned long long)clock64() : 0ull, diagStart = diagPrev;
    uint32_t diagRuns[3] = { 0u, 0u, 0u }, diagPhase = 0u, diagClaims = 0u;
    unsigned long long diagClaimClock = 0ull, diagExhausted = 0ull;   // when this wave found the work queue empty   // inside the refill phase: waiting for the work cursor's atomic
    uint32_t drainIterations = 0u;   // (wave-uniform) loop iterations since the work queue ran dry
    for (;;)
    {
        if (kDiag) { const unsigned long long now = (unsigned long long)clock64(); diagClock[diagPhase] += now - diagPrev; diagPrev = now; }
        if (exhausted && tune.drainAbortAfter != 0u && ++drainIterations == tune.drainAbortAfter && have) { overflow = true; cur = RT_QUANT_DONE; }
        const bool interior = have && (cur >> RT_NODE_LEAVES_SHIFT) == 0u;
        const bool other = have && !interior;      // at a leaf, or finished
        const unsigned long long mI = __ballot(interior), mO = __ballot(other);
        const uint32_t nIdle = 64u - (uint32_t)__popcll(mI) - (uint32_t)__popcll(mO);
        if (!exhausted && (nIdle == 64u || nIdle >= tune.refillMinIdle))
        {
            // ---- refill ----
            if (kDiag) { diagPhase = 0u; diagRuns[0]++; }
            if (chunk.next >= chunk.end)
            {
                const unsigned long long claim0 = kDiag ? (unsigned long long)clock64() : 0ull;
                waveClaimChunk(chunk, cursor, chunkSize, count);
                if (kDiag) { diagClaimClock += (unsigned long long)clock64() - claim0; diagClaims++; }
                if (chunk.next >= chunk.end) { exhausted = true; if (kDiag) diagExhausted = (unsigned long long)clock64(); continue; }
            }
            uint32_t idx = waveTake(!have, chunk);
            bool tookUntrusted = false, tookShadow = false;
            if (idx != 0xFFFFFFFFu)
            {
                shadow = idx >= numClosest;
                const uint32_t request = shadow ? shadowQueue[idx - numClosest]
                                                : (tune.denseCounts ? denseLiveSlot(sDensePrefix, tune.denseShardCapacity, idx) : (queue ? queue[idx] : idx));
                float maxDistance = inf;
                float4 origin, dir;
                if (shadow)
                {
                    // request = light * capacity + slot; one request per vertex (LightSamplingStrategy::Single: the arena holds one light's records) needs no division
                    if (paths.maxLights == 1u) { light = 0u; slot = request; } else { light = request / paths.capacity; slot = request - light * paths.capacity; }
                    origin = ldStream(prec(paths, shadowOriginRecord(paths), slot)); dir = ldStream(pshadow(paths, light, 0, slot));
                    maxDistance = dir.w;           // hitPoint.distance = illuminateResult.distance * 0.999f
                }
                else
                {
                    slot = request; light = 0u;
                    origin = ldStream(prec(paths, R_ORIGIN, slot)); dir = ldStream(prec(paths, R_DIR, slot));
                }
                const Ray world = wideWorldRay(origin, dir, shadow, tune.shadowOffset);   // one ray construction for both kinds of request (a wave usually refills both at once)
                M4 invTransform;
                for (int r = 0; r < 4; ++r) invTransform.r[r] = V4(invTransformWords[4 * r], invTransformWords[4 * r + 1], invTransformWords[4 * r + 2], invTransformWords[4 * r + 3]);
                const Ray local = makeRayUnsafe3(transformPoint(invTransform, world.origin), transformVector(invTransform, world.dir));   // = transformRayUnsafe: MeshShape is entered in object space, Scene.cpp:128-145
                RT_WIDE_FOLD_TEST(local, bvh)
                if (!trusted)
                {
                    // a zero direction component (NaNs in the reference's slab test) or an origin far outside the mesh: the reference's walk only
                    widePushExact(tune, handOver, shadow, shadow ? request : slot);
                    tookUntrusted = true;
                }
                else
                {
                    ox = local.origin.x; oy = local.origin.y; oz = local.origin.z; dx = local.dir.x; dy = local.dir.y; dz = local.dir.z;
                    RT_WIDE_FOLD_SET(local, bvh)
                    park[0] = local.invDir.x; park[RT_BLOCK] = local.invDir.y; park[2 * RT_BLOCK] = local.invDir.z;
                    park[3 * RT_BLOCK] = local.originDivDir.x; park[4 * RT_BLOCK] = local.originDivDir.y; park[5 * RT_BLOCK] = local.originDivDir.z;
                    tol = shadow ? 0.0f : RT_WIDE_FOLD_TOL;
                    best = maxDistance; second = inf; occluded = false; overflow = false;
                    sp = 0u; cur = 0u;   // node 0 holds the children of the binary tree's root
                    if (kDiag) diagMaxSp = 0u;
                    have = true;
                    tookShadow = shadow;   // (a request handed to the binary-tree kernel is counted there)
                }
            }
            { const uint32_t n = (uint32_t)__popcll(__ballot(tookUntrusted)); numRetraced += n; numUntrusted += n; numShadowRays += (uint32_t)__popcll(__ballot(tookShadow)); }
            continue;
        }
        if ((mI | mO) == 0ull) break;
        if (mI != 0ull && (uint32_t)__popcll(mO) < tune.otherMinLanes)
        {
            // ---- interior phase: four conservative slab tests per step, until enough lanes wait at a leaf or are finished ----
            if (kDiag) { diagPhase = 1u; diagRuns[1]++; }
            bool in = interior;
            const float limit = best + (tol + tol);
            // which plane of an axis the ray meets first: byte selectors of the slab test, rebuilt per phase (three registers less across the leaf and refill phases)
            const uint32_t selX = ax < 0.0f ? RT_WIDE_SEL_X_NEG : RT_WIDE_SEL_X_POS, selY = ay < 0.0f ? RT_WIDE_SEL_Y_NEG : RT_WIDE_SEL_Y_POS, selZ = az < 0.0f ? RT_WIDE_SEL_Z_NEG : RT_WIDE_SEL_Z_POS;
            for (;;)
            {
                if (kDiag) { diagSlots++; if (in) diagVisits++; }
                if (in)
                {
                    const WideStep next = wideInteriorStep(bvh.nodes + 4u * cur, stack, 0u, sp, ax, ay, az, bx, by, bz, selX, selY, selZ, limit, tol);
                    cur = next.cur; sp = next.sp;
                    if (kDiag && sp > diagMaxSp) diagMaxSp = sp;
                    if (sp + 3u > (uint32_t)kStack) { overflow = true; cur = RT_QUANT_DONE; }   // the next step could not push: the binary-tree kernel takes the ray
                }
                in = in && (cur >> RT_NODE_LEAVES_SHIFT) == 0u;
                const unsigned long long m = __ballot(in);
                if (m == 0ull || 64u - nIdle - (uint32_t)__popcll(m) >= tune.otherMinLanes) break;
            }
        }
        else
        {
        if (kDiag) { diagPhase = 2u; diagRuns[2]++; }
        bool handedOver = false, overflowed = false, uncountShadow = false;
        if (other)
        {
            // ---- leaves (the current one and the one set aside): MeshShape::Traverse_Leaf(_Shadow), MeshShape.cpp:134-207 ----
            for (int once = 0; once < 1; ++once)
            {
                const uint32_t leaf = cur;
                if (!RT_WIDE_IS_LEAF(leaf) || occluded) continue;
                if (kDiag) diagLeaves++;
                const uint32_t first = leaf & RT_NODE_CHILD_MASK;
                Ray ray; ray.origin = V4(ox, oy, oz, 0.0f); ray.dir = V4(dx, dy, dz, 0.0f);
                float u0, v0_, t0, u1, v1, t1;
                const float lo = wideLeafPair(tris, leaf, ray, t0, u0, v0_, t1, u1, v1);
                if (lo < best + tol)
                {
                    // a hit that matters: it counts only if the ray passes the leaf's exact box, as in the reference's walk
                    if (kDiag) diagGates++;
                    Ray gateRay;   // = the ray transformRayUnsafe built at refill (makeRayUnsafe3 of the same origin and direction: its quotients were parked then)
                    gateRay.origin = ray.origin; gateRay.dir = ray.dir;
                    gateRay.invDir = V4(park[0], park[RT_BLOCK], park[2 * RT_BLOCK], 0.0f);
                    gateRay.originDivDir = V4(park[3 * RT_BLOCK], park[4 * RT_BLOCK], park[5 * RT_BLOCK], 0.0f);
                    float entry;
                    const bool pass = wideLeafGate(bvh.gate, first, gateRay, shadow, best, entry);
                    if (pass)
                    {
                        if (shadow) { if (lo < best) occluded = true; }
                        else
                        {
                            const bool wrote = wideAcceptPair(paths, slot, 0u, first, t0, u0, v0_, t1, u1, v1, lo, entry, tol, best, second);
                            if (kDiag && wrote) diagHitWrites++;
                        }
                    }
                }
            }
            if (occluded) cur = RT_QUANT_DONE;
            if (cur != RT_QUANT_DONE)
            {
                if (sp == 0u) cur = RT_QUANT_DONE;
                else { --sp; cur = stack[sp * RT_BLOCK]; }
            }
            if (cur == RT_QUANT_DONE)
            {
                // ---- finished ----
                if (kDiag) { if (diagMaxSp > 9u) diagDeep[0]++; if (diagMaxSp > 13u) diagDeep[1]++; if (diagMaxSp > 17u) diagDeep[2]++; }
                handedOver = wideFinishRay(paths, tune, handOver, shadow, light, slot, overflow, occluded, best, second, tol);
                overflowed = overflow;
                uncountShadow = overflow && shadow;   // counted by the kernel that resolves it
                have = false;
            }
        }
        numRetraced += (uint32_t)__popcll(__ballot(handedOver)); numOverflow += (uint32_t)__popcll(__ballot(overflowed)); numShadowRays -= (uint32_t)__popcll(__ballot(uncountShadow));
        }
    }
    // counters: shadow rays traced here, rays handed to the binary-tree kernel
    __shared__ uint32_t sTally[4];
    // tallies per wave (lane 0 of each adds), sTally not yet cleared; the diagnostic instantiation keeps the two spare counters for its own use below
    wideFlushTallies<15u>(sTally, false, (threadIdx.x & 63u) == 0u, numShadowRays, numRetraced, numUntrusted, numOverflow, !kDiag, counters);
    if (kDiag)
    {
        // RTGPU_WIDE_DIAG=1: the three spare counters hold the walk's statistics instead
        const bool deep = tune.localExact == 2u, bytes = tune.localExact == 3u;   // (the diagnostic kernel has no block-local lists: the field carries RTGPU_WIDE_DIAG's mode)
        atomicAdd(&counters[RT_COUNTER_RETRACED + 1], (unsigned long long)(deep ? diagDeep[0] : diagVisits));
        atomicAdd(&counters[RT_COUNTER_RETRACED + 2], (unsigned long long)(bytes ? diagGates : (deep ? diagDeep[1] : diagSlots)));   // 3: exact-box fetches
        atomicAdd(&counters[RT_COUNTER_RETRACED + 3], (unsigned long long)(deep ? diagDeep[2] : diagLeaves));
        // 3: the hit records written through get a 64-bit slot of their own (round 5 packed them into the upper half of the exact-box count, which wraps into
        // them past 2^32 boxes -- a 256-pass bench run is within a factor of two of that): the reference's shadow triangle-test counter, free in this walk; the
        // phase clocks that otherwise ride in these slots are not written in this mode
        if (bytes) atomicAdd(&counters[C_TRI_SHADOW], (unsigned long long)diagHitWrites);
        else if ((threadIdx.x & 63u) == 0u)
        {
            // the reference's intersection counters are not used by this walk: per-wave clocks and phase counts ride in their slots
            atomicAdd(&counters[C_BOX], diagClock[0]); atomicAdd(&counters[C_BOX_PASS], diagClock[1]); atomicAdd(&counters[C_TRI], diagClock[2]);
            atomicAdd(&counters[C_TRI_PASS], (unsigned long long)clock64() - diagStart);
            atomicAdd(&counters[C_BOX_SHADOW], (unsigned long long)diagRuns[1]);
            atomicAdd(&counters[C_TRI_SHADOW], diagExhausted ? diagPrev - diagExhausted : 0ull);   // the wave's drain phase: from the empty queue to its last ray
            atomicAdd(&counters[C_ANALYTIC_HITS], (unsigned long long)diagRuns[0]);   // (free in a mesh-only scene)
            atomicAdd(&counters[C_PRIMARY], diagClaimClock); atomicAdd(&counters[C_SHADOW_HIT], (unsigned long long)diagClaims);   // (k_shade adds to these two as well: subtract a run without RTGPU_WIDE_DIAG)
        }
    }
}


// kLocalExact: the block traces the rays its walk does not decide itself (small frames: rtgpu_set_schedule / launchTraceWide's policy).  A template
// parameter, not a run-time switch: the second walk's state cost the full-frame instantiation 148 bytes of scratch per lane and 2 KB of LDS
// (profiles/r04_kernel_stats_serial.txt against r03's) although a full frame never runs it.
template <int kStack, bool kDiag = false, bool kLocalExact = false>
__global__ void __launch_bounds__(RT_BLOCK) __attribute__((amdgpu_waves_per_eu(kStack <= 24 ? 5 : 1))) k_trace_wide(const RtSceneDesc scene, const WideBvh bvh, const Paths paths,
                                                         const uint32_t* __restrict__ queue, const uint32_t* __restrict__ queueCount,
                                                         const uint32_t* __restrict__ shadowQueue, const uint32_t* __restrict__ shadowCount,
                                                         uint32_t* __restrict__ cursor, unsigned long long* counters, const WideTuning tune)
{
    // the 4-wide walk's own stack: RT_WIDE_STACK entries per lane (measured on the benchmark frame, RTGPU_WIDE_DIAG=2: 18 of 48.8 M rays ever hold
    // more than 13 deferred children, none more than 17 -- profiles/r05_wide_diag_phases.txt; a ray that would need more goes to the re-trace launch)
    // + the parked words; the block-local second walk runs the reference's binary walk on kStack entries of the same memory
    constexpr int kWords = kLocalExact && kStack > RT_WIDE_STACK + (int)RT_WIDE_PARK ? kStack : RT_WIDE_STACK + (int)RT_WIDE_PARK;
    __shared__ uint32_t sStack[kWords * RT_BLOCK];
    __shared__ uint32_t sDensePrefix[RT_DENSE_SHARDS + 1u];
    if constexpr (!kLocalExact)
    {
        const WideLocal none = { nullptr, nullptr, nullptr, nullptr, 0u };
        traceWideLoop<RT_WIDE_STACK, kDiag>(scene, bvh, paths, queue, queueCount, shadowQueue, shadowCount, cursor, counters, tune, none, sStack, sDensePrefix, gridDim.x * ((uint32_t)RT_BLOCK / 64u));
    }
    else
    {
        __shared__ uint32_t sLocalExact[RT_WIDE_LOCAL_EXACT], sLocalShadow[RT_WIDE_LOCAL_EXACT], sLocalCounts[4];   // counts: closest, any-hit, work cursor of the second walk
        if (threadIdx.x < 4u) sLocalCounts[threadIdx.x] = 0u;
        __syncthreads();
        const WideLocal local = { sLocalExact, &sLocalCounts[0], sLocalShadow, &sLocalCounts[1], RT_WIDE_LOCAL_EXACT };
        traceWideLoop<RT_WIDE_STACK, kDiag>(scene, bvh, paths, queue, queueCount, shadowQueue, shadowCount, cursor, counters, tune, local, sStack, sDensePrefix, gridDim.x * ((uint32_t)RT_BLOCK / 64u));
        // the rays this block's walk did not decide, by the reference's own walk (block-uniform branch: the counts are final behind the walk's barrier)
        __syncthreads();
        if (threadIdx.x < 2u && sLocalCounts[threadIdx.x] > RT_WIDE_LOCAL_EXACT) sLocalCounts[threadIdx.x] = RT_WIDE_LOCAL_EXACT;
        __syncthreads();
        if (sLocalCounts[0] + sLocalCounts[1] != 0u)
        {
            // a degenerate closest-hit ray (an axis-parallel direction: it walks most of the tree) does not keep the block: past RT_ABORT_LOCAL_AFTER rounds
            // it goes to the launch's exact queue, i.e. to the re-trace launch behind this one (one block per CU instead of this block's slot of the traversal grid)
            const TravTuning exactTune = { tune.refillMinIdle, tune.otherMinLanes, tune.shadowOffset, tune.exactQueue, tune.exactCount, RT_ABORT_LOCAL_AFTER, nullptr, 0u, RT_RETRACE_SPLIT_AFTER };
            traceBinaryLoop<kStack, false>(scene, paths, sLocalExact, &sLocalCounts[0], sLocalShadow, &sLocalCounts[1], &sLocalCounts[2], counters, exactTune, sStack, sDensePrefix,
                                                  (uint32_t)RT_BLOCK / 64u);
        }
    }
}
