// rt_dense.inl -- PathTracerMIS / PathTracer passes with DENSE path state (LightSamplingStrategy::Single).  Included by rt_shade.hip (and rt_tail.hip for the vertex body).
//
// The first layout kept a path in the slot of its pixel for its whole life: after a few bounces the live slots are sparse, every
// 16-byte record access of k_shade pulls its own 64/128-byte line from HBM (measured: 3.1x the bytes the kernel needs, L2 hit rate
// 27 %, profiles/r02_diag0_pmc_8.txt) and costs its own L1 access.  Here the state ping-pongs between two arenas: k_shade_dense reads
// the records of bounce k at consecutive slots and writes the survivors to consecutive slots of the other arena, so that every record
// access of every kernel is a fully coalesced 1 KB per wave.
//   * Slot allocation: a block counts its survivors in LDS and takes its range with ONE returning atomic per 256 vertices, on one of
//     RT_DENSE_SHARDS counters selected by the block index (a single word sustains only ~88 returning atomics per microsecond).  An
//     arena is therefore RT_DENSE_SHARDS regions; region s holds its live paths upwards from s * shardCapacity.
//   * A path that ends at a vertex whose next-event request still needs its shadow ray becomes a ZOMBIE: only what the resolution
//     needs is written, downwards from the top of the region; the next k_shade_dense folds the visibility result in and parks the
//     radiance.
//   * Finished paths park their radiance at home[pass * slotsPerPass + pixelSlot]; k_accumulate_home adds the passes of a batch to the
//     film per pixel in pass order -- the float sums are those of the reference's pass-after-pass accumulation, whatever order the
//     paths were compacted in.
// Arithmetic and consumption order of the samples are those of k_shade: denseShadeVertex calls the same vertex stages in the same sequence (misGlobalLights,
// misHitLight, misRoulette, misSampleBsdf, computeLightSample: rt_shade.inl) and keeps only what the layout decides -- record loads and stores, the pending
// request's resolution, next-event staging, zombies and home[].  The images are bit-identical.
#ifndef RT_SHADE_FUNCTIONS_ONLY
// k_generate for dense state (generatePaths, rt_device_state.h): slot i = home i; the regions of the first arena are simply filled one after the other
__global__ void __launch_bounds__(RT_BLOCK) k_generate_dense(const RtSceneDesc scene, const DevPass* __restrict__ passes, uint32_t slotsPerPass, const Paths paths,
                                                             const uint32_t* __restrict__ slotPixel, uint32_t numSlots, uint32_t shardCapacity, uint32_t* __restrict__ counts,
                                                             unsigned long long* counters)
{
    generatePaths<true>(RT_GRID_STRIDE, scene.blueNoise, passes, slotsPerPass, paths, slotPixel, numSlots, nullptr, CameraRayOf());
    generateShardCounts(counts, shardCapacity, counters, numSlots);
}

#endif   // RT_SHADE_FUNCTIONS_ONLY

// What a vertex leaves behind (denseShadeVertex): outcome 0 nothing (its radiance is parked at home[]), 1 a live path, 2 a zombie (radiance + one
// pending next-event request); the records of the survivor, for the caller to store -- k_shade_dense at a fresh dense slot of the other arena,
// k_tail (rt_tail.hip) in place.
struct DenseVertex
{
    uint32_t outcome;
    float4 oOrigin, oDir, oTp, oResult, oSampler, oRng;   // (oSampler.w: densePack(home, requests); with requests, stage[3][thread] holds R_SH_TP and, for a zombie, stage[2][thread] its R_ORIGIN)
    bool rayNeeded;      // the vertex's next-event request needs its shadow ray
    uint32_t rayMask;
};

// resolvePendingLightSamples (rt_shade.inl) over a dense arena: the verdict of a request rides in its contribution record (.w < 0: no ray was needed, or
// the walk found an occluder), and the records -- the contributions and the throughput at the vertex -- are fetched as ONE group: one wait, not three.
// Same sum, same order, same fma.
template <bool kAll>
RT_DEV void denseResolvePending(const Paths& in, uint32_t slot, uint32_t numRequests, V4 lightSamplingWeight, V4& resultColor, Counters& cnt)
{
    if (numRequests == 0u) return;
    const float4 tp = ldStream(prec(in, R_SH_TP, slot));
    V4 accumulated = zero4();
    bool any = false;
    const uint32_t n = kAll ? numRequests : 1u;
    for (uint32_t l = 0; l < n; ++l)
    {
        const float4 c = ldStream(pshadow(in, l, 1, slot));
        if (c.w < 0.0f) continue;
        accumulated = accumulated + V4(c.x, c.y, c.z, 0.0f);
        any = true;
        cnt.c[C_SHADOW_HIT]++;   // counters.numShadowRaysHit: the shadow ray reached the light (PathTracerMIS.cpp:96-99)
    }
    if (!any) return;
    accumulated = accumulated * lightSamplingWeight;
    resultColor = mulAdd(V4(tp.x, tp.y, tp.z, 0.0f), accumulated, resultColor);
}

// What k_shade_dense copies to LDS in front of its first vertex (rt_device_state.h: RT_STAGE_*): the scene's small tables and the seed rows of the batch's passes
struct DenseStageTables
{
    RtObject objects[RT_STAGE_MAX_OBJECTS];
    RtMesh meshes[RT_STAGE_MAX_MESHES];
    RtMaterial materials[RT_STAGE_MAX_MATERIALS];
    RtLight lights[RT_STAGE_MAX_LIGHTS];
    uint32_t globalLights[RT_STAGE_MAX_LIGHTS];
    uint32_t seeds[RT_STAGE_SEED_WORDS];   // row p: pass p of the batch, stageSeedRow(numDimensions) words
};
// all threads of the block; `bytes` is a multiple of 16 and both ends are 16-byte aligned
RT_DEV void denseStageCopy(void* dst, const void* src, uint32_t bytes)
{
    const uint4* __restrict__ s = (const uint4*)src;
    uint4* d = (uint4*)dst;
    for (uint32_t k = threadIdx.x; k < bytes / 16u; k += RT_BLOCK) d[k] = s[k];
}
// The block's copy of the tables (the host checked them against the capacities: denseStageMask) and, `seeds`, of the seed rows, made per launch from the
// device tables, so that rtgpu_update_objects and scene uploads need nothing extra.  All threads of the block; the caller synchronises.
RT_DEV void denseStageLoad(DenseStageTables& t, const RtSceneDesc& scene, const DevPass* __restrict__ passes, uint32_t numPasses, uint32_t numDims, bool seeds)
{
    denseStageCopy(t.objects, scene.objects, scene.numObjects * (uint32_t)sizeof(RtObject));
    denseStageCopy(t.meshes, scene.meshes, scene.numMeshes * (uint32_t)sizeof(RtMesh));
    denseStageCopy(t.materials, scene.materials, scene.numMaterials * (uint32_t)sizeof(RtMaterial));
    denseStageCopy(t.lights, scene.lights, scene.numLights * (uint32_t)sizeof(RtLight));
    if (threadIdx.x < scene.numGlobalLights) t.globalLights[threadIdx.x] = scene.globalLights[threadIdx.x];
    if (seeds)
    {
        // the ring rows are RTGPU_MAX_DIMENSIONS words apart: only the words the samplers read are copied (a row's tail up to the next multiple of four rides along)
        const uint32_t quads = stageSeedRow(numDims) / 4u;
        for (uint32_t k = threadIdx.x; k < numPasses * quads; k += RT_BLOCK)
        {
            const uint32_t p = k / quads, q = k - p * quads;
            ((uint4*)t.seeds)[k] = ((const uint4*)passes[p].seed)[q];
        }
    }
}

// The seed row of pass `row` of the batch: the staged copy (kStage 2) or the ring's row in memory
template <int kStage>
RT_DEV const uint32_t* denseSeedRow(const DevPass* __restrict__ passes, uint32_t row, const uint32_t* stagedSeeds, uint32_t seedRow)
{
    if (kStage == 2) return stagedSeeds + row * seedRow;
    return passes[row].seed;
}

// The body of PathTracerMIS::RenderPixel's loop for one path vertex (PathTracerMIS.cpp:276-395) over the records of arena `in` at `slot`;
// kPlain: PathTracer::RenderPixel (Core/Rendering/PathTracer.cpp:73-171).  `stage` = four LDS rows of RT_BLOCK float4 (the next-event request
// waits there, see k_shade_dense).
// kStage says where the launch-uniform tables are, at compile time, so that a staged table is LDS to the compiler and a table in memory is addressed as it
// always was: 0 in memory, all of them; 1 `scene`'s objects, meshes, materials, lights and global lights are the block's LDS copies, the seed rows are in
// memory; 2 the seed rows too (`stagedSeeds`, rows `seedRow` words apart).  k_tail runs kStage 0.
template <int kLean, bool kPlain, bool kAll, int kStage = 0>
__device__ __forceinline__ static void denseShadeVertex(const RtSceneDesc& scene, const DevPass* __restrict__ passes, uint32_t slotsPerPass, const DevPass& pass, const Paths& in,
                                                        uint32_t slot, bool zombie, V4 lightSamplingWeight, V4 bsdfSamplingWeight, float lightPickProbability,
                                                        float4 (*stage)[RT_BLOCK], float4* __restrict__ home, Counters& cnt, DenseVertex& v,
                                                        const uint32_t* __restrict__ primarySlotPixel = nullptr, const uint32_t* stagedSeeds = nullptr, uint32_t seedRow = 0u)
{
    // Bounce 0 (primarySlotPixel != null): k_generate_dense stores only what depends on the camera sample -- origin and direction.  The other five
    // records of a fresh path are functions of its slot (radiance 0 | pixel, throughput 1, home = slot, the sampler and the per-pixel generator as
    // the camera left them) and are rebuilt here instead of being written and read back: 64 of 96 bytes per path in each direction.
    // Two trips to memory before the geometry gather: every record whose address the slot alone decides is requested here, at the top (a zombie has only
    // the first two); the pending request's records follow as one group (denseResolvePending) as soon as R_SAMPLER.w says there is one.
    // (The plain path tracer has no requests to resolve, so nothing waits between the top and loadSampler: its R_RNG stays where it was, four registers
    // the tail's plain instantiation does not have.)
    constexpr bool kEarlyRng = !kPlain;
    const bool primary = primarySlotPixel != nullptr;
    float4 rResult, rSampler;
    float4 rOrigin = f4(0.0f, 0.0f, 0.0f, 0.0f), rDir = rOrigin, rHit = rOrigin, rRng = rOrigin, rTp = f4(1.0f, 1.0f, 1.0f, 1.0f);
    if (primary)
    {
        rResult = f4(0.0f, 0.0f, 0.0f, fbits(primarySlotPixel[slot - (slot / slotsPerPass) * slotsPerPass]));
        rSampler = f4(prec(in, R_SAMPLER, slot).x, 0.0f, 0.0f, fbits(densePack(slot, 0u)));   // .x: the hit's v, written by the traversal; no request is pending
    }
    else { rResult = ldStream(prec(in, R_RESULT, slot)); rSampler = ldStream(prec(in, R_SAMPLER, slot)); }
    if (!zombie)
    {
        rOrigin = ldStream(prec(in, R_ORIGIN, slot)); rDir = ldStream(prec(in, R_DIR, slot)); rHit = ldStream(prec(in, R_HIT, slot));
        if (!primary) { rTp = ldStream(prec(in, R_TP, slot)); if (kEarlyRng) rRng = ldStream(prec(in, R_RNG, slot)); }
    }
    const uint32_t pix = ubits(rResult.w), homeIndex = denseHome(ubits(rSampler.w));
    V4 resultColor(rResult.x, rResult.y, rResult.z, 0.0f);
    denseResolvePending<kAll>(in, slot, densePending(ubits(rSampler.w)), lightSamplingWeight, resultColor, cnt);   // NEE of the previous vertex
    if (!zombie)
    {
        const uint32_t flags = ubits(rOrigin.w);
        const uint32_t depth = flags & 0xFFu;
        const bool lastSpecular = (flags & 0x100u) != 0;
        const float lastPdfW = rDir.w;
        const Ray ray = makePathRay(rOrigin, rDir, depth);
        V4 throughput(rTp.x, rTp.y, rTp.z, rTp.w);
        const Hit hit = unpackHit(rHit, rSampler.x);
        uint32_t numRequests = 0;
        do
        {
            if (hit.objectId == RT_INVALID_OBJECT)
            {
                // EvaluateGlobalLights
                resultColor = mulAdd(throughput, misGlobalLights<kLean, kPlain>(scene, ray, depth, lastSpecular, lastPdfW, lightPickProbability, bsdfSamplingWeight), resultColor);
                break;
            }
            ShadingData sd;
            sd.intersection.material = (flags >> 9) - 1u;   // the previous vertex's material (see k_shade)
            if (hit.distance < FLT_MAX) sceneEvaluateIntersection<kLean>(scene, ray, hit, sd.intersection, cnt);
            if (!RT_LEAN(kLean) && hit.subObjectId == RT_LIGHT_OBJECT)
            {
                // EvaluateLight
                misHitLight<kPlain>(scene, hit, ray, sd.intersection, throughput, depth, lastSpecular, lastPdfW, lightPickProbability, bsdfSamplingWeight, resultColor);
                break;
            }
            sd.outgoingDirWorldSpace = neg(ray.dir);
            const RtMaterial& mat = scene.materials[sd.intersection.material];
            materialEvaluateShadingData<kLean>(scene, mat, sd);
            resultColor = mulAdd(throughput, kPlain ? sd.mp.emission : sd.mp.emission * bsdfSamplingWeight, resultColor);   // emission, :309-317

            Sampler sampler;
            if (primary)
            {
                // the sampler and the per-pixel generator as Camera::GenerateRay left them: reset as k_generate_dense does and let the camera draw again
                const DevPass& own = passes[homeIndex / slotsPerPass];
                const uint32_t x = pix & 0xFFFFu, y = pix >> 16;
                sampler.seed = denseSeedRow<kStage>(passes, homeIndex / slotsPerPass, stagedSeeds, seedRow); sampler.numDims = own.numDimensions; sampler.blueNoiseLayers = own.blueNoiseLayers; sampler.blueNoise = scene.blueNoise;
                sampler.resetPixel(x, y, own.rngKey[0], own.rngKey[1]);
                const float invW = 1.0f / (float)(int32_t)own.width, invH = 1.0f / (float)(int32_t)own.height;
                const V4 coords(((float)(int32_t)x + own.sampleOffset[0]) * invW, ((float)(int32_t)(own.height - 1u - y) + own.sampleOffset[1]) * invH, 0.0f, 0.0f);
                V4 cameraOrigin, cameraDirection;
                cameraGenerateRayParts(own.camera, coords, sampler, cameraOrigin, cameraDirection);
            }
            else { if (!kEarlyRng) rRng = ldStream(prec(in, R_RNG, slot)); loadSampler(sampler, pix, rSampler, rRng, pass, scene.blueNoise); sampler.seed = denseSeedRow<kStage>(passes, homeIndex / slotsPerPass, stagedSeeds, seedRow); }

            // SampleLights (next event estimation), PathTracerMIS.cpp:125-155
            if (!kPlain && kAll && scene.numLights != 0)
            {
                for (uint32_t l = 0; l < scene.numLights; ++l)
                {
                    float4 dirTmax, contribution;
                    if (computeLightSample<kLean>(scene, pass, sampler, scene.lights[l], sd, mat, depth, lightPickProbability, dirTmax, contribution)) v.rayMask |= 1u << l;
                    else contribution.w = -1.0f;   // a request without a ray: the mark the walks leave on an occluded one (verdictRecord)
                    pshadow(in, l, 0, slot) = dirTmax; pshadow(in, l, 1, slot) = contribution;
                }
                v.rayNeeded = v.rayMask != 0u;
                numRequests = v.rayNeeded ? scene.numLights : 0u;
                stage[2][threadIdx.x] = f4(sd.intersection.frame.r[3].x, sd.intersection.frame.r[3].y, sd.intersection.frame.r[3].z, 0.0f);
                stage[3][threadIdx.x] = f4(throughput.x, throughput.y, throughput.z, 0.0f);
            }
            else if (!kPlain && scene.numLights != 0)
            {
                uint32_t lightIndex = 0;
                if (scene.numLights > 1) lightIndex = sampler.fallbackInt() % scene.numLights;
                float4 oShadow0, oShadow1;
                v.rayNeeded = computeLightSample<kLean>(scene, pass, sampler, scene.lights[lightIndex], sd, mat, depth, lightPickProbability, oShadow0, oShadow1);
                numRequests = v.rayNeeded ? 1u : 0u;   // a request without a ray contributes nothing (resolvePendingLightSamples skips it): not kept
                stage[0][threadIdx.x] = oShadow0; stage[1][threadIdx.x] = oShadow1;
                stage[2][threadIdx.x] = f4(sd.intersection.frame.r[3].x, sd.intersection.frame.r[3].y, sd.intersection.frame.r[3].z, 0.0f);
                stage[3][threadIdx.x] = f4(throughput.x, throughput.y, throughput.z, 0.0f);
            }
            bool cont = depth < pass.maxRayDepth;
            if (cont && depth >= pass.minRussianRouletteDepth) cont = misRoulette(sampler, sd.mp.baseColor, throughput);
            if (cont)   // BSDF sampling; the next ray's records
            {
                uint32_t event;
                if (misSampleBsdf<kLean>(sampler, mat, sd, depth, throughput, event, v.oOrigin, v.oDir, v.oTp)) v.outcome = 1;
            }
            if (v.outcome == 1)
            {
                v.oSampler = f4(0.0f, fbits(sampler.salt), fbits(sampler.generated), fbits(densePack(homeIndex, numRequests)));
                v.oRng = packRng(sampler);
            }
            else if (v.rayNeeded)
            {
                v.outcome = 2;   // the path ends here, its last next-event sample still needs its shadow ray
                v.oSampler = f4(0.0f, 0.0f, 0.0f, fbits(densePack(homeIndex, numRequests)));
            }
        } while (false);
        if (v.outcome != 1) cnt.c[C_RAYS] += depth + 1u;   // counters.numRays += depth + 1, PathTracerMIS.cpp:412
    }
    v.oResult = f4(resultColor.x, resultColor.y, resultColor.z, fbits(pix));
    if (v.outcome == 0) stStream(home[homeIndex], f4(resultColor.x, resultColor.y, resultColor.z, 0.0f));
}

#ifndef RT_SHADE_FUNCTIONS_ONLY
// The body of PathTracerMIS::RenderPixel's loop for one path vertex (PathTracerMIS.cpp:276-395), as k_shade, reading arena `in`
// and writing the survivors densely into arena `out`.  kPlain: PathTracer::RenderPixel (Core/Rendering/PathTracer.cpp:73-171).
//
// kAll: LightSamplingStrategy::All (PathTracerMIS.cpp:141-147: every light is sampled at every vertex, up to RT_DENSE_MAX_LIGHTS of them here).
// The 2 x numLights request records of a vertex cannot wait in registers or LDS for its output slot, so they are written to the vertex's OWN
// slot of the input arena first -- its previous requests were folded in at the top of the iteration, the space is free -- and copied to the
// output slot once the block has allocated it (the copy reads what the same lane just wrote: L2 hits).
//
// kStage: where the launch-uniform tables behind a vertex's records are (denseShadeVertex), chosen by the host per launch (denseStageMask).  One kernel per
// place, not one kernel with three copies of the vertex: the copies' live ranges add up at the branch (the lean class 116 -> 125 VGPRs, scratch gained in two of
// the register-capped classes), while a kernel with one vertex keeps every class within its waves and its scratch (profiles/shade_tables_resources_diff.txt),
// and kStage 0 is the kernel as it was, without the tables' LDS.
template <int kLean, bool kPlain = false, bool kAll = false, int kStage = 0>
__global__ void RT_SHADE_DENSE_ATTR(kLean, kAll) k_shade_dense(const RtSceneDesc scene, const DevPass* __restrict__ passes, uint32_t slotsPerPass, const Paths in, const Paths out,
                                                          const DenseCounts dense, uint32_t* __restrict__ shadowQueue, uint32_t* __restrict__ shadowCount,
                                                          float4* __restrict__ home, unsigned long long* counters)
{
    __shared__ uint32_t sShadowBuf[RT_APPEND_BUFFER];
    // The four records of a vertex's next-event request are known long before the vertex knows whether and where it survives (Russian roulette,
    // BSDF sampling and the block's slot allocation come after): they wait in LDS instead of 16 registers.  142 -> 127 VGPRs for the lean
    // variant = four waves per SIMD instead of three in a kernel that spends most of its time waiting for dependent gathers (-14 % kernel time).
    __shared__ float4 sStage[4][RT_BLOCK];   // [request direction | contribution | shading point | throughput at the vertex][thread]
    __shared__ uint32_t sShadowCount, sShadowBase;
    __shared__ uint32_t sLive, sZombies, sLiveBase, sZombieBase;
    __shared__ uint32_t sLivePrefix[RT_DENSE_SHARDS + 1u], sZombiePrefix[RT_DENSE_SHARDS + 1u];
    // the launch-uniform tables behind a vertex's records (rt_device_state.h, RT_STAGE_*): an LDS read in the vertex's dependent chain where a trip to L2 was
    __shared__ __attribute__((aligned(16))) DenseStageTables sTables;
    if (threadIdx.x == 0) { sShadowCount = 0; sLive = 0; sZombies = 0; }
    denseLoadPrefix(dense.in, sLivePrefix);
    denseLoadZombiePrefix(dense.in, dense.shardCapacity, dense.errorFlags, sZombiePrefix);
    const DevPass pass = passes[0];   // the structural parameters are those of every pass of the batch
    if (kStage != 0) denseStageLoad(sTables, scene, passes, dense.numPasses, pass.numDimensions, kStage == 2);
    __syncthreads();
    RtSceneDesc staged = scene;
    if (kStage != 0) { staged.objects = sTables.objects; staged.meshes = sTables.meshes; staged.materials = sTables.materials; staged.lights = sTables.lights; staged.globalLights = sTables.globalLights; }
    const uint32_t seedRow = stageSeedRow(pass.numDimensions);
    Counters cnt; zeroCounters(cnt);
    const uint32_t numLive = sLivePrefix[RT_DENSE_SHARDS], count = numLive + sZombiePrefix[RT_DENSE_SHARDS];
    const uint32_t stride = gridDim.x * blockDim.x;
    const V4 lightSamplingWeight = load4(pass.lightSamplingWeight), bsdfSamplingWeight = load4(pass.bsdfSamplingWeight);
    const float lightPickProbability = kAll ? 1.0f : 1.0f / (float)(scene.numLights ? scene.numLights : 1u);   // GetLightPickingProbability, PathTracerMIS.cpp:157-172

    const uint32_t rounded = (count + RT_BLOCK - 1) / RT_BLOCK * RT_BLOCK;
    for (uint32_t first = blockIdx.x * blockDim.x; first < rounded; first += stride)
    {
        const uint32_t i = first + threadIdx.x;
        // what this vertex leaves behind: 0 nothing (radiance parked), 1 a live path, 2 a zombie (radiance + one pending request)
        DenseVertex v;
        v.outcome = 0; v.rayNeeded = false; v.rayMask = 0u;
        uint32_t inSlot = 0u;
        if (i < count)
        {
            bool zombie;
            const uint32_t slot = denseVertexSlot(sLivePrefix, sZombiePrefix, numLive, dense.shardCapacity, i, zombie);
            inSlot = slot;
            denseShadeVertex<kLean, kPlain, kAll, kStage>(staged, passes, slotsPerPass, pass, in, slot, zombie, lightSamplingWeight, bsdfSamplingWeight, lightPickProbability, sStage, home, cnt, v,
                                                          dense.primarySlotPixel, kStage == 2 ? sTables.seeds : nullptr, seedRow);
        }
        uint32_t outcome = v.outcome;

        // dense slots of the other arena: ranks from LDS counters, the block's two ranges with one global atomic each.  The region follows
        // the CHUNK of 256 vertices, not the block: consecutive chunks take the regions in turn whatever the grid size, so the regions
        // fill evenly (a region is a sixteenth of the arena plus a margin of 65536 slots); what still does not fit raises a flag the host
        // checks instead of overwriting the neighbouring region.
        const uint32_t shard = (first / RT_BLOCK) & (RT_DENSE_SHARDS - 1u);
        uint32_t rank = 0;
        if (outcome == 1) rank = atomicAdd(&sLive, 1u);
        else if (outcome == 2) rank = atomicAdd(&sZombies, 1u);
        __syncthreads();
        if (threadIdx.x == 0 && sLive != 0u) sLiveBase = atomicAdd(&dense.out[shard], sLive);
        if (threadIdx.x == 64 && sZombies != 0u) sZombieBase = atomicAdd(&dense.out[RT_DENSE_SHARDS + shard], sZombies);
        __syncthreads();
        // never outside the region (live paths grow upwards from its start, zombies downwards from its end); whether the two met is
        // checked on the final counts by the next launch's prologue above
        if ((outcome == 1 && sLiveBase + rank >= dense.shardCapacity) || (outcome == 2 && sZombieBase + rank >= dense.shardCapacity)) 
        {
            // the vertex is dropped and the frame is invalid until the next reset (every synchronising call reports the flag); its home still gets what
            // the path had gathered, so that k_accumulate_home never adds a previous batch's value
            dense.errorFlags[0] = 1u; outcome = 0;
            stStream(home[denseHome(ubits(v.oSampler.w))], f4(v.oResult.x, v.oResult.y, v.oResult.z, 0.0f));
        }
        if (outcome != 0)
        {
            const uint32_t slot = outcome == 1 ? shard * dense.shardCapacity + sLiveBase + rank : (shard + 1u) * dense.shardCapacity - 1u - (sZombieBase + rank);
            stStream(prec(out, R_RESULT, slot), v.oResult);
            stStream(prec(out, R_SAMPLER, slot), v.oSampler);
            if (outcome == 1) { stStream(prec(out, R_ORIGIN, slot), v.oOrigin); stStream(prec(out, R_DIR, slot), v.oDir); stStream(prec(out, R_TP, slot), v.oTp); stStream(prec(out, R_RNG, slot), v.oRng); }
            else stStream(prec(out, R_ORIGIN, slot), sStage[2][threadIdx.x]);   // a zombie: the origin of its any-hit rays (a live path's R_ORIGIN is that point already)
            if (densePending(ubits(v.oSampler.w)) != 0u)
            {
                stStream(prec(out, R_SH_TP, slot), sStage[3][threadIdx.x]);
                if (kAll)
                {
                    for (uint32_t l = 0; l < scene.numLights; ++l)
                    {
                        stStream(pshadow(out, l, 0, slot), pshadow(in, l, 0, inSlot)); stStream(pshadow(out, l, 1, slot), pshadow(in, l, 1, inSlot));
                        if (v.rayMask & (1u << l)) sShadowBuf[atomicAdd(&sShadowCount, 1u)] = l * out.capacity + slot;
                    }
                }
                else
                {
                stStream(pshadow(out, 0, 0, slot), sStage[0][threadIdx.x]);
                stStream(pshadow(out, 0, 1, slot), sStage[1][threadIdx.x]);
                if (v.rayNeeded) sShadowBuf[atomicAdd(&sShadowCount, 1u)] = slot;   // request index = light 0 * capacity + slot
                }
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) { sLive = 0; sZombies = 0; }
        const bool last = first + stride >= rounded;
        if (last || sShadowCount + RT_BLOCK * (kAll ? RT_DENSE_MAX_LIGHTS : 1u) > RT_APPEND_BUFFER) flushAppendBuffer(sShadowBuf, sShadowCount, sShadowBase, shadowQueue, shadowCount);
        else __syncthreads();
    }
    flushCounters(cnt, counters);
}

// Film::AccumulateColor (Film.cpp:25-39) from the parked radiance: the passes of a batch are added per pixel IN PASS ORDER; the
// secondary sum receives the even passes (Viewport.cpp:303)
__global__ void __launch_bounds__(RT_BLOCK) k_accumulate_home(const float4* __restrict__ home, const uint32_t* __restrict__ slotPixel, uint32_t slotsPerPass, uint32_t numPasses,
                                                              float* __restrict__ sum, float* __restrict__ secondary, uint32_t width, const DevPass* __restrict__ passes)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t pixelSlot = blockIdx.x * blockDim.x + threadIdx.x; pixelSlot < slotsPerPass; pixelSlot += stride)
    {
        const uint32_t pix = slotPixel[pixelSlot];
        const size_t idx = 3 * ((size_t)(pix >> 16) * width + (pix & 0xFFFFu));
        float sr = sum[idx + 0], sg = sum[idx + 1], sb = sum[idx + 2];
        float tr = secondary[idx + 0], tg = secondary[idx + 1], tb = secondary[idx + 2];
        for (uint32_t b = 0; b < numPasses; ++b)
        {
            const float4 c = ldStream(home[(size_t)b * slotsPerPass + pixelSlot]);
            sr = sr + c.x; sg = sg + c.y; sb = sb + c.z;
            if ((passes[b].passIndex % 2u) == 0u) { tr = tr + c.x; tg = tg + c.y; tb = tb + c.z; }
        }
        sum[idx + 0] = sr; sum[idx + 1] = sg; sum[idx + 2] = sb;
        secondary[idx + 0] = tr; secondary[idx + 1] = tg; secondary[idx + 2] = tb;
    }
}
#endif   // RT_SHADE_FUNCTIONS_ONLY
