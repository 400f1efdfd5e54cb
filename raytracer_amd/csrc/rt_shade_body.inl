// rt_shade_body.inl -- the shading kernel of the slot-per-pixel pipeline.  rt_shade.inl includes it three times: as k_shade (RT_SHADE_RECORDING 0,
// RT_SHADE_CHAIN 0: the blocks under those switches are not there), as k_shade_record (RT_SHADE_RECORDING 1), rtgpu_record_paths' variant, which also
// writes the path's vertices, and as k_shade_chain (RT_SHADE_CHAIN 1), rtgpu_render_aovs_chain's variant.
//
// k_shade_chain walks a path to its guide vertex (include/rtgpu.h, "Guide chains") and keeps no radiance: no light is evaluated, no emission added,
// no next-event request written or resolved and no shadow ray queued -- none of that takes a sampler draw -- but the next-event draws are taken, in
// order, so the roulette and BSDF draws behind them are the path tracer's.  A vertex the path goes on from through a specular event of a mirror or
// glass material (depth < maxChain) writes the next ray into the slot and queues it; every other vertex STOPS: it writes nothing, so the slot still
// holds that vertex's own R_ORIGIN / R_DIR / R_TP / R_HIT for k_aov_resolve_chain (misSampleBsdf's results go through locals here for that reason).
// Early stop: a miss, a light, a material kind that cannot pass and a vertex at depth maxChain stop before a draw is taken -- what the draws would
// decide no longer matters -- so a frame without mirrors and glass pays one evaluated intersection per pixel.  R_RESULT.x carries the sum of the hit
// distances of the vertices passed so far (no radiance is kept there); R_SH_P / R_SH_TP, the next-event request's records, carry the primary ray of a path
// whose vertex 0 may be passed, for RT_AOV_VIRTUAL_POSITION.
//
// The body of PathTracerMIS::RenderPixel's loop for one path vertex (PathTracerMIS.cpp:276-395).  What does not depend on where a path's records live
// -- the lights a ray hits, Russian roulette, BSDF sampling with the packing of the next ray -- are the mis* stages of rt_shade.inl, which
// denseShadeVertex (rt_dense.inl) calls too; here are the slot's loads and stores, next event estimation into the slot's request records, and the recorder.
// kPlain: the renderer "Path Tracer" instead (PathTracer::RenderPixel, Core/Rendering/PathTracer.cpp:73-171): the same walk without
// next event estimation, MIS weights and sampling weights.
template <bool kLean, bool kPlain = false>
__global__ void __launch_bounds__(RT_BLOCK) RT_SHADE_KERNEL(const RtSceneDesc scene, const DevPass* __restrict__ passes, uint32_t slotsPerPass, const Paths paths,
                                                    const uint32_t* __restrict__ queueIn, const uint32_t* __restrict__ countIn,
                                                    uint32_t* __restrict__ queueOut, uint32_t* __restrict__ countOut,
                                                    uint32_t* __restrict__ shadowQueue, uint32_t* __restrict__ shadowCount,
                                                    unsigned long long* counters
#if RT_SHADE_CHAIN
                                                    , uint32_t maxChain   // RT_K_SHADE_CHAIN_ARGS (rt_shade_kernels.h)
#endif
#if RT_SHADE_RECORDING
                                                    , float4* __restrict__ records, uint32_t recordStride   // RT_K_SHADE_RECORD_ARGS (rt_shade_kernels.h)
#endif
                                                    )
{
#if RT_SHADE_CHAIN
    __shared__ uint32_t sPathBuf[RT_APPEND_BUFFER];
    __shared__ uint32_t sPathCount, sPathBase;
    if (threadIdx.x == 0) sPathCount = 0;
#else
    __shared__ uint32_t sPathBuf[RT_APPEND_BUFFER], sShadowBuf[RT_APPEND_BUFFER];
    __shared__ uint32_t sPathCount, sShadowCount, sPathBase, sShadowBase;
    if (threadIdx.x == 0) { sPathCount = 0; sShadowCount = 0; }
#endif
    __syncthreads();
    Counters cnt; zeroCounters(cnt);
    const uint32_t count = *countIn;
    const uint32_t stride = gridDim.x * blockDim.x;
    // the structural parameters are identical for all passes of a batch (the host flushes when they change);
    // seeds, camera, anti-aliasing offset and rng keys are per pass
    const DevPass pass = passes[0];
#if !RT_SHADE_CHAIN
    const V4 lightSamplingWeight = load4(pass.lightSamplingWeight), bsdfSamplingWeight = load4(pass.bsdfSamplingWeight);
    // GetLightPickingProbability, PathTracerMIS.cpp:157-172
    const float lightPickProbability = pass.lightSamplingStrategy == RT_LIGHT_SAMPLING_SINGLE ? 1.0f / (float)scene.numLights : 1.0f;
    const uint32_t maxRequestsPerVertex = pass.lightSamplingStrategy == RT_LIGHT_SAMPLING_SINGLE ? 1u : (scene.numLights < 8u ? scene.numLights : 8u);
#endif

    // every lane of a wave runs the same number of iterations so that the ballot below sees whole waves
    const uint32_t rounded = (count + RT_BLOCK - 1) / RT_BLOCK * RT_BLOCK;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < rounded; i += stride)
    {
        bool alive = false;
        uint32_t slot = 0;
#if !RT_SHADE_CHAIN
        unsigned long long rayMask = 0ull;   // NEE requests of this vertex that need a shadow ray (bit = request index)
#endif
        if (i < count)
        {
            slot = queueIn[i];
            const float4 rOrigin = prec(paths, R_ORIGIN, slot), rDir = prec(paths, R_DIR, slot), rTp = prec(paths, R_TP, slot);
            const float4 rResult = prec(paths, R_RESULT, slot), rHit = prec(paths, R_HIT, slot), rSampler = prec(paths, R_SAMPLER, slot);
            const uint32_t flags = ubits(rOrigin.w);
            uint32_t depth = flags & 0xFFu;
#if !RT_SHADE_CHAIN
            const bool lastSpecular = (flags & 0x100u) != 0;
            const float lastPdfW = rDir.w;
#endif
            const uint32_t pix = ubits(rResult.w);
            const Ray ray = makePathRay(rOrigin, rDir, depth);
            V4 throughput(rTp.x, rTp.y, rTp.z, rTp.w);
#if !RT_SHADE_CHAIN
            V4 resultColor(rResult.x, rResult.y, rResult.z, 0.0f);
            resolvePendingLightSamples(paths, slot, ubits(rSampler.w), lightSamplingWeight, resultColor, cnt);   // NEE of the previous vertex
#endif
            const Hit hit = unpackHit(rHit, rSampler.x);
#if !RT_SHADE_CHAIN
            bool samplerStored = false;
#endif
#if RT_SHADE_RECORDING
            uint32_t reason = 0u;   // PathTerminationReason, set where PathTracerMIS.cpp:280-367 sets it
            uint32_t recordedEvent = 0u;   // the sampled BSDF event of a vertex the path goes on from
#endif

            do
            {
                if (hit.objectId == RT_INVALID_OBJECT)
                {
#if !RT_SHADE_CHAIN
                    // EvaluateGlobalLights
                    resultColor = mulAdd(throughput, misGlobalLights<kLean, kPlain>(scene, ray, depth, lastSpecular, lastPdfW, lightPickProbability, bsdfSamplingWeight), resultColor);
#endif
#if RT_SHADE_RECORDING
                    reason = RT_PATH_END_HIT_BACKGROUND;
                    storePathVertex(records, recordStride, slot, depth, ray, hit.objectId, 0u, hit.distance, 0.0f, 0.0f, zero4(), zero4(), zero4(), zero4(), throughput, 0u);
#endif
                    break;
                }

                ShadingData sd;
                // The reference keeps ONE ShadingData for the whole path (PathTracerMIS.cpp:258) and LightSceneObject::
                // EvaluateIntersection does not touch `material` (SceneObject_Light.cpp:62-73): when a path hits an area light,
                // IntersectionData::material is still the PREVIOUS vertex's, and its normal map (if any) is applied to the
                // light's frame (Scene.cpp:327).  The previous material rides in the flags word: (index + 1) << 9.
                sd.intersection.material = (flags >> 9) - 1u;   // 0 -> RT_NO_MATERIAL
                if (hit.distance < FLT_MAX) sceneEvaluateIntersection<kLean>(scene, ray, hit, sd.intersection, cnt);

                if (!kLean && hit.subObjectId == RT_LIGHT_OBJECT)
                {
#if !RT_SHADE_CHAIN
                    // EvaluateLight
                    misHitLight<kPlain>(scene, hit, ray, sd.intersection, throughput, depth, lastSpecular, lastPdfW, lightPickProbability, bsdfSamplingWeight, resultColor);
#endif
#if RT_SHADE_RECORDING
                    reason = RT_PATH_END_HIT_LIGHT;
                    storePathVertex(records, recordStride, slot, depth, ray, hit.objectId, hit.subObjectId, hit.distance, 0.0f, 0.0f, sd.intersection.frame.r[3], sd.intersection.frame.r[2],
                                    sd.intersection.frame.r[0], sd.intersection.texCoord, throughput, 0u);
#endif
                    break;
                }

                sd.outgoingDirWorldSpace = neg(ray.dir);
                const RtMaterial& mat = scene.materials[sd.intersection.material];
#if RT_SHADE_CHAIN
                // the early stop: this vertex cannot be passed whatever is drawn
                if (depth >= maxChain || !(mat.bsdf == RT_BSDF_DIELECTRIC || mat.bsdf == RT_BSDF_ROUGH_DIELECTRIC || mat.bsdf == RT_BSDF_METAL || mat.bsdf == RT_BSDF_ROUGH_METAL)) break;
                // vertex 0 may be passed: the primary ray as generated, for RT_AOV_VIRTUAL_POSITION (k_aov_resolve_chain reads it for k > 0 only).  The two records are
                // the next-event request's, which this variant never writes.  Stored here, while the ray is live, and not where the vertex is known to be passed:
                // carried across the BSDF sampling the six words cost 8 VGPRs and a wave per SIMD
                if (depth == 0u)
                {
                    prec(paths, R_SH_P, slot) = f4(ray.origin.x, ray.origin.y, ray.origin.z, 0.0f);
                    prec(paths, R_SH_TP, slot) = f4(ray.dir.x, ray.dir.y, ray.dir.z, 0.0f);
                }
#endif
                materialEvaluateShadingData<kLean>(scene, mat, sd);

#if !RT_SHADE_CHAIN
                // emission, PathTracerMIS.cpp:309-317
                resultColor = mulAdd(throughput, kPlain ? sd.mp.emission : sd.mp.emission * bsdfSamplingWeight, resultColor);
#endif

                Sampler sampler; loadSampler(sampler, paths, slot, pix, rSampler, pass, scene.blueNoise);
                sampler.seed = passes[slot / slotsPerPass].seed;

#if RT_SHADE_CHAIN
                // the draws of SampleLights (an optional light pick, then computeLightSample's three floats per request), and nothing of what they are for
                if (scene.numLights != 0)
                {
                    const bool single = pass.lightSamplingStrategy == RT_LIGHT_SAMPLING_SINGLE;
                    if (single && scene.numLights > 1) (void)sampler.fallbackInt();
                    for (uint32_t l = 0; l < (single ? 1u : scene.numLights); ++l) { (void)sampler.getFloat(); (void)sampler.getFloat(); (void)sampler.getFloat(); }
                }
#else
                // SampleLights (next event estimation), PathTracerMIS.cpp:125-155
                uint32_t numRequests = 0;
                if (!kPlain && scene.numLights != 0)
                {
                    if (pass.lightSamplingStrategy == RT_LIGHT_SAMPLING_SINGLE)
                    {
                        uint32_t lightIndex = 0;
                        if (scene.numLights > 1) lightIndex = sampler.fallbackInt() % scene.numLights;
                        if (prepareLightSample<kLean>(scene, pass, sampler, scene.lights[lightIndex], sd, mat, depth, lightPickProbability, paths, slot, 0)) rayMask = 1ull;
                        numRequests = 1;
                    }
                    else
                    {
                        for (uint32_t l = 0; l < scene.numLights; ++l)
                        {
                            const bool ray = prepareLightSample<kLean>(scene, pass, sampler, scene.lights[l], sd, mat, depth, lightPickProbability, paths, slot, l);
                            if (ray)
                            {
                                if (l < 8u) rayMask |= 1ull << l;
                                else shadowQueue[atomicAdd(shadowCount, 1u)] = l * paths.capacity + slot;   // more than 64 lights: per-lane append
                            }
                        }
                        numRequests = scene.numLights;
                    }
                    prec(paths, R_SH_P, slot) = f4(sd.intersection.frame.r[3].x, sd.intersection.frame.r[3].y, sd.intersection.frame.r[3].z, 0.0f);
                    prec(paths, R_SH_TP, slot) = f4(throughput.x, throughput.y, throughput.z, 0.0f);
                }
#endif

                bool cont = true;
                if (depth >= pass.maxRayDepth) cont = false;
#if RT_SHADE_RECORDING
                if (!cont) reason = RT_PATH_END_DEPTH;
#endif

                if (cont && depth >= pass.minRussianRouletteDepth)   // Russian roulette
                {
                    cont = misRoulette(sampler, sd.mp.baseColor, throughput);
#if RT_SHADE_RECORDING
                    if (!cont) reason = RT_PATH_END_RUSSIAN_ROULETTE;
#endif
                }

                if (cont)   // BSDF sampling; the next ray's records
                {
                    // (straight into the slot's records: through locals, k_shade<false, true> and <true, false> each need ~15 VGPRs more and lose a wave per SIMD)
                    uint32_t event;
#if RT_SHADE_CHAIN
                    float4 nextOrigin, nextDir, nextTp;
                    alive = misSampleBsdf<kLean>(sampler, mat, sd, depth, throughput, event, nextOrigin, nextDir, nextTp) && (event & EV_SPECULAR) != 0;
                    if (alive)   // passed
                    {
                        prec(paths, R_ORIGIN, slot) = nextOrigin; prec(paths, R_DIR, slot) = nextDir; prec(paths, R_TP, slot) = nextTp;
                        prec(paths, R_RESULT, slot) = f4(rResult.x + hit.distance, 0.0f, 0.0f, rResult.w);
                        storeSampler(sampler, paths, slot, hit.v, 0u);
                    }
#else
                    alive = misSampleBsdf<kLean>(sampler, mat, sd, depth, throughput, event, prec(paths, R_ORIGIN, slot), prec(paths, R_DIR, slot), prec(paths, R_TP, slot));
#endif
#if RT_SHADE_RECORDING
                    if (!alive) reason = event == EV_NULL ? RT_PATH_END_NO_SAMPLED_EVENT : RT_PATH_END_THROUGHPUT;
                    else recordedEvent = event;
#endif
                }
#if RT_SHADE_RECORDING
                {
                    // the vertex the path goes on from (PathTracerMIS.cpp:377-388, with the sampled event), or the one it ends on (:398-409)
                    const bool triangle = pathHitIsMeshTriangle(scene, hit);
                    storePathVertex(records, recordStride, slot, depth, ray, hit.objectId, hit.subObjectId, hit.distance, triangle ? hit.u : 0.0f, triangle ? hit.v : 0.0f,
                                    sd.intersection.frame.r[3], sd.intersection.frame.r[2], sd.intersection.frame.r[0], sd.intersection.texCoord, throughput, recordedEvent);
                }
#endif
#if !RT_SHADE_CHAIN
                storeSampler(sampler, paths, slot, hit.v, numRequests);
                samplerStored = true;
#endif
            } while (false);

#if !RT_SHADE_CHAIN
            if (!samplerStored && ubits(rSampler.w) != 0u) prec(paths, R_SAMPLER, slot).w = fbits(0u);   // the resolved requests are spent
            prec(paths, R_RESULT, slot) = f4(resultColor.x, resultColor.y, resultColor.z, rResult.w);
            if (!alive) cnt.c[C_RAYS] += depth + 1u;   // counters.numRays += depth + 1, PathTracerMIS.cpp:412
#endif
#if RT_SHADE_RECORDING
            if (!alive) records[(size_t)slot * recordStride + (recordStride - 1u)] = f4(fbits(depth + 1u), fbits(reason), 0.0f, 0.0f);   // the path's vertex count and why it ended
#endif
        }

        // Queue appends go through per-block LDS buffers: a returning atomic on ONE global word sustains only ~88
        // operations per microsecond on this chip, so per-wave appends (hundreds of thousands per launch) would
        // dominate the kernel; a block publishes ~RT_APPEND_BUFFER entries per global atomic instead.
#if !RT_SHADE_CHAIN
        for (unsigned long long pending = rayMask; pending != 0ull; pending &= pending - 1ull)
        {
            const uint32_t l = (uint32_t)(__ffsll((long long)pending) - 1);
            sShadowBuf[atomicAdd(&sShadowCount, 1u)] = l * paths.capacity + slot;
        }
#endif
        if (alive) sPathBuf[atomicAdd(&sPathCount, 1u)] = slot;
        __syncthreads();
        // flush when the next iteration could overflow a buffer (wave-uniform decision on block-shared counters)
        const bool last = (i - threadIdx.x) + stride >= rounded;
        if (last || sPathCount + RT_BLOCK > RT_APPEND_BUFFER) flushAppendBuffer(sPathBuf, sPathCount, sPathBase, queueOut, countOut);
#if !RT_SHADE_CHAIN
        if (last || sShadowCount + RT_BLOCK * maxRequestsPerVertex > RT_APPEND_BUFFER) flushAppendBuffer(sShadowBuf, sShadowCount, sShadowBase, shadowQueue, shadowCount);
#endif
    }
    flushCounters(cnt, counters);
}
