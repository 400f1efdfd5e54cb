// rt_shade.inl -- PathTracerMIS / PathTracer / Debug shading over slot-per-pixel path state, and Film::AccumulateColor (k_accumulate).
// Its functions-only part also holds the vertex stages that every PathTracerMIS shading kernel shares, whatever its path state: misGlobalLights,
// misHitLight, misRoulette, misSampleBsdf and computeLightSample.  Included by rt_shade.hip, and by rt_tail.hip for those functions.
RT_DEV float CombineMis(float samplePdf, float otherPdf) { return FastDivide(samplePdf, samplePdf + otherPdf); }        // PathTracerMIS.cpp:16-24
RT_DEV float PdfAtoW(float pdfA, float distance, float cosThere) { return FastDivide(pdfA * Sqr(distance), Abs(cosThere)); }   // :26-29

// PathTracerMIS::SampleLight up to the shadow ray (PathTracerMIS.cpp:43-79, 97-119): produces the NEE
// request {direction, tmax, contribution}; the occlusion test and the accumulation happen in k_trace_shadow.
template <int kLean>
__device__ __forceinline__ static bool computeLightSample(const RtSceneDesc& scene, const DevPass& pass, Sampler& sampler, const RtLight& light,
                               const ShadingData& sd, const RtMaterial& mat, uint32_t depth, float lightPickProbability,
                               float4& outDirTmax, float4& outContribution)
{
    float u[3]; u[0] = sampler.getFloat(); u[1] = sampler.getFloat(); u[2] = sampler.getFloat();
    float tmax = -1.0f; V4 dir = zero4(); V4 contribution = zero4();
    IlluminateResult ir;
    const V4 radiance = lightIlluminate<kLean>(scene, light, sd.intersection, u, ir);
    if (!almostZero4(radiance))
    {
        float bsdfPdfW = 0.0f;
        const V4 factor = materialEvaluate<kLean>(mat, sd, neg(ir.directionToLight), bsdfPdfW);
        if (!almostZero4(factor))
        {
            float weight = 1.0f;
            const bool isLastPathSegment = depth >= pass.maxRayDepth;
            if (!(light.flags & RT_LIGHT_FLAG_DELTA) && !isLastPathSegment)
            {
                const float continuationProbability = 1.0f;
                bsdfPdfW *= continuationProbability;
                weight = CombineMis(ir.directPdfW * lightPickProbability, bsdfPdfW);
            }
            contribution = (radiance * factor) * FastDivide(weight, lightPickProbability * ir.directPdfW);
            dir = ir.directionToLight;
            tmax = ir.distance * 0.999f;
        }
    }
    outDirTmax = f4(dir.x, dir.y, dir.z, tmax);
    outContribution = f4(contribution.x, contribution.y, contribution.z, 0.0f);
    return tmax >= 0.0f;   // a shadow ray has to be traced for this request
}
template <int kLean>
__device__ __forceinline__ static bool prepareLightSample(const RtSceneDesc& scene, const DevPass& pass, Sampler& sampler, const RtLight& light,
                               const ShadingData& sd, const RtMaterial& mat, uint32_t depth, float lightPickProbability,
                               const Paths& paths, uint32_t slot, uint32_t requestIndex)
{
    float4 dirTmax, contribution;
    const bool ray = computeLightSample<kLean>(scene, pass, sampler, light, sd, mat, depth, lightPickProbability, dirTmax, contribution);
    pshadow(paths, requestIndex, 0, slot) = dirTmax;
    pshadow(paths, requestIndex, 1, slot) = contribution;
    return ray;
}

// Folds the finished NEE requests of the path's previous vertex into its radiance:
// accumulatedColor = sum of the unoccluded SampleLight() results in light order, times mLightSamplingWeight,
// then resultColor.MulAndAccumulate(throughput, ...) (PathTracerMIS.cpp:141-151, 320).  k_trace_shadow marks
// occluded requests with tmax < 0.
RT_DEV void resolvePendingLightSamples(const Paths& paths, uint32_t slot, uint32_t numRequests, V4 lightSamplingWeight, V4& resultColor, Counters& cnt)
{
    if (numRequests == 0) return;
    V4 accumulated = zero4();
    bool any = false;
    for (uint32_t l = 0; l < numRequests; ++l)
    {
        if (pshadow(paths, l, 0, slot).w < 0.0f) continue;   // no shadow ray was needed, or k_trace found an occluder
        const float4 c = pshadow(paths, l, 1, slot);
        accumulated = accumulated + V4(c.x, c.y, c.z, 0.0f);
        any = true;
        cnt.c[C_SHADOW_HIT]++;   // counters.numShadowRaysHit: the shadow ray reached the light (PathTracerMIS.cpp:96-99)
    }
    if (!any) return;
    accumulated = accumulated * lightSamplingWeight;
    const float4 tp = prec(paths, R_SH_TP, slot);
    resultColor = mulAdd(V4(tp.x, tp.y, tp.z, 0.0f), accumulated, resultColor);
}

// ---- The stages of one vertex of PathTracerMIS::RenderPixel's loop (PathTracerMIS.cpp:276-395) that do not depend on where the path's records live:
// the slot-per-pixel body (rt_shade_body.inl) and denseShadeVertex (rt_dense.inl) call them in the same order around their own loads, stores and
// next-event code.  kPlain: the renderer "Path Tracer" (PathTracer::RenderPixel, Core/Rendering/PathTracer.cpp:73-171), the same walk without MIS
// weights and sampling weights. ----

// EvaluateGlobalLights, PathTracerMIS.cpp:214-252: what a ray that left the scene sees; the caller multiplies it into the throughput
template <int kLean, bool kPlain>
__device__ __forceinline__ static V4 misGlobalLights(const RtSceneDesc& scene, const Ray& ray, uint32_t depth, bool lastSpecular, float lastPdfW,
                                                     float lightPickProbability, V4 bsdfSamplingWeight)
{
    V4 result = zero4();
    for (uint32_t g = 0; g < scene.numGlobalLights; ++g)
    {
        const RtLight& light = scene.lights[scene.globalLights[g]];
        const Ray lightSpaceRay = transformRayUnsafe(loadM4(light.invTransform), ray);
        float directPdfW = 0.0f;
        const V4 lightContribution = lightGetRadiance<kLean>(scene, light, lightSpaceRay, zero4(), 1.0f, directPdfW);
        if (kPlain) result = result + lightContribution;   // PathTracer::EvaluateGlobalLights, PathTracer.cpp:47-71
        else if (!almostZero4(lightContribution))
        {
            float misWeight = 1.0f;
            if (depth > 0 && !lastSpecular) misWeight = CombineMis(lastPdfW, directPdfW * lightPickProbability);
            result = mulAdd(lightContribution, misWeight, result);
        }
    }
    if (!kPlain) result = result * bsdfSamplingWeight;
    return result;
}

// EvaluateLight, PathTracerMIS.cpp:174-212: the path hit an area light (hit.subObjectId == RT_LIGHT_OBJECT) and ends there
template <bool kPlain>
__device__ __forceinline__ static void misHitLight(const RtSceneDesc& scene, const Hit& hit, const Ray& ray, const Intersection& intersection, V4 throughput,
                                                   uint32_t depth, bool lastSpecular, float lastPdfW, float lightPickProbability, V4 bsdfSamplingWeight, V4& resultColor)
{
    const RtObject& obj = scene.objects[hit.objectId];
    const RtLight& light = scene.lights[obj.lightIndex];
    const M4 worldToLight = loadM4(obj.invTransform);
    const Ray lightSpaceRay = transformRayUnsafe(worldToLight, ray);
    const V4 lightSpaceHitPoint = transformPoint(worldToLight, intersection.frame.r[3]);
    const float cosAtLight = -dot3(intersection.frame.r[2], ray.dir);
    float directPdfA = 0.0f;
    V4 lightContribution = lightGetRadiance<false>(scene, light, lightSpaceRay, lightSpaceHitPoint, cosAtLight, directPdfA);
    if (kPlain) resultColor = mulAdd(throughput, lightContribution, resultColor);   // PathTracer::EvaluateLight, PathTracer.cpp:26-45
    else if (!almostZero4(lightContribution))
    {
        float misWeight = 1.0f;
        if (depth > 0 && !lastSpecular)
        {
            const float directPdfW = PdfAtoW(directPdfA, hit.distance, cosAtLight);
            misWeight = CombineMis(lastPdfW, directPdfW * lightPickProbability);
        }
        lightContribution = lightContribution * bsdfSamplingWeight;
        resultColor = mulAdd(throughput, lightContribution * misWeight, resultColor);
    }
    else resultColor = mulAdd(throughput, zero4(), resultColor);   // (the reference's fma with a zero contribution: kept for the bits of resultColor)
}

// Russian roulette, PathTracerMIS.cpp:330-347: false = the path ends here; else the throughput is divided by the survival probability
__device__ __forceinline__ static bool misRoulette(Sampler& sampler, V4 baseColor, V4& throughput)
{
    bool cont = true;
    const float minColorValue = 0.125f;
    const float threshold = minColorValue + (1.0f - minColorValue) * colorMax(baseColor);
    if (sampler.getFloat() > threshold) cont = false;
    else throughput = throughput * (1.0f / threshold);
    return cont;
}

// BSDF sampling, PathTracerMIS.cpp:349-395: true = the path goes on, and oOrigin / oDir / oTp are the next ray's R_ORIGIN, R_DIR and R_TP.
// `event` is the sampled event either way: EV_NULL tells a path that ended without one from one whose throughput went to zero.
template <int kLean>
__device__ __forceinline__ static bool misSampleBsdf(Sampler& sampler, const RtMaterial& mat, const ShadingData& sd, uint32_t depth, V4& throughput, uint32_t& event,
                                                     float4& oOrigin, float4& oDir, float4& oTp)
{
    bool alive = false;
    float pdf = 0.0f; V4 incomingDirWorldSpace = zero4(); event = EV_NULL;
    float u[3]; u[0] = sampler.getFloat(); u[1] = sampler.getFloat(); u[2] = sampler.getFloat();
    const V4 bsdfValue = materialSample<kLean>(mat, sd, u, incomingDirWorldSpace, pdf, event);
    if (event != EV_NULL)
    {
        throughput = throughput * bsdfValue;
        if (!almostZero4(throughput))
        {
            // flags of the next vertex: depth, lastSpecular, and the material it leaves (see PathRecord, rt_device_state.h)
            oOrigin = f4(sd.intersection.frame.r[3].x, sd.intersection.frame.r[3].y, sd.intersection.frame.r[3].z,
                         fbits((depth + 1u) | (((event & EV_SPECULAR) != 0) ? 0x100u : 0u) | ((sd.intersection.material + 1u) << 9)));
            oDir = f4(incomingDirWorldSpace.x, incomingDirWorldSpace.y, incomingDirWorldSpace.z, pdf);
            oTp = f4(throughput.x, throughput.y, throughput.z, throughput.w);
            alive = true;
        }
    }
    return alive;
}

#define RT_APPEND_BUFFER 2048u

// Publishes a block's LDS append buffer with ONE global atomic and coalesced stores.  Called by all threads of
// the block at a block-uniform point (after a __syncthreads()).
RT_DEV void flushAppendBuffer(const uint32_t* buf, uint32_t& count, uint32_t& base, uint32_t* __restrict__ queue, uint32_t* __restrict__ queueCount)
{
    const uint32_t n = count;
    if (n != 0)
    {
        if (threadIdx.x == 0) base = atomicAdd(queueCount, n);
        __syncthreads();
        const uint32_t b = base;
        for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) queue[b + k] = buf[k];
        __syncthreads();
        if (threadIdx.x == 0) count = 0;
    }
    __syncthreads();
}

#ifndef RT_SHADE_FUNCTIONS_ONLY   // (rt_tail.hip takes the functions above and none of the kernels below)
// k_shade, rtgpu_record_paths' k_shade_record and rtgpu_render_aovs_chain's k_shade_chain: ONE body (rt_shade_body.inl), compiled three times.  The
// recording and chain blocks are preprocessor blocks, so k_shade is the token stream it was before the recorder and the chain existed.
#define RT_SHADE_KERNEL k_shade
#define RT_SHADE_RECORDING 0
#define RT_SHADE_CHAIN 0
#include "rt_shade_body.inl"
#undef RT_SHADE_KERNEL
#undef RT_SHADE_RECORDING
#undef RT_SHADE_CHAIN

// ---- path records (include/rtgpu.h, rtgpu_record_paths; host side: rt_runtime_paths.inl) ------------------------------------------------------
// The reference's PathDebugData hook (Core/Rendering/PathDebugging.h:27-53, filled at PathTracerMIS.cpp:377-410).  A slot's records are `stride`
// float4: seven per vertex (RtPathVertex: 28 words), vertex k of the path at 7 k, and in the last one the vertex count and the termination reason,
// which the shade launch that ends the path writes.  Vertices the buffer has no room for ((stride - 1) / 7 of them fit) are counted, not stored.
enum { RT_PATH_END_HIT_BACKGROUND = 1, RT_PATH_END_HIT_LIGHT, RT_PATH_END_DEPTH, RT_PATH_END_THROUGHPUT, RT_PATH_END_NO_SAMPLED_EVENT, RT_PATH_END_RUSSIAN_ROULETTE };   // PathTerminationReason
// u and v are barycentrics: only MeshShape::Traverse writes them (the reference's HitPoint keeps an earlier vertex's otherwise, the record holds 0)
RT_DEV bool pathHitIsMeshTriangle(const RtSceneDesc& scene, const Hit& hit)
{
    const RtObject& obj = scene.objects[hit.objectId];
    return obj.objectKind != RT_OBJECT_LIGHT && obj.shapeKind == RT_SHAPE_MESH;
}
// position, normal, tangent, texCoord: the evaluated intersection.  The caller passes zeros on a miss, for them and for the sub-object id: the reference's
// ShadingData and HitPoint still hold an earlier vertex's there
RT_DEV void storePathVertex(float4* __restrict__ records, uint32_t stride, uint32_t slot, uint32_t index, const Ray& ray, uint32_t objectId, uint32_t subObjectId, float distance,
                            float u, float v, V4 position, V4 normal, V4 tangent, V4 texCoord, V4 throughput, uint32_t bsdfEvent)
{
    if (7u * index + 7u > stride - 1u) return;
    float4* rec = records + (size_t)slot * stride + 7u * index;
    rec[0] = f4(ray.origin.x, ray.origin.y, ray.origin.z, ray.dir.x);
    rec[1] = f4(ray.dir.y, ray.dir.z, fbits(objectId), fbits(subObjectId));
    rec[2] = f4(distance, u, v, position.x);
    rec[3] = f4(position.y, position.z, normal.x, normal.y);
    rec[4] = f4(normal.z, tangent.x, tangent.y, tangent.z);
    rec[5] = f4(texCoord.x, texCoord.y, throughput.x, throughput.y);
    rec[6] = f4(throughput.z, throughput.w, fbits(bsdfEvent), 0.0f);
}
#define RT_SHADE_KERNEL k_shade_record
#define RT_SHADE_RECORDING 1
#define RT_SHADE_CHAIN 0
#include "rt_shade_body.inl"
#undef RT_SHADE_KERNEL
#undef RT_SHADE_RECORDING
#undef RT_SHADE_CHAIN

// ---- guide chains (include/rtgpu.h, rtgpu_render_aovs_chain; host side: rt_runtime_aov.inl; the resolve: k_aov_resolve_chain, rt_aov.inl) ------
#define RT_SHADE_KERNEL k_shade_chain
#define RT_SHADE_RECORDING 0
#define RT_SHADE_CHAIN 1
#include "rt_shade_body.inl"
#undef RT_SHADE_KERNEL
#undef RT_SHADE_RECORDING
#undef RT_SHADE_CHAIN

// The end of a recording: folds the next-event results of every path's last vertex into its radiance (what k_accumulate does before it adds the
// pixel) and writes the slot's RtPathInfo {numVertices, terminationReason, radiance[3], 0, 0, 0} as two float4.
__global__ void __launch_bounds__(RT_BLOCK) k_paths_finish(const Paths paths, uint32_t numSlots, const DevPass* __restrict__ passes, const float4* __restrict__ records,
                                                           uint32_t recordStride, float4* __restrict__ infos, unsigned long long* counters)
{
    Counters cnt; zeroCounters(cnt);
    const V4 lightSamplingWeight = load4(passes[0].lightSamplingWeight);
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < numSlots; slot += stride)
    {
        const float4 rResult = prec(paths, R_RESULT, slot);
        V4 resultColor(rResult.x, rResult.y, rResult.z, 0.0f);
        resolvePendingLightSamples(paths, slot, ubits(prec(paths, R_SAMPLER, slot).w), lightSamplingWeight, resultColor, cnt);
        const float4 end = records[(size_t)slot * recordStride + (recordStride - 1u)];
        infos[2u * slot] = f4(end.x, end.y, resultColor.x, resultColor.y);
        infos[2u * slot + 1u] = f4(resultColor.z, 0.0f, 0.0f, 0.0f);
    }
    flushCounters(cnt, counters);
}

__global__ void __launch_bounds__(RT_BLOCK) k_debug_shade(const RtSceneDesc scene, const Paths paths, const uint32_t* __restrict__ queueIn, const uint32_t* __restrict__ countIn,
                                                          uint32_t mode, unsigned long long* counters)
{
    Counters cnt; zeroCounters(cnt);
    const uint32_t count = *countIn;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride)
    {
        const uint32_t slot = queueIn[i];
        const float4 rOrigin = prec(paths, R_ORIGIN, slot), rDir = prec(paths, R_DIR, slot), rHit = prec(paths, R_HIT, slot);
        const Ray ray = makePathRay(rOrigin, rDir, 0u);
        const Hit hit = unpackHit(rHit, prec(paths, R_SAMPLER, slot).x);
        V4 color = zero4();
        if (hit.objectId != RT_INVALID_OBJECT)
        {
            if (hit.subObjectId == RT_LIGHT_OBJECT) color = V4(1.0f, 1.0f, 0.0f, 0.0f);
            else
            {
                ShadingData sd; sd.intersection.material = RT_NO_MATERIAL;
                if (mode != DBG_TRIANGLE_ID && mode != DBG_DEPTH)
                {
                    if (hit.distance < FLT_MAX) sceneEvaluateIntersection<false>(scene, ray, hit, sd.intersection, cnt);
                    materialEvaluateShadingData<false>(scene, scene.materials[sd.intersection.material], sd);
                }
                switch (mode)
                {
                case DBG_CAMERA_LIGHT: { const float NdotL = dot3(ray.dir, sd.intersection.frame.r[2]); color = sd.mp.baseColor * Abs(NdotL); break; }
                case DBG_DEPTH: { const float invDepth = 1.0f - 1.0f / (1.0f + hit.distance / 10.0f); color = splat(invDepth); break; }
                case DBG_TRIANGLE_ID:
                {
                    color = debugTriangleIdColor(hit.objectId, hit.subObjectId);
                    break;
                }
                case DBG_TANGENTS: color = min4(splat(1.0f), max4(zero4(), mulAdd(sd.intersection.frame.r[0], splat(0.5f), splat(0.5f)))); break;
                case DBG_BITANGENTS: color = min4(splat(1.0f), max4(zero4(), mulAdd(sd.intersection.frame.r[1], splat(0.5f), splat(0.5f)))); break;
                case DBG_NORMALS: color = min4(splat(1.0f), max4(zero4(), mulAdd(sd.intersection.frame.r[2], splat(0.5f), splat(0.5f)))); break;
                case DBG_POSITION: color = max4(zero4(), sd.intersection.frame.r[3]); break;
                case DBG_TEXCOORDS: color = V4(sd.intersection.texCoord.x - floorf(sd.intersection.texCoord.x), sd.intersection.texCoord.y - floorf(sd.intersection.texCoord.y), 0.0f, 0.0f); break;
                case DBG_BASE_COLOR: color = sd.mp.baseColor; break;
                case DBG_EMISSION: color = sd.mp.emission; break;
                case DBG_ROUGHNESS: color = splat(sd.mp.roughness); break;
                case DBG_METALNESS: color = splat(sd.mp.metalness); break;
                default: color = splat(sd.mp.IoR); break;
                }
            }
        }
        prec(paths, R_RESULT, slot) = f4(color.x, color.y, color.z, prec(paths, R_RESULT, slot).w);
    }
    flushCounters(cnt, counters);
}

// Film::AccumulateColor (Film.cpp:25-39): float3 sum buffers, tight stride, row y = tile row y.  The passes of a
// batch are added per pixel IN PASS ORDER, so the float sum is the one the reference builds pass after pass; the
// secondary sum receives the even passes (Viewport.cpp:303).
__global__ void __launch_bounds__(RT_BLOCK) k_accumulate(const Paths paths, uint32_t slotsPerPass, uint32_t numPasses, float* __restrict__ sum,
                                                         float* __restrict__ secondary, uint32_t width, const DevPass* __restrict__ passes,
                                                         unsigned long long* counters)
{
    Counters cnt; zeroCounters(cnt);
    const V4 lightSamplingWeight = load4(passes[0].lightSamplingWeight);
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t pixelSlot = blockIdx.x * blockDim.x + threadIdx.x; pixelSlot < slotsPerPass; pixelSlot += stride)
    {
        const uint32_t pix = ubits(prec(paths, R_RESULT, pixelSlot).w);
        const size_t idx = 3 * ((size_t)(pix >> 16) * width + (pix & 0xFFFFu));
        float sr = sum[idx + 0], sg = sum[idx + 1], sb = sum[idx + 2];
        float tr = secondary[idx + 0], tg = secondary[idx + 1], tb = secondary[idx + 2];
        for (uint32_t b = 0; b < numPasses; ++b)
        {
            const uint32_t slot = b * slotsPerPass + pixelSlot;
            const float4 rResult = prec(paths, R_RESULT, slot);
            V4 resultColor(rResult.x, rResult.y, rResult.z, 0.0f);
            resolvePendingLightSamples(paths, slot, ubits(prec(paths, R_SAMPLER, slot).w), lightSamplingWeight, resultColor, cnt);   // NEE of the path's last vertex
            sr = sr + resultColor.x; sg = sg + resultColor.y; sb = sb + resultColor.z;
            if ((passes[b].passIndex % 2u) == 0u) { tr = tr + resultColor.x; tg = tg + resultColor.y; tb = tb + resultColor.z; }
        }
        sum[idx + 0] = sr; sum[idx + 1] = sg; sum[idx + 2] = sb;
        secondary[idx + 0] = tr; secondary[idx + 1] = tg; secondary[idx + 2] = tb;
    }
    flushCounters(cnt, counters);
}
#endif   // RT_SHADE_FUNCTIONS_ONLY
