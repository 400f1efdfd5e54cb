// rt_aov.inl -- the kernels around rtgpu_render_aovs (include/rtgpu.h; host side: rt_runtime_aov.inl).  Included by rt_shade.hip.
// An AOV call is the first bounce of the slot-per-pixel pipeline with another end: k_aov_pixels names the chunk's pixels, k_generate makes their
// primary rays, the walk the context renders with (or the counting k_trace, for the cost planes) leaves a hit record per slot, and k_aov_resolve
// turns that record into the planes the caller asked for.
//   k_aov_pixels    slot i of the chunk = pixel firstPixel + i of the frame, row-major in sum-buffer coordinates (k_generate flips the film row)
//   k_aov_resolve   Scene::EvaluateIntersection + Material::EvaluateShadingData of every hit -> channel-major planes
//   k_aov_resolve_chain   the same body for rtgpu_render_aovs_chain: the slot holds its path's guide vertex (k_shade_chain, rt_shade_body.inl), whose depth and
//                   previous material ride in the flags word of R_ORIGIN; it also writes the three chain planes and, for rtgpu_render_aovs_virtual, the virtual position.  The planes are resolved here, behind the
//                   bounce loop, and not from inside the shade variant: slot i is pixel firstPixel + i, so the stores stay pixel-ordered and coalesced
// Slot i of the arena is pixel firstPixel + i, so a wave's 64 stores to one channel of one plane are 256 consecutive bytes.

__global__ void __launch_bounds__(RT_BLOCK) k_aov_pixels(uint32_t* __restrict__ slotPixel, uint32_t count, unsigned long long firstPixel, uint32_t width)
{
    const uint32_t i = blockIdx.x * RT_BLOCK + threadIdx.x;
    if (i >= count) return;
    const unsigned long long p = firstPixel + i;
    const uint32_t y = (uint32_t)(p / width), x = (uint32_t)(p - (unsigned long long)y * width);
    slotPixel[i] = x | (y << 16);
}

// planes that need Scene::EvaluateIntersection (the frame, the texture coordinates, the triangle's material), and those that need the material evaluated
#define RT_AOV_BIT(p) (1u << (p))
#define RT_AOV_FRAME_PLANES (RT_AOV_BIT(RT_AOV_POSITION) | RT_AOV_BIT(RT_AOV_NORMAL) | RT_AOV_BIT(RT_AOV_TANGENT) | RT_AOV_BIT(RT_AOV_BITANGENT) | RT_AOV_BIT(RT_AOV_TEXCOORD) | \
                             RT_AOV_BIT(RT_AOV_MATERIAL))
#define RT_AOV_MATERIAL_PLANES (RT_AOV_BIT(RT_AOV_BASE_COLOR) | RT_AOV_BIT(RT_AOV_EMISSION) | RT_AOV_BIT(RT_AOV_ROUGHNESS) | RT_AOV_BIT(RT_AOV_METALNESS) | RT_AOV_BIT(RT_AOV_IOR))

// kLean: the scene class, as for the other shading kernels (rt_device_core.h): 0 = anything, 3 = anything without textures.
// `mask` (bit = RtAovPlane) and the plane pointers are kernel arguments, so every `if (mask & ...)` below is a scalar branch.
// kChain: the vertex is the slot's current one at whatever depth (false: the primary ray's); `plane`: AovOutputs::plane or AovChainOutputs::plane
template <int kLean, bool kChain>
__device__ __forceinline__ static void aovResolve(const RtSceneDesc& scene, const Paths& paths, uint32_t count, uint32_t mask, void* const* plane, size_t channelStride, size_t firstOut,
                                                  const uint4* __restrict__ rayCounts)
{
    const uint32_t i = blockIdx.x * RT_BLOCK + threadIdx.x;
    if (i >= count) return;
    const float4 rHit = prec(paths, R_HIT, i);
    const Hit hit = unpackHit(rHit, prec(paths, R_SAMPLER, i).x);
    const bool isHit = hit.objectId != RT_INVALID_OBJECT;
    const bool isLight = isHit && hit.subObjectId == RT_LIGHT_OBJECT;

    ShadingData sd;
    for (int k = 0; k < 4; ++k) sd.intersection.frame.r[k] = zero4();
    sd.intersection.texCoord = zero4(); sd.intersection.material = RT_NO_MATERIAL;
    sd.mp.baseColor = zero4(); sd.mp.emission = zero4(); sd.mp.roughness = 0.0f; sd.mp.metalness = 0.0f; sd.mp.IoR = 0.0f;
    // a chain's guide vertex: its depth, and the material of the vertex before it, which a finite light's evaluation still finds in IntersectionData::material
    // (k_shade's rule, rt_shade_body.inl: that material's normal map is applied to the light's frame)
    const uint32_t flags = kChain ? ubits(prec(paths, R_ORIGIN, i).w) : 0u;
    // (the virtual position of a pixel whose path passes nothing is its POSITION)
    if (isHit && (mask & (RT_AOV_FRAME_PLANES | RT_AOV_MATERIAL_PLANES | (kChain ? RT_AOV_BIT(RT_AOV_VIRTUAL_POSITION) : 0u))) != 0u)
    {
        // the primary ray as k_generate left it (depth 0: no origin offset), the evaluation as DebugRenderer::RenderPixel and PathTracerMIS::RenderPixel run it
        const Ray ray = makePathRay(prec(paths, R_ORIGIN, i), prec(paths, R_DIR, i), kChain ? flags & 0xFFu : 0u);
        if (kChain) sd.intersection.material = (flags >> 9) - 1u;   // 0 -> RT_NO_MATERIAL
        DiscardCounters cnt;
        if (hit.distance < FLT_MAX) sceneEvaluateIntersection<kLean>(scene, ray, hit, sd.intersection, cnt);
        // a finite light has no material (LightSceneObject::EvaluateIntersection leaves IntersectionData::material alone): its material planes stay 0
        if (!isLight && sd.intersection.material != RT_NO_MATERIAL && (mask & RT_AOV_MATERIAL_PLANES) != 0u) materialEvaluateShadingData<kLean>(scene, scene.materials[sd.intersection.material], sd);
    }

    const size_t at = firstOut + i;
    auto storeF = [&](uint32_t id, uint32_t channel, float v) { ((float*)plane[id])[(size_t)channel * channelStride + at] = v; };
    auto storeU = [&](uint32_t id, uint32_t v) { ((uint32_t*)plane[id])[at] = v; };
    auto store3 = [&](uint32_t id, V4 v) { storeF(id, 0u, v.x); storeF(id, 1u, v.y); storeF(id, 2u, v.z); };
    if (mask & RT_AOV_BIT(RT_AOV_DEPTH)) storeF(RT_AOV_DEPTH, 0u, hit.distance);   // (+inf on a miss: the walks leave it in the record)
    if (mask & RT_AOV_BIT(RT_AOV_POSITION)) store3(RT_AOV_POSITION, sd.intersection.frame.r[3]);
    if (mask & RT_AOV_BIT(RT_AOV_NORMAL)) store3(RT_AOV_NORMAL, sd.intersection.frame.r[2]);
    if (mask & RT_AOV_BIT(RT_AOV_TANGENT)) store3(RT_AOV_TANGENT, sd.intersection.frame.r[0]);
    if (mask & RT_AOV_BIT(RT_AOV_BITANGENT)) store3(RT_AOV_BITANGENT, sd.intersection.frame.r[1]);
    if (mask & RT_AOV_BIT(RT_AOV_TEXCOORD)) { storeF(RT_AOV_TEXCOORD, 0u, sd.intersection.texCoord.x); storeF(RT_AOV_TEXCOORD, 1u, sd.intersection.texCoord.y); }
    if (mask & RT_AOV_BIT(RT_AOV_BARYCENTRICS))
    {
        // u and v are barycentrics: only MeshShape::Traverse writes them (pathHitIsMeshTriangle's rule, rt_shade.inl)
        bool triangle = false;
        if (isHit) { const RtObject& obj = scene.objects[hit.objectId]; triangle = obj.objectKind != RT_OBJECT_LIGHT && obj.shapeKind == RT_SHAPE_MESH; }
        storeF(RT_AOV_BARYCENTRICS, 0u, triangle ? hit.u : 0.0f); storeF(RT_AOV_BARYCENTRICS, 1u, triangle ? hit.v : 0.0f);
    }
    if (mask & RT_AOV_BIT(RT_AOV_BASE_COLOR)) store3(RT_AOV_BASE_COLOR, sd.mp.baseColor);
    if (mask & RT_AOV_BIT(RT_AOV_EMISSION)) store3(RT_AOV_EMISSION, sd.mp.emission);
    if (mask & RT_AOV_BIT(RT_AOV_ROUGHNESS)) storeF(RT_AOV_ROUGHNESS, 0u, sd.mp.roughness);
    if (mask & RT_AOV_BIT(RT_AOV_METALNESS)) storeF(RT_AOV_METALNESS, 0u, sd.mp.metalness);
    if (mask & RT_AOV_BIT(RT_AOV_IOR)) storeF(RT_AOV_IOR, 0u, sd.mp.IoR);
    if (mask & RT_AOV_BIT(RT_AOV_OBJECT_ID)) storeU(RT_AOV_OBJECT_ID, hit.objectId);
    if (mask & RT_AOV_BIT(RT_AOV_SUB_OBJECT_ID)) storeU(RT_AOV_SUB_OBJECT_ID, isHit ? hit.subObjectId : 0u);
    if (mask & RT_AOV_BIT(RT_AOV_MATERIAL)) storeU(RT_AOV_MATERIAL, kChain && isLight ? RT_NO_MATERIAL : sd.intersection.material);
    if (kChain)
    {
        if (mask & RT_AOV_BIT(RT_AOV_CHAIN_LENGTH)) storeU(RT_AOV_CHAIN_LENGTH, flags & 0xFFu);
        // R_RESULT.x: the distances of the vertices passed, summed left to right by k_shade_chain (0 at depth 0)
        if (mask & RT_AOV_BIT(RT_AOV_CHAIN_DISTANCE)) storeF(RT_AOV_CHAIN_DISTANCE, 0u, prec(paths, R_RESULT, i).x + hit.distance);
        if (mask & RT_AOV_BIT(RT_AOV_CHAIN_THROUGHPUT)) { const float4 tp = prec(paths, R_TP, i); store3(RT_AOV_CHAIN_THROUGHPUT, V4(tp.x, tp.y, tp.z, 0.0f)); }
        if (mask & RT_AOV_BIT(RT_AOV_VIRTUAL_POSITION))
        {
            // the point on the primary ray at the unfolded path length: o + w * D, a rounded multiply and a rounded add, spelled out (the library is built with
            // -ffp-contract=off; the two intrinsics say the same where it counts).  o and w: what k_shade_chain left in R_SH_P / R_SH_TP when vertex 0 was passed; never written for k == 0, never read then
            const float distance = prec(paths, R_RESULT, i).x + hit.distance;
            V4 v = sd.intersection.frame.r[3];
            if ((flags & 0xFFu) != 0u)
            {
                const float4 o = prec(paths, R_SH_P, i), w = prec(paths, R_SH_TP, i);
                v = V4(__fadd_rn(o.x, __fmul_rn(w.x, distance)), __fadd_rn(o.y, __fmul_rn(w.y, distance)), __fadd_rn(o.z, __fmul_rn(w.z, distance)), 0.0f);
            }
            if ((ubits(distance) & 0x7FFFFFFFu) == 0x7F800000u) v = zero4();   // a miss
            store3(RT_AOV_VIRTUAL_POSITION, v);
        }
    }
    if (rayCounts)
    {
        // the counting walk's record of this slot's ray (TravTuning::rayCounts): box tests, passed box tests, triangle tests, passed triangle tests
        const uint4 n = rayCounts[i];
        if (mask & RT_AOV_BIT(RT_AOV_BOX_TESTS)) storeU(RT_AOV_BOX_TESTS, n.x);
        if (mask & RT_AOV_BIT(RT_AOV_BOX_TESTS_PASSED)) storeU(RT_AOV_BOX_TESTS_PASSED, n.y);
        if (mask & RT_AOV_BIT(RT_AOV_TRIANGLE_TESTS)) storeU(RT_AOV_TRIANGLE_TESTS, n.z);
        if (mask & RT_AOV_BIT(RT_AOV_TRIANGLE_TESTS_PASSED)) storeU(RT_AOV_TRIANGLE_TESTS_PASSED, n.w);
    }
}

template <int kLean>
__global__ void __launch_bounds__(RT_BLOCK) k_aov_resolve RT_K_AOV_RESOLVE_ARGS
{
    aovResolve<kLean, false>(scene, paths, count, mask, out.plane, channelStride, firstOut, rayCounts);
}

template <int kLean>
__global__ void __launch_bounds__(RT_BLOCK) k_aov_resolve_chain RT_K_AOV_RESOLVE_CHAIN_ARGS
{
    aovResolve<kLean, true>(scene, paths, count, mask, out.plane, channelStride, firstOut, nullptr);
}
