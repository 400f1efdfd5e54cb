// rt_query.inl -- the kernels around a batched ray query (rtgpu_trace_rays, include/rtgpu.h).  Included by rt_trace.hip.
// A query is not a second traversal: the user's rays become path records and queue entries of the interface the integrators already use, and
// the launch the context renders with walks them (k_trace_wide / k_trace_wide2 + the re-trace launch, or k_trace):
//   k_query_load      RtQueryRay -> closest-hit rays: R_ORIGIN / R_DIR at depth 0 (no 1e-3 offset, no depth-dependent tolerance), slot in the queue;
//                                   any-hit requests: R_SH_P and pshadow(0, 0) = {dir, tmax}, request = slot (light 0) in the queue.
//                     The queue is the identity; a degenerate ray (queryRayIsDegenerate) walks a parked stand-in that misses the root box.
//   k_query_store     R_HIT + R_SAMPLER.x (the hit's v) -> RtQueryHit with the maxDistance rule; pshadow.w < 0 -> occluded = 1; degenerate rays:
//                     a miss / 0
//   k_query_evaluate  Scene::EvaluateIntersection of every hit -> RtQuerySurface
// Slot i of the query's arena is ray i of the chunk.

__global__ void __launch_bounds__(RT_BLOCK) k_query_load(const float4* __restrict__ rays, uint32_t count, uint32_t mode, const Paths paths,
                                                         uint32_t* __restrict__ queue, uint32_t* __restrict__ queueCount, unsigned long long* counters)
{
    // The queue is the identity and a degenerate ray walks a parked stand-in that leaves the root box behind at once (k_query_store answers it from
    // the user's record): compacting the queue took a returning atomic per wave on one word, 0.4 ms per 2 M rays.
    const uint32_t i = blockIdx.x * RT_BLOCK + threadIdx.x;
    if (i == 0u)
    {
        *queueCount = count;
        if (mode == RTGPU_TRACE_CLOSEST) atomicAdd(&counters[C_RAYS], (unsigned long long)count);
    }
    if (i >= count) return;
    float4 a = rays[2u * i], b = rays[2u * i + 1u];   // {origin, maxDistance}, {direction, -}
    if (queryRayIsDegenerate(a.x, a.y, a.z, a.w, b.x, b.y, b.z)) { a = f4(1e30f, 1e30f, 1e30f, 1.0f); b = f4(1.0f, 1.0f, 1.0f, 0.0f); }
    if (mode == RTGPU_TRACE_CLOSEST)
    {
        prec(paths, R_ORIGIN, i) = f4(a.x, a.y, a.z, fbits(0u));   // flags: depth 0
        prec(paths, R_DIR, i) = f4(b.x, b.y, b.z, 0.0f);
        prec(paths, R_HIT, i) = f4(fbits(RT_INVALID_OBJECT), fbits(0u), __uint_as_float(0x7f800000u), 0.0f);
        prec(paths, R_SAMPLER, i) = f4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    else
    {
        prec(paths, R_SH_P, i) = f4(a.x, a.y, a.z, 0.0f);
        pshadow(paths, 0u, 0u, i) = f4(b.x, b.y, b.z, a.w);   // tmax (the walks mark an occluded request with -1)
    }
    queue[i] = i;
}

__global__ void __launch_bounds__(RT_BLOCK) k_query_store(const RtSceneDesc scene, const float4* __restrict__ rays, uint32_t count, uint32_t mode, const Paths paths,
                                                          float4* __restrict__ hits, uint32_t* __restrict__ occluded)
{
    const uint32_t i = blockIdx.x * RT_BLOCK + threadIdx.x;
    if (i >= count) return;
    const float4 a = rays[2u * i], b = rays[2u * i + 1u];
    const bool degenerate = queryRayIsDegenerate(a.x, a.y, a.z, a.w, b.x, b.y, b.z);
    if (mode != RTGPU_TRACE_CLOSEST)
    {
        occluded[i] = !degenerate && pshadow(paths, 0u, 0u, i).w < 0.0f ? 1u : 0u;
        return;
    }
    // Scene::Traverse with hitPoint.distance = maxDistance: the walks start every closest-hit ray at +inf, a hit at or beyond maxDistance is none
    const float maxDistance = a.w;
    const float4 h = prec(paths, R_HIT, i);
    const uint32_t objectId = ubits(h.x);
    const bool hit = !degenerate && objectId != RT_INVALID_OBJECT && h.z < maxDistance;
    bool mesh = false;
    if (hit)
    {
        const RtObject& obj = scene.objects[objectId];
        mesh = obj.objectKind == RT_OBJECT_SHAPE && obj.shapeKind == RT_SHAPE_MESH;   // u, v: mesh triangles only
    }
    const float v = mesh ? prec(paths, R_SAMPLER, i).x : 0.0f;
    hits[2u * i] = f4(hit ? h.z : maxDistance, fbits(hit ? objectId : RT_INVALID_OBJECT), hit ? h.y : fbits(0u), mesh ? h.w : 0.0f);
    hits[2u * i + 1u] = f4(v, 0.0f, 0.0f, 0.0f);
}

__global__ void __launch_bounds__(RT_BLOCK) k_query_evaluate(const RtSceneDesc scene, const float4* __restrict__ rays, uint32_t count, const float4* __restrict__ hits,
                                                             float4* __restrict__ surfaces, unsigned long long* counters)
{
    const uint32_t i = blockIdx.x * RT_BLOCK + threadIdx.x;
    bool meshHit = false, analyticHit = false;
    if (i < count)
    {
        const float4 h0 = hits[2u * i], h1 = hits[2u * i + 1u];
        float4 s0 = f4(0.0f, 0.0f, 0.0f, 0.0f), s1 = s0, s2 = f4(0.0f, 0.0f, 0.0f, fbits(RT_NO_MATERIAL));
        if (ubits(h0.y) != RT_INVALID_OBJECT)
        {
            // numMeshHits / numAnalyticHits are tallied per block below: the function's own tally (one of two counters picked per lane) would live in scratch
            DiscardCounters cnt;
            const RtObject& obj = scene.objects[ubits(h0.y)];
            meshHit = obj.objectKind == RT_OBJECT_SHAPE && obj.shapeKind == RT_SHAPE_MESH;
            analyticHit = !meshHit;
            const float4 a = rays[2u * i], b = rays[2u * i + 1u];
            const Ray ray = makeRay(V4(a.x, a.y, a.z, 0.0f), V4(b.x, b.y, b.z, 0.0f));
            Hit hit; hit.objectId = ubits(h0.y); hit.subObjectId = ubits(h0.z); hit.distance = h0.x; hit.u = h0.w; hit.v = h1.x;
            Intersection is;
            for (int k = 0; k < 4; ++k) is.frame.r[k] = zero4();
            is.texCoord = zero4(); is.material = RT_NO_MATERIAL;
            sceneEvaluateIntersection<0>(scene, ray, hit, is, cnt);
            const V4 p = is.frame.r[3], n = is.frame.r[2], t = is.frame.r[0];
            s0 = f4(p.x, p.y, p.z, n.x); s1 = f4(n.y, n.z, t.x, t.y); s2 = f4(t.z, is.texCoord.x, is.texCoord.y, fbits(is.material));
        }
        surfaces[3u * i] = s0; surfaces[3u * i + 1u] = s1; surfaces[3u * i + 2u] = s2;
    }
    const int meshHits = __syncthreads_count(meshHit), analyticHits = __syncthreads_count(analyticHit);   // one atomic per block and counter
    if (threadIdx.x == 0u)
    {
        if (meshHits) atomicAdd(&counters[C_MESH_HITS], (unsigned long long)meshHits);
        if (analyticHits) atomicAdd(&counters[C_ANALYTIC_HITS], (unsigned long long)analyticHits);
    }
}
