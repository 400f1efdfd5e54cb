// ray_query_oracle.cpp -- the CPU oracle's own scene walk behind the ray queries of include/rtgpu.h (rtgpu_trace_rays), for the tests:
// oracle/rto_core.h has sceneTraverse / sceneTraverseShadow / sceneEvaluateIntersection as static inline functions that liboracle.so does not
// export.  This file states the query semantics of rtgpu.h on top of them, record for record, and nothing else.
// Built by tests/test_ray_queries_cpu.py into tests/cpp/_build with the oracle Makefile's flags.
#include "../../oracle/rto_core.h"

using namespace rto;

static bool degenerate(const RtQueryRay& r)
{
    const float dx = r.direction[0], dy = r.direction[1], dz = r.direction[2];
    const float lengthSq = (dx * dx + dy * dy) + (dz * dz + 0.0f);
    const bool originFinite = std::isfinite(r.origin[0]) && std::isfinite(r.origin[1]) && std::isfinite(r.origin[2]);
    return !originFinite || !(lengthSq > 0.0f && lengthSq <= 3.402823466e+38f) || !(r.maxDistance > 0.0f);
}

static Ray queryRay(const RtQueryRay& r)
{
    return makeRay(V4(r.origin[0], r.origin[1], r.origin[2], 0.0f), V4(r.direction[0], r.direction[1], r.direction[2], 0.0f));
}

extern "C" {

// RTGPU_TRACE_CLOSEST: Scene::Traverse with hitPoint.distance = maxDistance, then (surfaces != NULL) Scene::EvaluateIntersection.
// counters: 16 x u64 in the oracle's (= RtCounters') order, accumulated.
int rqo_trace_closest(const RtSceneDesc* d, const RtQueryRay* rays, uint32_t n, RtQueryHit* hits, RtQuerySurface* surfaces, uint64_t* counters)
{
    for (uint32_t i = 0; i < n; ++i)
    {
        const RtQueryRay& r = rays[i];
        RtQueryHit& out = hits[i];
        memset(&out, 0, sizeof(out));
        out.distance = r.maxDistance; out.objectId = RT_INVALID_OBJECT;
        if (surfaces) { memset(&surfaces[i], 0, sizeof(RtQuerySurface)); surfaces[i].material = RT_NO_MATERIAL; }
        counters[C_RAYS]++;   // numRays: the closest-hit rays of the call
        if (degenerate(r)) continue;
        Counters cnt; memset(&cnt, 0, sizeof(cnt));
        const Ray ray = queryRay(r);
        Hit hit; hit.objectId = RT_INVALID_OBJECT; hit.subObjectId = 0; hit.distance = r.maxDistance; hit.u = 0.0f; hit.v = 0.0f;
        sceneTraverse(d, ray, hit, cnt);
        if (hit.objectId != RT_INVALID_OBJECT)
        {
            const RtObject& obj = d->objects[hit.objectId];
            const bool mesh = obj.objectKind == RT_OBJECT_SHAPE && obj.shapeKind == RT_SHAPE_MESH;
            if (!mesh) { hit.u = 0.0f; hit.v = 0.0f; }   // u, v: mesh triangles only
            out.distance = hit.distance; out.objectId = hit.objectId; out.subObjectId = hit.subObjectId; out.u = hit.u; out.v = hit.v;
            if (surfaces)
            {
                Intersection is;
                for (int k = 0; k < 4; ++k) is.frame.r[k] = V4(0.0f, 0.0f, 0.0f, 0.0f);
                is.texCoord = V4(0.0f, 0.0f, 0.0f, 0.0f); is.material = RT_NO_MATERIAL;
                sceneEvaluateIntersection(d, ray, hit, is, cnt);
                RtQuerySurface& s = surfaces[i];
                const V4 p = is.frame.r[3], nrm = is.frame.r[2], t = is.frame.r[0];
                s.position[0] = p.x; s.position[1] = p.y; s.position[2] = p.z;
                s.normal[0] = nrm.x; s.normal[1] = nrm.y; s.normal[2] = nrm.z;
                s.tangent[0] = t.x; s.tangent[1] = t.y; s.tangent[2] = t.z;
                s.texCoord[0] = is.texCoord.x; s.texCoord[1] = is.texCoord.y; s.material = is.material;
            }
        }
        for (int k = 0; k < 16; ++k) counters[k] += cnt.c[k];
    }
    return 0;
}

// RTGPU_TRACE_ANY: Scene::Traverse_Shadow with hitPoint.distance = maxDistance on Ray(origin, direction) moved by direction * 0 (the
// Light Tracer's offset, as the walks apply it)
int rqo_trace_any(const RtSceneDesc* d, const RtQueryRay* rays, uint32_t n, uint32_t* occluded, uint64_t* counters)
{
    for (uint32_t i = 0; i < n; ++i)
    {
        const RtQueryRay& r = rays[i];
        occluded[i] = 0u;
        if (degenerate(r)) continue;
        Counters cnt; memset(&cnt, 0, sizeof(cnt));
        cnt.c[C_SHADOW] = 1;
        Ray ray = queryRay(r);
        ray.origin = ray.origin + ray.dir * 0.0f;
        Hit hit; hit.objectId = RT_INVALID_OBJECT; hit.subObjectId = 0; hit.distance = r.maxDistance; hit.u = 0.0f; hit.v = 0.0f;
        occluded[i] = sceneTraverseShadow(d, ray, hit, cnt) ? 1u : 0u;
        for (int k = 0; k < 16; ++k) counters[k] += cnt.c[k];
    }
    return 0;
}

}
