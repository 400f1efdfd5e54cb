// rt_runtime_scene.inl -- rtgpu_upload_scene: validate, prepare (rt_scene_prepare.h: mesh nodes, shading records, the 4-wide trees, the scene class -- all on the
// host), then free the old scene and copy; rtgpu_update_objects: validate, rebuild the top level (same header), copy new transforms and the top level in
// place.  Included by rt_runtime.hip behind rt_scene_prepare.h.

template <typename T>
static int uploadArray(RtgpuContext* c, const T* host, size_t count, const T** outDev, size_t capacity = 0)   // capacity: elements to allocate, where more than count
{
    *outDev = nullptr;
    if (count == 0 && capacity == 0) return RTGPU_OK;
    if (!host && count) return fail(RTGPU_ERR_INVALID_ARGUMENT, "scene array pointer is NULL but its count is not zero");
    void* dev = nullptr;
    HIP_TRY(hipMalloc(&dev, (capacity > count ? capacity : count) * sizeof(T)));
    c->sceneAllocs.push_back(dev);
    HIP_TRY(rtMemcpy(dev, host, count * sizeof(T), hipMemcpyHostToDevice));
    *outDev = static_cast<const T*>(dev);
    return RTGPU_OK;
}

#define RT_SCENE_CHECK(expr) do { const SceneStatus _s = (expr); if (_s.code != RTGPU_OK) return fail(_s.code, _s.message); } while (0)   // a check of rt_scene_prepare.h

// rtgpu_upload_scene: the caller's tables are checked, then everything the device needs beside them is built on the host (prepareScene), then the old scene
// is freed and the new one copied
RTGPU_API int rtgpu_upload_scene(RtgpuContext* c, const RtSceneDesc* s)
{
    if (!c || !s) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    RT_FAN_OUT(c, rtgpu_upload_scene(peer, s));   // the scene is replicated: every device traverses its own copy
    if (s->abiVersion != RTGPU_ABI_VERSION) return fail(RTGPU_ERR_INVALID_ARGUMENT, "RtSceneDesc::abiVersion mismatch");
    HIP_TRY(hipSetDevice(c->device));
    { int fr = flushQueued(c); if (fr) return fr; }
    HIP_TRY(syncLanes(c));
    waitQueries(c);   // an asynchronous ray query or AOV call may still walk the old scene

    // validation: indices in range, stacks deep enough
    if (s->numObjects > 1 && s->numTopNodes == 0) return fail(RTGPU_ERR_INVALID_ARGUMENT, "scene with more than one object needs a top-level BVH");
    const uint32_t topDepth = bvhDepth(s->topNodes, s->numTopNodes);
    uint32_t maxMeshDepth = 0;
    RT_SCENE_CHECK(checkTreeDepth(topDepth, "malformed top-level BVH"));
    for (uint32_t i = 0; i < s->numMeshes; ++i)
    {
        const RtMesh& m = s->meshes[i];
        if ((uint64_t)m.firstNode + m.numNodes > s->numMeshNodes || (uint64_t)m.firstTriangle + m.numTriangles > s->numTriangles || (uint64_t)m.firstVertex + m.numVertices > s->numVertices)
            return fail(RTGPU_ERR_INVALID_ARGUMENT, "mesh ranges out of bounds");
        for (uint32_t t = 0; t < m.numTriangles; ++t)
        {
            const RtVertexIndices& idx = s->vertexIndices[m.firstTriangle + t];
            if (idx.i0 >= m.numVertices || idx.i1 >= m.numVertices || idx.i2 >= m.numVertices) return fail(RTGPU_ERR_INVALID_ARGUMENT, "triangle vertex index out of range");
        }
        const uint32_t md = bvhDepth(s->meshNodes + m.firstNode, m.numNodes);
        RT_SCENE_CHECK(checkTreeDepth(md, "malformed mesh BVH"));
        if (md > maxMeshDepth) maxMeshDepth = md;
    }
    RT_SCENE_CHECK(checkStack(topDepth, maxMeshDepth));
    RT_SCENE_CHECK(checkLeaves(s->topNodes, s->numTopNodes));
    RT_SCENE_CHECK(checkLeaves(s->meshNodes, s->numMeshNodes));
    for (uint32_t i = 0; i < s->numObjects; ++i)
    {
        const RtObject& o = s->objects[i];
        if (o.objectKind == RT_OBJECT_LIGHT) { if (o.lightIndex >= s->numLights) return fail(RTGPU_ERR_INVALID_ARGUMENT, "object light index out of range"); }
        else
        {
            if (o.materialIndex >= s->numMaterials) return fail(RTGPU_ERR_INVALID_ARGUMENT, "object material index out of range");
            if (o.shapeKind == RT_SHAPE_MESH && o.meshIndex >= s->numMeshes) return fail(RTGPU_ERR_INVALID_ARGUMENT, "object mesh index out of range");
            if (o.shapeKind > RT_SHAPE_MESH) return fail(RTGPU_ERR_UNSUPPORTED, "unknown shape kind");
        }
    }
    for (uint32_t i = 0; i < s->numTriangles; ++i)
        if (s->vertexIndices[i].materialIndex != RT_NO_MATERIAL && s->vertexIndices[i].materialIndex >= s->numMaterials) return fail(RTGPU_ERR_INVALID_ARGUMENT, "triangle material index out of range");
    for (uint32_t i = 0; i < s->numGlobalLights; ++i) if (s->globalLights[i] >= s->numLights) return fail(RTGPU_ERR_INVALID_ARGUMENT, "global light index out of range");
    for (uint32_t i = 0; i < s->numMaterials; ++i) if (s->materials[i].bsdf > RT_BSDF_ROUGH_PLASTIC) return fail(RTGPU_ERR_UNSUPPORTED, "unknown BSDF kind");
    if (s->numMaterials >= (1u << 22)) return fail(RTGPU_ERR_UNSUPPORTED, "more than 4M materials");   // the path flags hold a material index in 23 bits
    // textures: known kinds and formats, rows / blocks / palettes inside the texel blob, mixes nested at most one level deep
    for (uint32_t i = 0; i < s->numTextures; ++i)
    {
        const RtTexture& t = s->textures[i];
        if (t.kind == RT_TEXTURE_CHECKERBOARD || t.kind == RT_TEXTURE_CONST) continue;
        if (t.kind == RT_TEXTURE_NOISE) { if (t.numOctaves == 0 || t.numOctaves > 20) return fail(RTGPU_ERR_INVALID_ARGUMENT, "noise octaves must be 1..20"); continue; }
        if (t.kind == RT_TEXTURE_MIX)
        {
            const uint32_t children[3] = { t.mixA, t.mixB, t.mixWeight };
            for (uint32_t child : children)
            {
                if (child >= s->numTextures) return fail(RTGPU_ERR_INVALID_ARGUMENT, "mix texture child index out of range");
                const RtTexture& c = s->textures[child];
                if (c.kind != RT_TEXTURE_MIX) continue;
                const uint32_t grandChildren[3] = { c.mixA, c.mixB, c.mixWeight };
                for (uint32_t g : grandChildren)
                    if (g >= s->numTextures || s->textures[g].kind == RT_TEXTURE_MIX) return fail(RTGPU_ERR_UNSUPPORTED, "mix textures nested more than one level deep");
            }
            continue;
        }
        if (t.kind != RT_TEXTURE_BITMAP) return fail(RTGPU_ERR_UNSUPPORTED, "unknown texture kind");
        uint32_t bits = 0;
        switch (t.format)
        {
        case RT_FORMAT_R8_UNORM: case RT_FORMAT_B8G8R8A8_UNORM_PALETTE: case RT_FORMAT_BC5: bits = 8; break;
        case RT_FORMAT_R8G8_UNORM: case RT_FORMAT_R16_UNORM: case RT_FORMAT_R16_HALF: case RT_FORMAT_B5G6R5_UNORM: bits = 16; break;
        case RT_FORMAT_B8G8R8_UNORM: bits = 24; break;
        case RT_FORMAT_B8G8R8A8_UNORM: case RT_FORMAT_R8G8B8A8_UNORM: case RT_FORMAT_R16G16_UNORM: case RT_FORMAT_R32_FLOAT: case RT_FORMAT_R16G16_HALF:
        case RT_FORMAT_R11G11B10_FLOAT: case RT_FORMAT_R9G9B9E5_SHAREDEXP: bits = 32; break;
        case RT_FORMAT_R16G16B16_HALF: bits = 48; break;
        case RT_FORMAT_R16G16B16A16_UNORM: case RT_FORMAT_R32G32_FLOAT: case RT_FORMAT_R16G16B16A16_HALF: bits = 64; break;
        case RT_FORMAT_R32G32B32_FLOAT: bits = 96; break;
        case RT_FORMAT_R32G32B32A32_FLOAT: bits = 128; break;
        case RT_FORMAT_BC1: case RT_FORMAT_BC4: bits = 4; break;
        default: return fail(RTGPU_ERR_UNSUPPORTED, "unknown bitmap format");
        }
        if (t.width == 0 || t.height == 0 || t.width > 65536u || t.height > 65536u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "invalid texture size");
        if (t.filter > RT_FILTER_BILINEAR_SMOOTHSTEP) return fail(RTGPU_ERR_INVALID_ARGUMENT, "unknown texture filter");
        const bool blocks = t.format == RT_FORMAT_BC1 || t.format == RT_FORMAT_BC4 || t.format == RT_FORMAT_BC5;
        uint64_t extent;
        if (blocks)
        {
            if ((t.width & 3u) || (t.height & 3u)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "block-compressed textures need dimensions that are multiples of 4");
            extent = (uint64_t)(t.width / 4u) * (t.height / 4u) * (t.format == RT_FORMAT_BC5 ? 16u : 8u);
        }
        else
        {
            const uint32_t texelSize = bits / 8u;
            if (t.stride < t.width * texelSize) return fail(RTGPU_ERR_INVALID_ARGUMENT, "texture stride smaller than a row");
            extent = (uint64_t)t.stride * (t.height - 1u) + (uint64_t)t.width * texelSize;
        }
        if (!s->texelData || t.dataOffset + extent > s->texelBytes) return fail(RTGPU_ERR_INVALID_ARGUMENT, "texture data outside texelData");
        if (t.format == RT_FORMAT_B8G8R8A8_UNORM_PALETTE && t.paletteOffset + 1024u > s->texelBytes) return fail(RTGPU_ERR_INVALID_ARGUMENT, "texture palette (256 entries) outside texelData");
    }
    auto textureOk = [&](uint32_t index) { return index == RT_NO_TEXTURE || index < s->numTextures; };
    for (uint32_t i = 0; i < s->numMaterials; ++i)
    {
        const RtMaterial& m = s->materials[i];
        if (!textureOk(m.baseColorTexture) || !textureOk(m.emissionTexture) || !textureOk(m.roughnessTexture) || !textureOk(m.metalnessTexture) || !textureOk(m.normalMapTexture))
            return fail(RTGPU_ERR_INVALID_ARGUMENT, "material texture index out of range");
    }
    for (uint32_t i = 0; i < s->numLights; ++i) if (!textureOk(s->lights[i].texture)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "light texture index out of range");

    // prepare: the breadth-first mesh nodes, the shading records, the 4-wide trees, the scene class (RTGPU_NO_SIMPLE_TEXTURES=1: class 2 instead of 4)
    const PreparedScene p = prepareScene(*s, topDepth, maxMeshDepth, !knobs::noLean(), !knobs::noSimpleTextures());

    // copy (nothing of the context has changed up to here: a refused scene leaves the old one, its photons and the temporal history as they were)
    c->temporal.have = false;   // rtgpu_denoise_temporal's history shows the old scene
    beamInvalidate(c); beamFreeRetired(c);   // beam lists hold the old tree's leaves (the lanes are idle)
    freeScene(c);
    RtSceneDesc d = *s;
    int r;
    // (room for the largest tree over numObjects leaves -- 2 n - 1 nodes and the unused node 1 --: rtgpu_update_objects replaces the top level in place)
    c->updatable = RtgpuContext::Updatable();
    c->updatable.topNodeCapacity = s->numTopNodes > 2u * s->numObjects + 2u ? s->numTopNodes : 2u * s->numObjects + 2u;
    if ((r = uploadArray(c, s->topNodes, s->numTopNodes, &d.topNodes, s->numObjects ? c->updatable.topNodeCapacity : 0u))) return r;
    if ((r = uploadArray(c, s->objects, s->numObjects, &d.objects))) return r;
    if ((r = uploadArray(c, s->lights, s->numLights, &d.lights))) return r;
    if ((r = uploadArray(c, s->globalLights, s->numGlobalLights, &d.globalLights))) return r;
    if ((r = uploadArray(c, s->materials, s->numMaterials, &d.materials))) return r;
    if ((r = uploadArray(c, s->meshes, s->numMeshes, &d.meshes))) return r;
    if ((r = uploadArray(c, p.meshNodes.data(), p.meshNodes.size(), &d.meshNodes))) return r;
    if ((r = uploadArray(c, s->triangles, s->numTriangles, &d.triangles))) return r;
    {
        const TriangleShading* dev = nullptr;   // where the C ABI's vertexIndices[] would be (rt_wide_format.h)
        if ((r = uploadArray(c, p.shading.data(), p.shading.size(), &dev))) return r;
        d.vertexIndices = reinterpret_cast<const RtVertexIndices*>(dev);
        d.vertexShading = nullptr;
    }
    if ((r = uploadArray(c, s->blueNoise, s->blueNoise ? (size_t)128 * 128 * 4 : 0, &d.blueNoise))) return r;
    if ((r = uploadArray(c, s->textures, s->numTextures, &d.textures))) return r;
    if ((r = uploadArray(c, s->texelData, s->numTextures ? (size_t)s->texelBytes : 0, &d.texelData))) return r;
    memset(&c->wide, 0, sizeof(c->wide));
    memset(&c->wide2, 0, sizeof(c->wide2));
    if (p.twoLevel.ok)
    {
        // the two-level 4-wide walk (rt_trace_wide2.inl); the top level's slab is the end of the node array: rtgpu_update_objects rebuilds it there
        const TwoLevelBuild& t = p.twoLevel;
        const float4* devNodes = nullptr; const float4* devGates = nullptr; const WideLevel* devLevels = nullptr;
        if ((r = uploadArray(c, t.nodes.data(), t.nodes.size(), &devNodes))) return r;
        if ((r = uploadArray(c, t.gates.data(), t.gates.size(), &devGates))) return r;
        if ((r = uploadArray(c, t.levels.data(), t.levels.size(), &devLevels))) return r;
        c->wide2.nodes = devNodes; c->wide2.gate = devGates; c->wide2.levels = devLevels; c->wide2.numObjects = s->numObjects;
        c->walkNodeBytes[RTGPU_WALK_WIDE2] = t.usedNodes * sizeof(float4); c->walkLeafBoxBytes[RTGPU_WALK_WIDE2] = t.gates.size() * sizeof(float4);
        c->updatable.levels = t.levels; c->updatable.wide2 = c->wide2; c->updatable.topWideNodeCapacity = t.topNodeCapacity;
        c->updatable.meshNodeBytes = t.meshNodes * sizeof(float4); c->updatable.meshGateBytes = t.meshGates * sizeof(float4);
    }
    if (p.single.ok)
    {
        // a single-mesh scene (Scene::Traverse's one-object bypass): the re-encoded tree of the default traversal kernel (rt_trace_wide.inl)
        const float4* devGate = nullptr; const float4* devWide = nullptr;
        if ((r = uploadArray(c, p.singleGrid.gate.data(), p.singleGrid.gate.size(), &devGate))) return r;
        if ((r = uploadArray(c, p.single.nodes.data(), p.single.nodes.size(), &devWide))) return r;
        c->wide.nodes = devWide; c->wide.gate = devGate; c->wide.numNodes = (uint32_t)(p.single.nodes.size() / 4u);
        c->walkNodeBytes[RTGPU_WALK_WIDE] = p.single.nodes.size() * sizeof(float4); c->walkLeafBoxBytes[RTGPU_WALK_WIDE] = p.singleGrid.gate.size() * sizeof(float4);
        copyGrid(c->wide, p.singleGrid.grid);
    }
    {
        // what rtgpu_update_mesh refits by (rt_runtime_refit.inl)
        RtgpuContext::Updatable& up = c->updatable;
        if (p.twoLevel.ok && (r = uploadArray(c, p.wide2SlotNode.data(), p.wide2SlotNode.size(), &up.wide2SlotNode))) return r;
        if (p.single.ok && (r = uploadArray(c, p.wideSlotNode.data(), p.wideSlotNode.size(), &up.wideSlotNode))) return r;
        up.meshTable.assign(s->meshes, s->meshes + s->numMeshes);
        up.vertexIndices.assign(s->vertexIndices, s->vertexIndices + s->numTriangles);
        up.meshes.resize(s->numMeshes);
        for (uint32_t m = 0; m < s->numMeshes; ++m) { up.meshes[m].plan = p.refit[m]; up.meshes[m].level = p.meshLevels[m]; }
    }
    c->sceneDev = d;
    c->walkNodeBytes[RTGPU_WALK_BINARY] = ((uint64_t)s->numTopNodes + s->numMeshNodes) * sizeof(RtNode); c->walkTriangleBytes = (uint64_t)s->numTriangles * sizeof(RtTriangle);
    c->numLights = s->numLights;
    c->traversalStackNeed = topDepth + maxMeshDepth;
    c->updatable.maxMeshDepth = maxMeshDepth;
    c->updatable.objects.assign(s->objects, s->objects + s->numObjects); c->updatable.lights.assign(s->lights, s->lights + s->numLights);
    c->leanScene = p.leanScene;
    c->axisParallelSun = p.axisParallelSun;
    c->sceneReady = true;
    c->vcm.havePhotons = false;   // photons of another scene
    return RTGPU_OK;
}

// ---- rtgpu_update_objects (include/rtgpu.h): new transforms and a new top level in place ------------------------------------------------------------
// Everything is checked and built on the host first -- against the host copies RtgpuContext::Updatable keeps of the device's tables --, then copied: a refused
// update has touched nothing.  The device arrays keep their addresses (the top-level nodes and the 4-wide top level were allocated with room for the largest
// tree over numObjects leaves), so kernels launched afterwards read the new scene through the same RtSceneDesc / WideScene pointers.
template <class T> static bool sameBut2Matrices(const T& a, const T& b)   // RtObject / RtLight: transform and invTransform come first
{
    return memcmp((const char*)&a + 128, (const char*)&b + 128, sizeof(T) - 128u) == 0;
}

RTGPU_API int rtgpu_update_objects(RtgpuContext* c, const RtSceneUpdate* u)
{
    if (!c || !u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    RT_FAN_OUT(c, rtgpu_update_objects(peer, u));   // every device traverses its own copy (a refusal is the same on each: the first peer returns it)
    if (u->abiVersion != RTGPU_ABI_VERSION) return fail(RTGPU_ERR_INVALID_ARGUMENT, "RtSceneUpdate::abiVersion mismatch");
    if (!c->sceneReady) return fail(RTGPU_ERR_NOT_READY, "rtgpu_upload_scene has not been called");
    HIP_TRY(hipSetDevice(c->device));
    { int fr = flushQueued(c); if (fr) return fr; }
    HIP_TRY(syncLanes(c));
    waitQueries(c);
    RtgpuContext::Updatable& up = c->updatable;
    const uint32_t n = u->numObjects;
    if (n != c->sceneDev.numObjects || u->numLights != c->sceneDev.numLights) return fail(RTGPU_ERR_INVALID_ARGUMENT, "an update keeps the scene's object and light counts");
    if ((n && (!u->objects || !u->previousIndex)) || (u->numTopNodes && !u->topNodes)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "update array pointer is NULL but its count is not zero");
    if (n > 1u && u->numTopNodes == 0u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "scene with more than one object needs a top-level BVH");
    if (u->numTopNodes > up.topNodeCapacity) return fail(RTGPU_ERR_INVALID_ARGUMENT, "more top-level nodes than a tree over the scene's objects can have");
    {
        std::vector<uint8_t> seen(n, 0u);
        for (uint32_t i = 0; i < n; ++i)
        {
            const uint32_t p = u->previousIndex[i];
            if (p >= n || seen[p]) return fail(RTGPU_ERR_INVALID_ARGUMENT, "previousIndex is not a permutation");
            seen[p] = 1u;
            if (!sameBut2Matrices(u->objects[i], up.objects[p])) return fail(RTGPU_ERR_INVALID_ARGUMENT, "an update changes transforms only: an object differs from its predecessor in another field");
        }
    }
    for (uint32_t i = 0; u->lights && i < u->numLights; ++i)
        if (!sameBut2Matrices(u->lights[i], up.lights[i])) return fail(RTGPU_ERR_INVALID_ARGUMENT, "an update changes transforms only: a light differs from its predecessor in another field");
    const uint32_t topDepth = bvhDepth(u->topNodes, u->numTopNodes);
    RT_SCENE_CHECK(checkTreeDepth(topDepth, "malformed top-level BVH"));
    RT_SCENE_CHECK(checkLeaves(u->topNodes, u->numTopNodes, n));
    RT_SCENE_CHECK(checkStack(topDepth, up.maxMeshDepth));

    // rebuild: the 4-wide top level and the level table in the new order (two-level scenes; the slab holds a top level over n objects whatever its tree)
    TopLevelRebuild rebuilt;
    if (!up.levels.empty()) rebuilt = rebuildTopLevel(up.levels, u->previousIndex, u->topNodes, u->numTopNodes, n, topDepth, up.topWideNodeCapacity);
    const std::vector<WideLevel>& levels = rebuilt.levels;
    const WideLevelBuild& top = rebuilt.top;
    const bool topFits = top.ok;

    // copy
    uint64_t bytes = 0;
    auto put = [&](const void* dev, const void* host, size_t size) -> hipError_t { bytes += size; return rtMemcpy(const_cast<void*>(dev), host, size, hipMemcpyHostToDevice); };
    HIP_TRY(put(c->sceneDev.objects, u->objects, (size_t)n * sizeof(RtObject)));
    HIP_TRY(put(c->sceneDev.topNodes, u->topNodes, (size_t)u->numTopNodes * sizeof(RtNode)));
    if (u->lights) HIP_TRY(put(c->sceneDev.lights, u->lights, (size_t)u->numLights * sizeof(RtLight)));
    if (!levels.empty())
    {
        if (topFits)
        {
            HIP_TRY(put(up.wide2.nodes + 4u * (size_t)levels[n].nodeBase, top.nodes.data(), top.nodes.size() * sizeof(float4)));
            HIP_TRY(put(up.wide2.gate + levels[n].gateBase, top.gate.data(), top.gate.size() * sizeof(float4)));
        }
        HIP_TRY(put(up.wide2.levels, levels.data(), levels.size() * sizeof(WideLevel)));
        // (a top level that cannot be built leaves the scene to the binary walk, as at upload, until an update brings one that can)
        if (topFits) c->wide2 = up.wide2; else memset(&c->wide2, 0, sizeof(c->wide2));
        c->walkNodeBytes[RTGPU_WALK_WIDE2] = up.meshNodeBytes + top.nodes.size() * sizeof(float4);
        up.levels = levels;
    }
    c->sceneDev.numTopNodes = u->numTopNodes;
    c->walkNodeBytes[RTGPU_WALK_BINARY] = ((uint64_t)u->numTopNodes + c->sceneDev.numMeshNodes) * sizeof(RtNode);
    up.objects.assign(u->objects, u->objects + n);
    if (u->lights) { up.lights.assign(u->lights, u->lights + u->numLights); c->axisParallelSun = hasAxisParallelSun(u->lights, u->numLights); }
    c->traversalStackNeed = topDepth + up.maxMeshDepth;
    c->vcm.havePhotons = false;   // photons of the scene as it was
    beamInvalidate(c); beamFreeRetired(c);   // (and beam lists in the mesh object's frame as it was; the lanes are idle)
    if (c->temporal.have && c->temporal.then.size() == n)
    {
        // rtgpu_denoise_temporal's history stays: current object i is the one that was previousIndex[i], and carries that one's id and transform of then
        std::vector<RtgpuContext::Temporal::Then> then(n);
        for (uint32_t i = 0; i < n; ++i) then[i] = c->temporal.then[u->previousIndex[i]];
        c->temporal.then.swap(then);
        c->temporal.movedSince = true;
    }
    else c->temporal.have = false;
    up.info.bytesUploaded = bytes; up.info.numUpdates++; up.info.topDepth = topDepth;
    return RTGPU_OK;
}
