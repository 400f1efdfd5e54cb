// rt_runtime_scene.inl -- rtgpu_upload_scene: validation, the device copies of the scene, the 4-wide trees, the scene class; rtgpu_update_objects: new transforms
// and a new top level in place.  Included by rt_runtime.hip.

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

// depth of a BVH in stack entries: the traversal pushes at most one node per interior level
static uint32_t bvhDepth(const RtNode* nodes, uint32_t numNodes)
{
    if (numNodes == 0) return 0;
    uint32_t maxDepth = 0;
    std::vector<std::pair<uint32_t, uint32_t>> stack;
    stack.push_back({ 0u, 0u });
    while (!stack.empty())
    {
        const auto [idx, depth] = stack.back(); stack.pop_back();
        if (idx >= numNodes) return 0xFFFFFFFFu;
        const RtNode& n = nodes[idx];
        if ((n.leaves & 0x3FFFFFFFu) != 0) { if (depth > maxDepth) maxDepth = depth; continue; }
        if (depth > 4096) return 0xFFFFFFFFu;
        stack.push_back({ n.childIndex, depth + 1 }); stack.push_back({ n.childIndex + 1, depth + 1 });
    }
    return maxDepth;
}

// a delta directional light whose direction has an exactly-zero component: EVERY next-event ray towards it is axis-parallel and goes through the re-trace launches (launchRetrace)
static bool hasAxisParallelSun(const RtLight* lights, uint32_t numLights)
{
    for (uint32_t i = 0; i < numLights; ++i)
        if (lights[i].type == RT_LIGHT_DIRECTIONAL && lights[i].isDelta && (lights[i].transform[8] == 0.0f || lights[i].transform[9] == 0.0f || lights[i].transform[10] == 0.0f)) return true;
    return false;
}

RTGPU_API int rtgpu_upload_scene(RtgpuContext* c, const RtSceneDesc* s)
{
    if (!c || !s) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    RT_FAN_OUT(c, rtgpu_upload_scene(peer, s));   // the scene is replicated: every device traverses its own copy
    if (s->abiVersion != RTGPU_ABI_VERSION) return fail(RTGPU_ERR_INVALID_ARGUMENT, "RtSceneDesc::abiVersion mismatch");
    HIP_TRY(hipSetDevice(c->device));
    { int fr = flushPending(c); if (fr) return fr; }
    HIP_TRY(syncLanes(c));
    waitQueries(c);   // an asynchronous ray query or AOV call may still walk the old scene
    c->temporal.have = false;   // rtgpu_denoise_temporal's history shows the old scene

    // validation: indices in range, stacks deep enough
    if (s->numObjects > 1 && s->numTopNodes == 0) return fail(RTGPU_ERR_INVALID_ARGUMENT, "scene with more than one object needs a top-level BVH");
    const uint32_t topDepth = bvhDepth(s->topNodes, s->numTopNodes);
    uint32_t maxMeshDepth = 0;
    if (topDepth == 0xFFFFFFFFu) return fail(RTGPU_ERR_INVALID_ARGUMENT, "malformed top-level BVH");
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
        if (md == 0xFFFFFFFFu) return fail(RTGPU_ERR_INVALID_ARGUMENT, "malformed mesh BVH");
        if (md > maxMeshDepth) maxMeshDepth = md;
    }
    if (topDepth + maxMeshDepth > 64) return fail(RTGPU_ERR_UNSUPPORTED, "BVH deeper than the 64-entry traversal stack");
    for (uint32_t i = 0; i < s->numTopNodes; ++i) if ((s->topNodes[i].leaves & 0x3FFFFFFFu) > RT_MAX_PACKED_LEAVES) return fail(RTGPU_ERR_UNSUPPORTED, "BVH leaves with more than 3 items are not supported");
    for (uint32_t i = 0; i < s->numMeshNodes; ++i) if ((s->meshNodes[i].leaves & 0x3FFFFFFFu) > RT_MAX_PACKED_LEAVES) return fail(RTGPU_ERR_UNSUPPORTED, "BVH leaves with more than 3 items are not supported");
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
    {
        // mesh trees go to the device in BREADTH-FIRST order (root at 0, node 1 unused, child pairs from 2 on as the reference lays them
        // out, levels one after the other): the same tree -- a node's childIndex is only a pointer -- with the top levels every ray
        // walks through contiguous at the front, which k_trace stages in LDS.  Leaves keep their triangle ranges.
        std::vector<RtNode> ordered(s->meshNodes, s->meshNodes + s->numMeshNodes);
        for (uint32_t m = 0; m < s->numMeshes; ++m)
        {
            const RtMesh& mesh = s->meshes[m];
            if (mesh.numNodes < 3u) continue;
            const RtNode* src = s->meshNodes + mesh.firstNode;
            RtNode* dst = ordered.data() + mesh.firstNode;
            std::vector<uint32_t> oldIndex; oldIndex.reserve(mesh.numNodes);   // oldIndex[new position]
            oldIndex.push_back(0u); oldIndex.push_back(1u);
            for (size_t k = 0; k < oldIndex.size() && oldIndex.size() + 2u <= mesh.numNodes; ++k)
            {
                if (k == 1u) continue;
                const RtNode& n = src[oldIndex[k]];
                if ((n.leaves & 0x3FFFFFFFu) != 0u) continue;
                dst[k] = n; dst[k].childIndex = (uint32_t)oldIndex.size();
                oldIndex.push_back(n.childIndex); oldIndex.push_back(n.childIndex + 1u);
            }
            for (size_t k = 0; k < oldIndex.size(); ++k) if (k != 1u && (src[oldIndex[k]].leaves & 0x3FFFFFFFu) != 0u) dst[k] = src[oldIndex[k]];
        }
        if ((r = uploadArray(c, ordered.data(), ordered.size(), &d.meshNodes))) return r;
    }
    if ((r = uploadArray(c, s->triangles, s->numTriangles, &d.triangles))) return r;
    {
        // de-indexed shading records (rt_device_core.h, TriangleShading), built once here
        std::vector<TriangleShading> records(s->numTriangles);
        if (!records.empty()) memset(records.data(), 0, records.size() * sizeof(TriangleShading));
        for (uint32_t m = 0; m < s->numMeshes; ++m)
        {
            const RtMesh& mesh = s->meshes[m];
            const RtVertexShading* vs = s->vertexShading + mesh.firstVertex;
            for (uint32_t t = 0; t < mesh.numTriangles; ++t)
            {
                const RtVertexIndices& idx = s->vertexIndices[mesh.firstTriangle + t];
                TriangleShading& out = records[mesh.firstTriangle + t];
                out.v[0] = vs[idx.i0]; out.v[1] = vs[idx.i1]; out.v[2] = vs[idx.i2];
                out.materialIndex = idx.materialIndex;
            }
        }
        const TriangleShading* dev = nullptr;
        if ((r = uploadArray(c, records.data(), records.size(), &dev))) return r;
        d.vertexIndices = reinterpret_cast<const RtVertexIndices*>(dev);
        d.vertexShading = nullptr;
    }
    if ((r = uploadArray(c, s->blueNoise, s->blueNoise ? (size_t)128 * 128 * 4 : 0, &d.blueNoise))) return r;
    if ((r = uploadArray(c, s->textures, s->numTextures, &d.textures))) return r;
    if ((r = uploadArray(c, s->texelData, s->numTextures ? (size_t)s->texelBytes : 0, &d.texelData))) return r;
    // single-mesh scenes (Scene::Traverse's one-object bypass): the re-encoded tree of the default traversal kernel
    memset(&c->wide, 0, sizeof(c->wide));
    memset(&c->wide2, 0, sizeof(c->wide2));
    const bool singleMesh = s->numObjects == 1u && s->objects[0].objectKind == RT_OBJECT_SHAPE && s->objects[0].shapeKind == RT_SHAPE_MESH;
    bool anyMesh = false;
    for (uint32_t o = 0; o < s->numObjects; ++o) anyMesh = anyMesh || (s->objects[o].objectKind == RT_OBJECT_SHAPE && s->objects[o].shapeKind == RT_SHAPE_MESH);
    // (a handful of analytic objects -- sphere + area light: a top-level tree of one or three nodes -- gain nothing from wider nodes and pay
    //  for the re-trace launch: measured 3-5 % slower, the binary kernel keeps them)
    if (!singleMesh && s->numObjects > 1u && (anyMesh || s->numTopNodes >= 7u))
    {
        // every other scene: the two-level 4-wide walk (rt_trace_wide2.inl).  One node / gate array for all levels; levels[o] for mesh object o,
        // levels[numObjects] for the top-level tree.  A level that cannot be built (a malformed tree) leaves the scene to the binary walk.
        std::vector<float4> allNodes, allGates;
        std::vector<WideLevel> levels(s->numObjects + 1u);
        memset(levels.data(), 0, levels.size() * sizeof(WideLevel));
        bool ok = true;
        auto append = [&](const WideLevelBuild& b, WideLevel& level, uint32_t triBase)
        {
            level.nodeBase = (uint32_t)(allNodes.size() / 4u); level.gateBase = (uint32_t)allGates.size(); level.triBase = triBase; level.valid = 1u;
            memcpy(level.base, b.base, sizeof(b.base)); memcpy(level.step, b.step, sizeof(b.step)); memcpy(level.bound, b.bound, sizeof(b.bound));
            allNodes.insert(allNodes.end(), b.nodes.begin(), b.nodes.end()); allGates.insert(allGates.end(), b.gate.begin(), b.gate.end());
        };
        std::unordered_map<uint32_t, uint32_t> builtMesh;   // mesh index -> the first object whose level holds its tree (instances share it)
        for (uint32_t o = 0; o < s->numObjects && ok; ++o)
        {
            const RtObject& obj = s->objects[o];
            if (obj.objectKind != RT_OBJECT_SHAPE || obj.shapeKind != RT_SHAPE_MESH) continue;
            const RtMesh& mesh = s->meshes[obj.meshIndex];
            if (mesh.numNodes == 0u) continue;   // nothing to hit (Traverse_Object returns at once)
            const auto found = builtMesh.find(obj.meshIndex);
            if (found != builtMesh.end()) { levels[o] = levels[found->second]; continue; }
            const WideLevelBuild b = buildWideLevel(s->meshNodes + mesh.firstNode, mesh.numNodes, mesh.numTriangles, bvhDepth(s->meshNodes + mesh.firstNode, mesh.numNodes));
            if (!b.ok) { ok = false; break; }
            append(b, levels[o], mesh.firstTriangle);
            builtMesh[obj.meshIndex] = o;
        }
        // the top level goes BEHIND the mesh levels, into a slab that holds the largest one numObjects leaves can have (fewer 4-wide nodes than the binary
        // tree has interior ones; two gate records per object whatever the tree): rtgpu_update_objects rebuilds it there and no mesh base moves
        const size_t meshNodes = allNodes.size(), meshGates = allGates.size();
        size_t usedNodes = meshNodes;
        if (ok)
        {
            const WideLevelBuild top = buildWideLevel(s->topNodes, s->numTopNodes, s->numObjects, topDepth);
            if (top.ok && top.nodes.size() / 4u <= s->numObjects && top.gate.size() == 2u * (size_t)s->numObjects)
            {
                append(top, levels[s->numObjects], 0u);
                usedNodes = allNodes.size();
                allNodes.resize(meshNodes + 4u * (size_t)s->numObjects, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
            }
            else ok = false;
        }
        if (ok && (allNodes.size() / 4u) < RT_NODE_CHILD_MASK && allGates.size() < 0xFFFFFFFFull)
        {
            const float4* devNodes = nullptr; const float4* devGates = nullptr; const WideLevel* devLevels = nullptr;
            if ((r = uploadArray(c, allNodes.data(), allNodes.size(), &devNodes))) return r;
            if ((r = uploadArray(c, allGates.data(), allGates.size(), &devGates))) return r;
            if ((r = uploadArray(c, levels.data(), levels.size(), &devLevels))) return r;
            c->wide2.nodes = devNodes; c->wide2.gate = devGates; c->wide2.levels = devLevels; c->wide2.numObjects = s->numObjects;
            c->walkNodeBytes[RTGPU_WALK_WIDE2] = usedNodes * sizeof(float4); c->walkLeafBoxBytes[RTGPU_WALK_WIDE2] = allGates.size() * sizeof(float4);
            c->updatable.levels = levels; c->updatable.wide2 = c->wide2; c->updatable.topWideNodeCapacity = s->numObjects;
            c->updatable.meshNodeBytes = meshNodes * sizeof(float4); c->updatable.meshGateBytes = meshGates * sizeof(float4);
        }
    }
    if (singleMesh)
    {
        const RtMesh& mesh = s->meshes[s->objects[0].meshIndex];
        const QuantBuild q = buildQuantBvh(s->meshNodes + mesh.firstNode, mesh.numNodes, mesh.numTriangles, maxMeshDepth);
        if (q.ok)
        {
            const float4* devGate = nullptr;
            if ((r = uploadArray(c, q.gate.data(), q.gate.size(), &devGate))) return r;
            const WideBuild w = buildWideBvh(s->meshNodes + mesh.firstNode, mesh.numNodes, q);
            if (w.ok)
            {
                const float4* devWide = nullptr;
                if ((r = uploadArray(c, w.nodes.data(), w.nodes.size(), &devWide))) return r;
                c->wide.nodes = devWide; c->wide.gate = devGate; c->wide.numNodes = (uint32_t)(w.nodes.size() / 4u);
                c->walkNodeBytes[RTGPU_WALK_WIDE] = w.nodes.size() * sizeof(float4); c->walkLeafBoxBytes[RTGPU_WALK_WIDE] = q.gate.size() * sizeof(float4);
                memcpy(c->wide.base, q.base, sizeof(q.base)); memcpy(c->wide.step, q.step, sizeof(q.step)); memcpy(c->wide.bound, q.bound, sizeof(q.bound));
            }
        }
    }
    c->sceneDev = d;
    c->walkNodeBytes[RTGPU_WALK_BINARY] = ((uint64_t)s->numTopNodes + s->numMeshNodes) * sizeof(RtNode); c->walkTriangleBytes = (uint64_t)s->numTriangles * sizeof(RtTriangle);
    c->numLights = s->numLights;
    c->traversalStackNeed = topDepth + maxMeshDepth;
    c->updatable.maxMeshDepth = maxMeshDepth;
    c->updatable.objects.assign(s->objects, s->objects + s->numObjects); c->updatable.lights.assign(s->lights, s->lights + s->numLights);
    bool lean = !knobs::noLean();
    for (uint32_t i = 0; i < s->numObjects && lean; ++i) lean = s->objects[i].objectKind == RT_OBJECT_SHAPE && s->objects[i].shapeKind == RT_SHAPE_MESH;
    for (uint32_t i = 0; i < s->numMaterials && lean; ++i) lean = s->materials[i].bsdf == RT_BSDF_DIFFUSE;
    for (uint32_t i = 0; i < s->numLights && lean; ++i) lean = s->lights[i].type == RT_LIGHT_BACKGROUND || s->lights[i].type == RT_LIGHT_DIRECTIONAL;
    bool textured = false;
    for (uint32_t i = 0; i < s->numMaterials; ++i)
        textured = textured || (s->materials[i].baseColorTexture & s->materials[i].emissionTexture & s->materials[i].roughnessTexture & s->materials[i].metalnessTexture & s->materials[i].normalMapTexture) != RT_NO_TEXTURE;
    for (uint32_t i = 0; i < s->numLights; ++i) textured = textured || s->lights[i].texture != RT_NO_TEXTURE;
    c->leanScene = lean ? (textured ? 2 : 1) : (textured ? 0 : 3);
    {
        // class 4: a lean scene whose textures are all plain 8-bit BGR(A) / RGBA or half-float RGBA bitmaps (what Demo/MeshLoader.cpp makes of an OBJ's
        // diffuse and normal maps: 24-bit .bmp files) -- the shading kernel inlines their evaluation.  RTGPU_NO_SIMPLE_TEXTURES=1: class 2 instead.
        bool simple = c->leanScene == 2 && s->numTextures != 0u && !knobs::noSimpleTextures();
        for (uint32_t i = 0; i < s->numTextures && simple; ++i) simple = s->textures[i].kind == RT_TEXTURE_BITMAP && RT_FORMAT_IS_SIMPLE(s->textures[i].format);
        if (simple) c->leanScene = 4;
    }
    c->axisParallelSun = hasAxisParallelSun(s->lights, s->numLights);
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
    { int fr = flushPending(c); if (fr) return fr; }
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
    if (topDepth == 0xFFFFFFFFu) return fail(RTGPU_ERR_INVALID_ARGUMENT, "malformed top-level BVH");
    for (uint32_t i = 0; i < u->numTopNodes; ++i)
    {
        const uint32_t leaves = u->topNodes[i].leaves & 0x3FFFFFFFu;
        if (leaves > RT_MAX_PACKED_LEAVES) return fail(RTGPU_ERR_UNSUPPORTED, "BVH leaves with more than 3 items are not supported");
        if (leaves && (uint64_t)u->topNodes[i].childIndex + leaves > n) return fail(RTGPU_ERR_INVALID_ARGUMENT, "a top-level leaf holds objects out of range");
    }
    if (topDepth + up.maxMeshDepth > 64) return fail(RTGPU_ERR_UNSUPPORTED, "BVH deeper than the 64-entry traversal stack");

    // the 4-wide top level and the level table in the new order (two-level scenes)
    WideLevelBuild top;
    std::vector<WideLevel> levels;
    bool topFits = false;
    if (!up.levels.empty())
    {
        levels.resize((size_t)n + 1u);
        for (uint32_t i = 0; i < n; ++i) levels[i] = up.levels[u->previousIndex[i]];
        levels[n] = up.levels[n];
        top = buildWideLevel(u->topNodes, u->numTopNodes, n, topDepth);
        topFits = top.ok && top.nodes.size() / 4u <= up.topWideNodeCapacity && top.gate.size() == 2u * (size_t)n;
        if (topFits)
        {
            memcpy(levels[n].base, top.base, sizeof(top.base)); memcpy(levels[n].step, top.step, sizeof(top.step)); memcpy(levels[n].bound, top.bound, sizeof(top.bound));
        }
    }

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
