// rt_runtime_refit.inl -- rtgpu_update_mesh (include/rtgpu.h): a mesh whose vertices moved is refitted on the device, from 12 bytes per vertex.  The model of
// these kernels is refitMesh (rt_scene_prepare.h), operation for operation; tests hold the device's tables to it bit for bit.  Four steps on one stream:
// triangles (and shading records), leaf boxes and gates, interior boxes depth by depth from the deepest, then -- after the root box came back and the host
// made the grid an upload would make -- the 16-bit boxes of the 4-wide slots.  No kernel writes a child reference, a leaf count or a level base: a wrong box
// is a wrong picture, never a walk that does not end.  Every index a kernel follows was checked on the host: vertex indices at upload, the tree's shape and
// its leaves' triangle ranges by planMeshRefit, the slot table by construction; and that the new grid can hold the new boxes with the margin the walks rest on.  Also the two read-back entries the tests stand on.  Included by rt_runtime.hip.

#define RT_REFIT_BLOCK 256u
#define RT_REFIT_TOP_BLOCK 1024u   // depths of at most this many nodes share one single-block launch with a barrier between depths

struct RefitBoxDev { float lo[3], hi[3]; };
__device__ static inline float refitMinDev(float a, float b) { return a < b ? a : b; }   // Math.h's Min / Max: the second operand where they compare equal
__device__ static inline float refitMaxDev(float a, float b) { return a > b ? a : b; }
__device__ static inline void refitJoinDev(RefitBoxDev& a, const RefitBoxDev& b)
{
    for (int k = 0; k < 3; ++k) { a.lo[k] = refitMinDev(a.lo[k], b.lo[k]); a.hi[k] = refitMaxDev(a.hi[k], b.hi[k]); }
}
__device__ static inline RefitBoxDev refitNodeBox(const float4* nodes, uint32_t n)
{
    const float4 a = nodes[2u * n], b = nodes[2u * n + 1u];
    return RefitBoxDev{ { a.x, a.y, a.z }, { b.x, b.y, b.z } };
}
__device__ static inline void refitStoreBox(float4* nodes, uint32_t n, const RefitBoxDev& box)   // the 12 + 12 box bytes: childIndex and leaves are not written
{
    float* out = reinterpret_cast<float*>(nodes + 2u * n);
    out[0] = box.lo[0]; out[1] = box.lo[1]; out[2] = box.lo[2];
    out[4] = box.hi[0]; out[5] = box.hi[1]; out[6] = box.hi[2];
}

// one thread per triangle: the 36-byte record from three gathered positions; with `vertexShading` the 96 bytes of its shading record's three vertices
__global__ void __launch_bounds__(RT_REFIT_BLOCK) k_refit_triangles(const RtVertexIndices* __restrict__ indices, const float* __restrict__ positions,
                                                                    const RtVertexShading* __restrict__ vertexShading, RtTriangle* __restrict__ triangles,
                                                                    TriangleShading* __restrict__ shading, uint32_t numTriangles)
{
    const uint32_t t = blockIdx.x * RT_REFIT_BLOCK + threadIdx.x;
    if (t >= numTriangles) return;
    const uint4 idx = reinterpret_cast<const uint4*>(indices)[t];
    const float* a = positions + 3u * (size_t)idx.x; const float* b = positions + 3u * (size_t)idx.y; const float* c = positions + 3u * (size_t)idx.z;
    float* out = reinterpret_cast<float*>(triangles + t);
    for (int k = 0; k < 3; ++k) { const float v0 = a[k]; out[k] = v0; out[3 + k] = b[k] - v0; out[6 + k] = c[k] - v0; }
    if (!vertexShading) return;
    const float4* src = reinterpret_cast<const float4*>(vertexShading);   // 32 bytes per vertex
    float4* dst = reinterpret_cast<float4*>(shading + t);                 // v[0..2] are the first 96 bytes; the material and the padding behind them stay
    const uint32_t v[3] = { idx.x, idx.y, idx.z };
    for (int k = 0; k < 3; ++k) { dst[2 * k] = src[2u * (size_t)v[k]]; dst[2 * k + 1] = src[2u * (size_t)v[k] + 1u]; }
}

// one thread per node position: a leaf takes the box of its triangles, from the positions themselves, and writes it to its two gate records (gate: null
// where the scene has no 4-wide tables)
__global__ void __launch_bounds__(RT_REFIT_BLOCK) k_refit_leaves(float4* __restrict__ nodes, uint32_t numPositions, const RtVertexIndices* __restrict__ indices,
                                                                 const float* __restrict__ positions, float4* __restrict__ gate)
{
    const uint32_t n = blockIdx.x * RT_REFIT_BLOCK + threadIdx.x;
    if (n >= numPositions || n == 1u) return;
    const uint32_t first = __float_as_uint(nodes[2u * n].w), leaves = __float_as_uint(nodes[2u * n + 1u].w) & 0x3FFFFFFFu;
    if (leaves == 0u) return;
    RefitBoxDev box;
    for (uint32_t j = 0; j < leaves; ++j)
    {
        const uint4 idx = reinterpret_cast<const uint4*>(indices)[first + j];
        const float* a = positions + 3u * (size_t)idx.x; const float* b = positions + 3u * (size_t)idx.y; const float* c = positions + 3u * (size_t)idx.z;
        RefitBoxDev tri;
        for (int k = 0; k < 3; ++k) { tri.lo[k] = refitMinDev(a[k], refitMinDev(b[k], c[k])); tri.hi[k] = refitMaxDev(a[k], refitMaxDev(b[k], c[k])); }
        if (j == 0u) box = tri; else refitJoinDev(box, tri);
    }
    refitStoreBox(nodes, n, box);
    if (gate)
    {
        gate[2u * (size_t)first] = make_float4(box.lo[0], box.lo[1], box.lo[2], 0.0f);
        gate[2u * (size_t)first + 1u] = make_float4(box.hi[0], box.hi[1], box.hi[2], 0.0f);
    }
}

__device__ static inline void refitInterior(float4* nodes, uint32_t n)
{
    if (n == 1u || (__float_as_uint(nodes[2u * n + 1u].w) & 0x3FFFFFFFu) != 0u) return;
    const uint32_t child = __float_as_uint(nodes[2u * n].w);
    RefitBoxDev box = refitNodeBox(nodes, child);
    refitJoinDev(box, refitNodeBox(nodes, child + 1u));
    refitStoreBox(nodes, n, box);
}
// one depth: a thread per position; the children, one depth down, are finished (the launch before this one, or the leaves' kernel)
__global__ void __launch_bounds__(RT_REFIT_BLOCK) k_refit_depth(float4* nodes, uint32_t first, uint32_t count)
{
    const uint32_t i = blockIdx.x * RT_REFIT_BLOCK + threadIdx.x;
    if (i < count) refitInterior(nodes, first + i);
}
// depths `from` down to `to`, each of at most RT_REFIT_TOP_BLOCK positions, by ONE block: a barrier between a depth and the one above it
__global__ void __launch_bounds__(RT_REFIT_TOP_BLOCK) k_refit_depths(float4* nodes, const uint32_t* __restrict__ levelFirst, uint32_t from, uint32_t to)
{
    for (uint32_t d = from + 1u; d-- > to;)
    {
        const uint32_t first = levelFirst[d], count = levelFirst[d + 1u] - first;
        if (threadIdx.x < count) refitInterior(nodes, first + threadIdx.x);
        __threadfence_block();
        __syncthreads();
    }
}

// one thread per 4-wide child slot: its binary node's new box on the new grid, by the builder's rule in double; the 12 box bytes only
__global__ void __launch_bounds__(RT_REFIT_BLOCK) k_refit_slots(const float4* __restrict__ meshNodes, const uint32_t* __restrict__ slotNode, float4* __restrict__ wide,
                                                                uint32_t numSlots, WideGrid grid)
{
    const uint32_t i = blockIdx.x * RT_REFIT_BLOCK + threadIdx.x;
    if (i >= numSlots) return;
    const uint32_t n = slotNode[i];
    if (n == 0xFFFFFFFFu) return;
    const RefitBoxDev box = refitNodeBox(meshNodes, n);
    uint32_t v[6];
    wideQuantiseBox(grid.base, grid.step, box.lo, box.hi, v);
    uint32_t* out = reinterpret_cast<uint32_t*>(wide + i);
    out[0] = v[0] | (v[1] << 16); out[1] = v[2] | (v[3] << 16); out[2] = v[4] | (v[5] << 16);
}

template <typename T>
static int refitBuffer(RtgpuContext* c, T*& dev, size_t count)   // a per-mesh device array, made with the mesh's first update and freed with the scene
{
    if (dev || count == 0) return RTGPU_OK;
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, count * sizeof(T)));
    c->sceneAllocs.push_back(p);
    dev = static_cast<T*>(p);
    return RTGPU_OK;
}

RTGPU_API int rtgpu_update_mesh(RtgpuContext* c, const RtMeshUpdate* u)
{
    if (!c || !u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    RT_FAN_OUT(c, rtgpu_update_mesh(peer, u));   // every device traverses its own copy (a refusal is the same on each: the first peer returns it)
    if (u->abiVersion != RTGPU_ABI_VERSION) return fail(RTGPU_ERR_INVALID_ARGUMENT, "RtMeshUpdate::abiVersion mismatch");
    if (!c->sceneReady) return fail(RTGPU_ERR_NOT_READY, "rtgpu_upload_scene has not been called");
    HIP_TRY(hipSetDevice(c->device));
    { int fr = flushQueued(c); if (fr) return fr; }
    HIP_TRY(syncLanes(c));
    waitQueries(c);
    RtgpuContext::Updatable& up = c->updatable;
    if (u->flags != 0u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "RtMeshUpdate::flags must be 0");
    if (u->meshIndex >= up.meshTable.size()) return fail(RTGPU_ERR_INVALID_ARGUMENT, "mesh index out of range");
    const RtMesh& mesh = up.meshTable[u->meshIndex];
    RtgpuContext::Updatable::Mesh& state = up.meshes[u->meshIndex];
    if (u->numVertices != mesh.numVertices) return fail(RTGPU_ERR_INVALID_ARGUMENT, "a mesh update keeps the mesh's vertex count");
    if (u->numVertices && !u->positions) return fail(RTGPU_ERR_INVALID_ARGUMENT, "positions is NULL");
    for (size_t i = 0; i < (size_t)3 * u->numVertices; ++i)
        if (!std::isfinite(u->positions[i])) return fail(RTGPU_ERR_INVALID_ARGUMENT, "a position is not finite");
    if (mesh.numTriangles == 0u || mesh.numNodes == 0u) return RTGPU_OK;   // nothing to hit, nothing to refit
    if (!state.plan.ok) return fail(RTGPU_ERR_UNSUPPORTED, "the mesh's uploaded BVH is not an exact tree over all its triangles: it cannot be refitted");
    const bool twoLevel = !up.levels.empty();
    const bool haveWide = state.level.have && (twoLevel ? up.wide2.nodes != nullptr : c->wide.nodes != nullptr);
    if (haveWide)
    {
        // The 4-wide level must be able to hold the new boxes BEFORE anything is written.  The plan's leaves hold every triangle once, so the new root box is
        // the box of the positions the triangles refer to (a vertex no triangle uses does not count); an upload refuses a level whose grid cannot keep the half
        // step of margin (buildQuantBvh checks every record) and leaves the scene to the binary walk -- an update cannot change the walk, so it refuses.
        float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
        for (uint32_t t = 0; t < mesh.numTriangles; ++t)
        {
            const RtVertexIndices& idx = up.vertexIndices[mesh.firstTriangle + t];
            const uint32_t v[3] = { idx.i0, idx.i1, idx.i2 };
            for (const uint32_t k : v)
                for (int a = 0; a < 3; ++a) { const float x = u->positions[3u * (size_t)k + a]; lo[a] = fminf(lo[a], x); hi[a] = fmaxf(hi[a], x); }
        }
        WideGrid wanted;
        if (!wideGridOver(lo, hi, wanted)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the positions span more than a float holds");
        if (!wideGridHolds(wanted, lo, hi))
            return fail(RTGPU_ERR_UNSUPPORTED, "the 16-bit grid over the new box cannot hold it with its margin (a mesh far from its origin for its size, or flat off zero): upload the scene instead");
    }

    // device state of the mesh (first update) and the new positions
    int r;
    const uint32_t numPositions = (uint32_t)state.plan.order.size(), numDepths = (uint32_t)state.plan.levelFirst.size() - 1u;
    const bool firstUpdate = !state.indices;
    if ((r = refitBuffer(c, state.indices, mesh.numTriangles))) return r;
    if ((r = refitBuffer(c, state.positions, (size_t)3 * mesh.numVertices))) return r;
    if ((r = refitBuffer(c, state.levelFirst, state.plan.levelFirst.size()))) return r;
    if (u->shading && (r = refitBuffer(c, state.shading, mesh.numVertices))) return r;
    uint64_t bytes = 0;
    auto put = [&](void* dev, const void* host, size_t size) -> hipError_t { bytes += size; return rtMemcpy(dev, host, size, hipMemcpyHostToDevice); };
    if (firstUpdate)
    {
        HIP_TRY(put(state.indices, up.vertexIndices.data() + mesh.firstTriangle, (size_t)mesh.numTriangles * sizeof(RtVertexIndices)));
        HIP_TRY(put(state.levelFirst, state.plan.levelFirst.data(), state.plan.levelFirst.size() * sizeof(uint32_t)));
    }
    HIP_TRY(put(state.positions, u->positions, (size_t)3 * mesh.numVertices * sizeof(float)));
    if (u->shading) HIP_TRY(put(state.shading, u->shading, (size_t)mesh.numVertices * sizeof(RtVertexShading)));

    // the tables
    float4* const wideNodes = !haveWide ? nullptr : const_cast<float4*>(twoLevel ? up.wide2.nodes : c->wide.nodes) + 4u * (size_t)state.level.nodeBase;
    float4* const gate = !haveWide ? nullptr : const_cast<float4*>(twoLevel ? up.wide2.gate : c->wide.gate) + state.level.gateBase;
    const uint32_t* const slotNode = !haveWide ? nullptr : (twoLevel ? up.wide2SlotNode : up.wideSlotNode) + 4u * (size_t)state.level.nodeBase;
    float4* const nodes = reinterpret_cast<float4*>(const_cast<RtNode*>(c->sceneDev.meshNodes) + mesh.firstNode);
    RtTriangle* const triangles = const_cast<RtTriangle*>(c->sceneDev.triangles) + mesh.firstTriangle;
    TriangleShading* const shading = reinterpret_cast<TriangleShading*>(const_cast<RtVertexIndices*>(c->sceneDev.vertexIndices)) + mesh.firstTriangle;
    const hipStream_t stream = c->lanes[0].stream;
    auto blocks = [](uint32_t n) { return dim3((n + RT_REFIT_BLOCK - 1u) / RT_REFIT_BLOCK); };
    // rtgpu_set_deform_tracking: the records as the temporal history saw them, kept before the first kernel overwrites them -- once per mesh and history: a
    // second update before the next temporal call leaves the snapshot alone.  (Every check has passed: a refused update takes none.)
    const bool haveHistory = c->temporal.have && c->temporal.then.size() == up.objects.size();
    if (up.deformState.size() != up.meshTable.size()) up.deformState.assign(up.meshTable.size(), (uint8_t)0u);
    uint8_t& deformState = up.deformState[u->meshIndex];
    if (!haveHistory) deformState = 0u;
    else if (!c->temporal.trackDeform) deformState = 2u;
    else if (deformState == 0u)
    {
        if ((r = refitBuffer(c, up.deformSnapshot, c->sceneDev.numTriangles))) return r;
        if (c->denoise.done) HIP_TRY(hipEventSynchronize(c->denoise.done));   // (the temporal call that followed the last deformation may still read the array, on a stream of the caller's)
        HIP_TRY(hipMemcpyAsync(up.deformSnapshot + mesh.firstTriangle, triangles, (size_t)mesh.numTriangles * sizeof(RtTriangle), hipMemcpyDeviceToDevice, stream));
        deformState = 1u;
    }
    hipLaunchKernelGGL(k_refit_triangles, blocks(mesh.numTriangles), dim3(RT_REFIT_BLOCK), 0, stream, state.indices, state.positions, u->shading ? state.shading : nullptr,
                       triangles, shading, mesh.numTriangles);
    hipLaunchKernelGGL(k_refit_leaves, blocks(numPositions), dim3(RT_REFIT_BLOCK), 0, stream, nodes, numPositions, state.indices, state.positions, gate);
    // interior nodes: the deepest depth holds leaves only; runs of narrow depths share a single-block launch, a wider depth gets its own (at most one launch per depth)
    const std::vector<uint32_t>& first = state.plan.levelFirst;
    auto width = [&](uint32_t d) { return first[d + 1u] - first[d]; };
    for (uint32_t d = numDepths - 1u; d-- > 0u;)
    {
        if (width(d) > RT_REFIT_TOP_BLOCK) { hipLaunchKernelGGL(k_refit_depth, blocks(width(d)), dim3(RT_REFIT_BLOCK), 0, stream, nodes, first[d], width(d)); continue; }
        uint32_t to = d;
        while (to > 0u && width(to - 1u) <= RT_REFIT_TOP_BLOCK) --to;
        hipLaunchKernelGGL(k_refit_depths, dim3(1), dim3(RT_REFIT_TOP_BLOCK), 0, stream, nodes, state.levelFirst, d, to);
        d = to;
    }
    HIP_TRY(hipGetLastError());
    WideGrid grid;
    if (haveWide)
    {
        RtNode root;
        HIP_TRY(hipMemcpyAsync(&root, nodes, sizeof(root), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        bytes += sizeof(root);
        if (!wideGridOver(root.min, root.max, grid)) return fail(RTGPU_ERR_DEVICE, "the refitted root box has no grid");   // (the box the host asked about above: the device's folds return its floats)
        hipLaunchKernelGGL(k_refit_slots, blocks(4u * state.level.numNodes), dim3(RT_REFIT_BLOCK), 0, stream, reinterpret_cast<const float4*>(c->sceneDev.meshNodes), slotNode,
                           wideNodes, 4u * state.level.numNodes, grid);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(stream));
    if (haveWide && twoLevel)
    {
        // instances share the level: every object of the mesh takes the new grid, on the device and in the copy rtgpu_update_objects permutes
        for (size_t o = 0; o < up.objects.size(); ++o)
            if (up.objects[o].objectKind == RT_OBJECT_SHAPE && up.objects[o].shapeKind == RT_SHAPE_MESH && up.objects[o].meshIndex == u->meshIndex && up.levels[o].valid) copyGrid(up.levels[o], grid);
        HIP_TRY(put(const_cast<WideLevel*>(up.wide2.levels), up.levels.data(), up.levels.size() * sizeof(WideLevel)));
    }
    if (haveWide && !twoLevel) copyGrid(c->wide, grid);
    c->vcm.havePhotons = false;   // photons of the mesh as it was
    if (haveHistory)
    {
        // rtgpu_denoise_temporal's history stays.  Under a snapshot the objects of this mesh keep the id they had and are marked: the next call follows the
        // deformation.  Otherwise no tap of the history matches an object of this mesh any more: those pixels start
        for (size_t o = 0; o < up.objects.size(); ++o)
            if (up.objects[o].objectKind == RT_OBJECT_SHAPE && up.objects[o].shapeKind == RT_SHAPE_MESH && up.objects[o].meshIndex == u->meshIndex)
            {
                if (deformState == 1u) c->temporal.then[o].deformed = 1u;
                else { c->temporal.then[o].id = 0xFFFFFFFFu; c->temporal.then[o].deformed = 0u; }
            }
        c->temporal.movedSince = true;
    }
    else c->temporal.have = false;
    up.info.bytesUploaded = bytes; up.info._pad[0]++;   // RtUpdateInfo: mesh updates so far
    return RTGPU_OK;
}

RTGPU_API int rtgpu_read_mesh(RtgpuContext* c, uint32_t meshIndex, RtNode* nodes, RtTriangle* triangles)
{
    if (!c) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL context");
    if (!c->sceneReady) return fail(RTGPU_ERR_NOT_READY, "rtgpu_upload_scene has not been called");
    int r = rtgpu_synchronize(c); if (r) return r;
    const RtgpuContext::Updatable& up = c->updatable;
    if (meshIndex >= up.meshTable.size()) return fail(RTGPU_ERR_INVALID_ARGUMENT, "mesh index out of range");
    const RtMesh& mesh = up.meshTable[meshIndex];
    HIP_TRY(hipSetDevice(c->device));
    if (triangles) HIP_TRY(rtMemcpy(triangles, c->sceneDev.triangles + mesh.firstTriangle, (size_t)mesh.numTriangles * sizeof(RtTriangle), hipMemcpyDeviceToHost));
    if (!nodes || mesh.numNodes == 0u) return RTGPU_OK;
    // back from the device's breadth-first order: position k holds the caller's node order[k]; a node no path from the root reaches comes back zero
    const std::vector<uint32_t>& order = up.meshes[meshIndex].plan.order;
    std::vector<RtNode> dev(mesh.numNodes);
    HIP_TRY(rtMemcpy(dev.data(), c->sceneDev.meshNodes + mesh.firstNode, dev.size() * sizeof(RtNode), hipMemcpyDeviceToHost));
    memset(nodes, 0, dev.size() * sizeof(RtNode));
    for (size_t k = 0; k < order.size(); ++k)
    {
        if (order[k] >= mesh.numNodes) continue;
        RtNode n = dev[k];
        if (k != 1u && (n.leaves & 0x3FFFFFFFu) == 0u && n.childIndex < order.size()) n.childIndex = order[n.childIndex];
        nodes[order[k]] = n;
    }
    return RTGPU_OK;
}

RTGPU_API int rtgpu_read_wide_level(RtgpuContext* c, uint32_t objectIndex, RtWideLevelInfo* info, void* nodes, uint64_t nodeBytes, void* gates, uint64_t gateBytes)
{
    static_assert(sizeof(RtWideLevelInfo) == sizeof(WideLevel), "RtWideLevelInfo");
    if (!c || !info) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!c->sceneReady) return fail(RTGPU_ERR_NOT_READY, "rtgpu_upload_scene has not been called");
    int r = rtgpu_synchronize(c); if (r) return r;
    const RtgpuContext::Updatable& up = c->updatable;
    if (objectIndex >= up.objects.size()) return fail(RTGPU_ERR_INVALID_ARGUMENT, "object index out of range");
    const RtObject& object = up.objects[objectIndex];
    if (object.objectKind != RT_OBJECT_SHAPE || object.shapeKind != RT_SHAPE_MESH) return fail(RTGPU_ERR_NOT_READY, "the object has no 4-wide level");
    const RtgpuContext::Updatable::Mesh& state = up.meshes[object.meshIndex];
    const bool twoLevel = !up.levels.empty();
    if (!state.level.have || (twoLevel ? !up.levels[objectIndex].valid : !c->wide.nodes)) return fail(RTGPU_ERR_NOT_READY, "the object has no 4-wide level");
    HIP_TRY(hipSetDevice(c->device));
    WideLevel level;
    if (twoLevel) HIP_TRY(rtMemcpy(&level, up.wide2.levels + objectIndex, sizeof(level), hipMemcpyDeviceToHost));   // the record the kernels read
    else { memset(&level, 0, sizeof(level)); level.valid = 1u; memcpy(level.base, c->wide.base, sizeof(level.base)); memcpy(level.step, c->wide.step, sizeof(level.step)); memcpy(level.bound, c->wide.bound, sizeof(level.bound)); }
    const uint64_t numNodeRecords = 4u * (uint64_t)state.level.numNodes, numGateRecords = 2u * (uint64_t)up.meshTable[object.meshIndex].numTriangles;
    level.pad[0] = (uint32_t)numNodeRecords; level.pad[1] = (uint32_t)numGateRecords;
    memcpy(info, &level, sizeof(level));
    if ((nodes && nodeBytes < numNodeRecords * sizeof(float4)) || (gates && gateBytes < numGateRecords * sizeof(float4))) return fail(RTGPU_ERR_INVALID_ARGUMENT, "a buffer is smaller than the level");
    const float4* devNodes = (twoLevel ? up.wide2.nodes : c->wide.nodes) + 4u * (size_t)state.level.nodeBase;
    const float4* devGates = (twoLevel ? up.wide2.gate : c->wide.gate) + state.level.gateBase;
    if (nodes) HIP_TRY(rtMemcpy(nodes, devNodes, numNodeRecords * sizeof(float4), hipMemcpyDeviceToHost));
    if (gates) HIP_TRY(rtMemcpy(gates, devGates, numGateRecords * sizeof(float4), hipMemcpyDeviceToHost));
    return RTGPU_OK;
}
