// rt_runtime_refit.inl -- rtgpu_update_mesh and rtgpu_update_mesh_device (include/rtgpu.h): a mesh whose vertices moved is refitted on the device, from 12 bytes
// per vertex that come from the host or are on the device already (the two entries share refitTables; the second makes the first's host checks by k_refit_check).  The model of
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

// one thread per triangle: the 36-byte record from three gathered positions; with `vertexShading` the 96 bytes of its shading record's three vertices.  The
// kSplit variant (rtgpu_update_mesh_device) takes normals and tangents as tight float3 arrays instead, either of which may be null: it rewrites the first 24
// bytes of each of the three 32-byte vertex records, or the 12 of them that were given, and leaves texCoord alone
template <bool kSplit>
__global__ void __launch_bounds__(RT_REFIT_BLOCK) k_refit_triangles(const RtVertexIndices* __restrict__ indices, const float* __restrict__ positions,
                                                                    const RtVertexShading* __restrict__ vertexShading, const float* __restrict__ normals,
                                                                    const float* __restrict__ tangents, RtTriangle* __restrict__ triangles,
                                                                    TriangleShading* __restrict__ shading, uint32_t numTriangles)
{
    const uint32_t t = blockIdx.x * RT_REFIT_BLOCK + threadIdx.x;
    if (t >= numTriangles) return;
    const uint4 idx = reinterpret_cast<const uint4*>(indices)[t];
    const float* a = positions + 3u * (size_t)idx.x; const float* b = positions + 3u * (size_t)idx.y; const float* c = positions + 3u * (size_t)idx.z;
    float* out = reinterpret_cast<float*>(triangles + t);
    for (int k = 0; k < 3; ++k) { const float v0 = a[k]; out[k] = v0; out[3 + k] = b[k] - v0; out[6 + k] = c[k] - v0; }
    const uint32_t v[3] = { idx.x, idx.y, idx.z };
    if (kSplit)
    {
        float* dst = reinterpret_cast<float*>(shading + t);               // vertex k's record starts 8 floats after vertex k - 1's: normal, tangent, texCoord
        for (int k = 0; k < 3; ++k)
        {
            if (normals) for (int j = 0; j < 3; ++j) dst[8 * k + j] = normals[3u * (size_t)v[k] + j];
            if (tangents) for (int j = 0; j < 3; ++j) dst[8 * k + 3 + j] = tangents[3u * (size_t)v[k] + j];
        }
        return;
    }
    if (!vertexShading) return;
    const float4* src = reinterpret_cast<const float4*>(vertexShading);   // 32 bytes per vertex
    float4* dst = reinterpret_cast<float4*>(shading + t);                 // v[0..2] are the first 96 bytes; the material and the padding behind them stay
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

// ---- rtgpu_update_mesh_device's form of the two host checks: reads only, before any scene table is written --------------------------------------------
#define RT_REFIT_CHECK_WAVES (RT_REFIT_BLOCK / 64u)
__global__ void k_refit_check_init(RefitCheckRecord* out)   // one wave's worth of a launch: the identities, by plain vector stores
{
    if (threadIdx.x < 3u) { out->lo[threadIdx.x] = RT_REFIT_KEY_HIGHEST; out->hi[threadIdx.x] = RT_REFIT_KEY_LOWEST; }
    if (threadIdx.x == 3u) { out->nonFinite = 0u; out->pad = 0u; }
}
// Grid-stride, in one launch: whether any of the `numFloats` position floats is not finite (coalesced loads of the bits), and the box over the positions the
// `numTriangles` triangles refer to (three gathers each), as keys (rt_refit_keys.h).  A wave folds its 64 lanes with __shfl_xor, a block its waves through
// LDS, and thread 0 of every block sends the block's seven words to `out` with atomicMin / atomicMax / atomicAdd: minimum and maximum are exact whatever the
// order, so the record is a function of the positions alone.  `positions` holds numFloats floats and every index is below numFloats / 3 (the caller's checks).
__global__ void __launch_bounds__(RT_REFIT_BLOCK) k_refit_check(const float* __restrict__ positions, uint32_t numFloats, const RtVertexIndices* __restrict__ indices,
                                                                uint32_t numTriangles, RefitCheckRecord* out)
{
    __shared__ uint32_t folded[RT_REFIT_CHECK_WAVES][7];
    const uint32_t stride = gridDim.x * RT_REFIT_BLOCK, start = blockIdx.x * RT_REFIT_BLOCK + threadIdx.x;
    uint32_t bad = 0u;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(positions);
    for (uint32_t i = start; i < numFloats; i += stride) bad |= refitBitsFinite(words[i]) ? 0u : 1u;
    uint32_t lo[3] = { RT_REFIT_KEY_HIGHEST, RT_REFIT_KEY_HIGHEST, RT_REFIT_KEY_HIGHEST }, hi[3] = { RT_REFIT_KEY_LOWEST, RT_REFIT_KEY_LOWEST, RT_REFIT_KEY_LOWEST };
    for (uint32_t t = start; t < numTriangles; t += stride)
    {
        const uint4 idx = reinterpret_cast<const uint4*>(indices)[t];
        const uint32_t v[3] = { idx.x, idx.y, idx.z };
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) { const uint32_t key = refitKey(positions[3u * (size_t)v[k] + a]); lo[a] = min(lo[a], key); hi[a] = max(hi[a], key); }
    }
    for (int offset = 32; offset > 0; offset >>= 1)
    {
        for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], offset, 64)); hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], offset, 64)); }
        bad |= (uint32_t)__shfl_xor((int)bad, offset, 64);
    }
    const uint32_t wave = threadIdx.x / 64u;
    if ((threadIdx.x & 63u) == 0u)
    {
        for (int a = 0; a < 3; ++a) { folded[wave][a] = lo[a]; folded[wave][3 + a] = hi[a]; }
        folded[wave][6] = bad;
    }
    __syncthreads();
    if (threadIdx.x != 0u) return;
    for (uint32_t w = 1u; w < RT_REFIT_CHECK_WAVES; ++w)
    {
        for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], folded[w][a]); hi[a] = max(hi[a], folded[w][3 + a]); }
        bad |= folded[w][6];
    }
    if (numTriangles)
        for (int a = 0; a < 3; ++a) { atomicMin(&out->lo[a], lo[a]); atomicMax(&out->hi[a], hi[a]); }
    if (bad) atomicAdd(&out->nonFinite, 1u);
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

// Where an update's arrays come from: the host's (rtgpu_update_mesh), or the device's (rtgpu_update_mesh_device, which has put lanes[0].stream behind the
// stream that made them).  Normals and tangents from the device are tight float3 arrays, either of which may be null.
struct RefitSource
{
    const float* hostPositions; const RtVertexShading* hostShading;
    const float* devPositions; const float* devNormals; const float* devTangents;
};
static bool refitHaveWide(const RtgpuContext* c, const RtgpuContext::Updatable::Mesh& state)
{
    return state.level.have && (!c->updatable.levels.empty() ? c->updatable.wide2.nodes != nullptr : c->wide.nodes != nullptr);
}
// The box of the positions the mesh's triangles refer to must leave the mesh's 4-wide level a grid that holds it BEFORE anything is written.  The plan's
// leaves hold every triangle once, so that box is the new root box (a vertex no triangle uses does not count); an upload refuses a level whose grid cannot keep
// the half step of margin (buildQuantBvh checks every record) and leaves the scene to the binary walk -- an update cannot change the walk, so it refuses.
static int refitGridHolds(const float lo[3], const float hi[3])
{
    WideGrid wanted;
    if (!wideGridOver(lo, hi, wanted)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the positions span more than a float holds");
    if (!wideGridHolds(wanted, lo, hi))
        return fail(RTGPU_ERR_UNSUPPORTED, "the 16-bit grid over the new box cannot hold it with its margin (a mesh far from its origin for its size, or flat off zero): upload the scene instead");
    return RTGPU_OK;
}
// a mesh's vertex indices in leaf order, sent with its first update (the device entry's check reads them, so it sends them before its check)
static int refitIndices(RtgpuContext* c, const RtMesh& mesh, RtgpuContext::Updatable::Mesh& state, uint64_t& bytes)
{
    if (state.indices) return RTGPU_OK;
    int r = refitBuffer(c, state.indices, mesh.numTriangles); if (r) return r;
    const size_t size = (size_t)mesh.numTriangles * sizeof(RtVertexIndices);
    HIP_TRY(rtMemcpy(state.indices, c->updatable.vertexIndices.data() + mesh.firstTriangle, size, hipMemcpyHostToDevice));
    bytes += size;
    return RTGPU_OK;
}

// The body both entries share, from "every check has passed" on: the new positions go into state.positions and the tables are refitted from them.  `bytes`:
// what the entry has sent already.  `outBox` (or null): the refitted root node's min and max.
static int refitTables(RtgpuContext* c, uint32_t meshIndex, const RefitSource& src, uint64_t bytes, float* outBox)
{
    RtgpuContext::Updatable& up = c->updatable;
    const RtMesh& mesh = up.meshTable[meshIndex];
    RtgpuContext::Updatable::Mesh& state = up.meshes[meshIndex];
    const bool twoLevel = !up.levels.empty(), haveWide = refitHaveWide(c, state);
    const bool fromDevice = src.devPositions != nullptr;
    const hipStream_t stream = c->lanes[0].stream;
    // beam lists hold the leaf boxes as they were: invalid from here on, BEFORE anything is rewritten -- an error return further down leaves tables half
    // refitted, and stale lists would change primary hits silently
    beamInvalidate(c);

    // device state of the mesh (first update) and the new positions
    int r;
    const uint32_t numPositions = (uint32_t)state.plan.order.size(), numDepths = (uint32_t)state.plan.levelFirst.size() - 1u;
    if ((r = refitIndices(c, mesh, state, bytes))) return r;
    const bool firstLevels = !state.levelFirst;
    const size_t vertexFloats = (size_t)3 * mesh.numVertices;
    if ((r = refitBuffer(c, state.positions, vertexFloats))) return r;
    if ((r = refitBuffer(c, state.levelFirst, state.plan.levelFirst.size()))) return r;
    if (src.hostShading && (r = refitBuffer(c, state.shading, mesh.numVertices))) return r;
    if (src.devNormals && (r = refitBuffer(c, state.normals, vertexFloats))) return r;
    if (src.devTangents && (r = refitBuffer(c, state.tangents, vertexFloats))) return r;
    auto put = [&](void* dev, const void* host, size_t size) -> hipError_t { bytes += size; return rtMemcpy(dev, host, size, hipMemcpyHostToDevice); };
    if (firstLevels) HIP_TRY(put(state.levelFirst, state.plan.levelFirst.data(), state.plan.levelFirst.size() * sizeof(uint32_t)));
    if (!fromDevice) HIP_TRY(put(state.positions, src.hostPositions, vertexFloats * sizeof(float)));
    else
    {
        // the mesh's own buffers: the caller's arrays are free again when the call returns
        HIP_TRY(hipMemcpyAsync(state.positions, src.devPositions, vertexFloats * sizeof(float), hipMemcpyDeviceToDevice, stream));
        if (src.devNormals) HIP_TRY(hipMemcpyAsync(state.normals, src.devNormals, vertexFloats * sizeof(float), hipMemcpyDeviceToDevice, stream));
        if (src.devTangents) HIP_TRY(hipMemcpyAsync(state.tangents, src.devTangents, vertexFloats * sizeof(float), hipMemcpyDeviceToDevice, stream));
    }
    if (src.hostShading) HIP_TRY(put(state.shading, src.hostShading, (size_t)mesh.numVertices * sizeof(RtVertexShading)));

    // the tables
    float4* const wideNodes = !haveWide ? nullptr : const_cast<float4*>(twoLevel ? up.wide2.nodes : c->wide.nodes) + 4u * (size_t)state.level.nodeBase;
    float4* const gate = !haveWide ? nullptr : const_cast<float4*>(twoLevel ? up.wide2.gate : c->wide.gate) + state.level.gateBase;
    const uint32_t* const slotNode = !haveWide ? nullptr : (twoLevel ? up.wide2SlotNode : up.wideSlotNode) + 4u * (size_t)state.level.nodeBase;
    float4* const nodes = reinterpret_cast<float4*>(const_cast<RtNode*>(c->sceneDev.meshNodes) + mesh.firstNode);
    RtTriangle* const triangles = const_cast<RtTriangle*>(c->sceneDev.triangles) + mesh.firstTriangle;
    TriangleShading* const shading = reinterpret_cast<TriangleShading*>(const_cast<RtVertexIndices*>(c->sceneDev.vertexIndices)) + mesh.firstTriangle;
    auto blocks = [](uint32_t n) { return dim3((n + RT_REFIT_BLOCK - 1u) / RT_REFIT_BLOCK); };
    // rtgpu_set_deform_tracking: the records as the temporal history saw them, kept before the first kernel overwrites them -- once per mesh and history: a
    // second update before the next temporal call leaves the snapshot alone.  (Every check has passed: a refused update takes none.)
    const bool haveHistory = c->temporal.have && c->temporal.then.size() == up.objects.size();
    if (up.deformState.size() != up.meshTable.size()) up.deformState.assign(up.meshTable.size(), (uint8_t)0u);
    uint8_t& deformState = up.deformState[meshIndex];
    if (!haveHistory) deformState = 0u;
    else if (!c->temporal.trackDeform) deformState = 2u;
    else if (deformState == 0u)
    {
        if ((r = refitBuffer(c, up.deformSnapshot, c->sceneDev.numTriangles))) return r;
        if (c->denoise.done) HIP_TRY(hipEventSynchronize(c->denoise.done));   // (the temporal call that followed the last deformation may still read the array, on a stream of the caller's)
        HIP_TRY(hipMemcpyAsync(up.deformSnapshot + mesh.firstTriangle, triangles, (size_t)mesh.numTriangles * sizeof(RtTriangle), hipMemcpyDeviceToDevice, stream));
        deformState = 1u;
    }
    if (fromDevice)
        hipLaunchKernelGGL(k_refit_triangles<true>, blocks(mesh.numTriangles), dim3(RT_REFIT_BLOCK), 0, stream, state.indices, state.positions, nullptr,
                           src.devNormals ? state.normals : nullptr, src.devTangents ? state.tangents : nullptr, triangles, shading, mesh.numTriangles);
    else
        hipLaunchKernelGGL(k_refit_triangles<false>, blocks(mesh.numTriangles), dim3(RT_REFIT_BLOCK), 0, stream, state.indices, state.positions,
                           src.hostShading ? state.shading : nullptr, nullptr, nullptr, triangles, shading, mesh.numTriangles);
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
    RtNode root;
    if (haveWide)
    {
        HIP_TRY(hipMemcpyAsync(&root, nodes, sizeof(root), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        bytes += sizeof(root);
        if (!wideGridOver(root.min, root.max, grid)) return fail(RTGPU_ERR_DEVICE, "the refitted root box has no grid");   // (the box the host asked about above: the device's folds return its floats)
        hipLaunchKernelGGL(k_refit_slots, blocks(4u * state.level.numNodes), dim3(RT_REFIT_BLOCK), 0, stream, reinterpret_cast<const float4*>(c->sceneDev.meshNodes), slotNode,
                           wideNodes, 4u * state.level.numNodes, grid);
        HIP_TRY(hipGetLastError());
    }
    // (the root the host mirror's fold produces, bit for bit: the check's box may differ from it in the sign of a zero)
    if (outBox && !haveWide) HIP_TRY(hipMemcpyAsync(&root, nodes, sizeof(root), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (outBox) { memcpy(outBox, root.min, sizeof(root.min)); memcpy(outBox + 3, root.max, sizeof(root.max)); }
    if (haveWide && twoLevel)
    {
        // instances share the level: every object of the mesh takes the new grid, on the device and in the copy rtgpu_update_objects permutes
        for (size_t o = 0; o < up.objects.size(); ++o)
            if (up.objects[o].objectKind == RT_OBJECT_SHAPE && up.objects[o].shapeKind == RT_SHAPE_MESH && up.objects[o].meshIndex == meshIndex && up.levels[o].valid) copyGrid(up.levels[o], grid);
        HIP_TRY(put(const_cast<WideLevel*>(up.wide2.levels), up.levels.data(), up.levels.size() * sizeof(WideLevel)));
    }
    if (haveWide && !twoLevel) copyGrid(c->wide, grid);
    c->vcm.havePhotons = false;   // photons of the mesh as it was
    if (haveHistory)
    {
        // rtgpu_denoise_temporal's history stays.  Under a snapshot the objects of this mesh keep the id they had and are marked: the next call follows the
        // deformation.  Otherwise no tap of the history matches an object of this mesh any more: those pixels start
        for (size_t o = 0; o < up.objects.size(); ++o)
            if (up.objects[o].objectKind == RT_OBJECT_SHAPE && up.objects[o].shapeKind == RT_SHAPE_MESH && up.objects[o].meshIndex == meshIndex)
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
    if (refitHaveWide(c, state))
    {
        float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
        for (uint32_t t = 0; t < mesh.numTriangles; ++t)
        {
            const RtVertexIndices& idx = up.vertexIndices[mesh.firstTriangle + t];
            const uint32_t v[3] = { idx.i0, idx.i1, idx.i2 };
            for (const uint32_t k : v)
                for (int a = 0; a < 3; ++a) { const float x = u->positions[3u * (size_t)k + a]; lo[a] = fminf(lo[a], x); hi[a] = fmaxf(hi[a], x); }
        }
        const int held = refitGridHolds(lo, hi); if (held) return held;
    }
    const RefitSource src = { u->positions, u->shading, nullptr, nullptr, nullptr };
    return refitTables(c, u->meshIndex, src, 0u, nullptr);
}

// a caller's device array of `bytes` bytes: device memory of the context's device, inside one allocation to its last byte -- no kernel reads past one
static int refitDeviceArray(const RtgpuContext* c, const float* p, size_t bytes, const char* name)
{
    return callerDeviceArray(c, p, bytes, 3u, name, "12 bytes per vertex");
}

// k_refit_check over `numVertices` positions and the mesh's triangles (none: the finite check alone) into `out`, on `stream`
static int refitCheckLaunch(const RtgpuContext* c, const RtMesh& mesh, const RtgpuContext::Updatable::Mesh& state, const float* positions, uint32_t numVertices,
                            bool haveTriangles, RefitCheckRecord* out, hipStream_t stream)
{
    const uint32_t numFloats = 3u * numVertices, numTriangles = haveTriangles ? mesh.numTriangles : 0u;
    // (every block ends in seven atomics on the same 28 bytes: two blocks per CU, and the loops stride -- 0.044 ms on the Sponza-class mesh against 0.121 ms with
    // eight per CU)
    const uint32_t work = numFloats > numTriangles ? numFloats : numTriangles, most = 2u * c->numCUs;
    const uint32_t wanted = (work + RT_REFIT_BLOCK - 1u) / RT_REFIT_BLOCK;
    hipLaunchKernelGGL(k_refit_check_init, dim3(1), dim3(64), 0, stream, out);
    hipLaunchKernelGGL(k_refit_check, dim3(wanted < most ? wanted : most), dim3(RT_REFIT_BLOCK), 0, stream, positions, numFloats, state.indices, numTriangles, out);
    HIP_TRY(hipGetLastError());
    return RTGPU_OK;
}

RTGPU_API int rtgpu_refit_check_async(RtgpuContext* c, uint32_t meshIndex, uint32_t numVertices, const float* positions, void* outRecord, void* streamHandle)
{
    if (!c || !positions || !outRecord) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!c->peers.empty() || c->isPeer) return fail(RTGPU_ERR_UNSUPPORTED, "rtgpu_refit_check_async takes arrays of one device, not a multi-device context's");
    if (!c->sceneReady) return fail(RTGPU_ERR_NOT_READY, "rtgpu_upload_scene has not been called");
    HIP_TRY(hipSetDevice(c->device));
    RtgpuContext::Updatable& up = c->updatable;
    if (meshIndex >= up.meshTable.size()) return fail(RTGPU_ERR_INVALID_ARGUMENT, "mesh index out of range");
    const RtMesh& mesh = up.meshTable[meshIndex];
    RtgpuContext::Updatable::Mesh& state = up.meshes[meshIndex];
    if (numVertices != mesh.numVertices || numVertices == 0u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "the positions of every vertex of the mesh, and at least one");
    int r;
    if ((r = refitDeviceArray(c, positions, (size_t)12 * numVertices, "positions"))) return r;
    if ((r = refitDeviceArray(c, static_cast<const float*>(outRecord), sizeof(RefitCheckRecord), "outRecord"))) return r;
    const bool haveTriangles = mesh.numTriangles != 0u && mesh.numNodes != 0u;
    uint64_t bytes = 0;
    if (haveTriangles && (r = refitIndices(c, mesh, state, bytes))) return r;
    return refitCheckLaunch(c, mesh, state, positions, numVertices, haveTriangles, static_cast<RefitCheckRecord*>(outRecord), streamHandle ? (hipStream_t)streamHandle : c->lanes[0].stream);
}

RTGPU_API int rtgpu_update_mesh_device(RtgpuContext* c, const RtMeshUpdateDevice* u, void* streamHandle, float outBox[6])
{
    if (!c || !u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!c->peers.empty() || c->isPeer) return fail(RTGPU_ERR_UNSUPPORTED, "rtgpu_update_mesh_device takes arrays of one device: a multi-device context takes rtgpu_update_mesh");
    if (u->abiVersion != RTGPU_ABI_VERSION) return fail(RTGPU_ERR_INVALID_ARGUMENT, "RtMeshUpdateDevice::abiVersion mismatch");
    if (!c->sceneReady) return fail(RTGPU_ERR_NOT_READY, "rtgpu_upload_scene has not been called");
    HIP_TRY(hipSetDevice(c->device));
    { int fr = flushQueued(c); if (fr) return fr; }
    HIP_TRY(syncLanes(c));
    waitQueries(c);
    RtgpuContext::Updatable& up = c->updatable;
    if (u->flags != 0u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "RtMeshUpdateDevice::flags must be 0");
    if (u->meshIndex >= up.meshTable.size()) return fail(RTGPU_ERR_INVALID_ARGUMENT, "mesh index out of range");
    const RtMesh& mesh = up.meshTable[u->meshIndex];
    RtgpuContext::Updatable::Mesh& state = up.meshes[u->meshIndex];
    if (u->numVertices != mesh.numVertices) return fail(RTGPU_ERR_INVALID_ARGUMENT, "a mesh update keeps the mesh's vertex count");
    if (u->numVertices && !u->positions) return fail(RTGPU_ERR_INVALID_ARGUMENT, "positions is NULL");
    if (u->numVertices == 0u) return RTGPU_OK;   // (its triangles would have no vertex to name: an upload has refused them)
    // the arrays, before anything is launched on them
    int r;
    const size_t arrayBytes = (size_t)12 * u->numVertices;
    if ((r = refitDeviceArray(c, u->positions, arrayBytes, "positions"))) return r;
    if (u->normals && (r = refitDeviceArray(c, u->normals, arrayBytes, "normals"))) return r;
    if (u->tangents && (r = refitDeviceArray(c, u->tangents, arrayBytes, "tangents"))) return r;

    // the refit's stream goes behind the stream that made the arrays
    const hipStream_t stream = c->lanes[0].stream;
    if (streamHandle && (hipStream_t)streamHandle != stream)
    {
        if (!c->refitOrder) HIP_TRY(hipEventCreateWithFlags(&c->refitOrder, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(c->refitOrder, (hipStream_t)streamHandle));
        HIP_TRY(hipStreamWaitEvent(stream, c->refitOrder, 0));
    }
    // The two checks rtgpu_update_mesh makes on the host, made where the positions are (k_refit_check): it reads the caller's array and the mesh's vertex
    // indices, which go up first with the mesh's first update -- a private array that no walk reads.
    uint64_t bytes = 0;
    const bool haveTriangles = mesh.numTriangles != 0u && mesh.numNodes != 0u;
    if (haveTriangles && (r = refitIndices(c, mesh, state, bytes))) return r;
    if ((r = refitBuffer(c, up.refitCheck, 1))) return r;
    if ((r = refitCheckLaunch(c, mesh, state, u->positions, u->numVertices, haveTriangles, up.refitCheck, stream))) return r;
    RefitCheckRecord found;
    HIP_TRY(hipMemcpyAsync(&found, up.refitCheck, sizeof(found), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (found.nonFinite) return fail(RTGPU_ERR_INVALID_ARGUMENT, "a position is not finite");
    if (!haveTriangles) return RTGPU_OK;   // nothing to hit, nothing to refit
    if (!state.plan.ok) return fail(RTGPU_ERR_UNSUPPORTED, "the mesh's uploaded BVH is not an exact tree over all its triangles: it cannot be refitted");
    if (refitHaveWide(c, state))
    {
        // The host entry folds the same positions with fminf / fmaxf; a minimum over keys is the same float except that -0 sorts below +0 where a fold keeps
        // the zero it met.  So the sign of a zero bound is the only thing in which this box can differ from the host loop's, and neither function below
        // depends on it: wideGridOver subtracts the bounds (x - (+0) and x - (-0) are the same float for x != 0, and where both bounds are zeros the
        // difference, +0 or -0, loses to the positive floor in fmaxf), takes their absolute values, and derives base = lo - 4 step with step > 0, which is
        // -4 step for either zero; wideGridHolds compares in double, where the zeros are equal.  The same refusals, with the same messages.
        float lo[3], hi[3];
        for (int a = 0; a < 3; ++a) { lo[a] = refitUnkey(found.lo[a]); hi[a] = refitUnkey(found.hi[a]); }
        const int held = refitGridHolds(lo, hi); if (held) return held;
    }
    const RefitSource src = { nullptr, nullptr, u->positions, u->normals, u->tangents };
    return refitTables(c, u->meshIndex, src, bytes, outBox);
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
