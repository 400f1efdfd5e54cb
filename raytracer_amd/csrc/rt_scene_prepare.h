// rt_scene_prepare.h -- everything rtgpu_upload_scene and rtgpu_update_objects compute on the HOST before a byte is copied: the checks of the trees, the
// breadth-first mesh nodes, the de-indexed shading records, the 4-wide trees (rt_wide_format.h has their layout), the scene class.  Pure functions of the
// caller's tables: no HIP call, no context, no environment variable.  Included by rt_runtime.hip (rt_runtime_scene.inl calls it) and, without HIP, by
// tests/cpp/scene_prepare_check.cpp, which checks on the CPU the promise the kernels' exactness argument (rt_wide_grid.inl) rests on: every stored 16-bit box
// contains the exact box with a grid step to spare, and every leaf's exact box is the reference's.
#pragma once

#include "rt_wide_format.h"

#include <math.h>
#include <string.h>
#include <cmath>
#include <unordered_map>
#include <utility>
#include <vector>

// ---- checks ------------------------------------------------------------------------------------------------------------------------------------------
struct SceneStatus { int code; const char* message; };   // code == RTGPU_OK: nothing to report
static const uint32_t kMalformedTree = 0xFFFFFFFFu;

// depth of a BVH in stack entries: the traversal pushes at most one node per interior level.  kMalformedTree: a child pair beyond the array, or a cycle
static uint32_t bvhDepth(const RtNode* nodes, uint32_t numNodes)
{
    if (numNodes == 0) return 0;
    uint32_t maxDepth = 0;
    std::vector<std::pair<uint32_t, uint32_t>> stack;
    stack.push_back({ 0u, 0u });
    while (!stack.empty())
    {
        const auto [idx, depth] = stack.back(); stack.pop_back();
        if (idx >= numNodes) return kMalformedTree;
        const RtNode& n = nodes[idx];
        if ((n.leaves & 0x3FFFFFFFu) != 0) { if (depth > maxDepth) maxDepth = depth; continue; }
        if (depth > 4096) return kMalformedTree;
        stack.push_back({ n.childIndex, depth + 1 }); stack.push_back({ n.childIndex + 1, depth + 1 });
    }
    return maxDepth;
}

// The checks of a tree, each with its status and message once; upload and update run them (upload reports a deep tree before a fat leaf, update after: the
// order a caller can observe is the one each had).  checkLeaves goes over the ARRAY, reachable or not; with numPrimitives (an update's top level over
// its objects) the leaf ranges too -- an upload leaves those to the builders, which do not re-encode a tree with a leaf out of range.
static const uint64_t kAnyLeafRange = ~0ull;
static SceneStatus checkTreeDepth(uint32_t depth, const char* malformedMessage)
{
    if (depth == kMalformedTree) return { RTGPU_ERR_INVALID_ARGUMENT, malformedMessage };
    return { RTGPU_OK, "" };
}
static SceneStatus checkLeaves(const RtNode* nodes, uint32_t numNodes, uint64_t numPrimitives = kAnyLeafRange)
{
    for (uint32_t i = 0; i < numNodes; ++i)
    {
        const uint32_t leaves = nodes[i].leaves & 0x3FFFFFFFu;
        if (leaves > RT_MAX_PACKED_LEAVES) return { RTGPU_ERR_UNSUPPORTED, "BVH leaves with more than 3 items are not supported" };
        if (numPrimitives != kAnyLeafRange && leaves && (uint64_t)nodes[i].childIndex + leaves > numPrimitives) return { RTGPU_ERR_INVALID_ARGUMENT, "a top-level leaf holds objects out of range" };
    }
    return { RTGPU_OK, "" };
}
static SceneStatus checkStack(uint32_t topDepth, uint32_t maxMeshDepth)
{
    if (topDepth + maxMeshDepth > 64) return { RTGPU_ERR_UNSUPPORTED, "BVH deeper than the 64-entry traversal stack" };
    return { RTGPU_OK, "" };
}

// ---- mesh nodes, shading records ---------------------------------------------------------------------------------------------------------------------
// Mesh trees go to the device in BREADTH-FIRST order (root at 0, node 1 unused, child pairs from 2 on as the reference lays them out, levels one after
// the other): the same tree -- a node's childIndex is only a pointer -- with the top levels every ray walks through contiguous at the front, which
// k_trace stages in LDS.  Leaves keep their triangle ranges.
// oldIndex[new position] of one mesh tree (a tree of fewer than three nodes keeps its order)
static std::vector<uint32_t> breadthFirstOrder(const RtNode* src, uint32_t numNodes)
{
    std::vector<uint32_t> oldIndex;
    if (numNodes < 3u) { for (uint32_t k = 0; k < numNodes; ++k) oldIndex.push_back(k); return oldIndex; }
    oldIndex.reserve(numNodes);
    oldIndex.push_back(0u); oldIndex.push_back(1u);
    for (size_t k = 0; k < oldIndex.size() && oldIndex.size() + 2u <= numNodes; ++k)
    {
        if (k == 1u) continue;
        const RtNode& n = src[oldIndex[k]];
        if ((n.leaves & 0x3FFFFFFFu) != 0u) continue;
        oldIndex.push_back(n.childIndex); oldIndex.push_back(n.childIndex + 1u);
    }
    return oldIndex;
}

static std::vector<RtNode> reorderMeshNodes(const RtSceneDesc& s)
{
    std::vector<RtNode> ordered(s.meshNodes, s.meshNodes + s.numMeshNodes);
    for (uint32_t m = 0; m < s.numMeshes; ++m)
    {
        const RtMesh& mesh = s.meshes[m];
        if (mesh.numNodes < 3u) continue;
        const RtNode* src = s.meshNodes + mesh.firstNode;
        RtNode* dst = ordered.data() + mesh.firstNode;
        const std::vector<uint32_t> oldIndex = breadthFirstOrder(src, mesh.numNodes);
        // (children are appended in the order the interior nodes are met: the k-th interior node's pair follows the pairs of those before it)
        uint32_t next = 2u;
        for (size_t k = 0; k < oldIndex.size() && next + 2u <= mesh.numNodes; ++k)
        {
            if (k == 1u) continue;
            const RtNode& n = src[oldIndex[k]];
            if ((n.leaves & 0x3FFFFFFFu) != 0u) continue;
            dst[k] = n; dst[k].childIndex = next;
            next += 2u;
        }
        for (size_t k = 0; k < oldIndex.size(); ++k) if (k != 1u && (src[oldIndex[k]].leaves & 0x3FFFFFFFu) != 0u) dst[k] = src[oldIndex[k]];
    }
    return ordered;
}

// the de-indexed shading records (rt_wide_format.h, TriangleShading)
static std::vector<TriangleShading> deindexShading(const RtSceneDesc& s)
{
    std::vector<TriangleShading> records(s.numTriangles);
    if (!records.empty()) memset(records.data(), 0, records.size() * sizeof(TriangleShading));
    for (uint32_t m = 0; m < s.numMeshes; ++m)
    {
        const RtMesh& mesh = s.meshes[m];
        const RtVertexShading* vs = s.vertexShading + mesh.firstVertex;
        for (uint32_t t = 0; t < mesh.numTriangles; ++t)
        {
            const RtVertexIndices& idx = s.vertexIndices[mesh.firstTriangle + t];
            TriangleShading& out = records[mesh.firstTriangle + t];
            out.v[0] = vs[idx.i0]; out.v[1] = vs[idx.i1]; out.v[2] = vs[idx.i2];
            out.materialIndex = idx.materialIndex;
        }
    }
    return records;
}

// ---- the 16-bit grid ---------------------------------------------------------------------------------------------------------------------------------
// The grid over the box [lo, hi]: 65535 - 8 steps across the box (an axis without extent takes its step from the largest one), four steps of margin below
// and above.  false: a box that is empty or not finite, or a step that is not a positive finite float.
struct WideGrid { float base[3] = { 0, 0, 0 }, step[3] = { 0, 0, 0 }, bound[3] = { 0, 0, 0 }; };
static bool wideGridOver(const float lo[3], const float hi[3], WideGrid& g)
{
    for (int a = 0; a < 3; ++a) if (!(lo[a] <= hi[a]) || !std::isfinite(lo[a]) || !std::isfinite(hi[a])) return false;
    const float largest = fmaxf(fmaxf(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
    for (int a = 0; a < 3; ++a)
    {
        g.step[a] = fmaxf(hi[a] - lo[a], 1e-6f * fmaxf(largest, 1e-30f)) / (RT_QUANT_GRID - 8.0f);
        g.base[a] = lo[a] - 4.0f * g.step[a];
        g.bound[a] = fmaxf(fabsf(lo[a]), fabsf(hi[a])) + 8.0f * g.step[a];
        if (!(g.step[a] > 0.0f) || !std::isfinite(g.step[a])) return false;
    }
    return true;
}
// Whether records on the grid can hold boxes inside [lo, hi] with the half step the walks rest on: planes lie between base and base + 65535 step, so the box that
// reaches lo needs base <= lo - step / 2 and the one that reaches hi the last plane >= hi + step / 2.  It fails where the float lo - 4 steps rounds back onto lo:
// a box far from the origin for its size, or flat at a coordinate that is not zero.  Sufficient for every box inside [lo, hi] (wideQuantiseBox pushes a plane that
// is not clamped a full step out).  The builders find the same by checking every record; a refit asks BEFORE it writes.
static bool wideGridHolds(const WideGrid& g, const float lo[3], const float hi[3])
{
    for (int a = 0; a < 3; ++a)
        if ((double)g.base[a] > (double)lo[a] - 0.5 * (double)g.step[a] || (double)g.base[a] + 65535.0 * (double)g.step[a] < (double)hi[a] + 0.5 * (double)g.step[a]) return false;
    return true;
}
template <class T> static void copyGrid(T& to, const WideGrid& g) { memcpy(to.base, g.base, sizeof(g.base)); memcpy(to.step, g.step, sizeof(g.step)); memcpy(to.bound, g.bound, sizeof(g.bound)); }
static float4 wideRecord(const uint32_t v[6], uint32_t ref)   // v: min.xyz, max.xyz on the grid
{
    const uint32_t d0 = v[0] | (v[1] << 16), d1 = v[2] | (v[3] << 16), d2 = v[4] | (v[5] << 16);
    return make_float4(__builtin_bit_cast(float, d0), __builtin_bit_cast(float, d1), __builtin_bit_cast(float, d2), __builtin_bit_cast(float, ref));
}

// ---- the reference's binary BVH (BVH::Node, 32 bytes, children adjacent) re-encoded ----------------------------------------------------------------------
struct QuantBuild
{
    std::vector<float4> pairs, gate;   // pairs: one 16-byte record per BINARY node, host-side only -- buildWideBvh copies them into the 4-wide nodes; gate: uploaded
    uint32_t root = 0, stackNeed = 0;
    WideGrid grid;
    bool ok = false;
};

static QuantBuild buildQuantBvh(const RtNode* nodes, uint32_t numNodes, uint32_t numTriangles, uint32_t depth)
{
    QuantBuild q;
    if (numNodes < 3u || (nodes[0].leaves & 0x3FFFFFFFu) != 0u) return q;   // a root that is a leaf: nothing to walk
    // bounds from every node actually stored (node 1 is never written by the reference's builder)
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    std::vector<uint8_t> reachable(numNodes, 0);
    {
        std::vector<uint32_t> todo; todo.push_back(0u); reachable[0] = 1;
        while (!todo.empty())
        {
            const uint32_t n = todo.back(); todo.pop_back();
            for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], nodes[n].min[a]); hi[a] = fmaxf(hi[a], nodes[n].max[a]); }
            if ((nodes[n].leaves & 0x3FFFFFFFu) != 0u) continue;
            const uint32_t c = nodes[n].childIndex;
            if ((c & 1u) != 0u || (uint64_t)c + 1u >= numNodes || reachable[c] || reachable[c + 1u]) return q;   // pairs are even-aligned in the reference's layout
            reachable[c] = reachable[c + 1u] = 1; todo.push_back(c); todo.push_back(c + 1u);
        }
    }
    if (!wideGridOver(lo, hi, q.grid)) return q;
    const WideGrid& g = q.grid;
    // plane(qv) as the device could see it at worst: the kernel folds base and step into the ray's constants, whose rounding is
    // covered by the one spare step; here the stored coordinate is pushed out until the plain float plane is a full step outside
    auto plane = [&](int a, uint32_t v) { return (double)g.base[a] + (double)v * (double)g.step[a]; };
    q.pairs.assign(numNodes, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    q.gate.assign((size_t)2 * numTriangles, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (uint32_t n = 2u; n < numNodes; ++n)
    {
        if (!reachable[n]) continue;
        const RtNode& node = nodes[n];
        const uint32_t numLeaves = node.leaves & 0x3FFFFFFFu;
        if (numLeaves > 2u || node.childIndex > RT_NODE_CHILD_MASK) return q;   // the reference builds leaves of at most two triangles (BVHBuilder.h:16)
        uint32_t v[6];
        for (int a = 0; a < 3; ++a) if (!(node.min[a] <= node.max[a])) return q;   // a NaN or an inverted box: fminf / fmaxf above passed over it
        wideQuantiseBox(g.base, g.step, node.min, node.max, v);   // (rt_wide_format.h: the rule the device's refit shares)
        for (int a = 0; a < 3; ++a)
        {
            if (plane(a, v[a]) > (double)node.min[a] - 0.5 * (double)g.step[a] || plane(a, v[3 + a]) < (double)node.max[a] + 0.5 * (double)g.step[a]) return q;   // the grid has room by construction
        }
        q.pairs[n] = wideRecord(v, node.childIndex | (numLeaves << RT_NODE_LEAVES_SHIFT));
        if (numLeaves != 0u)
        {
            if ((uint64_t)node.childIndex + numLeaves > numTriangles) return q;
            q.gate[2u * (size_t)node.childIndex] = make_float4(node.min[0], node.min[1], node.min[2], 0.0f);
            q.gate[2u * (size_t)node.childIndex + 1u] = make_float4(node.max[0], node.max[1], node.max[2], 0.0f);
        }
    }
    q.root = nodes[0].childIndex;   // interior: its packed reference is its child index
    q.stackNeed = depth;
    q.ok = true;
    return q;
}

// ---- collapse of the reference's binary tree.  A wide node starts as the two children of a binary node; while it has a free
// slot, its interior child with the largest surface area is replaced by that child's own two children.  Node indices are breadth first.
struct WideBuild
{
    std::vector<float4> nodes;
    std::vector<uint32_t> slotNode;   // per record of `nodes`: the binary node it was copied from (the caller's index; 0xFFFFFFFF: an empty slot) -- what a refit re-quantises
    bool ok = false;
};

static WideBuild buildWideBvh(const RtNode* nodes, uint32_t numNodes, const QuantBuild& q)
{
    WideBuild w;
    if (!q.ok) return w;
    auto isLeaf = [&](uint32_t n) { return (nodes[n].leaves & 0x3FFFFFFFu) != 0u; };
    auto area = [&](uint32_t n)
    {
        const double ex = (double)nodes[n].max[0] - nodes[n].min[0], ey = (double)nodes[n].max[1] - nodes[n].min[1], ez = (double)nodes[n].max[2] - nodes[n].min[2];
        return ex * ey + ey * ez + ez * ex;
    };
    std::vector<uint32_t> wideOf(numNodes, 0xFFFFFFFFu);   // binary interior node -> wide node
    std::vector<uint32_t> order;                            // wide node -> binary node
    order.push_back(0u); wideOf[0] = 0u;
    std::vector<uint32_t> children;                         // 4 binary node indices per wide node (0xFFFFFFFF: empty)
    for (size_t i = 0; i < order.size(); ++i)
    {
        const uint32_t n = order[i];
        uint32_t list[4]; uint32_t num = 2;
        list[0] = nodes[n].childIndex; list[1] = nodes[n].childIndex + 1u;
        while (num < 4u)
        {
            int pick = -1; double bestArea = -1.0;
            for (uint32_t k = 0; k < num; ++k) if (!isLeaf(list[k]) && area(list[k]) > bestArea) { bestArea = area(list[k]); pick = (int)k; }
            if (pick < 0) break;
            const uint32_t c = nodes[list[pick]].childIndex;
            list[pick] = c; list[num++] = c + 1u;
        }
        for (uint32_t k = 0; k < 4u; ++k)
        {
            const uint32_t child = k < num ? list[k] : 0xFFFFFFFFu;
            children.push_back(child);
            if (child != 0xFFFFFFFFu && !isLeaf(child))
            {
                if (order.size() >= RT_NODE_CHILD_MASK) return w;
                wideOf[child] = (uint32_t)order.size(); order.push_back(child);
            }
        }
    }
    w.nodes.resize(order.size() * 4u);
    for (size_t i = 0; i < order.size(); ++i)
        for (uint32_t k = 0; k < 4u; ++k)
        {
            const uint32_t child = children[i * 4u + k];
            float4 rec = make_float4(0.0f, 0.0f, 0.0f, __builtin_bit_cast(float, (uint32_t)RT_WIDE_EMPTY));   // a point at the grid's corner, outside the mesh's bounds
            if (child != 0xFFFFFFFFu)
            {
                rec = q.pairs[child];   // the child's box on the grid; its packed reference is replaced for interior children
                if (!isLeaf(child)) rec.w = __builtin_bit_cast(float, wideOf[child]);
            }
            w.nodes[i * 4u + k] = rec;
        }
    w.slotNode = std::move(children);
    w.ok = true;
    return w;
}

// ---- one level of a two-level scene (the top-level tree over the objects, or a mesh's tree over its triangles) ----------------------------------------
struct WideLevelBuild
{
    std::vector<float4> nodes, gate;   // gate: 2 float4 per primitive index
    std::vector<uint32_t> slotNode;    // WideBuild::slotNode; a root that is a leaf: 0xFFFFFFFF throughout (its one record does not depend on the box)
    WideGrid grid;
    bool ok = false;
};

// A tree whose root is a leaf (one or two primitives: a quad, two objects) gets a single wide node with that leaf as its only child.
static WideLevelBuild buildWideLevel(const RtNode* nodes, uint32_t numNodes, uint32_t numPrimitives, uint32_t depth)
{
    WideLevelBuild out;
    if (numNodes == 0u || numPrimitives == 0u) return out;
    const uint32_t rootLeaves = nodes[0].leaves & 0x3FFFFFFFu;
    if (rootLeaves == 0u)
    {
        QuantBuild q = buildQuantBvh(nodes, numNodes, numPrimitives, depth);
        if (!q.ok) return out;
        WideBuild w = buildWideBvh(nodes, numNodes, q);
        if (!w.ok) return out;
        out.nodes = std::move(w.nodes); out.gate = std::move(q.gate); out.grid = q.grid; out.slotNode = std::move(w.slotNode);
        out.ok = true;
        return out;
    }
    if (rootLeaves > 2u || (uint64_t)nodes[0].childIndex + rootLeaves > numPrimitives) return out;
    // the grid over the root's box; the leaf's stored box a full step outside the exact one
    const RtNode& root = nodes[0];
    if (!wideGridOver(root.min, root.max, out.grid)) return out;
    const WideGrid& g = out.grid;
    const uint32_t v[6] = { 1u, 1u, 1u, 65534u, 65534u, 65534u };   // planes at base + step and base + 65534 step: more than a step outside [min, max] on both sides
    for (int a = 0; a < 3; ++a)
        if ((double)g.base[a] + (double)g.step[a] > (double)root.min[a] - (double)g.step[a] || (double)g.base[a] + 65534.0 * (double)g.step[a] < (double)root.max[a] + (double)g.step[a]) return out;
    out.nodes.assign(4u, make_float4(0.0f, 0.0f, 0.0f, __builtin_bit_cast(float, (uint32_t)RT_WIDE_EMPTY)));
    out.nodes[0] = wideRecord(v, root.childIndex | (rootLeaves << RT_NODE_LEAVES_SHIFT));
    out.slotNode.assign(4u, 0xFFFFFFFFu);
    out.gate.assign((size_t)2 * numPrimitives, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    out.gate[2u * (size_t)root.childIndex] = make_float4(root.min[0], root.min[1], root.min[2], 0.0f);
    out.gate[2u * (size_t)root.childIndex + 1u] = make_float4(root.max[0], root.max[1], root.max[2], 0.0f);
    out.ok = true;
    return out;
}

// The top level as upload and update need it: built, and inside the slab the upload leaves for it behind the mesh levels -- the largest one numObjects leaves
// can have (fewer 4-wide nodes than the binary tree has interior ones; two gate records per object whatever the tree)
static WideLevelBuild buildTopLevel(const RtNode* topNodes, uint32_t numTopNodes, uint32_t numObjects, uint32_t topDepth, uint32_t slabNodes)
{
    WideLevelBuild top = buildWideLevel(topNodes, numTopNodes, numObjects, topDepth);
    top.ok = top.ok && top.nodes.size() / 4u <= slabNodes && top.gate.size() == 2u * (size_t)numObjects;
    return top;
}

// ---- the 4-wide trees of a two-level scene -----------------------------------------------------------------------------------------------------------
// One node / gate array for all levels; levels[o] for mesh object o (instances of a mesh share a level, an empty mesh gets none), levels[numObjects] for
// the top-level tree, which goes BEHIND the mesh levels into its slab: rtgpu_update_objects rebuilds it there and no mesh base moves.  !ok: a level that
// cannot be built (a malformed tree) leaves the scene to the binary walk.
struct TwoLevelBuild
{
    std::vector<float4> nodes, gates;    // nodes: the mesh levels, the top level, zeros up to the end of the slab
    std::vector<WideLevel> levels;
    std::vector<uint32_t> slotNode;      // per record of the MESH levels: WideLevelBuild::slotNode (mesh-relative, the caller's order)
    struct MeshLevel { uint32_t meshIndex, nodeBase, numNodes, gateBase; };
    std::vector<MeshLevel> meshLevels;   // the level each mesh got: first 4-wide node, their count, first gate record
    size_t meshNodes = 0, meshGates = 0; // float4s of the mesh levels: where the top level starts
    size_t usedNodes = 0;                // float4s up to the end of the top level as built
    uint32_t topNodeCapacity = 0;        // 4-wide nodes the slab holds
    bool ok = false;
};

static TwoLevelBuild buildTwoLevel(const RtSceneDesc& s, uint32_t topDepth)
{
    TwoLevelBuild out;
    out.levels.resize((size_t)s.numObjects + 1u);
    memset(out.levels.data(), 0, out.levels.size() * sizeof(WideLevel));
    auto append = [&](const WideLevelBuild& b, WideLevel& level, uint32_t triBase)
    {
        level.nodeBase = (uint32_t)(out.nodes.size() / 4u); level.gateBase = (uint32_t)out.gates.size(); level.triBase = triBase; level.valid = 1u;
        copyGrid(level, b.grid);
        out.nodes.insert(out.nodes.end(), b.nodes.begin(), b.nodes.end()); out.gates.insert(out.gates.end(), b.gate.begin(), b.gate.end());
    };
    std::unordered_map<uint32_t, uint32_t> builtMesh;   // mesh index -> the first object whose level holds its tree (instances share it)
    for (uint32_t o = 0; o < s.numObjects; ++o)
    {
        const RtObject& obj = s.objects[o];
        if (obj.objectKind != RT_OBJECT_SHAPE || obj.shapeKind != RT_SHAPE_MESH) continue;
        const RtMesh& mesh = s.meshes[obj.meshIndex];
        if (mesh.numNodes == 0u) continue;   // nothing to hit (Traverse_Object returns at once)
        const auto found = builtMesh.find(obj.meshIndex);
        if (found != builtMesh.end()) { out.levels[o] = out.levels[found->second]; continue; }
        const WideLevelBuild b = buildWideLevel(s.meshNodes + mesh.firstNode, mesh.numNodes, mesh.numTriangles, bvhDepth(s.meshNodes + mesh.firstNode, mesh.numNodes));
        if (!b.ok) return out;
        append(b, out.levels[o], mesh.firstTriangle);
        out.slotNode.insert(out.slotNode.end(), b.slotNode.begin(), b.slotNode.end());
        out.meshLevels.push_back({ obj.meshIndex, out.levels[o].nodeBase, (uint32_t)(b.nodes.size() / 4u), out.levels[o].gateBase });
        builtMesh[obj.meshIndex] = o;
    }
    out.meshNodes = out.nodes.size(); out.meshGates = out.gates.size();
    out.topNodeCapacity = s.numObjects;   // (tests/cpp/scene_prepare_check.cpp: a top level over n objects has at most n nodes)
    const WideLevelBuild top = buildTopLevel(s.topNodes, s.numTopNodes, s.numObjects, topDepth, out.topNodeCapacity);
    if (!top.ok) return out;
    append(top, out.levels[s.numObjects], 0u);
    out.usedNodes = out.nodes.size();
    out.nodes.resize(out.meshNodes + 4u * (size_t)out.topNodeCapacity, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    out.ok = (out.nodes.size() / 4u) < RT_NODE_CHILD_MASK && out.gates.size() < 0xFFFFFFFFull;
    return out;
}

// An update: the level table in the new order of the objects (current object i was previousIndex[i]) and the new top level for the slab.  !top.ok: it
// cannot be built or does not fit -- the table keeps the old top level's grid and the scene goes to the binary walk until an update brings one that can.
struct TopLevelRebuild
{
    std::vector<WideLevel> levels;
    WideLevelBuild top;
};

static TopLevelRebuild rebuildTopLevel(const std::vector<WideLevel>& levels, const uint32_t* previousIndex, const RtNode* topNodes, uint32_t numTopNodes, uint32_t numObjects,
                                       uint32_t topDepth, uint32_t slabNodes)
{
    TopLevelRebuild out;
    out.levels.resize((size_t)numObjects + 1u);
    for (uint32_t i = 0; i < numObjects; ++i) out.levels[i] = levels[previousIndex[i]];
    out.levels[numObjects] = levels[numObjects];
    out.top = buildTopLevel(topNodes, numTopNodes, numObjects, topDepth, slabNodes);
    if (out.top.ok) copyGrid(out.levels[numObjects], out.top.grid);
    return out;
}

// ---- refitting a mesh whose vertices moved (rtgpu_update_mesh) ------------------------------------------------------------------------------------------
// The reference's Box operations (Math.h): Min(a, b) = a < b ? a : b per lane, Box(a, b, c) = Min(a, Min(b, c)), Box(b0, b1) = Min(b0.min, b1.min); Max alike.
// The fold order is part of the contract: it decides the sign of a zero.
struct RefitBox { float min[3], max[3]; };
static inline float refitMin(float a, float b) { return a < b ? a : b; }
static inline float refitMax(float a, float b) { return a > b ? a : b; }
static inline RefitBox refitTriangleBox(const float* a, const float* b, const float* c)
{
    RefitBox r;
    for (int k = 0; k < 3; ++k) { r.min[k] = refitMin(a[k], refitMin(b[k], c[k])); r.max[k] = refitMax(a[k], refitMax(b[k], c[k])); }
    return r;
}
static inline RefitBox refitJoin(const RefitBox& a, const RefitBox& b)
{
    RefitBox r;
    for (int k = 0; k < 3; ++k) { r.min[k] = refitMin(a.min[k], b.min[k]); r.max[k] = refitMax(a.max[k], b.max[k]); }
    return r;
}

// What a refit of one mesh needs beside its tables, made from the BREADTH-FIRST nodes at upload.  ok: the stored nodes are an exact tree laid out depth after
// depth (every child pair behind its parent and claimed once, every leaf's triangles inside the mesh) -- what the refit kernels rely on for their bounds -- and
// its leaves hold every triangle of the mesh once, so the new root box is the box of the positions the triangles refer to: the host knows it before the device does.
struct MeshRefitPlan
{
    std::vector<uint32_t> order;        // order[breadth-first position] = the caller's node index (reorderMeshNodes' permutation)
    std::vector<uint32_t> levelFirst;   // first breadth-first position of every depth, then the number of positions: depth d is [levelFirst[d], levelFirst[d + 1]) (node 1 lies in depth 0's range and is skipped)
    bool ok = false;
};
static MeshRefitPlan planMeshRefit(const RtNode* callerNodes, const RtNode* ordered, uint32_t numNodes, uint32_t numTriangles)
{
    MeshRefitPlan p;
    if (numNodes == 0u) return p;
    p.order = breadthFirstOrder(callerNodes, numNodes);
    if (numNodes < 3u) p.order.resize(1u);   // only a root that is a leaf can be walked
    const uint32_t count = (uint32_t)p.order.size();
    std::vector<uint32_t> depth(count, 0xFFFFFFFFu);
    depth[0] = 0u;
    uint32_t next = 2u, last = 0u;
    std::vector<uint8_t> held(numTriangles, 0u);
    p.levelFirst.push_back(0u);
    for (uint32_t k = 0; k < count; ++k)
    {
        if (k == 1u) continue;
        if (depth[k] == 0xFFFFFFFFu || depth[k] < last || depth[k] > 64u) return p;
        if (depth[k] > last) { if (depth[k] != last + 1u) return p; p.levelFirst.push_back(k); last = depth[k]; }
        const RtNode& n = ordered[k];
        const uint32_t leaves = n.leaves & 0x3FFFFFFFu;
        if (leaves != 0u)
        {
            if (leaves > RT_MAX_PACKED_LEAVES || (uint64_t)n.childIndex + leaves > numTriangles) return p;
            for (uint32_t j = 0; j < leaves; ++j) { if (held[n.childIndex + j]) return p; held[n.childIndex + j] = 1u; }
            continue;
        }
        if (n.childIndex != next || (uint64_t)next + 2u > count) return p;
        depth[next] = depth[next + 1u] = depth[k] + 1u;
        next += 2u;
    }
    if (next != (count < 2u ? 2u : count)) return p;
    for (const uint8_t h : held) if (!h) return p;
    p.levelFirst.push_back(count);
    p.ok = true;
    return p;
}

// The refit, pure: new nodes, triangles, gates, grid and 4-wide records of one mesh from its new positions.  `nodes` in any order with mesh-relative child
// indices (the caller's or the breadth-first one); boxes are folded child0 then child1, a leaf's triangles first to last.  childIndex, leaves and node 1 are
// kept.  slotNode[i] = the node record i of `wide` takes its box from (0xFFFFFFFF: the record is kept); its .w is kept.  gates: 2 per triangle, zero where no
// leaf starts.  ok: every index was in range; gridOk: the new root box has a grid and every box fits it with the builder's margin (slotNode empty: not asked).
struct MeshRefit
{
    std::vector<RtNode> nodes;
    std::vector<RtTriangle> triangles;
    std::vector<float4> gates, wide;
    WideGrid grid;
    bool ok = false, gridOk = false;
};
static MeshRefit refitMesh(const std::vector<RtNode>& nodes, const std::vector<RtVertexIndices>& indices, const float* positions, uint32_t numVertices,
                           const std::vector<uint32_t>& slotNode, const std::vector<float4>& wide)
{
    MeshRefit out;
    out.nodes = nodes; out.wide = wide;
    const uint32_t numTriangles = (uint32_t)indices.size();
    out.triangles.resize(numTriangles);
    std::vector<RefitBox> triBox(numTriangles);
    for (uint32_t t = 0; t < numTriangles; ++t)
    {
        const RtVertexIndices& idx = indices[t];
        if (idx.i0 >= numVertices || idx.i1 >= numVertices || idx.i2 >= numVertices) return out;
        const float* a = positions + 3u * (size_t)idx.i0; const float* b = positions + 3u * (size_t)idx.i1; const float* c = positions + 3u * (size_t)idx.i2;
        RtTriangle& tri = out.triangles[t];
        for (int k = 0; k < 3; ++k) { tri.v0[k] = a[k]; tri.edge1[k] = b[k] - a[k]; tri.edge2[k] = c[k] - a[k]; }
        triBox[t] = refitTriangleBox(a, b, c);
    }
    out.gates.assign((size_t)2 * numTriangles, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    if (nodes.empty() || numTriangles == 0u) { out.ok = true; return out; }
    // post order from the root: a node is folded once both children are
    std::vector<std::pair<uint32_t, bool>> stack;
    stack.push_back({ 0u, false });
    size_t visits = 0;
    while (!stack.empty())
    {
        const auto [n, childrenDone] = stack.back(); stack.pop_back();
        if (n >= out.nodes.size() || ++visits > 2u * out.nodes.size()) return out;
        RtNode& node = out.nodes[n];
        const uint32_t leaves = node.leaves & 0x3FFFFFFFu;
        RefitBox box;
        if (leaves != 0u)
        {
            if ((uint64_t)node.childIndex + leaves > numTriangles) return out;
            box = triBox[node.childIndex];
            for (uint32_t j = 1; j < leaves; ++j) box = refitJoin(box, triBox[node.childIndex + j]);
            out.gates[2u * (size_t)node.childIndex] = make_float4(box.min[0], box.min[1], box.min[2], 0.0f);
            out.gates[2u * (size_t)node.childIndex + 1u] = make_float4(box.max[0], box.max[1], box.max[2], 0.0f);
        }
        else if (!childrenDone)
        {
            stack.push_back({ n, true }); stack.push_back({ node.childIndex + 1u, false }); stack.push_back({ node.childIndex, false });
            continue;
        }
        else
        {
            const RtNode& c0 = out.nodes[node.childIndex]; const RtNode& c1 = out.nodes[node.childIndex + 1u];
            RefitBox b0, b1;
            memcpy(b0.min, c0.min, 12); memcpy(b0.max, c0.max, 12); memcpy(b1.min, c1.min, 12); memcpy(b1.max, c1.max, 12);
            box = refitJoin(b0, b1);
        }
        memcpy(node.min, box.min, 12); memcpy(node.max, box.max, 12);
    }
    out.ok = true;
    if (slotNode.empty()) return out;
    if (slotNode.size() != wide.size() || !wideGridOver(out.nodes[0].min, out.nodes[0].max, out.grid)) return out;
    out.gridOk = wideGridHolds(out.grid, out.nodes[0].min, out.nodes[0].max);   // false: the records below are clamped and must not be walked (rtgpu_update_mesh refuses before it writes)
    for (size_t i = 0; i < slotNode.size(); ++i)
    {
        if (slotNode[i] == 0xFFFFFFFFu) continue;
        if (slotNode[i] >= out.nodes.size()) { out.ok = out.gridOk = false; return out; }
        const RtNode& node = out.nodes[slotNode[i]];
        uint32_t v[6];
        wideQuantiseBox(out.grid.base, out.grid.step, node.min, node.max, v);
        for (int a = 0; a < 3; ++a)
        {
            const double lo = (double)out.grid.base[a] + (double)v[a] * (double)out.grid.step[a], hi = (double)out.grid.base[a] + (double)v[3 + a] * (double)out.grid.step[a];
            if (lo > (double)node.min[a] - 0.5 * (double)out.grid.step[a] || hi < (double)node.max[a] + 0.5 * (double)out.grid.step[a]) out.gridOk = false;
        }
        const float4 rec = wideRecord(v, 0u);
        out.wide[i].x = rec.x; out.wide[i].y = rec.y; out.wide[i].z = rec.z;
    }
    return out;
}

// ---- the scene class ---------------------------------------------------------------------------------------------------------------------------------
// a delta directional light whose direction has an exactly-zero component: EVERY next-event ray towards it is axis-parallel and goes through the re-trace launches (launchRetrace)
static bool hasAxisParallelSun(const RtLight* lights, uint32_t numLights)
{
    for (uint32_t i = 0; i < numLights; ++i)
        if (lights[i].type == RT_LIGHT_DIRECTIONAL && lights[i].isDelta && (lights[i].transform[8] == 0.0f || lights[i].transform[9] == 0.0f || lights[i].transform[10] == 0.0f)) return true;
    return false;
}

// RtgpuContext::leanScene.  1: mesh objects only, diffuse materials, background / directional lights, no textures; 2: the same with textures; 3: any other
// scene without textures; 0: any other scene with them; 4: a class-2 scene whose textures are all plain 8-bit BGR(A) / RGBA or half-float RGBA bitmaps
// (what Demo/MeshLoader.cpp makes of an OBJ's diffuse and normal maps: 24-bit .bmp files) -- the shading kernel inlines their evaluation.
// allowLean / allowSimpleTextures: the knobs RTGPU_NO_LEAN, RTGPU_NO_SIMPLE_TEXTURES (class 2 instead of 4) as the caller read them.
static int sceneClass(const RtSceneDesc& s, bool allowLean, bool allowSimpleTextures)
{
    bool lean = allowLean;
    for (uint32_t i = 0; i < s.numObjects && lean; ++i) lean = s.objects[i].objectKind == RT_OBJECT_SHAPE && s.objects[i].shapeKind == RT_SHAPE_MESH;
    for (uint32_t i = 0; i < s.numMaterials && lean; ++i) lean = s.materials[i].bsdf == RT_BSDF_DIFFUSE;
    for (uint32_t i = 0; i < s.numLights && lean; ++i) lean = s.lights[i].type == RT_LIGHT_BACKGROUND || s.lights[i].type == RT_LIGHT_DIRECTIONAL;
    bool textured = false;
    for (uint32_t i = 0; i < s.numMaterials; ++i)
        textured = textured || (s.materials[i].baseColorTexture & s.materials[i].emissionTexture & s.materials[i].roughnessTexture & s.materials[i].metalnessTexture & s.materials[i].normalMapTexture) != RT_NO_TEXTURE;
    for (uint32_t i = 0; i < s.numLights; ++i) textured = textured || s.lights[i].texture != RT_NO_TEXTURE;
    const int cls = lean ? (textured ? 2 : 1) : (textured ? 0 : 3);
    bool simple = cls == 2 && s.numTextures != 0u && allowSimpleTextures;
    for (uint32_t i = 0; i < s.numTextures && simple; ++i) simple = s.textures[i].kind == RT_TEXTURE_BITMAP && RT_FORMAT_IS_SIMPLE(s.textures[i].format);
    return simple ? 4 : cls;
}

// ---- a scene, prepared -------------------------------------------------------------------------------------------------------------------------------
// Everything rtgpu_upload_scene copies that is not the caller's own array, from a scene that passed its checks (topDepth, maxMeshDepth: from them).
struct PreparedScene
{
    std::vector<RtNode> meshNodes;             // breadth first
    std::vector<TriangleShading> shading;
    TwoLevelBuild twoLevel;                    // ok: the scene takes the two-level 4-wide walk
    QuantBuild singleGrid; WideBuild single;   // single.ok: a single-mesh scene (Scene::Traverse's one-object bypass) with its 4-wide tree
    int leanScene = 0;
    bool axisParallelSun = false;
    // what rtgpu_update_mesh needs (new beside the tables above, which are what they were): per mesh its plan and where its 4-wide level lies; per record of
    // twoLevel.nodes' mesh levels / of single.nodes the node of `meshNodes` (a global, breadth-first index) whose box it holds, 0xFFFFFFFF: none
    struct MeshLevel { uint32_t nodeBase = 0, numNodes = 0, gateBase = 0; bool have = false; };
    std::vector<MeshRefitPlan> refit;
    std::vector<MeshLevel> meshLevels;
    std::vector<uint32_t> wide2SlotNode, wideSlotNode;
};

// WideBuild::slotNode of one mesh (the caller's node order, mesh-relative) as indices into the scene's breadth-first mesh nodes
static void appendSlotNodes(std::vector<uint32_t>& to, const std::vector<uint32_t>& slotNode, const MeshRefitPlan& plan, const RtMesh& mesh)
{
    std::vector<uint32_t> position(mesh.numNodes, 0xFFFFFFFFu);   // the caller's index -> breadth-first position
    for (size_t k = 0; k < plan.order.size(); ++k) if (plan.order[k] < mesh.numNodes) position[plan.order[k]] = (uint32_t)k;
    for (const uint32_t n : slotNode) to.push_back(n < mesh.numNodes && position[n] != 0xFFFFFFFFu && plan.ok ? mesh.firstNode + position[n] : 0xFFFFFFFFu);
}

static PreparedScene prepareScene(const RtSceneDesc& s, uint32_t topDepth, uint32_t maxMeshDepth, bool allowLean, bool allowSimpleTextures)
{
    PreparedScene p;
    p.meshNodes = reorderMeshNodes(s);
    p.shading = deindexShading(s);
    const bool singleMesh = s.numObjects == 1u && s.objects[0].objectKind == RT_OBJECT_SHAPE && s.objects[0].shapeKind == RT_SHAPE_MESH;
    bool anyMesh = false;
    for (uint32_t o = 0; o < s.numObjects; ++o) anyMesh = anyMesh || (s.objects[o].objectKind == RT_OBJECT_SHAPE && s.objects[o].shapeKind == RT_SHAPE_MESH);
    // (a handful of analytic objects -- sphere + area light: a top-level tree of one or three nodes -- gain nothing from wider nodes and pay
    //  for the re-trace launch: measured 3-5 % slower, the binary kernel keeps them)
    if (!singleMesh && s.numObjects > 1u && (anyMesh || s.numTopNodes >= 7u)) p.twoLevel = buildTwoLevel(s, topDepth);
    if (singleMesh)
    {
        const RtMesh& mesh = s.meshes[s.objects[0].meshIndex];
        p.singleGrid = buildQuantBvh(s.meshNodes + mesh.firstNode, mesh.numNodes, mesh.numTriangles, maxMeshDepth);
        p.single = buildWideBvh(s.meshNodes + mesh.firstNode, mesh.numNodes, p.singleGrid);
    }
    p.leanScene = sceneClass(s, allowLean, allowSimpleTextures);
    p.axisParallelSun = hasAxisParallelSun(s.lights, s.numLights);
    p.refit.resize(s.numMeshes); p.meshLevels.resize(s.numMeshes);
    for (uint32_t m = 0; m < s.numMeshes; ++m)
        p.refit[m] = planMeshRefit(s.meshNodes + s.meshes[m].firstNode, p.meshNodes.data() + s.meshes[m].firstNode, s.meshes[m].numNodes, s.meshes[m].numTriangles);
    if (p.twoLevel.ok)
    {
        size_t record = 0;
        for (const TwoLevelBuild::MeshLevel& l : p.twoLevel.meshLevels)   // in the order their records lie in twoLevel.nodes
        {
            const std::vector<uint32_t> slots(p.twoLevel.slotNode.begin() + record, p.twoLevel.slotNode.begin() + record + 4u * (size_t)l.numNodes);
            appendSlotNodes(p.wide2SlotNode, slots, p.refit[l.meshIndex], s.meshes[l.meshIndex]);
            p.meshLevels[l.meshIndex].nodeBase = l.nodeBase; p.meshLevels[l.meshIndex].numNodes = l.numNodes; p.meshLevels[l.meshIndex].gateBase = l.gateBase;
            p.meshLevels[l.meshIndex].have = true;
            record += 4u * (size_t)l.numNodes;
        }
    }
    if (p.single.ok)
    {
        const uint32_t m = s.objects[0].meshIndex;
        appendSlotNodes(p.wideSlotNode, p.single.slotNode, p.refit[m], s.meshes[m]);
        p.meshLevels[m].nodeBase = 0u; p.meshLevels[m].numNodes = (uint32_t)(p.single.nodes.size() / 4u); p.meshLevels[m].gateBase = 0u; p.meshLevels[m].have = true;
    }
    return p;
}
