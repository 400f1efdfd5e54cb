// scene_prepare_check -- the contract between the host-built 4-wide trees (raytracer_amd/csrc/rt_scene_prepare.h) and the kernels that walk them, checked on the
// CPU.  The kernels return the reference's hits only while every stored 16-bit box contains the exact box with a grid step to spare and every leaf's exact
// box ("gate") is the reference's; this program restates that, independently of the builders' own postcondition checks, and stops at the first violation:
//   (a) every reachable leaf of the binary tree appears exactly once as a 4-wide child, with the same first primitive and the same count;
//   (b) interior references are below the node count and breadth first;
//   (c) base + q * step, in double, lies at least half a step below the exact minimum and at least half a step above the exact maximum, per child and axis;
//   (d) gate[2 p], gate[2 p + 1] are the leaf's exact box, bit for bit;
//   (e) unused slots carry RT_WIDE_EMPTY behind the degenerate corner box;
//   (f) a top level over n objects has at most n 4-wide nodes and exactly 2 n gate records (the slab of rtgpu_update_objects), n = 2 .. 64, chain and balanced;
//   (g) the breadth-first mesh nodes describe the same tree: child pairs adjacent and even-aligned, leaves keep their ranges, node 1 unused.
// Stand-alone: it includes the two headers and include/rtgpu.h, nothing of HIP.  tests/test_scene_prepare_cpu.py builds and runs it.
//
//   scene_prepare_check synthetic          trees built here: the smallest ones at which each part can go wrong, and malformed ones that must be refused
//   scene_prepare_check scenes FILE        every scene of FILE (the tables of tests/update_scenes.desc_arrays, see readScenes): checks, then one line per array
//                                          with its FNV-1a 64 hash -- tests/golden/prepared_scenes.json holds the parent commit's
//   scene_prepare_check update FILE        FILE = a scene, the same scene after Scene.update() with its previousIndex, the moved scene built afresh: the update's
//                                          rebuild must equal the fresh assembly word for word and leave the mesh slabs alone
#include "../../raytracer_amd/csrc/rt_scene_prepare.h"

#include <stdio.h>
#include <stdlib.h>
#include <map>
#include <string>

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static uint32_t bitsOf(float f) { return __builtin_bit_cast(uint32_t, f); }
static uint32_t leavesOf(const RtNode& n) { return n.leaves & 0x3FFFFFFFu; }

// ---- one level against its binary tree -------------------------------------------------------------------------------------------------------------
struct LeafSet { uint64_t sum = 0; uint32_t count = 0; };   // the leaves below a node, as an order-free signature
static uint64_t mix(uint64_t x) { x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33; return x; }
static void add(LeafSet& to, const LeafSet& s) { to.sum += s.sum; to.count += s.count; }
static LeafSet oneLeaf(uint32_t first, uint32_t count) { LeafSet s; s.sum = mix(((uint64_t)first << 2) | count); s.count = 1; return s; }

static void checkLevel(const char* what, const RtNode* bin, uint32_t numBin, uint32_t numPrimitives, const float4* wide, size_t numWideRecords, const float4* gate,
                       size_t numGate, const float base[3], const float step[3])
{
    CHECK(numWideRecords >= 4 && numWideRecords % 4 == 0, "%s: %zu records", what, numWideRecords);
    CHECK(numGate == 2 * (size_t)numPrimitives, "%s: %zu gate records for %u primitives", what, numGate, numPrimitives);
    const uint32_t numWide = (uint32_t)(numWideRecords / 4);
    // the binary tree's reachable leaves and the leaf set below every node (children before parents: a post-order of our own)
    std::vector<LeafSet> below(numBin);
    std::map<uint32_t, uint32_t> leafNode;   // first primitive -> binary node
    {
        std::vector<std::pair<uint32_t, bool>> todo; todo.push_back({ 0u, false });
        while (!todo.empty())
        {
            const auto [n, done] = todo.back(); todo.pop_back();
            CHECK(n < numBin, "%s: binary node %u", what, n);
            if (leavesOf(bin[n])) { CHECK(leafNode.emplace(bin[n].childIndex, n).second, "%s: two leaves start at %u", what, bin[n].childIndex); below[n] = oneLeaf(bin[n].childIndex, leavesOf(bin[n])); continue; }
            const uint32_t c = bin[n].childIndex;
            if (done) { add(below[n], below[c]); add(below[n], below[c + 1]); continue; }
            todo.push_back({ n, true }); todo.push_back({ c, false }); todo.push_back({ c + 1, false });
        }
    }
    // (b) references in range and breadth first: the interior references, read in array order, count 1, 2, 3, ...
    uint32_t nextInterior = 1;
    for (size_t r = 0; r < numWideRecords; ++r)
    {
        const uint32_t ref = bitsOf(wide[r].w);
        if ((ref >> RT_NODE_LEAVES_SHIFT) == 0u) { CHECK(ref < numWide && ref == nextInterior, "%s: record %zu refers to node %u, expected %u of %u", what, r, ref, nextInterior, numWide); ++nextInterior; }
    }
    CHECK(nextInterior == numWide, "%s: %u nodes, %u referred to", what, numWide, nextInterior);
    // leaf sets below the wide nodes (children have larger indices: from the back)
    std::vector<LeafSet> wideBelow(numWide);
    for (uint32_t n = numWide; n-- > 0;)
        for (uint32_t k = 0; k < 4; ++k)
        {
            const uint32_t ref = bitsOf(wide[4 * n + k].w), kind = ref >> RT_NODE_LEAVES_SHIFT;
            if (kind == 0u) add(wideBelow[n], wideBelow[ref]);
            else if (kind < 3u) add(wideBelow[n], oneLeaf(ref & RT_NODE_CHILD_MASK, kind));
        }
    CHECK(wideBelow[0].sum == below[0].sum && wideBelow[0].count == below[0].count && below[0].count == leafNode.size(), "%s: (a) %u leaves below the 4-wide root, %u in the binary tree",
          what, wideBelow[0].count, below[0].count);
    // walk both trees together: wide node <-> the binary node it was collapsed from
    std::vector<uint8_t> leafSeen(numBin, 0);
    std::vector<std::pair<uint32_t, uint32_t>> todo; todo.push_back({ 0u, 0u });
    while (!todo.empty())
    {
        const auto [w, b] = todo.back(); todo.pop_back();
        // the binary nodes a child of w can be: b itself where the root is a leaf, else b's descendants down to three levels (two children, each expansion one deeper)
        std::vector<uint32_t> candidates;
        if (leavesOf(bin[b])) candidates.push_back(b);
        else
        {
            std::vector<std::pair<uint32_t, uint32_t>> level; level.push_back({ b, 0u });
            for (size_t i = 0; i < level.size(); ++i)
            {
                const auto [n, depth] = level[i];
                if (depth) candidates.push_back(n);
                if (!leavesOf(bin[n]) && depth < 3u) { level.push_back({ bin[n].childIndex, depth + 1 }); level.push_back({ bin[n].childIndex + 1, depth + 1 }); }
            }
        }
        LeafSet children;
        for (uint32_t k = 0; k < 4; ++k)
        {
            const float4& rec = wide[4 * w + k];
            const uint32_t ref = bitsOf(rec.w), kind = ref >> RT_NODE_LEAVES_SHIFT;
            if (kind == 3u)
            {
                // (e)
                CHECK(ref == RT_WIDE_EMPTY && bitsOf(rec.x) == 0u && bitsOf(rec.y) == 0u && bitsOf(rec.z) == 0u, "%s: (e) node %u slot %u: %08x %08x %08x %08x", what, w, k, bitsOf(rec.x), bitsOf(rec.y), bitsOf(rec.z), ref);
                continue;
            }
            uint32_t match = 0xFFFFFFFFu;
            for (uint32_t cand : candidates)
            {
                const bool same = kind == 0u ? (!leavesOf(bin[cand]) && below[cand].sum == wideBelow[ref].sum && below[cand].count == wideBelow[ref].count)
                                             : (leavesOf(bin[cand]) == kind && bin[cand].childIndex == (ref & RT_NODE_CHILD_MASK));
                if (same) { match = cand; break; }
            }
            CHECK(match != 0xFFFFFFFFu, "%s: node %u slot %u (%08x) is no descendant of binary node %u", what, w, k, ref, b);
            const RtNode& exact = bin[match];
            add(children, below[match]);
            // (c)
            const uint32_t q[6] = { bitsOf(rec.x) & 0xFFFFu, bitsOf(rec.x) >> 16, bitsOf(rec.y) & 0xFFFFu, bitsOf(rec.y) >> 16, bitsOf(rec.z) & 0xFFFFu, bitsOf(rec.z) >> 16 };
            for (int a = 0; a < 3; ++a)
            {
                const double lo = (double)base[a] + (double)q[a] * (double)step[a], hi = (double)base[a] + (double)q[3 + a] * (double)step[a], half = 0.5 * (double)step[a];
                CHECK(lo <= (double)exact.min[a] - half && hi >= (double)exact.max[a] + half, "%s: (c) node %u slot %u axis %d: stored [%.17g, %.17g], exact [%.9g, %.9g], step %.9g", what, w, k, a, lo, hi,
                      exact.min[a], exact.max[a], step[a]);
            }
            if (kind == 0u) { todo.push_back({ ref, match }); continue; }
            // (a), (d)
            CHECK(!leafSeen[match], "%s: (a) the leaf at primitive %u appears twice", what, exact.childIndex);
            leafSeen[match] = 1;
            const uint32_t p = exact.childIndex;
            CHECK((uint64_t)p + kind <= numPrimitives, "%s: leaf %u + %u beyond %u primitives", what, p, kind, numPrimitives);
            const float4 gmin = gate[2 * (size_t)p], gmax = gate[2 * (size_t)p + 1];
            CHECK(bitsOf(gmin.x) == bitsOf(exact.min[0]) && bitsOf(gmin.y) == bitsOf(exact.min[1]) && bitsOf(gmin.z) == bitsOf(exact.min[2]) && bitsOf(gmin.w) == 0u &&
                  bitsOf(gmax.x) == bitsOf(exact.max[0]) && bitsOf(gmax.y) == bitsOf(exact.max[1]) && bitsOf(gmax.z) == bitsOf(exact.max[2]) && bitsOf(gmax.w) == 0u, "%s: (d) gate of primitive %u", what, p);
        }
        CHECK(children.sum == below[b].sum && children.count == below[b].count, "%s: (a) the children of node %u hold %u leaves, binary node %u holds %u", what, w, children.count, b, below[b].count);
    }
    for (const auto& leaf : leafNode) CHECK(leafSeen[leaf.second], "%s: (a) the leaf at primitive %u is missing", what, leaf.first);
}

static void checkLevel(const char* what, const RtNode* bin, uint32_t numBin, uint32_t numPrimitives, const WideLevelBuild& b)
{
    CHECK(b.ok, "%s: not built", what);
    checkLevel(what, bin, numBin, numPrimitives, b.nodes.data(), b.nodes.size(), b.gate.data(), b.gate.size(), b.grid.base, b.grid.step);
}

// (g)
static void checkReordered(const char* what, const RtNode* src, const RtNode* dst, uint32_t numNodes)
{
    if (numNodes == 0u) return;
    if (numNodes < 3u) { CHECK(memcmp(src, dst, numNodes * sizeof(RtNode)) == 0, "%s: a tree without child pairs moved", what); return; }
    std::vector<std::pair<uint32_t, uint32_t>> level; level.push_back({ 0u, 0u });   // breadth first over (old, new)
    uint32_t nextPair = 2;
    for (size_t i = 0; i < level.size(); ++i)
    {
        const auto [o, n] = level[i];
        CHECK(o < numNodes && n < numNodes && n != 1u, "%s: (g) node %u -> %u", what, o, n);
        CHECK(memcmp(src[o].min, dst[n].min, 12) == 0 && memcmp(src[o].max, dst[n].max, 12) == 0 && src[o].leaves == dst[n].leaves, "%s: (g) node %u -> %u: another box or leaf word", what, o, n);
        if (leavesOf(src[o])) { CHECK(src[o].childIndex == dst[n].childIndex, "%s: (g) leaf %u -> %u: range moved", what, o, n); continue; }
        const uint32_t c = dst[n].childIndex;
        CHECK(c == nextPair && (c & 1u) == 0u && (uint64_t)c + 1u < numNodes, "%s: (g) node %u -> %u: child pair at %u, expected %u", what, o, n, c, nextPair);
        nextPair += 2;
        level.push_back({ src[o].childIndex, c }); level.push_back({ src[o].childIndex + 1, c + 1 });
    }
}

// ---- a whole scene ------------------------------------------------------------------------------------------------------------------------------------
struct SceneDepths { uint32_t top = 0, mesh = 0; };
// the tree checks of rtgpu_upload_scene, in its order
static SceneStatus validateTrees(const RtSceneDesc& s, SceneDepths& d)
{
    d.top = bvhDepth(s.topNodes, s.numTopNodes);
    SceneStatus st = checkTreeDepth(d.top, "malformed top-level BVH");
    for (uint32_t m = 0; m < s.numMeshes && st.code == RTGPU_OK; ++m)
    {
        const uint32_t md = bvhDepth(s.meshNodes + s.meshes[m].firstNode, s.meshes[m].numNodes);
        st = checkTreeDepth(md, "malformed mesh BVH");
        if (st.code == RTGPU_OK && md > d.mesh) d.mesh = md;
    }
    if (st.code == RTGPU_OK) st = checkStack(d.top, d.mesh);
    if (st.code == RTGPU_OK) st = checkLeaves(s.topNodes, s.numTopNodes);
    if (st.code == RTGPU_OK) st = checkLeaves(s.meshNodes, s.numMeshNodes);
    return st;
}

static void checkPrepared(const char* name, const RtSceneDesc& s, const PreparedScene& p)
{
    CHECK(p.meshNodes.size() == s.numMeshNodes && p.shading.size() == s.numTriangles, "%s: array sizes", name);
    for (uint32_t m = 0; m < s.numMeshes; ++m)
        checkReordered(name, s.meshNodes + s.meshes[m].firstNode, p.meshNodes.data() + s.meshes[m].firstNode, s.meshes[m].numNodes);
    for (uint32_t m = 0; m < s.numMeshes; ++m)
        for (uint32_t t = 0; t < s.meshes[m].numTriangles; ++t)
        {
            const RtVertexIndices& idx = s.vertexIndices[s.meshes[m].firstTriangle + t];
            const TriangleShading& rec = p.shading[s.meshes[m].firstTriangle + t];
            const RtVertexShading* vs = s.vertexShading + s.meshes[m].firstVertex;
            CHECK(memcmp(&rec.v[0], vs + idx.i0, 32) == 0 && memcmp(&rec.v[1], vs + idx.i1, 32) == 0 && memcmp(&rec.v[2], vs + idx.i2, 32) == 0 && rec.materialIndex == idx.materialIndex,
                  "%s: shading record of triangle %u of mesh %u", name, t, m);
        }
    if (p.twoLevel.ok)
    {
        const TwoLevelBuild& t = p.twoLevel;
        const uint32_t n = s.numObjects;
        CHECK(t.levels.size() == (size_t)n + 1 && t.levels[n].valid == 1u, "%s: level table", name);
        CHECK(t.topNodeCapacity == n && t.nodes.size() == t.meshNodes + 4 * (size_t)t.topNodeCapacity && t.usedNodes <= t.nodes.size() && t.gates.size() == t.meshGates + 2 * (size_t)n, "%s: (f) the slab", name);
        for (uint32_t o = 0; o <= n; ++o)
        {
            const WideLevel& level = t.levels[o];
            const bool top = o == n;
            const bool mesh = !top && s.objects[o].objectKind == RT_OBJECT_SHAPE && s.objects[o].shapeKind == RT_SHAPE_MESH && s.meshes[s.objects[o].meshIndex].numNodes != 0u;
            CHECK((level.valid != 0u) == (top || mesh), "%s: level %u valid = %u", name, o, level.valid);
            if (!level.valid) continue;
            const RtMesh* m = top ? nullptr : &s.meshes[s.objects[o].meshIndex];
            const RtNode* bin = top ? s.topNodes : s.meshNodes + m->firstNode;
            const uint32_t numBin = top ? s.numTopNodes : m->numNodes, numPrimitives = top ? n : m->numTriangles;
            CHECK(level.triBase == (top ? 0u : m->firstTriangle), "%s: level %u triBase", name, o);
            // the level's records end where the next base of the array begins
            size_t end = top ? t.usedNodes / 4 : t.meshNodes / 4;
            for (uint32_t other = 0; other <= n; ++other) if (t.levels[other].valid && t.levels[other].nodeBase > level.nodeBase && t.levels[other].nodeBase < end) end = t.levels[other].nodeBase;
            CHECK(level.nodeBase < end && (size_t)level.gateBase + 2 * (size_t)numPrimitives <= t.gates.size(), "%s: level %u bases", name, o);
            const std::string what = std::string(name) + (top ? " top level" : " mesh level " + std::to_string(o));
            checkLevel(what.c_str(), bin, numBin, numPrimitives, t.nodes.data() + 4 * (size_t)level.nodeBase, 4 * (end - level.nodeBase), t.gates.data() + level.gateBase, 2 * (size_t)numPrimitives, level.base, level.step);
        }
        for (size_t i = t.usedNodes; i < t.nodes.size(); ++i) CHECK(bitsOf(t.nodes[i].x) == 0u && bitsOf(t.nodes[i].y) == 0u && bitsOf(t.nodes[i].z) == 0u && bitsOf(t.nodes[i].w) == 0u, "%s: the slab behind the top level", name);
    }
    if (p.single.ok)
    {
        const RtMesh& m = s.meshes[s.objects[0].meshIndex];
        checkLevel((std::string(name) + " single mesh").c_str(), s.meshNodes + m.firstNode, m.numNodes, m.numTriangles, p.single.nodes.data(), p.single.nodes.size(), p.singleGrid.gate.data(), p.singleGrid.gate.size(),
                   p.singleGrid.grid.base, p.singleGrid.grid.step);
    }
}

// ---- scene files -------------------------------------------------------------------------------------------------------------------------------------
// "RTPREP1\0", uint32 number of scenes; per scene: char name[32]; uint32 counts[10] = top nodes, objects, lights, materials, meshes, mesh nodes, triangles,
// vertices, textures, previousIndex entries (0, or the number of objects); uint32 bytes per element of objects, lights, materials, meshes, textures; then the
// arrays: topNodes, objects, lights, materials, meshes, meshNodes, vertexIndices, vertexShading, textures, previousIndex.
struct SceneFile
{
    std::string name;
    std::vector<RtNode> topNodes, meshNodes; std::vector<RtObject> objects; std::vector<RtLight> lights; std::vector<RtMaterial> materials; std::vector<RtMesh> meshes;
    std::vector<RtVertexIndices> vertexIndices; std::vector<RtVertexShading> vertexShading; std::vector<RtTexture> textures; std::vector<uint32_t> previousIndex;
    RtSceneDesc desc() const
    {
        RtSceneDesc d; memset(&d, 0, sizeof(d));
        d.abiVersion = RTGPU_ABI_VERSION;
        d.numObjects = (uint32_t)objects.size(); d.numTopNodes = (uint32_t)topNodes.size(); d.numLights = (uint32_t)lights.size(); d.numMaterials = (uint32_t)materials.size();
        d.numMeshes = (uint32_t)meshes.size(); d.numMeshNodes = (uint32_t)meshNodes.size(); d.numTriangles = (uint32_t)vertexIndices.size(); d.numVertices = (uint32_t)vertexShading.size();
        d.numTextures = (uint32_t)textures.size();
        d.topNodes = topNodes.data(); d.objects = objects.data(); d.lights = lights.data(); d.materials = materials.data(); d.meshes = meshes.data(); d.meshNodes = meshNodes.data();
        d.vertexIndices = vertexIndices.data(); d.vertexShading = vertexShading.data(); d.textures = textures.data();
        return d;
    }
};
template <class T> static void readArray(FILE* f, std::vector<T>& out, uint32_t count)
{
    out.resize(count);
    CHECK(count == 0 || fread(out.data(), sizeof(T), count, f) == count, "short file");
}
static std::vector<SceneFile> readScenes(const char* path)
{
    FILE* f = fopen(path, "rb");
    CHECK(f, "cannot open %s", path);
    char magic[8]; uint32_t numScenes = 0;
    CHECK(fread(magic, 1, 8, f) == 8 && memcmp(magic, "RTPREP1", 8) == 0 && fread(&numScenes, 4, 1, f) == 1, "%s: not a scene file", path);
    std::vector<SceneFile> scenes(numScenes);
    for (SceneFile& s : scenes)
    {
        char name[33] = { 0 }; uint32_t n[10], bytes[5];
        CHECK(fread(name, 1, 32, f) == 32 && fread(n, 4, 10, f) == 10 && fread(bytes, 4, 5, f) == 5, "%s: short header", path);
        CHECK(bytes[0] == sizeof(RtObject) && bytes[1] == sizeof(RtLight) && bytes[2] == sizeof(RtMaterial) && bytes[3] == sizeof(RtMesh) && bytes[4] == sizeof(RtTexture), "%s: another ABI's element sizes", path);
        s.name = name;
        readArray(f, s.topNodes, n[0]); readArray(f, s.objects, n[1]); readArray(f, s.lights, n[2]); readArray(f, s.materials, n[3]); readArray(f, s.meshes, n[4]);
        readArray(f, s.meshNodes, n[5]); readArray(f, s.vertexIndices, n[6]); readArray(f, s.vertexShading, n[7]); readArray(f, s.textures, n[8]); readArray(f, s.previousIndex, n[9]);
    }
    fclose(f);
    return scenes;
}

static uint64_t fnv1a(const void* data, size_t bytes, uint64_t h = 0xcbf29ce484222325ull)
{
    const unsigned char* p = (const unsigned char*)data;
    for (size_t i = 0; i < bytes; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}
template <class T> static void printHash(const std::string& scene, const char* array, const std::vector<T>& v)
{
    printf("%s %s %016llx %zu\n", scene.c_str(), array, (unsigned long long)fnv1a(v.data(), v.size() * sizeof(T)), v.size() * sizeof(T));
}

static PreparedScene prepareChecked(const SceneFile& file, const RtSceneDesc& d)
{
    SceneDepths depths;
    const SceneStatus st = validateTrees(d, depths);
    CHECK(st.code == RTGPU_OK, "%s: refused: %s", file.name.c_str(), st.message);
    const PreparedScene p = prepareScene(d, depths.top, depths.mesh, true, true);
    checkPrepared(file.name.c_str(), d, p);
    return p;
}

static int runScenes(const char* path)
{
    for (const SceneFile& file : readScenes(path))
    {
        const RtSceneDesc d = file.desc();
        const PreparedScene p = prepareChecked(file, d);
        // what an upload of this scene sends beside the caller's own arrays, and what rtgpu_get_walk_info reports of it (rt_runtime_scene.inl)
        printHash(file.name, "meshNodes", p.meshNodes); printHash(file.name, "shading", p.shading);
        printHash(file.name, "wide2.nodes", p.twoLevel.ok ? p.twoLevel.nodes : std::vector<float4>()); printHash(file.name, "wide2.gates", p.twoLevel.ok ? p.twoLevel.gates : std::vector<float4>());
        printHash(file.name, "wide2.levels", p.twoLevel.ok ? p.twoLevel.levels : std::vector<WideLevel>());
        printHash(file.name, "wide.nodes", p.single.ok ? p.single.nodes : std::vector<float4>()); printHash(file.name, "wide.gates", p.single.ok ? p.singleGrid.gate : std::vector<float4>());
        std::vector<float> grid;
        if (p.single.ok) { grid.insert(grid.end(), p.singleGrid.grid.base, p.singleGrid.grid.base + 3); grid.insert(grid.end(), p.singleGrid.grid.step, p.singleGrid.grid.step + 3); grid.insert(grid.end(), p.singleGrid.grid.bound, p.singleGrid.grid.bound + 3); }
        printHash(file.name, "wide.grid", grid);
        const std::vector<uint64_t> info = { (uint64_t)(uint32_t)p.leanScene, (uint64_t)p.axisParallelSun,
                                             ((uint64_t)d.numTopNodes + d.numMeshNodes) * sizeof(RtNode),                                                      // binary walk: node bytes
                                             p.single.ok ? p.single.nodes.size() * sizeof(float4) : 0, p.single.ok ? p.singleGrid.gate.size() * sizeof(float4) : 0,   // single-mesh walk: nodes, leaf boxes
                                             p.twoLevel.ok ? p.twoLevel.usedNodes * sizeof(float4) : 0, p.twoLevel.ok ? p.twoLevel.gates.size() * sizeof(float4) : 0, // two-level walk
                                             p.twoLevel.ok ? p.twoLevel.meshNodes * sizeof(float4) : 0, p.twoLevel.ok ? p.twoLevel.meshGates * sizeof(float4) : 0 };
        printHash(file.name, "class+walk", info);
        printf("%s class %d sun %d\n", file.name.c_str(), p.leanScene, (int)p.axisParallelSun);
    }
    return 0;
}

static int runUpdate(const char* path)
{
    const std::vector<SceneFile> files = readScenes(path);
    CHECK(files.size() == 3, "%s: before, updated, fresh", path);
    const SceneFile& before = files[0]; const SceneFile& after = files[1]; const SceneFile& fresh = files[2];
    const RtSceneDesc db = before.desc(), da = after.desc(), df = fresh.desc();
    const uint32_t n = db.numObjects;
    CHECK(da.numObjects == n && df.numObjects == n && after.previousIndex.size() == n, "%s: object counts", path);
    const PreparedScene pb = prepareChecked(before, db), pf = prepareChecked(fresh, df);
    CHECK(pb.twoLevel.ok && pf.twoLevel.ok, "%s: not a two-level scene", path);
    // rtgpu_update_objects: its tree checks, the rebuild, and the copies into the arrays the upload left
    const uint32_t topDepth = bvhDepth(da.topNodes, da.numTopNodes);
    SceneStatus st = checkTreeDepth(topDepth, "");
    if (st.code == RTGPU_OK) st = checkLeaves(da.topNodes, da.numTopNodes, n);
    CHECK(st.code == RTGPU_OK, "%s: the updated top level is refused", path);
    const TopLevelRebuild r = rebuildTopLevel(pb.twoLevel.levels, after.previousIndex.data(), da.topNodes, da.numTopNodes, n, topDepth, pb.twoLevel.topNodeCapacity);
    CHECK(r.top.ok && r.top.nodes.size() / 4 <= pb.twoLevel.topNodeCapacity, "%s: the rebuilt top level does not fit its slab", path);
    std::vector<float4> nodes = pb.twoLevel.nodes, gates = pb.twoLevel.gates;
    memcpy(nodes.data() + 4 * (size_t)r.levels[n].nodeBase, r.top.nodes.data(), r.top.nodes.size() * sizeof(float4));
    memcpy(gates.data() + r.levels[n].gateBase, r.top.gate.data(), r.top.gate.size() * sizeof(float4));
    // the mesh slabs are untouched ...
    CHECK(4 * (size_t)r.levels[n].nodeBase == pb.twoLevel.meshNodes && r.levels[n].gateBase == pb.twoLevel.meshGates, "%s: the top level moved", path);
    CHECK(memcmp(nodes.data(), pb.twoLevel.nodes.data(), pb.twoLevel.meshNodes * sizeof(float4)) == 0 && memcmp(gates.data(), pb.twoLevel.gates.data(), pb.twoLevel.meshGates * sizeof(float4)) == 0, "%s: a mesh slab changed", path);
    // ... and level table, top-level nodes and gates are the fresh assembly's, word for word
    const TwoLevelBuild& f = pf.twoLevel;
    CHECK(r.levels.size() == f.levels.size() && memcmp(r.levels.data(), f.levels.data(), f.levels.size() * sizeof(WideLevel)) == 0, "%s: the level table differs from the fresh scene's", path);
    CHECK(f.meshNodes == pb.twoLevel.meshNodes && f.usedNodes == f.meshNodes + r.top.nodes.size() && memcmp(nodes.data(), f.nodes.data(), f.usedNodes * sizeof(float4)) == 0, "%s: the nodes differ from the fresh scene's", path);
    CHECK(gates.size() == f.gates.size() && memcmp(gates.data(), f.gates.data(), gates.size() * sizeof(float4)) == 0, "%s: the gates differ from the fresh scene's", path);
    // the rebuilt tree itself
    checkLevel((after.name + " rebuilt top level").c_str(), da.topNodes, da.numTopNodes, n, r.top);
    printf("%s: update == fresh (%zu top-level nodes, %u objects)\n", after.name.c_str(), r.top.nodes.size() / 4, n);
    return 0;
}

// ---- synthetic trees ---------------------------------------------------------------------------------------------------------------------------------
static RtNode node(float x0, float y0, float z0, float x1, float y1, float z1, uint32_t childIndex, uint32_t leaves)
{
    RtNode n; n.min[0] = x0; n.min[1] = y0; n.min[2] = z0; n.max[0] = x1; n.max[1] = y1; n.max[2] = z1; n.childIndex = childIndex; n.leaves = leaves;
    return n;
}
static RtNode unite(const RtNode& a, const RtNode& b, uint32_t childIndex)
{
    RtNode n = node(0, 0, 0, 0, 0, 0, childIndex, 0u);
    for (int k = 0; k < 3; ++k) { n.min[k] = fminf(a.min[k], b.min[k]); n.max[k] = fmaxf(a.max[k], b.max[k]); }
    return n;
}
// a tree over `boxes` (one primitive per leaf) in the reference's layout (root at 0, node 1 unused, child pairs even-aligned): a chain (each right child splits again) or balanced
static std::vector<RtNode> treeOver(const std::vector<RtNode>& boxes, bool chain)
{
    std::vector<RtNode> nodes(2);
    struct Job { uint32_t at, first, count; };
    std::vector<Job> jobs; jobs.push_back({ 0u, 0u, (uint32_t)boxes.size() });
    for (size_t j = 0; j < jobs.size(); ++j)   // (boxes of interior nodes: filled in from the back, below)
    {
        const Job job = jobs[j];
        if (job.count == 1u) { nodes[job.at] = boxes[job.first]; nodes[job.at].childIndex = job.first; nodes[job.at].leaves = 1u; continue; }
        const uint32_t left = chain ? 1u : job.count / 2u, c = (uint32_t)nodes.size();
        nodes.resize(nodes.size() + 2);
        nodes[job.at] = node(0, 0, 0, 0, 0, 0, c, 0u);
        jobs.push_back({ c, job.first, left }); jobs.push_back({ c + 1, job.first + left, job.count - left });
    }
    for (size_t j = jobs.size(); j-- > 0;) { const uint32_t at = jobs[j].at; if (!nodes[at].leaves) nodes[at] = unite(nodes[nodes[at].childIndex], nodes[nodes[at].childIndex + 1], nodes[at].childIndex); }
    nodes[1] = node(0, 0, 0, 0, 0, 0, 0u, 0u);
    return nodes;
}
static std::vector<RtNode> unitBoxes(uint32_t n, float offset, bool flat)
{
    std::vector<RtNode> boxes;
    for (uint32_t i = 0; i < n; ++i)
    {
        const float t = (float)i / (float)(n > 1 ? n : 2), x = offset + t, y = offset + 0.37f * t * t, z = offset + (flat ? 0.0f : 0.61f * (1.0f - t));
        boxes.push_back(node(x, y, z, x + 0.13f, y + 0.07f, flat ? z : z + 0.11f, 0u, 0u));
    }
    return boxes;
}

static void expectRefused(const char* what, const std::vector<RtNode>& nodes, uint32_t numPrimitives, int status)
{
    // through the checks of an upload (what it answers today), then through the builder, which must not hand such a tree to the kernels
    const uint32_t depth = bvhDepth(nodes.data(), (uint32_t)nodes.size());
    SceneStatus st = checkTreeDepth(depth, "malformed");
    if (st.code == RTGPU_OK) st = checkStack(depth, 0u);
    if (st.code == RTGPU_OK) st = checkLeaves(nodes.data(), (uint32_t)nodes.size());
    CHECK(st.code == status, "%s: status %d, expected %d", what, st.code, status);
    if (depth == kMalformedTree) return;   // (an upload stops there)
    CHECK(!buildWideLevel(nodes.data(), (uint32_t)nodes.size(), numPrimitives, depth).ok, "%s: built", what);
    CHECK(!buildTopLevel(nodes.data(), (uint32_t)nodes.size(), numPrimitives, depth, numPrimitives).ok, "%s: built as a top level", what);
}

// Whether a grid over the box [lo, hi] can hold ANY conservative record, from the format alone (rt_wide_format.h: 65535 - 8 steps across the box, base four
// steps below lo, coordinates 0 .. 65535).  Planes do not lie below base, so (c) for the node that holds lo needs base <= lo - step / 2; where lo is so far
// from the origin that the float lo - 4 steps rounds back to within half a step of lo -- or the last plane, likewise, to within half a step of hi --, no
// record can keep the contract and refusing the tree (the binary walk keeps such a scene) is the only right answer.
static bool gridCannotHold(const RtNode& bounds)
{
    float largest = 0.0f;
    for (int a = 0; a < 3; ++a) largest = fmaxf(largest, bounds.max[a] - bounds.min[a]);
    for (int a = 0; a < 3; ++a)
    {
        const float step = fmaxf(bounds.max[a] - bounds.min[a], 1e-6f * largest) / (65535.0f - 8.0f), base = bounds.min[a] - 4.0f * step;
        if ((double)base > (double)bounds.min[a] - 0.5 * (double)step || (double)base + 65535.0 * (double)step < (double)bounds.max[a] + 0.5 * (double)step) return true;
    }
    return false;
}

static int runSynthetic()
{
    // a root that is a leaf of one primitive, and of two
    for (uint32_t count = 1; count <= 2; ++count)
    {
        const std::vector<RtNode> tree = { node(-1.0f, 0.5f, 2.0f, 3.0f, 0.75f, 2.5f, 0u, count) };
        checkLevel("root leaf", tree.data(), 1u, count, buildWideLevel(tree.data(), 1u, count, 0u));
    }
    // three primitives (a node with an empty slot), a mesh flat in one axis, meshes away from the origin; a few sizes around a node's four slots.  What each
    // variant must come to is worked out from the float format, not read off the builder:
    //   0  unit-sized at the origin, 1  the same, flat in z at 0                       base = -4 steps is exact: built
    //   2  unit-sized, displaced by 1e4 on every axis                                 a step is ~1.7e-5, one ulp of 1e4 is 9.8e-4: lo - 4 steps == lo, REFUSED
    //   3  flat in z at 0.25                                                          the flat axis's step is ~1.7e-11, one ulp of 0.25 is 3e-8: REFUSED
    //   4  displaced by 16 (ulp 1.9e-6), 5  by 100 (ulp 7.6e-6)                         base lands within half an ulp, a fraction of a step, of lo - 4 steps: built,
    //                                                                                 with the builder's outward push of the stored coordinates at work
    for (uint32_t n : { 2u, 3u, 4u, 5u, 7u, 33u })
        for (int variant = 0; variant < 6; ++variant)
            for (int chain = 0; chain < 2; ++chain)
            {
                static const float offsets[6] = { 0.0f, 0.0f, 1.0e4f, 0.25f, 16.0f, 100.0f };   // (1, 3: flat)
                const bool refused = variant == 2 || variant == 3;
                const std::vector<RtNode> tree = treeOver(unitBoxes(n, offsets[variant], variant == 1 || variant == 3), chain != 0);
                const std::string what = std::to_string(n) + " primitives, variant " + std::to_string(variant) + (chain ? ", chain" : ", balanced");
                CHECK(gridCannotHold(tree[0]) == refused, "%s: the grid over the tree's bounds %s hold a conservative record", what.c_str(), refused ? "can" : "cannot");
                const WideLevelBuild b = buildWideLevel(tree.data(), (uint32_t)tree.size(), n, bvhDepth(tree.data(), (uint32_t)tree.size()));
                if (refused) { CHECK(!b.ok, "%s: built on a grid that cannot hold it", what.c_str()); continue; }
                checkLevel(what.c_str(), tree.data(), (uint32_t)tree.size(), n, b);
                if (variant == 1) CHECK(b.grid.step[2] > 0.0f && b.grid.step[2] < b.grid.step[0], "%s: the flat axis takes its step from the largest extent", what.c_str());
                if (n == 3u) { uint32_t empty = 0; for (const float4& rec : b.nodes) empty += bitsOf(rec.w) == RT_WIDE_EMPTY; CHECK(empty == 1u && b.nodes.size() == 4u, "%s: one node with one empty slot", what.c_str()); }
            }
    // the same for a root that is a leaf (variants 0 .. 3: one box is a tenth of the unit mesh, at 16 and 100 its grid is no longer clearly on either side)
    for (int variant = 0; variant < 4; ++variant)
    {
        static const float offsets[4] = { 0.0f, 0.0f, 1.0e4f, 0.25f };
        const bool refused = variant >= 2;
        const std::vector<RtNode> boxes = unitBoxes(1, offsets[variant], variant == 1 || variant == 3);
        const std::vector<RtNode> tree = { node(boxes[0].min[0], boxes[0].min[1], boxes[0].min[2], boxes[0].max[0], boxes[0].max[1], boxes[0].max[2], 0u, 1u) };
        const WideLevelBuild b = buildWideLevel(tree.data(), 1u, 1u, 0u);
        CHECK(gridCannotHold(tree[0]) == refused && b.ok == !refused, "root leaf, variant %d: %s", variant, b.ok ? "built" : "refused");
        if (b.ok) checkLevel("root leaf, flat or not", tree.data(), 1u, 1u, b);
    }
    // (f) the slab of a top level: n = 2 .. 64, chain and balanced
    for (uint32_t n = 2; n <= 64; ++n)
        for (int chain = 0; chain < 2; ++chain)
        {
            const std::vector<RtNode> tree = treeOver(unitBoxes(n, 0.0f, false), chain != 0);
            const WideLevelBuild plain = buildWideLevel(tree.data(), (uint32_t)tree.size(), n, bvhDepth(tree.data(), (uint32_t)tree.size()));
            CHECK(plain.ok && plain.nodes.size() / 4 <= n && plain.gate.size() == 2 * (size_t)n, "(f) %u objects, %s: %zu nodes, %zu gate records", n, chain ? "chain" : "balanced", plain.nodes.size() / 4, plain.gate.size());
            CHECK(buildTopLevel(tree.data(), (uint32_t)tree.size(), n, bvhDepth(tree.data(), (uint32_t)tree.size()), n).ok, "(f) %u objects: refused", n);
        }
    // two objects that share one mesh, one object whose mesh has no nodes
    {
        const std::vector<RtNode> meshTree = treeOver(unitBoxes(5, 0.0f, false), false), topTree = treeOver(unitBoxes(3, 0.0f, false), true);
        RtMesh meshes[2]; memset(meshes, 0, sizeof(meshes));
        meshes[0].numNodes = (uint32_t)meshTree.size(); meshes[0].numTriangles = 5u; meshes[0].numVertices = 3u;
        meshes[1].firstNode = (uint32_t)meshTree.size(); meshes[1].firstTriangle = 5u; meshes[1].firstVertex = 3u;
        RtObject objects[3]; memset(objects, 0, sizeof(objects));
        for (RtObject& o : objects) { o.objectKind = RT_OBJECT_SHAPE; o.shapeKind = RT_SHAPE_MESH; }
        objects[2].meshIndex = 1u;
        std::vector<RtVertexIndices> indices(5); std::vector<RtVertexShading> vertices(3);
        memset(vertices.data(), 0, vertices.size() * sizeof(RtVertexShading));
        for (uint32_t t = 0; t < 5; ++t) { indices[t].i0 = t % 3u; indices[t].i1 = (t + 1u) % 3u; indices[t].i2 = (t + 2u) % 3u; indices[t].materialIndex = t; }
        for (uint32_t v = 0; v < 3; ++v) vertices[v].normal[0] = (float)(v + 1u);
        RtSceneDesc d; memset(&d, 0, sizeof(d));
        d.numObjects = 3u; d.objects = objects; d.numTopNodes = (uint32_t)topTree.size(); d.topNodes = topTree.data(); d.numMeshes = 2u; d.meshes = meshes;
        d.numMeshNodes = (uint32_t)meshTree.size(); d.meshNodes = meshTree.data(); d.numTriangles = 5u; d.vertexIndices = indices.data(); d.numVertices = 3u; d.vertexShading = vertices.data();
        SceneDepths depths;
        CHECK(validateTrees(d, depths).code == RTGPU_OK, "instances: refused");
        const PreparedScene p = prepareScene(d, depths.top, depths.mesh, true, true);
        CHECK(p.twoLevel.ok, "instances: not built");
        checkPrepared("instances", d, p);
        CHECK(memcmp(&p.twoLevel.levels[0], &p.twoLevel.levels[1], sizeof(WideLevel)) == 0 && p.twoLevel.levels[2].valid == 0u, "instances share a level, an empty mesh has none");
        CHECK(p.twoLevel.meshGates == 10u, "instances: one copy of the mesh's gates");
    }
    // malformed trees: refused by the builders; the status is what an upload answers today
    {
        const std::vector<RtNode> good = treeOver(unitBoxes(3, 0.0f, false), true);   // 0 -> (2, 3), 3 -> (4, 5)
        CHECK(good.size() == 6u && buildWideLevel(good.data(), 6u, 3u, 2u).ok, "the tree the malformed ones start from");
        std::vector<RtNode> t;
        t = good; t.push_back(good[5]); t[0].childIndex = 3u; t[3] = good[2]; t[4] = good[3]; t[4].childIndex = 5u; t[5] = good[4]; t[6] = good[5];
        expectRefused("an odd child index", t, 3u, RTGPU_OK);
        t = good; t[3].childIndex = 6u;
        expectRefused("a child pair beyond the array", t, 3u, RTGPU_ERR_INVALID_ARGUMENT);
        t = good; t.resize(8); t[2] = good[3]; t[2].childIndex = 4u; t[3].childIndex = 4u;
        expectRefused("a node reachable twice", t, 3u, RTGPU_OK);
        t = good; t[2].leaves = 3u;
        expectRefused("a leaf count of 3", t, 5u, RTGPU_OK);
        t = good; t[5].childIndex = 3u;
        expectRefused("a leaf range beyond the primitives", t, 3u, RTGPU_OK);
        CHECK(checkLeaves(t.data(), (uint32_t)t.size(), 3u).code == RTGPU_ERR_INVALID_ARGUMENT, "a leaf range beyond the primitives: an update's check of a top level over 3 objects");
        t = good; t[4].min[1] = NAN;
        expectRefused("a NaN box", t, 3u, RTGPU_OK);
        t = good; t[4].max[2] = INFINITY; t[3].max[2] = INFINITY; t[0].max[2] = INFINITY;
        expectRefused("an infinite box", t, 3u, RTGPU_OK);
        t = good; t[4].min[0] = t[4].max[0] + 0.01f;
        expectRefused("a min > max box", t, 3u, RTGPU_OK);
        // the same three in a root that is a leaf
        t = { node(0, 0, 0, 1, 1, 1, 0u, 1u) }; t[0].min[2] = NAN;
        expectRefused("a NaN root leaf", t, 1u, RTGPU_OK);
        t = { node(0, 0, 0, 1, INFINITY, 1, 0u, 1u) };
        expectRefused("an infinite root leaf", t, 1u, RTGPU_OK);
        t = { node(0, 2, 0, 1, 1, 1, 0u, 1u) };
        expectRefused("a min > max root leaf", t, 1u, RTGPU_OK);
    }
    printf("synthetic trees: ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && strcmp(argv[1], "synthetic") == 0) return runSynthetic();
    if (argc == 3 && strcmp(argv[1], "scenes") == 0) return runScenes(argv[2]);
    if (argc == 3 && strcmp(argv[1], "update") == 0) return runUpdate(argv[2]);
    fprintf(stderr, "usage: %s synthetic | scenes FILE | update FILE\n", argv[0]);
    return 2;
}
