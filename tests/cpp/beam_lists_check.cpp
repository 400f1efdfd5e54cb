// beam_lists_check.cpp -- the host builder of the beam lists (raytracer_amd/csrc/rt_beam_lists.h) against brute force, on the CPU (tests/test_beam_lists_cpu.py).
//
//   beam_lists_check <input file>
// Input (little endian): u32 width, height, numNodes, numTriangles, capacity; f32 margin; RtCamera; f32 invTransform[16]; RtNode nodes[numNodes] (one mesh's
// binary tree, the reference's layout).  The 4-wide tree is built as an upload builds it (rt_scene_prepare.h), the slot table as rt_runtime.hip builds a
// whole frame's on one shard, the lists by buildBeamLists.  Then, for every pixel and the sample offsets at the four corners and the centre of [-m, m]^2: the
// reference's camera ray (Camera::GenerateRay, then the Ray constructor and the object's transformRayUnsafe: the oracle's arithmetic, oracle/rto_math.h)
// against the exact box of EVERY leaf of the tree, by the reference's slab test.  A leaf whose box the ray passes must be in the list of the pixel's tile, and
// the ray parameter at which it enters must be at least the entry's dmin.  Lists ascend in dmin.  A tile without a list is one whose leaves outnumber the capacity.
// Prints "ok tiles <n> noList <n> longest <n> mean <x> pairs <n>" or the first failures, and exits accordingly.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../../raytracer_amd/csrc/rt_scene_prepare.h"
#include "../../raytracer_amd/csrc/rt_beam_lists.h"
#include "../../oracle/rto_math.h"

static std::vector<uint32_t> slotTable(uint32_t width, uint32_t height)
{
    std::vector<uint32_t> slots;
    const uint32_t tilesX = (width + 63u) / 64u, tilesY = (height + 63u) / 64u;
    for (uint32_t ty = 0; ty < tilesY; ++ty) for (uint32_t tx = 0; tx < tilesX; ++tx)
        for (uint32_t by = 0; by < 8; ++by) for (uint32_t bx = 0; bx < 8; ++bx)
            for (uint32_t py = 0; py < 8; ++py) for (uint32_t px = 0; px < 8; ++px)
            {
                const uint32_t x = tx * 64 + bx * 8 + px, y = ty * 64 + by * 8 + py;
                if (x < width && y < height) slots.push_back(x | (y << 16));
            }
    return slots;
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: beam_lists_check <input>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t head[5]; float margin; RtCamera cam; float inv[16];
    bool ok = fread(head, 4, 5, f) == 5 && fread(&margin, 4, 1, f) == 1 && fread(&cam, sizeof(cam), 1, f) == 1 && fread(inv, 4, 16, f) == 16;
    const uint32_t width = head[0], height = head[1], numNodes = head[2], numTriangles = head[3], capacity = head[4];
    std::vector<RtNode> nodes(ok ? numNodes : 0u);
    ok = ok && fread(nodes.data(), sizeof(RtNode), numNodes, f) == numNodes;
    fclose(f);
    if (!ok) { fprintf(stderr, "short input\n"); return 2; }

    const uint32_t depth = bvhDepth(nodes.data(), numNodes);
    const QuantBuild q = buildQuantBvh(nodes.data(), numNodes, numTriangles, depth);
    const WideBuild w = buildWideBvh(nodes.data(), numNodes, q);
    if (!q.ok || !w.ok) { fprintf(stderr, "the tree has no 4-wide collapse\n"); return 2; }
    const std::vector<uint32_t> slots = slotTable(width, height);
    BeamCamera local;
    float lo[3], hi[3];
    beamTreeBounds(q.grid.base, q.grid.step, lo, hi);
    if (!beamCameraFor(cam, inv, width, height, margin, lo, hi, local)) { printf("no lists for this camera and transform\n"); return 3; }
    const BeamListsHost lists = buildBeamLists(w.nodes.data(), q.gate.data(), q.grid.base, q.grid.step, slots.data(), (uint32_t)slots.size(), local, capacity);

    // every leaf: its reference as the records hold it, its exact box
    struct Leaf { uint32_t ref; rto::V4 mn, mx; };
    std::vector<Leaf> leaves;
    for (uint32_t n = 2; n < numNodes; ++n)
    {
        const uint32_t count = nodes[n].leaves & 0x3FFFFFFFu;
        if (count == 0u || count > 2u) continue;
        const float4 gmin = q.gate[2u * (size_t)nodes[n].childIndex], gmax = q.gate[2u * (size_t)nodes[n].childIndex + 1u];
        if (memcmp(&gmin, nodes[n].min, 12) != 0 || memcmp(&gmax, nodes[n].max, 12) != 0) continue;   // (not reachable: the builder left its gate zero)
        leaves.push_back(Leaf{ nodes[n].childIndex | (count << RT_NODE_LEAVES_SHIFT), rto::load3(nodes[n].min), rto::load3(nodes[n].max) });
    }

    int failures = 0;
    size_t noList = 0, longest = 0, total = 0, pairs = 0;
    const uint32_t numTiles = (uint32_t)lists.counts.size();
    std::vector<std::map<uint32_t, float>> members(numTiles);
    for (uint32_t t = 0; t < numTiles; ++t)
    {
        if (lists.counts[t] == RT_BEAM_NO_LIST) { noList++; continue; }
        const uint32_t n = lists.counts[t];
        if (n > lists.capacity) { printf("tile %u: count %u above the capacity\n", t, n); failures++; continue; }
        longest = n > longest ? n : longest; total += n;
        for (uint32_t i = 0; i < n; ++i)
        {
            const BeamEntry& e = lists.entries[(size_t)t * lists.capacity + i];
            const float d = __builtin_bit_cast(float, e.dminBits);
            if (i && d < __builtin_bit_cast(float, lists.entries[(size_t)t * lists.capacity + i - 1].dminBits)) { printf("tile %u: entry %u is nearer than the one before\n", t, i); failures++; }
            if (!members[t].emplace(e.leaf, d).second) { printf("tile %u: leaf %08x twice\n", t, e.leaf); failures++; }
        }
    }
    const rto::M4 toWorld = rto::loadM4(cam.localToWorld), toLocal = rto::loadM4(inv);
    const float invW = 1.0f / (float)(int32_t)width, invH = 1.0f / (float)(int32_t)height;
    const float offsets[5][2] = { { -margin, -margin }, { -margin, margin }, { margin, -margin }, { margin, margin }, { 0.0f, 0.0f } };
    for (size_t s = 0; s < slots.size() && failures < 20; ++s)
    {
        const uint32_t tile = (uint32_t)(s / 64u), x = slots[s] & 0xFFFFu, y = slots[s] >> 16;
        if (lists.counts[tile] == RT_BEAM_NO_LIST) continue;
        for (int o = 0; o < 5; ++o)
        {
            // filmCoords, Camera::GenerateRay (pinhole), Ray::Ray, Matrix4::TransformRayUnsafe
            const uint32_t realY = height - 1u - y;
            const rto::V4 coords(((float)(int32_t)x + offsets[o][0]) * invW, ((float)(int32_t)realY + offsets[o][1]) * invH, 0.0f, 0.0f);
            const rto::V4 oc = rto::mulSub(coords, 2.0f, rto::splat(1.0f));
            const rto::V4 direction = rto::mulAdd(rto::mulAdd(toWorld.r[0], oc.x * cam.aspectRatio, toWorld.r[1] * oc.y), cam.tanHalfFoV, toWorld.r[2]);
            const rto::Ray world = rto::makeRay(toWorld.r[3], direction);
            const rto::Ray ray = rto::transformRayUnsafe(toLocal, world);
            // a ray with a zero direction component never consults a list: the reference's slab test makes NaNs of it, k_trace_packet's refill does not
            // trust it (rayIsNaNFree, RT_WIDE_FOLD_TEST) and hands it to the reference's own walk
            if (ray.dir.x == 0.0f || ray.dir.y == 0.0f || ray.dir.z == 0.0f) continue;
            for (const Leaf& leaf : leaves)
            {
                float nearD;
                if (!rto::intersectBoxRay(ray, leaf.mn, leaf.mx, nearD)) continue;
                pairs++;
                const auto it = members[tile].find(leaf.ref);
                if (it == members[tile].end()) { printf("pixel (%u, %u) offset %d: leaf %08x is passed but not in the list of tile %u\n", x, y, o, leaf.ref, tile); failures++; continue; }
                // (an origin inside the box: the ray is in it from parameter 0 on)
                if (fmaxf(nearD, 0.0f) < it->second) { printf("pixel (%u, %u) offset %d: leaf %08x is entered at %.9g, before its dmin %.9g\n", x, y, o, leaf.ref, nearD, it->second); failures++; }
            }
        }
    }
    if (failures) return 1;
    printf("ok tiles %u noList %zu longest %zu mean %.2f pairs %zu\n", numTiles, noList, longest, numTiles > noList ? (double)total / (double)(numTiles - noList) : 0.0, pairs);
    return 0;
}
