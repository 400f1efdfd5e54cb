// rt_wide_format.h -- what the host and the device share about the 4-wide trees and the de-indexed shading records: the constants, the structs a launch
// passes, the layout of a node record and of a leaf's exact box.  The host builds these arrays (rt_scene_prepare.h), the kernels walk them (rt_wide_walk.h,
// rt_trace_wide.inl, rt_trace_packet.inl, rt_trace_wide2.inl); why a walk over them returns the reference's hits is argued where the kernels are, in
// rt_wide_grid.inl.  Included by rt_device_core.h (so by every unit of the library) and by rt_scene_prepare.h; compiles without HIP (a C++17 compiler and
// include/rtgpu.h are enough: tests/cpp/scene_prepare_check.cpp).
//
// Node n of a tree = records nodes[4 n .. 4 n + 3], one 16-byte record per child:
//   w0 = minx | miny << 16, w1 = minz | maxx << 16, w2 = maxy | maxz << 16      the child's box as 16-bit coordinates on the tree's grid,
//                                                                              plane(q) = base + q * step per axis, rounded OUTWARDS with a step to spare:
//                                                                              a stored box always contains the reference's box
//   w3 = the child's reference                                                 an interior node's index (breadth first, node 0 = the root's children), or a
//                                                                              leaf: first primitive | count << RT_NODE_LEAVES_SHIFT (the binary tree's own
//                                                                              leaves of one or two primitives), or RT_WIDE_EMPTY behind the degenerate box
//                                                                              {0, 0, 0, 0, 0, 0} (a point at the grid's corner, outside the tree's bounds)
//                                                                              for the unused slots of a node with two or three children
// Gates: the EXACT box of the leaf whose first primitive is p is gate[2 p] = {min.xyz, 0}, gate[2 p + 1] = {max.xyz, 0} -- the reference's floats, bit for
// bit; a leaf's primitives count only if the ray also passes this box.  Records of primitives that start no leaf are zero.
// A tree whose root is a leaf gets one node with that leaf as its only child.
#pragma once

#include <math.h>
#include <stdint.h>
#include "../../include/rtgpu.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#else
struct alignas(16) float4 { float x, y, z, w; };   // HIP's float4, for a host compiler
static inline float4 make_float4(float x, float y, float z, float w) { return float4{ x, y, z, w }; }
#endif

// a packed node reference (the binary walk's stack entries, rt_device_traverse.h, and the 4-wide records' w3): childIndex | numLeaves << 30
#define RT_NODE_LEAVES_SHIFT 30u
#define RT_NODE_CHILD_MASK 0x3FFFFFFFu
#define RT_MAX_PACKED_LEAVES 3u    // numLeaves must fit two bits (the reference builds leaves of <= 2, BVHBuilder.h:16)

#define RT_WIDE_EMPTY 0xC0000000u    // leaf count 3 never occurs in the reference's trees (BVHBuilder.h:16): "no child"
#define RT_QUANT_DONE 0xFFFFFFFFu   // cur: the ray is finished (same value as RT_LEVEL_EXHAUSTED: the mesh level has no node left)
#define RT_QUANT_GRID 65535.0f

// A box on a tree's grid: v = min.xyz, max.xyz, each the plane at least a full step outside the exact coordinate (in double, pushed out until it is), clamped to
// 0 .. 65535.  One copy for the upload's builder (buildQuantBvh, rt_scene_prepare.h), the host's refit (refitMesh) and the device's (rt_runtime_refit.inl): -ffp-contract=off keeps the double arithmetic the same on both.
#ifdef __HIPCC__
#define RT_WIDE_HD __host__ __device__
#else
#define RT_WIDE_HD
#endif
RT_WIDE_HD static inline void wideQuantiseBox(const float base[3], const float step[3], const float lo[3], const float hi[3], uint32_t v[6])
{
    for (int a = 0; a < 3; ++a)
    {
        const double b = (double)base[a], s = (double)step[a], xlo = (double)lo[a], xhi = (double)hi[a];
        long vmin = (long)floor((xlo - b) / s) - 1;
        while (vmin > 0 && b + (double)(uint32_t)vmin * s > xlo - s) --vmin;
        long vmax = (long)ceil((xhi - b) / s) + 1;
        while (vmax < 65535 && b + (double)(uint32_t)vmax * s < xhi + s) ++vmax;
        v[a] = (uint32_t)(vmin < 0 ? 0 : vmin); v[3 + a] = (uint32_t)(vmax > 65535 ? 65535 : vmax);
    }
}

// the 4-wide tree of a single-mesh scene (k_trace_wide, k_trace_packet, k_tail)
struct WideBvh
{
    const float4* nodes;
    const float4* gate;
    uint32_t numNodes;
    float base[3], step[3], bound[3];   // the grid; bound: the largest |coordinate| a plane of it has, which bounds a slab term of the fold (rt_wide_walk.h)
};

// Beam lists (rt_beam_lists.h builds them, host and device; k_trace_packet scans them): per TILE = 64 consecutive slots of the slot -> pixel table (one wave of
// k_trace_packet) the leaves of the tree above whose exact box a camera ray of the tile's pixels can pass at any sample offset of at most `margin` pixels per
// axis, nearest first.  Tile t: counts[t] entries at entries[t * capacity ..], each {the leaf's reference as the node records hold it, bits of dmin}, ascending
// in (dmin, reference); dmin: a lower bound of the ray parameter at which a unit-direction ray from the eye can enter the leaf's exact box.
// counts[t] == RT_BEAM_NO_LIST: the tile has none (more leaves than the capacity, or the builder's stack ran out) and walks the tree.
#define RT_BEAM_NO_LIST 0xFFFFFFFFu
#define RT_BEAM_MAX_CAPACITY 64u     // one entry per lane of the building wave
struct BeamEntry { uint32_t leaf; uint32_t dminBits; };
struct BeamLists
{
    const BeamEntry* entries;    // nullptr: the launch has no lists
    const uint32_t* counts;
    uint32_t capacity;           // entries per tile, <= RT_BEAM_MAX_CAPACITY
    uint32_t slotsPerPass;       // the slot -> pixel table's length: slot = pass in batch * slotsPerPass + pixel slot
    float margin;                // m, in pixels: a pass whose |sampleOffset| exceeds it on an axis walks
    const void* passes;          // the batch's DevPass records (their sampleOffset)
    unsigned long long* stats;   // [0] packets served from lists, [1] packets that walked for their pass's offset, [2] packets that walked for "no list"
};

// two-level scenes (k_trace_wide2): one node array and one gate array for all levels
struct WideLevel   // 64 bytes
{
    uint32_t nodeBase;    // first node of the level in WideScene::nodes, in nodes (a node = four float4)
    uint32_t gateBase;    // the exact box of the leaf whose first primitive is p: gate[gateBase + 2 p] (min), gate[gateBase + 2 p + 1] (max)
    uint32_t triBase;     // mesh levels: the mesh's first triangle in RtSceneDesc::triangles
    uint32_t valid;       // 0: an object without a tree (an empty mesh)
    float base[3], step[3], bound[3];
    uint32_t pad[3];
};
static_assert(sizeof(WideLevel) == 64, "WideLevel");
struct WideScene
{
    const float4* nodes;
    const float4* gate;
    const WideLevel* levels;   // [numObjects] mesh objects (valid only for those), [numObjects] = the top level
    uint32_t numObjects;       // >= 2 (one-object scenes are Scene::Traverse's bypass: no top-level tree; k_trace_wide or k_trace serve them)
};

// what a launch of any of the 4-wide walks is tuned by (the device parts they share, rt_wide_walk.h, read it too)
struct WideTuning
{
    uint32_t refillMinIdle, otherMinLanes;
    float shadowOffset;
    uint32_t* exactQueue; uint32_t* exactCount;               // closest-hit rays handed to the binary-tree kernel
    uint32_t* exactShadowQueue; uint32_t* exactShadowCount;   // any-hit requests handed to it
    const uint32_t* denseCounts; uint32_t denseShardCapacity; // dense path state (TravTuning)
    uint32_t chunkMin;                                        // smallest piece of the work queue a wave claims at once
    uint32_t localExact;                                      // != 0: a block traces the rays its walk does not decide itself (k_trace_wide)
    uint32_t drainAbortAfter;                                 // != 0: a wave whose work queue ran dry this many loop iterations ago hands the rays it still walks to the binary-tree kernel
};

// The device copy of the scene holds the shading data DE-INDEXED: one 128-byte record per triangle (its three VertexShadingData and
// its material), in triangle order, where the C ABI's vertexIndices[] would be (vertexShading[] is not uploaded).  A hit then costs
// one memory round trip to one aligned 128-byte line instead of the index record followed by three scattered 32-byte vertices.
struct __attribute__((aligned(16))) TriangleShading { RtVertexShading v[3]; uint32_t materialIndex; uint32_t _pad[7]; };
static_assert(sizeof(TriangleShading) == 128, "TriangleShading");
// the bitmap formats the shading kernel of scene class 4 decodes inline (rt_device_core.h, bitmapTexel<true>; rt_scene_prepare.h, sceneClass)
#define RT_FORMAT_IS_SIMPLE(f) ((f) == RT_FORMAT_B8G8R8_UNORM || (f) == RT_FORMAT_B8G8R8A8_UNORM || (f) == RT_FORMAT_R8G8B8A8_UNORM || (f) == RT_FORMAT_R16G16B16A16_HALF)
