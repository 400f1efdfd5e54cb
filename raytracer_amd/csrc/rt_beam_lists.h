// rt_beam_lists.h -- beam lists (the format: rt_wide_format.h): what the host and the device share about BUILDING them, and the pure host builder.
// Included by rt_runtime.hip (the policy: rt_runtime_render.inl), by rt_trace.hip in front of rt_beam_lists.inl (the build kernel) and by
// tests/cpp/beam_lists_check.cpp; compiles without HIP, like rt_scene_prepare.h.  The consumer is k_trace_packet (rt_trace_packet.inl), which also says why a
// scan of a list returns the reference's hits.
//
// A still camera sends the same few leaves' worth of rays through an 8 x 8 pixel block on every pass of a frame: from one pass to the next the block's rays
// differ by that pass's sub-pixel sampleOffset only.  The 4-wide tree of a single-mesh scene is therefore walked ONCE per tile, with the tile's frustum in place
// of a ray, and what it finds is kept: the leaves, nearest first.
//
// Membership.  The pinhole camera's direction through film point (X, Y) is r0 X + r1 Y + r2 (Camera::GenerateRay; X = (2 fx - 1) aspect tan(fov / 2), Y =
// (2 fy - 1) tan(fov / 2), fx = (x + offset) / width), here in the mesh's LOCAL space (the object's transform is rigid: the policy's condition).  The rays of a
// tile's pixels at any offset of at most m pixels per axis lie between four planes through the eye: X = L, X = R, Y = B, Y = T over the tile's pixel bounds
// pushed out by m -- and by 1e-4 of the tile's width plus 1e-5 (of a film whose half-width is of order one: a hundredth of a full-HD pixel), far above the float
// rounding of the generate kernel's coordinates (2^-23 of them).  A box is LEFT OUT if one of the four planes has all of it outside by more than `slack` =
// 1e-5 of the largest eye-to-tree-corner coordinate difference, far above the rounding of the three-term dot product that decides (a few 2^-24 of its largest
// term): a superset of the boxes the frustum touches.  False positives cost time, never results.
// The test is MONOTONE -- a box inside another gets the smaller float sum, term by term, under round-to-nearest -- so the hierarchical walk, which prunes with
// the stored 16-bit boxes (each contains its subtree's exact boxes with a grid step to spare, rt_wide_format.h), reaches every leaf whose exact box passes: the
// list is exactly {leaves whose exact box passes the test}, whatever the tree above looks like.  That is what the device's lists are compared with the host's on.
//
// dmin.  The Euclidean distance from the eye to the exact box, times 1 - 1e-4, less `dminSlack`, not below zero: a unit-direction ray from the eye cannot enter
// the box at a smaller parameter.  The relative part covers the lengths (the directions the kernels normalise are unit to a few 2^-24, the object's rigid
// transform to the 1e-5 the policy admits).  The absolute part covers the POSITIONS: the eye here is the host's product of the camera's origin with the
// object's matrix, the kernels' is their own transformPoint of the same origin, and the reference's entry parameter is a difference of products of box and
// origin coordinates with the inverse direction -- each good to a few 2^-24 of the coordinates' magnitude, not of the distance, which for a box right in
// front of the eye is far smaller.  dminSlack = 1e-5 of (the largest |eye coordinate| + the largest eye-to-tree-corner difference): a hundred times those
// roundings; for a box nearer than that the entry is simply "from the start".
//
// One arithmetic.  Host and device run the same float operations in the same order (this header; -ffp-contract=off; fmaf on both sides; sqrtf, which both
// compilers round correctly by default -- the device's native square root is not: it moved dmin by a bit -- and which decides no membership anyway), and the
// walk takes the tree in the same ROUNDS -- up to 16 nodes = 64 child records per round, one per lane of the building wave, what passes
// appended in lane order -- so that the two agree on overflow too: a tile whose list outgrows the capacity or whose pending nodes outgrow RT_BEAM_STACK has no
// list on either side.
#pragma once

#include "rt_wide_format.h"

#include <algorithm>
#include <cmath>
#include <vector>

#define RT_BEAM_STACK 1024u          // nodes a tile's walk may have pending
#define RT_BEAM_ROUND 16u            // nodes per round
#define RT_BEAM_MAX_RETIRED 4u       // arrays (two sets of lists) a context keeps for launches in flight beside the set in use

struct BeamCamera
{
    float eye[3], r0[3], r1[3], r2[3];   // the pinhole in the mesh's local space: direction(X, Y) = r0 X + r1 Y + r2
    float scaleX, scaleY;                // X = (2 fx - 1) scaleX, Y = (2 fy - 1) scaleY; both > 0
    uint32_t width, height;
    float margin;                        // m, pixels
    float slack;                         // of the plane test (above)
    float dminSlack;                     // what dmin gives way by, absolutely (above)
    float orient;                        // +1 / -1: the handedness of (r0, r1, r2)
};
struct BeamPlanes { float n[4][3]; };   // inward normals of the planes X = L, X = R, Y = B, Y = T through the eye

RT_WIDE_HD static inline bool beamIsLeaf(uint32_t ref) { return ((ref >> RT_NODE_LEAVES_SHIFT) - 1u) < 2u; }
RT_WIDE_HD static inline float beamSqrt(float x) { return sqrtf(x); }   // (not the device's native square root: above)

RT_WIDE_HD static inline void beamCross(const float a[3], const float b[3], float s, float out[3])
{
    out[0] = s * (a[1] * b[2] - a[2] * b[1]); out[1] = s * (a[2] * b[0] - a[0] * b[2]); out[2] = s * (a[0] * b[1] - a[1] * b[0]);
}
// the planes of the tile whose pixels span [x0, x1] x [y0, y1] (inclusive; y counts from the film's top row as the slot table does: the film row is height - 1 - y)
RT_WIDE_HD static inline BeamPlanes beamTilePlanes(const BeamCamera& c, uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1)
{
    const float invW = 1.0f / (float)c.width, invH = 1.0f / (float)c.height;
    const float rowLo = (float)(c.height - 1u - y1), rowHi = (float)(c.height - 1u - y0);
    float L = ((((float)x0 - c.margin) * invW) * 2.0f - 1.0f) * c.scaleX, R = ((((float)x1 + c.margin) * invW) * 2.0f - 1.0f) * c.scaleX;
    float B = (((rowLo - c.margin) * invH) * 2.0f - 1.0f) * c.scaleY, T = (((rowHi + c.margin) * invH) * 2.0f - 1.0f) * c.scaleY;
    const float padX = 1e-4f * (R - L) + 1e-5f * (1.0f + fabsf(L) + fabsf(R)), padY = 1e-4f * (T - B) + 1e-5f * (1.0f + fabsf(B) + fabsf(T));
    L -= padX; R += padX; B -= padY; T += padY;
    float a[3], b[3], d[3], e[3];
    for (int k = 0; k < 3; ++k) { a[k] = c.r2[k] + L * c.r0[k]; b[k] = c.r2[k] + R * c.r0[k]; d[k] = c.r2[k] + B * c.r1[k]; e[k] = c.r2[k] + T * c.r1[k]; }
    BeamPlanes p;
    beamCross(c.r1, a, c.orient, p.n[0]); beamCross(c.r1, b, -c.orient, p.n[1]);
    beamCross(d, c.r0, c.orient, p.n[2]); beamCross(e, c.r0, -c.orient, p.n[3]);
    return p;
}
// false: one of the four planes has the whole box [lo, hi] outside (by more than the slack)
RT_WIDE_HD static inline bool beamBoxTouches(const BeamPlanes& p, const BeamCamera& c, const float lo[3], const float hi[3])
{
    for (int k = 0; k < 4; ++k)
    {
        const float t0 = p.n[k][0] * ((p.n[k][0] >= 0.0f ? hi[0] : lo[0]) - c.eye[0]);
        const float t1 = p.n[k][1] * ((p.n[k][1] >= 0.0f ? hi[1] : lo[1]) - c.eye[1]);
        const float t2 = p.n[k][2] * ((p.n[k][2] >= 0.0f ? hi[2] : lo[2]) - c.eye[2]);
        if ((t0 + t1) + t2 < -c.slack) return false;
    }
    return true;
}
RT_WIDE_HD static inline float beamBoxDmin(const BeamCamera& c, const float lo[3], const float hi[3])
{
    const float dx = fmaxf(fmaxf(lo[0] - c.eye[0], c.eye[0] - hi[0]), 0.0f), dy = fmaxf(fmaxf(lo[1] - c.eye[1], c.eye[1] - hi[1]), 0.0f);
    const float dz = fmaxf(fmaxf(lo[2] - c.eye[2], c.eye[2] - hi[2]), 0.0f);
    return fmaxf(beamSqrt((dx * dx + dy * dy) + dz * dz) * 0.9999f - c.dminSlack, 0.0f);
}
// One child record of a round: `interior` / `leaf`: it goes on (to the pending nodes / into the list, with `dmin`)
struct BeamChild { bool interior, leaf; uint32_t ref; float dmin; };
RT_WIDE_HD static inline BeamChild beamClassify(const float4& rec, const float4* gate, const float base[3], const float step[3], const BeamPlanes& p, const BeamCamera& c)
{
    BeamChild out; out.interior = false; out.leaf = false; out.dmin = 0.0f;
    out.ref = __builtin_bit_cast(uint32_t, rec.w);
    if ((out.ref >> RT_NODE_LEAVES_SHIFT) == 0u)
    {
        const uint32_t w0 = __builtin_bit_cast(uint32_t, rec.x), w1 = __builtin_bit_cast(uint32_t, rec.y), w2 = __builtin_bit_cast(uint32_t, rec.z);
        const float lo[3] = { fmaf((float)(w0 & 0xFFFFu), step[0], base[0]), fmaf((float)(w0 >> 16), step[1], base[1]), fmaf((float)(w1 & 0xFFFFu), step[2], base[2]) };
        const float hi[3] = { fmaf((float)(w1 >> 16), step[0], base[0]), fmaf((float)(w2 & 0xFFFFu), step[1], base[1]), fmaf((float)(w2 >> 16), step[2], base[2]) };
        out.interior = beamBoxTouches(p, c, lo, hi);
    }
    else if (beamIsLeaf(out.ref))
    {
        const uint32_t first = out.ref & RT_NODE_CHILD_MASK;
        const float4 gmin = gate[2u * first], gmax = gate[2u * first + 1u];
        const float lo[3] = { gmin.x, gmin.y, gmin.z }, hi[3] = { gmax.x, gmax.y, gmax.z };
        out.leaf = beamBoxTouches(p, c, lo, hi);
        if (out.leaf) out.dmin = beamBoxDmin(c, lo, hi);
    }
    return out;
}
RT_WIDE_HD static inline bool beamEntryBefore(const BeamEntry& a, const BeamEntry& b)
{
    const float da = __builtin_bit_cast(float, a.dminBits), db = __builtin_bit_cast(float, b.dminBits);
    return da < db || (da == db && a.leaf < b.leaf);
}


// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------
// The camera of a pass in the local space of the scene's one mesh object (world -> local: the object's invTransform, rows as RtObject stores them).
// false: no lists for this pair -- a camera with depth of field or barrel distortion, a degenerate frame, an object transform that is not rigid (scale or shear:
// dmin would not be a distance).  `treeLo`, `treeHi`: the tree's bounds (for the slack).
static inline bool beamCameraFor(const RtCamera& cam, const float invTransform[16], uint32_t width, uint32_t height, float margin, const float treeLo[3], const float treeHi[3],
                                 BeamCamera& out)
{
    // (barrel distortion is applied where the VARIABLE factor is not zero -- Camera.cpp:86-91, cameraGenerateRayParts; the default camera carries a constant
    //  factor of 0.01 that nothing reads)
    if (cam.dofEnable || cam.barrelDistortionVariableFactor != 0.0f) return false;
    if (width == 0u || height == 0u || !(margin >= 0.0f) || !std::isfinite(margin)) return false;
    // rigid: the rows of the upper 3 x 3 are orthonormal to 1e-5 (transformVector: v.x r[0] + v.y r[1] + v.z r[2])
    const float* m = invTransform;
    for (int i = 0; i < 3; ++i) for (int j = i; j < 3; ++j)
    {
        const double d = (double)m[4 * i] * m[4 * j] + (double)m[4 * i + 1] * m[4 * j + 1] + (double)m[4 * i + 2] * m[4 * j + 2];
        if (!(fabs(d - (i == j ? 1.0 : 0.0)) <= 1e-5)) return false;
    }
    auto vec = [&](const float* v, float w, float o[3]) { for (int k = 0; k < 3; ++k) o[k] = (v[0] * m[k] + v[1] * m[4 + k]) + (v[2] * m[8 + k] + w * m[12 + k]); };
    vec(cam.localToWorld + 0, 0.0f, out.r0); vec(cam.localToWorld + 4, 0.0f, out.r1); vec(cam.localToWorld + 8, 0.0f, out.r2); vec(cam.localToWorld + 12, 1.0f, out.eye);
    out.scaleX = cam.aspectRatio * cam.tanHalfFoV; out.scaleY = cam.tanHalfFoV;
    if (!(out.scaleX > 0.0f) || !(out.scaleY > 0.0f) || !std::isfinite(out.scaleX) || !std::isfinite(out.scaleY)) return false;
    float n[3]; beamCross(out.r1, out.r2, 1.0f, n);
    const float triple = n[0] * out.r0[0] + n[1] * out.r0[1] + n[2] * out.r0[2];
    if (!std::isfinite(triple) || !(fabsf(triple) > 1e-6f)) return false;
    out.orient = triple > 0.0f ? 1.0f : -1.0f;
    out.width = width; out.height = height; out.margin = margin;
    float extent = 0.0f;
    for (int k = 0; k < 3; ++k)
    {
        if (!std::isfinite(out.eye[k])) return false;
        extent = fmaxf(extent, fmaxf(fabsf(treeLo[k] - out.eye[k]), fabsf(treeHi[k] - out.eye[k])));
    }
    // (the normals' largest component is of the order of the frame's: |r| (1 + |slope|))
    out.slack = 1e-5f * extent * (1.0f + out.scaleX + out.scaleY);
    out.dminSlack = 1e-5f * (extent + fmaxf(fmaxf(fabsf(out.eye[0]), fabsf(out.eye[1])), fabsf(out.eye[2])));
    return std::isfinite(out.slack) && std::isfinite(out.dminSlack);
}
// the bounds of the grid a tree's records lie on (every box of the tree is inside)
static inline void beamTreeBounds(const float base[3], const float step[3], float lo[3], float hi[3])
{
    for (int k = 0; k < 3; ++k) { lo[k] = base[k]; hi[k] = base[k] + 65535.0f * step[k]; }
}

struct BeamListsHost { std::vector<BeamEntry> entries; std::vector<uint32_t> counts; uint32_t capacity = 0; };
// The lists of every tile of `slotPixel` (x | y << 16 per slot) over the 4-wide tree `nodes` / `gate` on the grid base / step: the reference the device's build
// kernel is held to, tile by tile.
static inline BeamListsHost buildBeamLists(const float4* nodes, const float4* gate, const float base[3], const float step[3], const uint32_t* slotPixel, uint32_t numSlots,
                                           const BeamCamera& cam, uint32_t capacity)
{
    BeamListsHost out;
    out.capacity = capacity < 1u ? 1u : (capacity > RT_BEAM_MAX_CAPACITY ? RT_BEAM_MAX_CAPACITY : capacity);
    const uint32_t numTiles = (numSlots + 63u) / 64u;
    out.entries.assign((size_t)numTiles * out.capacity, BeamEntry{ 0u, 0u });
    out.counts.assign(numTiles, 0u);
    std::vector<uint32_t> stack(RT_BEAM_STACK);
    for (uint32_t tile = 0; tile < numTiles; ++tile)
    {
        uint32_t x0 = 0xFFFFu, x1 = 0u, y0 = 0xFFFFu, y1 = 0u;
        for (uint32_t s = tile * 64u; s < numSlots && s < tile * 64u + 64u; ++s)
        {
            const uint32_t x = slotPixel[s] & 0xFFFFu, y = slotPixel[s] >> 16;
            x0 = std::min(x0, x); x1 = std::max(x1, x); y0 = std::min(y0, y); y1 = std::max(y1, y);
        }
        const BeamPlanes planes = beamTilePlanes(cam, x0, x1, y0, y1);
        BeamEntry list[RT_BEAM_MAX_CAPACITY];
        uint32_t sp = 1u, count = 0u; bool over = false;
        stack[0] = 0u;
        while (sp != 0u)
        {
            const uint32_t take = sp < RT_BEAM_ROUND ? sp : RT_BEAM_ROUND;
            sp -= take;
            uint32_t pendI[64], numI = 0u, numL = 0u; BeamEntry pendL[64];
            for (uint32_t lane = 0; lane < 4u * take; ++lane)
            {
                const BeamChild ch = beamClassify(nodes[4u * (size_t)stack[sp + (lane >> 2)] + (lane & 3u)], gate, base, step, planes, cam);
                if (ch.interior) pendI[numI++] = ch.ref;
                if (ch.leaf) pendL[numL++] = BeamEntry{ ch.ref, __builtin_bit_cast(uint32_t, ch.dmin) };
            }
            if (sp + numI > RT_BEAM_STACK || count + numL > out.capacity) { over = true; break; }
            for (uint32_t i = 0; i < numI; ++i) stack[sp + i] = pendI[i];
            for (uint32_t i = 0; i < numL; ++i) list[count + i] = pendL[i];
            sp += numI; count += numL;
        }
        if (over) { out.counts[tile] = RT_BEAM_NO_LIST; continue; }
        std::sort(list, list + count, beamEntryBefore);
        for (uint32_t i = 0; i < count; ++i) out.entries[(size_t)tile * out.capacity + i] = list[i];
        out.counts[tile] = count;
    }
    return out;
}

