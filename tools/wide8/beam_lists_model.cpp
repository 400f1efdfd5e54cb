// beam_lists_model.cpp -- CPU gate for "serve a still camera's primary rays from per-tile leaf lists": how long would such a list be?
//
// Reads what tools/wide8/dump_walk_inputs.py wrote (nodes.bin, tris.bin, rays.bin, pixels.bin, meta.txt, camera.txt: the benchmark mesh's binary tree =
// the reference's BVH::Node array with its exact leaf boxes, the recorded primary rays with their pixels, the pinhole camera) and, for every 8 x 8 tile of the
// slot -> pixel table (64 consecutive slots, rt_runtime.hip buildSlotTable: one wave of k_trace_packet),
//   - takes the frustum of every ray of the tile's pixels at any sampleOffset with |offset| <= m pixels per axis: the four side planes through the eye over the
//     tile's pixel bounds pushed outwards by m pixels (and a relative margin of 1e-4 of the frustum's width, far above float rounding),
//   - collects the reference's leaves whose EXACT box those four planes do not separate from the frustum (and that do not lie behind the eye), by a
//     hierarchical walk of the binary tree with the same test on the interior boxes,
//   - sorts them by dmin = the Euclidean distance from the eye to the box (a lower bound of the ray parameter at which any unit-direction ray from the eye
//     can enter the box),
// and reports the list's length
//   (a) up to the first hit of the RECORDED primary rays of the tile (entries with dmin < the ray's hit distance): what one ray needs,
//   (b) up to the FARTHEST first hit of the tile's 64 pixel-centre rays, traced here: what a wave's scan runs through before it may leave the list
//       (the cut is dmin >= the wave's LARGEST best + 2 tol; a ray that hits nothing keeps the wave in the list to its end),
//   (c) in full (what the capacity K must hold),
// each as mean, median, p95, p99, and the share of tiles whose full list exceeds K = 32, 48, 64; all of it for m = 3 x antiAliasingSpread and, for the
// sensitivity, m = 0 and m = 6 x antiAliasingSpread.  Plain float arithmetic: a model of COUNTS, not of the kernel's exactness rules.
//
//   g++ -O2 -std=c++17 tools/wide8/beam_lists_model.cpp -o /tmp/walk_model/beam_lists_model && /tmp/walk_model/beam_lists_model /tmp/walk_model
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

struct Node { float mn[3]; uint32_t child; float mx[3]; uint32_t leaves; };
struct Tri { float v0[3], e1[3], e2[3]; };
struct RayIn { float o[3], d[3], dist, bounce, p[3], n[3]; };

static std::vector<Node> gNodes;
static std::vector<Tri> gTris;
static inline bool isLeaf(uint32_t n) { return (gNodes[n].leaves & 0x3FFFFFFFu) != 0u; }

// ---- the slot -> pixel table of a full frame on one shard (rt_runtime.hip buildSlotTable) ----
static std::vector<uint32_t> buildSlotTable(uint32_t width, uint32_t height)
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

// ---- camera (Camera::GenerateRay's pinhole: direction = (r0 * cx * aspect + r1 * cy) * tanHalfFoV + r2, c = 2 * film - 1) ----
static uint32_t gW, gH;
static float gSpread, gAspect, gTan, gM[16];
static double gEye[3], gR0[3], gR1[3], gR2[3];
static inline double filmX(double x) { return (2.0 * x / gW - 1.0) * gAspect * gTan; }     // camera-space slope dx/dz of the ray through film column x (pixels)
static inline double filmY(double ry) { return (2.0 * ry / gH - 1.0) * gTan; }              // ... of film row ry = height - 1 - y (+ offset)

struct Frustum { double n[4][3]; };   // inward normals of the four side planes through the eye, in WORLD space (the point is relative to the eye)
static Frustum tileFrustum(double x0, double x1, double ry0, double ry1)
{
    // slopes, pushed outwards by a relative margin
    double L = filmX(x0), R = filmX(x1), B = filmY(ry0), T = filmY(ry1);
    const double padX = 1e-4 * (R - L) + 1e-7, padY = 1e-4 * (T - B) + 1e-7;
    L -= padX; R += padX; B -= padY; T += padY;
    // camera space: inside iff px - L pz >= 0, R pz - px >= 0, py - B pz >= 0, T pz - py >= 0
    const double c[4][3] = { { 1, 0, -L }, { -1, 0, R }, { 0, 1, -B }, { 0, -1, T } };
    Frustum f;
    for (int k = 0; k < 4; ++k) for (int a = 0; a < 3; ++a) f.n[k][a] = c[k][0] * gR0[a] + c[k][1] * gR1[a] + c[k][2] * gR2[a];
    return f;
}
// false: one of the four planes (or the plane through the eye across the view axis) has the whole box outside
static inline bool boxTouches(const Frustum& f, const float mn[3], const float mx[3])
{
    for (int k = 0; k < 4; ++k)
    {
        double s = 0.0;
        for (int a = 0; a < 3; ++a) s += f.n[k][a] * ((f.n[k][a] >= 0.0 ? (double)mx[a] : (double)mn[a]) - gEye[a]);   // the corner farthest along the inward normal
        if (s < 0.0) return false;
    }
    double s = 0.0;
    for (int a = 0; a < 3; ++a) s += gR2[a] * ((gR2[a] >= 0.0 ? (double)mx[a] : (double)mn[a]) - gEye[a]);
    return s > 0.0;
}
static inline double eyeDistance(const float mn[3], const float mx[3])
{
    double d2 = 0.0;
    for (int a = 0; a < 3; ++a) { const double d = std::max(std::max((double)mn[a] - gEye[a], gEye[a] - (double)mx[a]), 0.0); d2 += d * d; }
    return sqrt(d2);
}

// ---- a plain closest-hit walk of the binary tree (pixel-centre rays of a tile) ----
static inline bool triHit(const double o[3], const double d[3], const Tri& t, double& dist)
{
    const double px = d[1] * t.e2[2] - d[2] * t.e2[1], py = d[2] * t.e2[0] - d[0] * t.e2[2], pz = d[0] * t.e2[1] - d[1] * t.e2[0];
    const double det = t.e1[0] * px + t.e1[1] * py + t.e1[2] * pz;
    if (det == 0.0) return false;
    const double inv = 1.0 / det, tx = o[0] - t.v0[0], ty = o[1] - t.v0[1], tz = o[2] - t.v0[2];
    const double u = (tx * px + ty * py + tz * pz) * inv;
    if (u < 0.0 || u > 1.0) return false;
    const double qx = ty * t.e1[2] - tz * t.e1[1], qy = tz * t.e1[0] - tx * t.e1[2], qz = tx * t.e1[1] - ty * t.e1[0];
    const double v = (d[0] * qx + d[1] * qy + d[2] * qz) * inv;
    if (v < 0.0 || u + v > 1.0) return false;
    dist = (t.e2[0] * qx + t.e2[1] * qy + t.e2[2] * qz) * inv;
    return dist > 0.0;
}
static double traceClosest(const double o[3], const double d[3])
{
    double inv[3]; for (int a = 0; a < 3; ++a) inv[a] = 1.0 / d[a];
    double best = INFINITY;
    uint32_t stack[128]; int sp = 0;
    stack[sp++] = gNodes[0].child; stack[sp++] = gNodes[0].child + 1u;
    while (sp)
    {
        const uint32_t n = stack[--sp];
        double tn = 0.0, tf = best;
        for (int a = 0; a < 3; ++a)
        {
            const double t0 = ((double)gNodes[n].mn[a] - o[a]) * inv[a], t1 = ((double)gNodes[n].mx[a] - o[a]) * inv[a];
            tn = std::max(tn, std::min(t0, t1)); tf = std::min(tf, std::max(t0, t1));
        }
        if (!(tf >= tn)) continue;
        if (isLeaf(n))
        {
            const uint32_t count = gNodes[n].leaves & 0x3FFFFFFFu;
            for (uint32_t i = 0; i < count; ++i) { double t; if (triHit(o, d, gTris[gNodes[n].child + i], t) && t < best) best = t; }
        }
        else if (sp + 2 <= 128) { stack[sp++] = gNodes[n].child; stack[sp++] = gNodes[n].child + 1u; }
    }
    return best;
}

struct Dist
{
    std::vector<double> v;
    void add(double x) { v.push_back(x); }
    void print(const char* what)
    {
        if (v.empty()) { printf("    %-72s (none)\n", what); return; }
        std::sort(v.begin(), v.end());
        double sum = 0; for (double x : v) sum += x;
        auto q = [&](double p) { return v[std::min(v.size() - 1, (size_t)(p * v.size()))]; };
        printf("    %-72s n %7zu  mean %7.2f  median %4.0f  p95 %5.0f  p99 %5.0f  max %5.0f\n", what, v.size(), sum / v.size(), q(0.5), q(0.95), q(0.99), v.back());
    }
};

int main(int argc, char** argv)
{
    const std::string dir = argc > 1 ? argv[1] : "/tmp/walk_model";
    size_t numNodes = 0, numTris = 0, numRays = 0; float sun[3];
    { FILE* f = fopen((dir + "/meta.txt").c_str(), "r"); if (!f || fscanf(f, "%zu %zu %zu %f %f %f", &numNodes, &numTris, &numRays, &sun[0], &sun[1], &sun[2]) != 6) { fprintf(stderr, "no meta.txt in %s\n", dir.c_str()); return 1; } fclose(f); }
    {
        FILE* f = fopen((dir + "/camera.txt").c_str(), "r");
        bool ok = f && fscanf(f, "%u %u %f %f %f", &gW, &gH, &gSpread, &gAspect, &gTan) == 5;
        for (int i = 0; ok && i < 16; ++i) ok = fscanf(f, "%f", &gM[i]) == 1;
        if (!ok) { fprintf(stderr, "no camera.txt in %s\n", dir.c_str()); return 1; }
        fclose(f);
    }
    gNodes.resize(numNodes); gTris.resize(numTris);
    std::vector<RayIn> in(numRays);
    auto slurp = [&](const char* name, void* dst, size_t bytes) { FILE* f = fopen((dir + "/" + name).c_str(), "rb"); if (!f || fread(dst, 1, bytes, f) != bytes) { fprintf(stderr, "bad %s\n", name); exit(1); } fclose(f); };
    slurp("nodes.bin", gNodes.data(), numNodes * sizeof(Node)); slurp("tris.bin", gTris.data(), numTris * sizeof(Tri)); slurp("rays.bin", in.data(), numRays * sizeof(RayIn));
    std::vector<RayIn> primary;
    for (const RayIn& r : in) if (r.bounce == 0.0f) primary.push_back(r);
    std::vector<int32_t> pixels(2 * primary.size());
    slurp("pixels.bin", pixels.data(), pixels.size() * sizeof(int32_t));
    for (int a = 0; a < 3; ++a) { gR0[a] = gM[a]; gR1[a] = gM[4 + a]; gR2[a] = gM[8 + a]; gEye[a] = gM[12 + a]; }
    // the model's frustum planes assume what the lists' dmin assumes: an orthonormal camera frame
    auto dot = [](const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    if (fabs(dot(gR0, gR1)) > 1e-5 || fabs(dot(gR0, gR2)) > 1e-5 || fabs(dot(gR1, gR2)) > 1e-5 || fabs(dot(gR0, gR0) - 1) > 1e-5 || fabs(dot(gR1, gR1) - 1) > 1e-5 || fabs(dot(gR2, gR2) - 1) > 1e-5)
    { fprintf(stderr, "the camera frame is not orthonormal\n"); return 1; }
    // every recorded primary ray starts at the eye (pinhole) -- and the check of the camera convention: its direction lies in its pixel's frustum
    size_t numLeaves = 0; for (size_t n = 0; n < numNodes; ++n) if (n != 1 && isLeaf((uint32_t)n)) numLeaves++;
    printf("benchmark frame %u x %u, antiAliasingSpread %.3g, tan(fov / 2) %.4f, aspect %.4f; %zu nodes, %zu leaves, %zu triangles; %zu recorded primary rays (%zu hit)\n",
           gW, gH, gSpread, gTan, gAspect, numNodes, numLeaves, numTris, primary.size(), (size_t)std::count_if(primary.begin(), primary.end(), [](const RayIn& r) { return r.dist < 1e30f; }));

    const std::vector<uint32_t> slots = buildSlotTable(gW, gH);
    const size_t numTiles = (slots.size() + 63u) / 64u;
    // tile of a pixel
    std::vector<uint32_t> tileOf((size_t)gW * gH, 0u);
    for (size_t s = 0; s < slots.size(); ++s) tileOf[(size_t)(slots[s] >> 16) * gW + (slots[s] & 0xFFFFu)] = (uint32_t)(s / 64u);
    std::vector<std::vector<uint32_t>> raysOfTile(numTiles);
    size_t outside = 0;
    for (size_t i = 0; i < primary.size(); ++i)
    {
        const int x = pixels[2 * i], y = pixels[2 * i + 1];
        raysOfTile[tileOf[(size_t)y * gW + x]].push_back((uint32_t)i);
        // convention check at m = 3 spread (the recorded passes' offsets are normal with sigma = spread: a few in a thousand may exceed it)
        const Frustum f = tileFrustum(x - 3.0 * gSpread, x + 3.0 * gSpread, (double)(gH - 1 - y) - 3.0 * gSpread, (double)(gH - 1 - y) + 3.0 * gSpread);
        const RayIn& r = primary[i];
        for (int k = 0; k < 4; ++k) if (f.n[k][0] * r.d[0] + f.n[k][1] * r.d[1] + f.n[k][2] * r.d[2] < 0.0) { outside++; break; }
    }
    printf("camera convention: %zu of %zu recorded primary directions lie outside their own pixel's frustum at m = 3 spread (expected: 0 -- a pass has ONE offset, and both recorded passes' lie within 3 sigma)\n", outside, primary.size());

    // (b)'s farthest hits do not depend on m: once
    std::vector<double> farthest(numTiles, 0.0);
    std::vector<int> bounds(4 * numTiles);
    for (size_t t = 0; t < numTiles; ++t)
    {
        int x0 = 1 << 30, x1 = -1, y0 = 1 << 30, y1 = -1;
        for (size_t s = 64 * t; s < std::min(slots.size(), 64 * t + 64); ++s)
        {
            const int x = (int)(slots[s] & 0xFFFFu), y = (int)(slots[s] >> 16);
            x0 = std::min(x0, x); x1 = std::max(x1, x); y0 = std::min(y0, y); y1 = std::max(y1, y);
            const double X = filmX(x), Y = filmY((double)(gH - 1 - y));
            double d[3]; for (int a = 0; a < 3; ++a) d[a] = gR0[a] * X + gR1[a] * Y + gR2[a];
            const double len = sqrt(dot(d, d)); for (int a = 0; a < 3; ++a) d[a] /= len;
            farthest[t] = std::max(farthest[t], traceClosest(gEye, d));
        }
        bounds[4 * t] = x0; bounds[4 * t + 1] = x1; bounds[4 * t + 2] = y0; bounds[4 * t + 3] = y1;
    }
    { size_t open = 0; for (double d : farthest) if (!(d < 1e30)) open++; printf("tiles: %zu, of which %zu hold a pixel-centre ray that hits nothing (their scan runs to the end of the list)\n", numTiles, open); }

    const double ms[3] = { 3.0 * gSpread, 0.0, 6.0 * gSpread };
    for (int mi = 0; mi < 3; ++mi)
    {
        const double m = ms[mi];
        Dist perRay, perTile, full, fullTris;
        size_t over[3] = { 0, 0, 0 };
        std::vector<std::pair<double, uint32_t>> list;
        std::vector<uint32_t> stack;
        for (size_t t = 0; t < numTiles; ++t)
        {
            const int x0 = bounds[4 * t], x1 = bounds[4 * t + 1], y0 = bounds[4 * t + 2], y1 = bounds[4 * t + 3];
            const Frustum f = tileFrustum(x0 - m, x1 + m, (double)(gH - 1 - y1) - m, (double)(gH - 1 - y0) + m);
            list.clear(); stack.clear();
            stack.push_back(gNodes[0].child); stack.push_back(gNodes[0].child + 1u);
            double tris = 0;
            while (!stack.empty())
            {
                const uint32_t n = stack.back(); stack.pop_back();
                if (!boxTouches(f, gNodes[n].mn, gNodes[n].mx)) continue;
                if (isLeaf(n)) { list.push_back({ eyeDistance(gNodes[n].mn, gNodes[n].mx), n }); tris += gNodes[n].leaves & 0x3FFFFFFFu; }
                else { stack.push_back(gNodes[n].child); stack.push_back(gNodes[n].child + 1u); }
            }
            std::sort(list.begin(), list.end());
            full.add((double)list.size()); fullTris.add(tris);
            if (list.size() > 32) over[0]++;
            if (list.size() > 48) over[1]++;
            if (list.size() > 64) over[2]++;
            auto upTo = [&](double dist) { size_t k = 0; while (k < list.size() && list[k].first < dist) ++k; return (double)k; };
            for (uint32_t i : raysOfTile[t]) if (primary[i].dist < 1e30f) perRay.add(upTo(primary[i].dist));
            perTile.add(upTo(farthest[t]));
        }
        printf("\nm = %.2f pixels (%s)\n", m, mi == 0 ? "3 x antiAliasingSpread: THE GATE'S CASE" : (mi == 1 ? "no sample offset: the tile's own pixels" : "6 x antiAliasingSpread"));
        perRay.print("(a) list entries in front of a recorded ray's first hit");
        perTile.print("(b) list entries in front of the tile's FARTHEST first hit (the scan)");
        full.print("(c) the whole list (leaves)");
        fullTris.print("    the whole list (triangles)");
        printf("    tiles whose whole list exceeds K = 32 / 48 / 64: %.2f %% / %.2f %% / %.2f %%\n", 100.0 * over[0] / numTiles, 100.0 * over[1] / numTiles, 100.0 * over[2] / numTiles);
    }
    return 0;
}
