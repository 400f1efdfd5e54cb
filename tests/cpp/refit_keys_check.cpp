// refit_keys_check.cpp -- the float keys of rt_refit_keys.h held to their contract on the CPU (k_refit_check reduces a mesh's box through them with integer
// atomics): strictly monotone, a round trip to the bit, and a reduction by keys equal to the `a < b ? a : b` fold of the floats wherever no zero is involved.
// A program of its own: g++ -std=c++17 refit_keys_check.cpp && ./a.out      (prints "refit keys: ok", exit status 0)
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <random>
#include <vector>

#include "../../raytracer_amd/csrc/rt_refit_keys.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint32_t bitsOf(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float floatOf(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

int main()
{
    static_assert(sizeof(RefitCheckRecord) == 32, "RefitCheckRecord");
    // the landmarks, in the floats' order: each key strictly above the one before it, each a round trip
    const float landmarks[] = { -INFINITY, -FLT_MAX, -1.0e10f, -1.0f, -FLT_MIN, -floatOf(0x007FFFFFu), -floatOf(1u), -0.0f, 0.0f, floatOf(1u), floatOf(0x007FFFFFu),
                                FLT_MIN, 1.0f, 1.0e10f, FLT_MAX, INFINITY };
    const size_t numLandmarks = sizeof(landmarks) / sizeof(landmarks[0]);
    for (size_t i = 0; i < numLandmarks; ++i)
    {
        CHECK(bitsOf(refitUnkey(refitKey(landmarks[i]))) == bitsOf(landmarks[i]), "landmark %zu (%g) does not round-trip", i, landmarks[i]);
        if (i) CHECK(refitKey(landmarks[i - 1]) < refitKey(landmarks[i]), "landmarks %zu and %zu: keys %08x, %08x", i - 1, i, refitKey(landmarks[i - 1]), refitKey(landmarks[i]));
        CHECK(refitKey(landmarks[i]) > RT_REFIT_KEY_LOWEST && refitKey(landmarks[i]) < RT_REFIT_KEY_HIGHEST, "landmark %zu meets an identity", i);
        CHECK(refitBitsFinite(bitsOf(landmarks[i])) == (bool)isfinite(landmarks[i]), "landmark %zu: finite", i);
    }
    CHECK(!refitBitsFinite(bitsOf(NAN)) && !refitBitsFinite(0xFFC00001u) && !refitBitsFinite(0x7F800001u), "a NaN passes for finite");
    // neighbours: the next float up has the next key up, across the whole line (every 2^12-th pair, and all pairs around zero and the infinities)
    auto nextUp = [](float f) { return nextafterf(f, INFINITY); };
    for (uint64_t u = 0; u < 0x7F800000u; u += (u < 4096u || u > 0x7F800000u - 4096u) ? 1u : 4093u)
    {
        const float p = floatOf((uint32_t)u), n = -p;
        CHECK(refitKey(nextUp(p)) == refitKey(p) + 1u, "+%08x", (uint32_t)u);
        if (u) CHECK(refitKey(nextUp(n)) == refitKey(n) + 1u, "-%08x", (uint32_t)u);
        CHECK(bitsOf(refitUnkey(refitKey(p))) == bitsOf(p) && bitsOf(refitUnkey(refitKey(n))) == bitsOf(n), "round trip %08x", (uint32_t)u);
    }
    CHECK(refitKey(0.0f) == refitKey(-0.0f) + 1u, "the zeros are not neighbours");
    // a random sweep over all finite bit patterns: the order of the keys is the order of the floats, and the zeros apart
    std::mt19937 rng(20240611u);
    auto randomFinite = [&]() { uint32_t u; do u = rng(); while (!refitBitsFinite(u)); return floatOf(u); };
    for (int i = 0; i < 2000000; ++i)
    {
        const float a = randomFinite(), b = randomFinite();
        CHECK(bitsOf(refitUnkey(refitKey(a))) == bitsOf(a), "round trip %08x", bitsOf(a));
        if (a < b) CHECK(refitKey(a) < refitKey(b), "%g < %g", a, b);
        if (a > b) CHECK(refitKey(a) > refitKey(b), "%g > %g", a, b);
        if (a == b && bitsOf(a) == bitsOf(b)) CHECK(refitKey(a) == refitKey(b), "%g == %g", a, b);
    }
    // reductions: random arrays, a few ranges of magnitude, duplicates on purpose; by keys in a shuffled order against the fold of the floats in the given one
    for (int round = 0; round < 2000; ++round)
    {
        const size_t n = 1u + rng() % 300u;
        const int kind = round % 4;
        std::vector<float> v(n);
        for (float& x : v)
        {
            if (kind == 0) x = randomFinite();
            else if (kind == 1) x = (float)((int)(rng() % 2001u) - 1000) * 0.001f + 0.0005f;     // about a unit across, never zero
            else if (kind == 2) x = floatOf((rng() & 0x807FFFFFu) | (rng() % 3u ? 0u : 0x00800000u)); // denormals, zeros of both signs and the smallest normals
            else x = (float)((int)(rng() % 7u) - 3);                                             // small integers: many duplicates, zeros among them
        }
        float lo = v[0], hi = v[0];
        for (size_t i = 1; i < n; ++i) { lo = lo < v[i] ? lo : v[i]; hi = hi > v[i] ? hi : v[i]; }     // the fold as the host and refitMinDev / refitMaxDev write it
        std::vector<float> shuffled(v);
        std::shuffle(shuffled.begin(), shuffled.end(), rng);
        uint32_t klo = RT_REFIT_KEY_HIGHEST, khi = RT_REFIT_KEY_LOWEST;
        for (const float x : shuffled) { klo = std::min(klo, refitKey(x)); khi = std::max(khi, refitKey(x)); }
        const float glo = refitUnkey(klo), ghi = refitUnkey(khi);
        CHECK(glo == lo && ghi == hi, "round %d: values differ (%g %g against %g %g)", round, glo, ghi, lo, hi);       // as values, always
        if (lo != 0.0f) CHECK(bitsOf(glo) == bitsOf(lo), "round %d: min bits %08x against %08x", round, bitsOf(glo), bitsOf(lo));
        if (hi != 0.0f) CHECK(bitsOf(ghi) == bitsOf(hi), "round %d: max bits %08x against %08x", round, bitsOf(ghi), bitsOf(hi));
        // a zero bound: the keys' choice is the fixed one, -0 for a minimum and +0 for a maximum where both are there
        if (lo == 0.0f) CHECK(bitsOf(glo) == (std::count_if(v.begin(), v.end(), [](float x) { return bitsOf(x) == 0x80000000u; }) ? 0x80000000u : 0u), "round %d: zero min", round);
        if (hi == 0.0f) CHECK(bitsOf(ghi) == (std::count_if(v.begin(), v.end(), [](float x) { return bitsOf(x) == 0u; }) ? 0u : 0x80000000u), "round %d: zero max", round);
    }
    if (failures) { printf("refit keys: %d FAILED\n", failures); return 1; }
    printf("refit keys: ok\n");
    return 0;
}
