// oracle/ref_harness/kat_edges.inl -- part of kat_gen.cpp (included before main): genEdges().
//
// The interior generators above draw their inputs from the inside of ordinary ranges.  genEdges() writes one more KAT1 file per function id
// into tests/golden/edges/, with the name, function id and strides of its interior sibling, from EXPLICIT bit patterns: the value a comparison
// of the reference tests against, that value's two float neighbours (nextafterf both ways: "around"), signed zeros, denormals, infinities and
// NaN.  Every record is produced by the same reference function the interior generator calls.  Where a threshold is the outcome of arithmetic
// (total internal reflection, the sphere light's FLT_MAX pdf, a BSDF's reflection probability), the generator finds the input at which the
// REFERENCE's own result changes -- by calling it -- and writes that input with its neighbours.  Each list is followed by at most 64 seeded
// records that mix the specials.  tests/golden/README.md describes the layout, the specials and the one exclusion class.
#include <sys/stat.h>

typedef std::vector<float> Floats;

static float ulpUp(float v) { return nextafterf(v, INFINITY); }
static float ulpDown(float v) { return nextafterf(v, -INFINITY); }
static void addAround(Floats& l, float v) { l.push_back(ulpDown(v)); l.push_back(v); l.push_back(ulpUp(v)); }
static const float kNaN = bitsf(0x7FC00000u), kInf = bitsf(0x7F800000u), kDenormal = bitsf(1u);

// the two ends of what GenericSampler::GetFloat returns and the values at which sampling code folds
static Floats unitSpecials() { return { 0.0f, FLT_MIN, 5.9604644775390625e-8f /* 2^-24 */, 0.25f, ulpDown(0.5f), 0.5f, ulpUp(0.5f), 0.75f, 0.99999994f }; }
// cosines and direction components: +-0, +-1 and the inner neighbour, +-{BSDF::CosEpsilon, FLT_EPSILON, RT_EPSILON} with both neighbours
static Floats cosineSpecials()
{
    Floats l;
    for (float s : { 1.0f, -1.0f })
    {
        l.push_back(s * 0.0f); l.push_back(s); l.push_back(s * ulpDown(1.0f));
        for (float t : { BSDF::CosEpsilon, FLT_EPSILON, RT_EPSILON }) { l.push_back(s * ulpDown(t)); l.push_back(s * t); l.push_back(s * ulpUp(t)); }
    }
    return l;
}
static Floats realSpecials() { return { 0.0f, -0.0f, kDenormal, -kDenormal, FLT_MIN, -FLT_MIN, 1.0f, -1.0f, FLT_MAX, -FLT_MAX, kInf, -kInf, kNaN }; }
static float pick(Lcg& g, const Floats& l) { return l[g.u32() % l.size()]; }

// a direction that carries exactly this z; the other two components are chosen so that the length rounds to 1
static Vector4 dirWithZ(float z, double phi = 0.7)
{
    const double s = sqrt(std::max(0.0, 1.0 - (double)z * (double)z));
    return Vector4((float)(s * cos(phi)), (float)(s * sin(phi)), z, 0.0f);
}

// the smallest float in (lo, hi] at which pred holds, for a pred that is false at lo and true at hi (both positive, lo < hi)
static float firstTrue(float lo, float hi, const std::function<bool(float)>& pred)
{
    if (pred(lo) || !pred(hi)) { fprintf(stderr, "genEdges: threshold search has no bracket in [%g, %g]\n", lo, hi); exit(1); }
    uint32_t a = fbits(lo), b = fbits(hi);
    while (b - a > 1u) { const uint32_t m = a + (b - a) / 2u; if (pred(bitsf(m))) b = m; else a = m; }
    return bitsf(b);
}
static void addNeighbourhood(Floats& l, float v, int radius) { float lo = v; for (int i = 0; i < radius; ++i) lo = ulpDown(lo); for (int i = 0; i <= 2 * radius; ++i) { l.push_back(lo); lo = ulpUp(lo); } }

struct EdgeWriter : KatWriter
{
    EdgeWriter(const char* n, uint32_t f, uint32_t is, uint32_t os) : KatWriter((std::string("edges/") + n).c_str(), f, is, os) {}
    void finish()
    {
        const size_t n = in.size() / inStride;
        if (n > 2048u || out.size() / outStride != n) { fprintf(stderr, "genEdges: %s has %zu records (limit 2048)\n", name.c_str(), n); exit(1); }
        save();
    }
};

// _mm_rsqrt_ps returns +inf for a denormal operand where 1 / sqrt does not: a FastNormalize3 of a vector whose squared length is positive and
// below FLT_MIN is decided by that instruction, not by the algorithm.  Such records are not written (the one exclusion class; counted and printed).
static bool rsqrtOperandDenormal(const Vector4& v) { const float l = v.SqrLength3(); return l > 0.0f && l < FLT_MIN; }
static const uint32_t kMaxRedraws = 16;

// ---- math --------------------------------------------------------------------------------------------
static void edgeMath()
{
    const Floats unit = unitSpecials(), cosines = cosineSpecials(), reals = realSpecials();
    {
        EdgeWriter k("math_sin_lane", KAT_SIN_LANE, 1, 1), k2("math_sincos", KAT_SINCOS, 1, 4);
        Floats xs = reals;
        for (float s : { 1.0f, -1.0f }) { addAround(xs, s * 0.5f * RT_PI); addAround(xs, s * RT_PI); addAround(xs, s * RT_2PI); addAround(xs, s * 1.5f * RT_PI); }
        for (int e = 1; e <= 20; ++e) { xs.push_back((float)(1 << e) * RT_PI); xs.push_back(-(float)(1 << e) * RT_PI); xs.push_back(((float)(1 << e) + 1.0f) * RT_PI); }
        for (float big : { 2147483648.0f * RT_PI, -2147483648.0f * RT_PI, 4294967296.0f * RT_PI * 1.5f, 6.0e9f, -6.0e9f, 6746518528.0f /* 2^31 * pi rounded down */, 1.0e20f,
                            1.5707963e10f /* quotient 5e9: beyond int32 and no multiple of 2^31 */, -1.5707963e10f, 1.0e10f, -1.0e10f, 3.0e10f, 2.0e10f, 7.0e9f, -7.0e9f, 9.0e9f, 1.0e15f, -1.0e15f })
            xs.push_back(big);
        Lcg g(201);
        for (int i = 0; i < 64; ++i) xs.push_back((i & 1) ? g.range(-1.0e7f, 1.0e7f) : pick(g, xs) * g.range(0.5f, 2.0f));
        for (float x : xs)
        {
            k.addIn()[0] = x; k.addOut()[0] = Sin(Vector4(x)).x;
            k2.addIn()[0] = x; put4(k2.addOut(), SinCos(x));
        }
        k.finish(); k2.finish();
    }
    {
        EdgeWriter k("math_fastlog", KAT_FASTLOG, 1, 1);
        Floats xs = reals;
        for (uint32_t b : { 0x3f2aaaaau, 0x3f2aaaabu, 0x3f2aaaacu, 0x00000002u, 0x007fffffu, 0x00800001u, 0x7f7ffffeu, 0x3f000000u, 0x40000000u }) xs.push_back(bitsf(b));
        addAround(xs, 1.0f); addAround(xs, RT_E);
        for (float u : unit) xs.push_back(u);
        Lcg g(203);
        // any exponent (zero and all-ones included: denormals, inf, NaN) over the mantissas next to the fold
        for (int i = 0; i < 64; ++i) xs.push_back(bitsf((g.u32() & 0x7F800000u) | (fbits(pick(g, { bitsf(0x3f2aaaaau), bitsf(0x3f2aaaabu), bitsf(0x3f2aaaacu), 1.0f, ulpDown(2.0f) })) & 0x007FFFFFu)));
        for (float x : xs) { k.addIn()[0] = x; k.addOut()[0] = FastLog(x); }
        k.finish();
    }
    {
        EdgeWriter k("math_float_normal2", KAT_FLOAT_NORMAL2, 2, 4);
        for (float a : unit) for (float b : unit) { float* in = k.addIn(); in[0] = a; in[1] = b; put4(k.addOut(), SamplingHelpers::GetFloatNormal2(Float2(a, b))); }
        for (float a : { ulpDown(1.0f), bitsf(0x3f2aaaaau), bitsf(0x3f2aaaabu), bitsf(0x3f2aaaacu), kDenormal }) for (float b : { 0.0f, 0.125f, 0.5f, 0.99999994f })
        { float* in = k.addIn(); in[0] = a; in[1] = b; put4(k.addOut(), SamplingHelpers::GetFloatNormal2(Float2(a, b))); }
        k.finish();
    }
    {
        EdgeWriter k("math_fastacos", KAT_FASTACOS, 1, 1);
        Floats xs = cosines;
        for (float x : { ulpUp(1.0f), -ulpUp(1.0f), 2.0f, -2.0f, kNaN, kInf, -kInf, kDenormal, -kDenormal, FLT_MIN, -FLT_MIN, 0.5f, -0.5f, ulpDown(ulpDown(1.0f)), -ulpDown(ulpDown(1.0f)) }) xs.push_back(x);
        Lcg g(204);
        for (int i = 0; i < 64; ++i) xs.push_back(pick(g, cosines) * ((i & 1) ? 1.0f : g.range(0.5f, 1.0f)));
        for (float x : xs) { k.addIn()[0] = x; k.addOut()[0] = FastACos(x); }
        k.finish();
    }
    {
        EdgeWriter k("math_fastatan2", KAT_FASTATAN2, 2, 1);
        std::vector<std::array<float, 2>> xs;
        for (float a : reals) for (float b : reals) xs.push_back({ a, b });          // (+-0, +-0), each axis in both signs, inf, NaN, denormal over FLT_MAX
        for (float m : { 1.0f, 0.3f, 1.0e-30f, 1.0e30f }) for (float sa : { 1.0f, -1.0f }) for (float sb : { 1.0f, -1.0f })
            for (float n : { ulpDown(m), m, ulpUp(m) }) { xs.push_back({ sa * m, sb * n }); xs.push_back({ sa * n, sb * m }); }   // |y| = |x| +- ulp
        Lcg g(205);
        for (int i = 0; i < 64; ++i) xs.push_back({ (i & 1) ? pick(g, reals) : g.range(-2.0f, 2.0f), (i & 2) ? pick(g, reals) : g.range(-2.0f, 2.0f) });
        for (const auto& x : xs) { float* in = k.addIn(); in[0] = x[0]; in[1] = x[1]; k.addOut()[0] = FastATan2(x[0], x[1]); }
        k.finish();
    }
    {
        EdgeWriter kh("math_hemisphere_cos", KAT_HEMISPHERE_COS, 2, 4), ks("math_sphere", KAT_SPHERE, 2, 4), kc("math_circle", KAT_CIRCLE, 2, 4);
        for (float a : unit) for (float b : unit)
        {
            float* in = kh.addIn(); in[0] = a; in[1] = b; put4(kh.addOut(), SamplingHelpers::GetHemishpereCos(Float2(a, b)));
            in = ks.addIn(); in[0] = a; in[1] = b; put4(ks.addOut(), SamplingHelpers::GetSphere(Float2(a, b)));
            in = kc.addIn(); in[0] = a; in[1] = b; put4(kc.addOut(), SamplingHelpers::GetCircle(Float2(a, b)));
        }
        kh.finish(); ks.finish(); kc.finish();
    }
    {
        EdgeWriter k("math_ortho_basis", KAT_ORTHO_BASIS, 4, 8);
        std::vector<Vector4> ns;
        for (float z : { 1.0f, -1.0f }) for (float x : { 0.0f, -0.0f }) for (float y : { 0.0f, -0.0f }) ns.push_back(Vector4(x, y, z, 0.0f));
        for (float z : { 0.0f, -0.0f }) for (float s : { 1.0f, -1.0f }) { ns.push_back(Vector4(s, 0.0f, z, 0.0f)); ns.push_back(Vector4(0.0f, s, z, 0.0f)); ns.push_back(Vector4(s, -0.0f, z, 0.0f)); }
        for (float z : { 0.0f, -0.0f }) ns.push_back(Vector4(0.0f, 0.0f, z, 0.0f));
        for (float z : cosines) { ns.push_back(dirWithZ(z)); ns.push_back(dirWithZ(z, 0.0)); ns.push_back(dirWithZ(z, 3.9)); }
        for (float z : { ulpUp(-1.0f), ulpUp(ulpUp(-1.0f)), -0.99999f, ulpDown(1.0f) }) { ns.push_back(dirWithZ(z, 0.0)); ns.push_back(dirWithZ(z, 1.5707963267948966)); ns.push_back(Vector4(0.0f, 0.0f, z, 0.0f)); }
        Lcg g(210);
        for (int i = 0; i < 64; ++i) ns.push_back(dirWithZ(pick(g, cosines), g.range(0.0f, 6.28f)));
        for (const Vector4& n : ns) { put4(k.addIn(), n); Vector4 u, v; BuildOrthonormalBasis(n, u, v); float* o = k.addOut(); put4(o, u); put4(o + 4, v); }
        k.finish();
    }
    {
        EdgeWriter k("math_fresnel_dielectric", KAT_FRESNEL_DIELECTRIC, 2, 1);
        const Floats etas = { 1.0f, ulpDown(1.0f), ulpUp(1.0f), 1.5f, 2.5f };
        std::vector<std::array<float, 2>> xs;
        for (float c : cosines) for (float e : etas) xs.push_back({ c, e });
        // total internal reflection: g = eta^2 (1 - c^2) against 1.  NdV < 0 keeps eta, NdV > 0 inverts it (so an eta below 1 reflects totally from above)
        for (float e : { 1.5f, 2.5f, ulpUp(1.0f) })
        {
            const float below = firstTrue(1.0e-4f, 0.99999f, [&](float c) { return FresnelDielectric(-c, e) < 1.0f; });
            Floats cs; addNeighbourhood(cs, below, 3);
            for (float c : cs) { xs.push_back({ -c, e }); xs.push_back({ c, 1.0f / e }); xs.push_back({ c, e }); }
        }
        Lcg g(211);
        for (int i = 0; i < 64; ++i) xs.push_back({ (i & 1) ? pick(g, cosines) : g.range(-1.0f, 1.0f), (i & 2) ? pick(g, etas) : g.range(0.4f, 2.5f) });
        for (const auto& x : xs) { float* in = k.addIn(); in[0] = x[0]; in[1] = x[1]; k.addOut()[0] = FresnelDielectric(x[0], x[1]); }
        k.finish();
    }
    {
        EdgeWriter k("math_fresnel_metal", KAT_FRESNEL_METAL, 3, 1);
        std::vector<std::array<float, 3>> xs;
        for (float c : cosines) for (float e : { 0.0f, 1.0f, 1.5f }) for (float kk : { 0.0f, 3.0f }) xs.push_back({ c, e, kk });
        Lcg g(212);
        for (int i = 0; i < 64; ++i) xs.push_back({ pick(g, cosines), (i & 1) ? 0.0f : g.range(0.0f, 3.0f), (i & 2) ? 0.0f : g.range(0.0f, 100.0f) });
        for (const auto& x : xs) { float* in = k.addIn(); in[0] = x[0]; in[1] = x[1]; in[2] = x[2]; k.addOut()[0] = FresnelMetal(x[0], x[1], x[2]); }
        k.finish();
    }
    {
        EdgeWriter k("math_refract3", KAT_REFRACT3, 9, 4), k2("math_reflect3", KAT_REFLECT3, 8, 4);
        struct Rec { Vector4 d, n; float eta; };
        std::vector<Rec> xs;
        const Floats etas = { 1.0f, ulpUp(1.0f), 1.5f, 1.0f / 1.5f };
        for (float c : cosines) for (float e : etas) { xs.push_back({ dirWithZ(c), VECTOR_Z, e }); xs.push_back({ dirWithZ(c, 2.0), -VECTOR_Z, e }); }
        // k = 1 - eta^2 (1 - NdotV^2) at 0: from above with eta > 1, from below with eta < 1
        for (float e : { 1.5f, 2.5f, ulpUp(1.0f) })
        {
            const float first = firstTrue(1.0e-4f, 0.99999f, [&](float c) { return Vector4::Refract3(dirWithZ(c), VECTOR_Z, e).SqrLength3() > 0.0f; });
            Floats cs; addNeighbourhood(cs, first, 3);
            for (float c : cs) { xs.push_back({ dirWithZ(c), VECTOR_Z, e }); xs.push_back({ dirWithZ(-c), VECTOR_Z, 1.0f / e }); xs.push_back({ dirWithZ(c, 0.0), VECTOR_Z, e }); }
        }
        Lcg g(213);
        for (int i = 0; i < 64; ++i) xs.push_back({ dirWithZ(pick(g, cosines), g.range(0.0f, 6.28f)), (i & 1) ? VECTOR_Z : g.dir(), pick(g, etas) });
        for (const Rec& r : xs)
        {
            float* in = k.addIn(); put4(in, r.d); put4(in + 4, r.n); in[8] = r.eta; put4(k.addOut(), Vector4::Refract3(r.d, r.n, r.eta));
            in = k2.addIn(); put4(in, r.d); put4(in + 4, r.n); put4(k2.addOut(), Vector4::Reflect3(r.d, r.n));
        }
        k.finish(); k2.finish();
    }
}

// ---- geometry ----------------------------------------------------------------------------------------
static void edgeGeometry()
{
    const Floats reals = realSpecials();
    {
        EdgeWriter k("geom_make_ray", KAT_MAKE_RAY, 8, 12);
        std::vector<std::array<Vector4, 2>> xs;
        const Floats comps = { 0.0f, -0.0f, 1.0f, -1.0f, kDenormal, FLT_MIN, FLT_MAX, 0.5f };
        for (float x : comps) for (float y : { 0.0f, -0.0f, 1.0f }) for (float z : { 0.0f, -0.0f, -1.0f })
            for (const Vector4& o : { Vector4(0.0f, 0.0f, 0.0f, 0.0f), Vector4(1.0f, -2.0f, 3.0f, 0.0f), Vector4(-0.0f, kInf, kDenormal, 0.0f) })
                xs.push_back({ o, Vector4(x, y, z, 0.0f) });
        Lcg g(220);
        for (int i = 0; i < 64; ++i) xs.push_back({ Vector4(pick(g, reals), pick(g, reals), g.range(-10.0f, 10.0f), 0.0f), Vector4(pick(g, comps), pick(g, comps), pick(g, comps), 0.0f) });
        for (const auto& x : xs)
        {
            float* in = k.addIn(); put4(in, x[0]); put4(in + 4, x[1]);
            const Ray r(x[0], x[1]);
            float* out = k.addOut(); put4(out, r.dir); put4(out + 4, r.invDir); put4(out + 8, r.originDivDir);
        }
        k.finish();
    }
    // matrices: identity, a 90 degree rotation (exact zeros), scales of 2^-20 and 2^20, with and without a translation
    // (an array, not a std::vector: Matrix4 is aligned to 32 bytes, which operator new does not promise before C++17)
    Matrix4 mats[18]; int numMats = 0;
    {
        Matrix4 rot = Matrix4::Identity(); rot.rows[0] = Vector4(0.0f, 1.0f, 0.0f, 0.0f); rot.rows[1] = Vector4(-1.0f, 0.0f, 0.0f, 0.0f);
        Matrix4 rotx = Matrix4::Identity(); rotx.rows[1] = Vector4(0.0f, 0.0f, 1.0f, 0.0f); rotx.rows[2] = Vector4(0.0f, -1.0f, 0.0f, 0.0f);
        for (const Matrix4& base : { Matrix4::Identity(), rot, rotx })
            for (float s : { 1.0f, 9.5367431640625e-7f /* 2^-20 */, 1048576.0f /* 2^20 */ })
                for (const Vector4& t : { Vector4(0.0f, 0.0f, 0.0f, 1.0f), Vector4(1.0f, -2.0f, 3.0f, 1.0f) })
                { Matrix4 m = base; for (int r = 0; r < 3; ++r) m.rows[r] = m.rows[r] * s; m.rows[3] = t; mats[numMats++] = m; }
    }
    std::vector<Vector4> vecs = { Vector4(0.0f, 0.0f, 0.0f, 0.0f), Vector4(-0.0f, -0.0f, -0.0f, 0.0f), Vector4(1.0f, 0.0f, 0.0f, 0.0f), Vector4(0.0f, -1.0f, 0.0f, 0.0f), Vector4(0.0f, 0.0f, 1.0f, 0.0f),
        Vector4(1.0f, -2.0f, 3.0f, 0.0f), Vector4(FLT_MAX, 1.0f, -1.0f, 0.0f), Vector4(kDenormal, FLT_MIN, -kDenormal, 0.0f), Vector4(kInf, 0.0f, 1.0f, 0.0f), Vector4(1.0f, kNaN, 0.0f, 0.0f) };
    {
        EdgeWriter k("geom_transform_ray", KAT_TRANSFORM_RAY, 24, 16), kf("geom_fast_inverse", KAT_FAST_INVERSE, 16, 16), ks("geom_transform_scaled", KAT_TRANSFORM_SCALED, 20, 12);
        for (const Matrix4& m : mats)
        {
            putM(kf.addIn(), m); putM(kf.addOut(), m.FastInverseNoScale());
            for (const Vector4& v : vecs)
            {
                float* in = ks.addIn(); putM(in, m); put4(in + 16, v);
                float* out = ks.addOut(); put4(out, m.TransformPoint(v)); put4(out + 4, m.TransformVector(v)); put4(out + 8, m.FastInverseNoScale().TransformPoint(v));
            }
            for (const Vector4& d : { Vector4(1.0f, 0.0f, 0.0f, 0.0f), Vector4(0.0f, -1.0f, 0.0f, 0.0f), Vector4(0.0f, 0.0f, 1.0f, 0.0f), Vector4(-0.0f, 0.6f, 0.8f, 0.0f), dirWithZ(BSDF::CosEpsilon) })
                for (const Vector4& o : { vecs[0], vecs[5], vecs[7] })
                {
                    const Ray w(o, d);
                    float* in = k.addIn(); putM(in, m); put4(in + 16, w.origin); put4(in + 20, w.dir);
                    const Ray l = m.TransformRay_Unsafe(w);
                    float* out = k.addOut(); put4(out, l.origin); put4(out + 4, l.dir); put4(out + 8, l.invDir); put4(out + 12, l.originDivDir);
                }
        }
        k.finish(); kf.finish(); ks.finish();
    }
    {
        // in: transform[16], ray origin[4], ray direction[4], {distance, normal-mapped?, 0, 0}, local tangent[4], local normal[4], tangent-space normal of the map[4]
        EdgeWriter k("frame_compose", KAT_FRAME_COMPOSE, 40, 20);
        uint32_t redraws = 0;
        Lcg g(227);
        struct Rec { Vector4 tangent, normal, mapNormal; bool mapped; };
        std::vector<Rec> recs;
        for (int mapped = 0; mapped < 2; ++mapped)
        {
            recs.push_back({ VECTOR_X, VECTOR_Z, VECTOR_Z, mapped != 0 });                                  // tangent-space normal (0, 0, 1)
            // tangent parallel to normal: Orthogonalize gives 0 and Normalized3 0 / 0.  Without a normal map only: with one, FastNormalized3 hands Orthogonalize a
            // normal a little SHORTER than 1 (_mm_rsqrt_ps rounds 1 / sqrt(1) down), the difference survives and the reference gets a finite tangent out of the
            // instruction's error (tests/golden/README.md)
            if (!mapped) { recs.push_back({ VECTOR_Z, VECTOR_Z, VECTOR_Z, false }); recs.push_back({ -VECTOR_Z, VECTOR_Z, VECTOR_Z, false }); recs.push_back({ Vector4(0.0f, 0.6f, 0.8f, 0.0f), Vector4(0.0f, 0.6f, 0.8f, 0.0f), VECTOR_Z, false }); }
            recs.push_back({ VECTOR_X, VECTOR_Z, Vector4(0.0f, 0.0f, 0.0f, 0.0f), mapped != 0 });           // a zero map normal: rsqrt(0) = inf both ways
            recs.push_back({ Vector4(0.0f, 0.0f, 0.0f, 0.0f), VECTOR_Z, VECTOR_Z, mapped != 0 });           // a zero tangent
            recs.push_back({ VECTOR_X, Vector4(0.0f, 0.0f, 0.0f, 0.0f), VECTOR_Z, mapped != 0 });           // a zero normal
            recs.push_back({ Vector4(1.0f, -0.0f, 0.0f, 0.0f), Vector4(-0.0f, 0.0f, -1.0f, 0.0f), Vector4(0.6f, -0.0f, 0.8f, 0.0f), mapped != 0 });
            recs.push_back({ Vector4(0.6f, 0.0f, 0.8f, 0.0f), Vector4(0.0f, 1.0f, 0.0f, 0.0f), Vector4(-0.6f, 0.6f, 0.52915026f, 0.0f), mapped != 0 });
        }
        for (const Matrix4& m : mats) for (const Rec& r : recs)
        {
            Rec rec = r;
            for (uint32_t attempt = 0;; ++attempt)
            {
                const Ray ray(Vector4(1.0f, -2.0f, 3.0f, 0.0f), Vector4(0.0f, 0.6f, -0.8f, 0.0f));
                const float distance = 2.5f;
                const Matrix4 invTransform = m.FastInverseNoScale();
                const Vector4 worldPosition = ray.GetAtDistance(distance);
                const Vector4 localPosition = invTransform.TransformPoint(worldPosition);
                Vector4 localSpaceTangent = rec.tangent, localSpaceNormal = rec.normal;
                const Vector4 localSpaceBitangent = Vector4::Cross3(localSpaceTangent, localSpaceNormal);
                bool excluded = false;
                if (rec.mapped)
                {
                    Vector4 newNormal = localSpaceTangent * rec.mapNormal.x;
                    newNormal = Vector4::MulAndAdd(localSpaceBitangent, rec.mapNormal.y, newNormal);
                    newNormal = Vector4::MulAndAdd(localSpaceNormal, rec.mapNormal.z, newNormal);
                    excluded = rsqrtOperandDenormal(newNormal);
                    localSpaceNormal = newNormal.FastNormalized3();
                }
                if (excluded)
                {
                    if (attempt >= kMaxRedraws || ++redraws > kMaxRedraws) { fprintf(stderr, "genEdges: frame_compose needs more than %u redraws\n", kMaxRedraws); exit(1); }
                    rec.mapNormal = Vector4(g.range(-0.6f, 0.6f), g.range(-0.6f, 0.6f), 0.7f, 0.0f);
                    continue;
                }
                localSpaceTangent = Vector4::Orthogonalize(localSpaceTangent, localSpaceNormal).Normalized3();
                Vector4 frame[4];
                frame[2] = m.TransformVector(localSpaceNormal);
                frame[0] = m.TransformVector(localSpaceTangent);
                frame[1] = Vector4::Cross3(frame[0], frame[2]);
                frame[3] = worldPosition;
                float* in = k.addIn(); putM(in, m); put4(in + 16, ray.origin); put4(in + 20, ray.dir); in[24] = distance; in[25] = rec.mapped ? 1.0f : 0.0f;
                put4(in + 28, rec.tangent); put4(in + 32, rec.normal); put4(in + 36, rec.mapNormal);
                float* out = k.addOut(); put4(out, localPosition); for (int r2 = 0; r2 < 4; ++r2) put4(out + 4 + 4 * r2, frame[r2]);
                break;
            }
        }
        printf("edges/frame_compose.kat: %u records redrawn (squared length of a FastNormalize3 operand denormal)\n", redraws);
        k.finish();
    }
    {
        EdgeWriter k("geom_box_ray", KAT_BOX_RAY, 14, 2), k2("geom_box_ray_twosided", KAT_BOX_RAY_TWOSIDED, 14, 3);
        struct Rec { Vector4 o, d, bmin, bmax; };
        std::vector<Rec> xs;
        const Vector4 lo(-1.0f, -2.0f, -3.0f, 0.0f), hi(1.0f, 2.0f, 3.0f, 0.0f);
        std::vector<std::array<Vector4, 2>> boxes = { { lo, hi },
            { Vector4(1.0f, -2.0f, -3.0f, 0.0f), hi }, { Vector4(1.0f, 2.0f, -3.0f, 0.0f), hi }, { hi, hi },       // flat on one, two and three axes
            { Vector4(0.0f, 0.0f, 0.0f, 0.0f), Vector4(0.0f, 1.0f, 1.0f, 0.0f) }, { Vector4(-0.0f, -0.0f, -0.0f, 0.0f), Vector4(0.0f, 0.0f, 0.0f, 0.0f) } };
        std::vector<Vector4> dirs;
        for (float x : { 0.0f, -0.0f, 1.0f, -1.0f }) for (float y : { 0.0f, -0.0f, 1.0f, -1.0f }) for (float z : { 0.0f, -0.0f, 1.0f, -1.0f }) dirs.push_back(Vector4(x, y, z, 0.0f));
        std::vector<Vector4> origins = { Vector4(0.0f, 0.0f, 0.0f, 0.0f), Vector4(1.0f, 0.0f, 0.0f, 0.0f) /* on a face */, Vector4(1.0f, 2.0f, 0.0f, 0.0f) /* an edge */, hi /* a corner */, lo,
            Vector4(-5.0f, 0.0f, 0.0f, 0.0f), Vector4(-5.0f, 2.0f, 0.0f, 0.0f) /* inside a face plane */, Vector4(-5.0f, 2.0f, 3.0f, 0.0f), Vector4(ulpUp(1.0f), 0.0f, 0.0f, 0.0f), Vector4(ulpDown(1.0f), 0.0f, 0.0f, 0.0f),
            Vector4(-5.0f, ulpUp(2.0f), 0.0f, 0.0f), Vector4(-5.0f, ulpDown(2.0f), 0.0f, 0.0f), Vector4(-3.0f, -4.0f, -5.0f, 0.0f) /* through the corner along (1, 1, 1): near equals far */, Vector4(3.0f, 0.0f, 5.0f, 0.0f) };
        for (size_t b = 0; b < boxes.size(); ++b) for (const Vector4& o : origins) for (const Vector4& d : dirs)
        {
            if (b > 0 && ((&d - dirs.data()) % 3 != 0 || (&o - origins.data()) > 7)) continue;    // the full cross only for the first box: stay under the record limit
            xs.push_back({ o, d, boxes[b][0], boxes[b][1] });
        }
        Lcg g(223);
        for (int i = 0; i < 64; ++i) { const auto& bx = boxes[g.u32() % boxes.size()]; xs.push_back({ Vector4(pick(g, reals), g.range(-4.0f, 4.0f), pick(g, { -3.0f, 3.0f, 0.0f, -0.0f }), 0.0f), dirs[g.u32() % dirs.size()] + ((i & 1) ? g.vec(-1.0f, 1.0f) : Vector4(0.0f, 0.0f, 0.0f, 0.0f)), bx[0], bx[1] }); }
        for (const Rec& x : xs)
        {
            Box box(x.bmin, x.bmax); box.min.w = 0.0f; box.max.w = 0.0f;
            const Ray r(x.o, x.d);
            float* in = k.addIn(); put4(in, x.o); put4(in + 4, x.d); in[8] = box.min.x; in[9] = box.min.y; in[10] = box.min.z; in[11] = box.max.x; in[12] = box.max.y; in[13] = box.max.z;
            float dist = 0.0f; const bool h = Intersect_BoxRay(r, box, dist);
            float* out = k.addOut(); out[0] = bitsf(h ? 1u : 0u); out[1] = dist;
            float* in2 = k2.addIn(); memcpy(in2, in, 14 * 4);
            float nd = 0.0f, fd = 0.0f; const bool h2 = Intersect_BoxRay_TwoSided(r, box, nd, fd);
            float* out2 = k2.addOut(); out2[0] = bitsf(h2 ? 1u : 0u); out2[1] = nd; out2[2] = fd;
        }
        k.finish(); k2.finish();
    }
    {
        EdgeWriter k("geom_triangle_ray", KAT_TRIANGLE_RAY, 17, 4);
        struct Rec { Vector4 o, d, v0, v1, v2; };
        std::vector<Rec> xs;
        const Vector4 a(0.0f, 0.0f, 0.0f, 0.0f), b(2.0f, 0.0f, 0.0f, 0.0f), c(0.0f, 2.0f, 0.0f, 0.0f);
        const Vector4 a2(1.0f, -2.0f, 3.0f, 0.0f), b2(2.5f, -1.0f, 3.5f, 0.0f), c2(0.5f, 0.25f, 2.0f, 0.0f);
        const std::vector<std::array<Vector4, 3>> tris = { { a, b, c }, { a2, b2, c2 },
            { a, b, Vector4(4.0f, 0.0f, 0.0f, 0.0f) } /* edge1 parallel to edge2 */, { a, a, c } /* a zero edge */, { a2, a2, a2 } };
        for (const auto& t : tris)
        {
            const Vector4 e1 = t[1] - t[0], e2 = t[2] - t[0];
            std::vector<Vector4> targets = { t[0], t[1], t[2], t[0] + e1 * 0.5f, t[0] + e2 * 0.5f, t[0] + e1 * 0.5f + e2 * 0.5f, t[0] + e1 * 0.25f + e2 * 0.25f, t[0] + e1 * 1.5f, t[0] - e2 * 0.5f,
                t[0] + e1 * ulpDown(0.5f) + e2 * 0.5f, t[0] + e1 * ulpUp(0.5f) + e2 * 0.5f, t[0] + e1 * kDenormal + e2 * 0.25f, t[0] + e1 * 0.25f + e2 * FLT_MIN };
            const std::vector<Vector4> origins = { Vector4(0.5f, 0.5f, 4.0f, 0.0f), Vector4(0.5f, 0.5f, -4.0f, 0.0f), Vector4(-3.0f, 1.0f, 5.0f, 0.0f) };
            for (const Vector4& o : origins) for (const Vector4& target : targets) xs.push_back({ o, target - o, t[0], t[1], t[2] });
            // in the triangle's plane: along each edge, from a vertex, and through the interior
            xs.push_back({ t[0] - e1, e1, t[0], t[1], t[2] }); xs.push_back({ t[0] - e2, e2, t[0], t[1], t[2] }); xs.push_back({ t[1] - (t[2] - t[1]), t[2] - t[1], t[0], t[1], t[2] });
            xs.push_back({ t[0], e1 + e2, t[0], t[1], t[2] }); xs.push_back({ t[0] - e1 - e2, e1 + e2, t[0], t[1], t[2] });
            // t = 0: the origin on the triangle, leaving along the normal and against it; and a zero direction
            const Vector4 inside = t[0] + e1 * 0.25f + e2 * 0.25f, n = Vector4::Cross3(e1, e2);
            xs.push_back({ inside, n, t[0], t[1], t[2] }); xs.push_back({ inside, -n, t[0], t[1], t[2] }); xs.push_back({ inside + n, Vector4(0.0f, 0.0f, 0.0f, 0.0f), t[0], t[1], t[2] });
            xs.push_back({ inside + n * kDenormal, -n, t[0], t[1], t[2] }); xs.push_back({ t[0], n, t[0], t[1], t[2] });
        }
        Lcg g(224);
        for (int i = 0; i < 64; ++i) { const auto& t = tris[g.u32() % tris.size()]; xs.push_back({ Vector4(pick(g, reals), g.range(-3.0f, 3.0f), 4.0f, 0.0f), Vector4(g.range(-1.0f, 1.0f), pick(g, { 0.0f, -0.0f, 1.0f, kDenormal }), -1.0f, 0.0f), t[0], t[1], t[2] }); }
        for (const Rec& x : xs)
        {
            const ProcessedTriangle tri(x.v0, x.v1, x.v2);
            const Ray r(x.o, x.d);
            float* in = k.addIn(); put4(in, x.o); put4(in + 4, x.d);
            in[8] = tri.v0.x; in[9] = tri.v0.y; in[10] = tri.v0.z; in[11] = tri.edge1.x; in[12] = tri.edge1.y; in[13] = tri.edge1.z; in[14] = tri.edge2.x; in[15] = tri.edge2.y; in[16] = tri.edge2.z;
            float u = 0, v = 0, t = 0;
            const bool h = Intersect_TriangleRay(r, Vector4(tri.v0), Vector4(tri.edge1), Vector4(tri.edge2), u, v, t);
            float* out = k.addOut(); out[0] = bitsf(h ? 1u : 0u); out[1] = u; out[2] = v; out[3] = t;
        }
        k.finish();
    }
}

// ---- shapes ------------------------------------------------------------------------------------------
struct EdgeShape
{
    uint32_t kind; float p[4], p2[4]; std::unique_ptr<IShape> shape;
};
static EdgeShape edgeSphere(float r) { EdgeShape s{ RT_SHAPE_SPHERE, { r, 1.0f / r, 0, 0 }, { 0, 0, 0, 0 }, std::make_unique<SphereShape>(r) }; return s; }
static EdgeShape edgeBox(float x, float y, float z)
{
    const Vector4 size(x, y, z, 0.0f), inv = VECTOR_ONE / size;
    EdgeShape s{ RT_SHAPE_BOX, { x, y, z, 0 }, { inv.x, inv.y, inv.z, 0 }, std::make_unique<BoxShape>(size) }; return s;
}
static EdgeShape edgeRect(float x, float y, float tx = 1.0f, float ty = 2.0f) { EdgeShape s{ RT_SHAPE_RECT, { x, y, tx, ty }, { 0, 0, 0, 0 }, std::make_unique<RectShape>(Float2(x, y), Float2(tx, ty)) }; return s; }

static void emitIntersect(KatWriter& ki, const EdgeShape& s, const Vector4& o, const Vector4& d)
{
    const Ray r(o, d);
    float* in = ki.addIn(); in[0] = bitsf(s.kind); memcpy(in + 1, s.p, 16); put4(in + 5, o); put4(in + 9, d);
    ShapeIntersection si; si.nearDist = 0.0f; si.farDist = 0.0f;
    const bool h = s.shape->Intersect(r, si);
    float* out = ki.addOut(); out[0] = bitsf(h ? 1u : 0u); out[1] = h ? si.nearDist : 0.0f; out[2] = h ? si.farDist : 0.0f; out[3] = bitsf(si.subObjectId);
}
static bool emitSample(KatWriter& ks, const EdgeShape& s, const Vector4& ref, const Float3& u, ShapeSampleResult* result = nullptr)
{
    float* in = ks.addIn(); in[0] = bitsf(s.kind); memcpy(in + 1, s.p, 16); put4(in + 5, ref); in[9] = u.x; in[10] = u.y; in[11] = u.z;
    ShapeSampleResult sr;
    const bool h = s.shape->Sample(ref, u, sr);
    float* out = ks.addOut(); out[0] = bitsf(h ? 1u : 0u);
    if (h) { put4(out + 1, sr.direction); out[5] = sr.distance; out[6] = sr.pdf; out[7] = sr.cosAtSurface; }
    if (result) *result = sr;
    return h;
}
static void emitPdf(KatWriter& kp, const EdgeShape& s, const Vector4& ref, const Vector4& pt)
{
    float* in = kp.addIn(); in[0] = bitsf(s.kind); memcpy(in + 1, s.p, 16); put4(in + 5, ref); put4(in + 9, pt);
    kp.addOut()[0] = s.shape->Pdf(ref, pt);
}
// false: the record falls into the exclusion class (a sphere frame vector whose squared length is a denormal) and was not written
static bool emitEval(KatWriter& ke, const EdgeShape& s, const Vector4& pos)
{
    IntersectionData id; id.frame = Matrix4::Zero(); id.frame[3] = pos; id.texCoord = Vector4::Zero();
    if (s.kind == RT_SHAPE_SPHERE)
    {
        // SphereShape::EvaluateIntersection's three FastNormalize3 operands
        const Vector4 n = pos * s.p[1];
        const Vector4 t = (n.Swizzle<2, 0, 0, 0>() & Vector4::MakeMask<1, 0, 1, 0>()).ChangeSign<1, 0, 0, 0>();
        const Vector4 b = -Vector4::Cross3(t, n);
        if (rsqrtOperandDenormal(n) || rsqrtOperandDenormal(t) || rsqrtOperandDenormal(b)) return false;
    }
    float* in = ke.addIn(); in[0] = bitsf(s.kind); memcpy(in + 1, s.p, 16); memcpy(in + 5, s.p2, 16); put4(in + 9, pos);
    HitPoint hp;
    s.shape->EvaluateIntersection(hp, id);
    float* out = ke.addOut(); put4(out, id.frame[0]); put4(out + 4, id.frame[1]); put4(out + 8, id.frame[2]); put4(out + 12, id.texCoord);
    return true;
}

// the distance at which a unit sphere's cosThetaMax crosses 0.999999 (SphereShape.cpp:98): found by calling SphereShape::Sample
static float sphereFlatDistance(const EdgeShape& sphere)
{
    return firstTrue(100.0f * sphere.p[0], 10000.0f * sphere.p[0], [&](float d) { ShapeSampleResult sr; return sphere.shape->Sample(Vector4(0.0f, 0.0f, d, 0.0f), Float3(0.5f, 0.5f, 0.5f), sr) && sr.pdf == FLT_MAX; });
}

static void edgeShapes()
{
    const Floats unit = unitSpecials(), cosines = cosineSpecials(), reals = realSpecials();
    EdgeWriter ki("shape_intersect", KAT_SHAPE_INTERSECT, 13, 4), ks("shape_sample", KAT_SHAPE_SAMPLE, 12, 8), kp("shape_pdf", KAT_SHAPE_PDF, 13, 1), ke("shape_eval", KAT_SHAPE_EVAL, 13, 16);
    const EdgeShape sphere = edgeSphere(1.0f), sphere2 = edgeSphere(0.75f), box = edgeBox(1.0f, 2.0f, 3.0f), boxCdf = edgeBox(1.0f, 1.0f, 0.5f), cube = edgeBox(1.0f, 1.0f, 1.0f), rect = edgeRect(1.0f, 2.0f);
    Lcg g(230);
    // --- Intersect: sphere
    for (const EdgeShape* s : { &sphere, &sphere2 })
    {
        const float r = s->p[0];
        Floats offsets; addNeighbourhood(offsets, r, 3); offsets.push_back(0.0f); offsets.push_back(-0.0f); offsets.push_back(r * 0.5f); offsets.push_back(-r);
        for (float x : offsets)                                                     // tangent rays: det at 0 with its neighbours
            for (const Vector4& d : { Vector4(0.0f, 0.0f, -1.0f, 0.0f), Vector4(0.0f, 0.0f, 1.0f, 0.0f), Vector4(0.0f, -0.0f, -2.0f, 0.0f) }) { emitIntersect(ki, *s, Vector4(x, 0.0f, r, 0.0f), d); emitIntersect(ki, *s, Vector4(x, 0.0f, 4.0f, 0.0f), d); emitIntersect(ki, *s, Vector4(0.0f, x, 0.0f, 0.0f), d); }
        for (const Vector4& d : { Vector4(0.0f, 0.0f, 1.0f, 0.0f), Vector4(1.0f, 0.0f, 0.0f, 0.0f), dirWithZ(0.5f), Vector4(0.0f, 0.0f, 0.0f, 0.0f) })
        {
            emitIntersect(ki, *s, Vector4(0.0f, 0.0f, 0.0f, 0.0f), d);                                                       // origin at the centre
            for (float z : { ulpDown(r), r, ulpUp(r), -r }) emitIntersect(ki, *s, Vector4(0.0f, 0.0f, z, 0.0f), d);           // on the surface
            emitIntersect(ki, *s, Vector4(0.25f, -0.25f, 0.5f, 0.0f), d);                                                    // inside
        }
    }
    // --- Intersect: box (as the two-sided box test)
    {
        std::vector<Vector4> dirs;
        for (float x : { 0.0f, -0.0f, 1.0f, -1.0f }) for (float y : { 0.0f, -0.0f, 1.0f }) for (float z : { 0.0f, -0.0f, -1.0f }) dirs.push_back(Vector4(x, y, z, 0.0f));
        const std::vector<Vector4> origins = { Vector4(0.0f, 0.0f, 0.0f, 0.0f), Vector4(1.0f, 0.0f, 0.0f, 0.0f), Vector4(1.0f, 2.0f, 0.0f, 0.0f), Vector4(1.0f, 2.0f, 3.0f, 0.0f), Vector4(-5.0f, 2.0f, 0.0f, 0.0f),
            Vector4(-5.0f, ulpUp(2.0f), 0.0f, 0.0f), Vector4(-5.0f, ulpDown(2.0f), 0.0f, 0.0f), Vector4(-3.0f, -4.0f, -5.0f, 0.0f), Vector4(0.0f, 0.0f, 7.0f, 0.0f) };
        for (const Vector4& o : origins) for (const Vector4& d : dirs) emitIntersect(ki, box, o, d);
    }
    // --- Intersect: rect.  t = -origin.z * invDir.z against FLT_EPSILON; |pos.x| against size.x, |pos.y| against size.y; rays parallel to the plane
    {
        Floats ts; addNeighbourhood(ts, FLT_EPSILON, 2); ts.push_back(0.0f); ts.push_back(-0.0f); ts.push_back(-FLT_EPSILON); ts.push_back(kDenormal); ts.push_back(1.0f);
        for (float z : ts) { emitIntersect(ki, rect, Vector4(0.25f, 0.5f, z, 0.0f), Vector4(0.0f, 0.0f, -1.0f, 0.0f)); emitIntersect(ki, rect, Vector4(0.25f, 0.5f, -z, 0.0f), Vector4(0.0f, 0.0f, 1.0f, 0.0f)); }
        for (float s : { 1.0f, -1.0f })
        {
            Floats xsv, ysv; addNeighbourhood(xsv, 1.0f, 2); addNeighbourhood(ysv, 2.0f, 2);
            for (float x : xsv) { emitIntersect(ki, rect, Vector4(s * x, 0.5f, 1.0f, 0.0f), Vector4(0.0f, 0.0f, -1.0f, 0.0f)); emitIntersect(ki, rect, Vector4(s * x, s * 2.0f, 1.0f, 0.0f), Vector4(0.0f, 0.0f, -1.0f, 0.0f)); }
            for (float y : ysv) emitIntersect(ki, rect, Vector4(0.25f, s * y, 1.0f, 0.0f), Vector4(0.0f, 0.0f, -1.0f, 0.0f));
        }
        for (float dz : { 0.0f, -0.0f }) for (float oz : { 0.0f, -0.0f, 1.0f, -1.0f, kDenormal }) { emitIntersect(ki, rect, Vector4(-3.0f, 0.5f, oz, 0.0f), Vector4(1.0f, 0.0f, dz, 0.0f)); emitIntersect(ki, rect, Vector4(0.0f, 0.0f, oz, 0.0f), Vector4(0.0f, 1.0f, dz, 0.0f)); }
    }
    for (int i = 0; i < 64; ++i)
    {
        const EdgeShape* s = (i % 3 == 0) ? &sphere : (i % 3 == 1 ? &box : &rect);
        emitIntersect(ki, *s, Vector4(pick(g, { 0.0f, 1.0f, -1.0f, 2.0f, ulpUp(1.0f), 4.0f }), g.range(-2.0f, 2.0f), pick(g, { 0.0f, -0.0f, FLT_EPSILON, 1.0f, 3.0f, 5.0f, kInf, kNaN }), 0.0f),
                      Vector4(pick(g, { 0.0f, -0.0f, 1.0f, -1.0f }), pick(g, { 0.0f, -0.0f, 0.5f }), pick(g, { 0.0f, -0.0f, -1.0f, 1.0f, kDenormal }), 0.0f));
    }
    // --- Sample: sphere.  The reference point at the centre, on the surface, and at the distance where cosThetaMax crosses 0.999999, times the unit specials
    {
        Floats dists = { 0.0f, -0.0f, 0.5f }; addAround(dists, 1.0f);
        const float flat = sphereFlatDistance(sphere);
        addNeighbourhood(dists, flat, 1);
        dists.push_back(1.0e6f); dists.push_back(1.0e19f); dists.push_back(FLT_MAX); dists.push_back(2.0f);
        for (float d : dists) for (float a : unit) for (float b : unit) emitSample(ks, sphere, Vector4(0.0f, 0.0f, d, 0.0f), Float3(a, b, 0.5f));
        for (float d : { ulpDown(flat), flat }) for (float a : { 0.0f, 0.5f, 0.99999994f }) { emitSample(ks, sphere, Vector4(d, 0.0f, 0.0f, 0.0f), Float3(a, 0.25f, 0.5f)); emitSample(ks, sphere, Vector4(0.0f, 0.0f, -d, 0.0f), Float3(a, 0.25f, 0.5f)); }
        const float flat2 = sphereFlatDistance(sphere2);
        for (float d : { ulpDown(flat2), flat2, ulpUp(flat2), ulpDown(0.75f), 0.75f, ulpUp(0.75f) }) for (float a : { 0.0f, 0.5f, 0.99999994f }) emitSample(ks, sphere2, Vector4(0.0f, -d, 0.0f, 0.0f), Float3(a, 0.75f, 0.5f));
    }
    // --- Sample: box.  u[2] * cdf.z on each cdf step (u = 0.25, 0.5 for half sizes (1, 1, 0.5): cdf = 0.5, 1, 2) and the 0.5 face flip (0.125, 0.375, 0.75)
    {
        const Vector4 ref(4.0f, 5.0f, 6.0f, 0.0f), ref2(-4.0f, -5.0f, -6.0f, 0.0f);
        Floats w; for (float v : { 0.125f, 0.25f, 0.375f, 0.5f, 0.75f }) addAround(w, v);
        w.push_back(0.0f); w.push_back(0.99999994f); w.push_back(FLT_MIN);
        for (float v : w) for (const Vector4& r : { ref, ref2 }) for (const auto& uv : { Float2(0.25f, 0.75f), Float2(0.0f, 0.99999994f), Float2(0.5f, 0.5f) }) emitSample(ks, boxCdf, r, Float3(uv.x, uv.y, v));
        Floats wc; for (float v : { 1.0f / 3.0f, 2.0f / 3.0f, 1.0f / 6.0f, 0.5f, 5.0f / 6.0f }) addNeighbourhood(wc, v, 2);
        for (float v : wc) for (const Vector4& r : { ref, ref2 }) emitSample(ks, cube, r, Float3(0.25f, 0.75f, v));
        for (float a : unit) for (float b : unit) emitSample(ks, box, ref, Float3(a, b, 0.9f));
    }
    // --- Sample: box and rect.  The reference point in the sampled face's plane (cosNormalDir at FLT_EPSILON) and on the sampled point (sqrDistance at FLT_EPSILON^2)
    {
        Floats cs; addNeighbourhood(cs, FLT_EPSILON, 3); cs.push_back(0.0f); cs.push_back(-0.0f); cs.push_back(-FLT_EPSILON); cs.push_back(kDenormal);
        Floats ds; addNeighbourhood(ds, FLT_EPSILON, 2); ds.push_back(0.0f); ds.push_back(kDenormal); ds.push_back(-FLT_EPSILON);
        const Float3 centre(0.5f, 0.5f, 0.5f);           // the rect's sampled point is its origin
        for (float c : cs) { emitSample(ks, rect, dirWithZ(c, 0.0), centre); emitSample(ks, rect, dirWithZ(c, 2.0) * 2.0f, centre); }
        for (float d : ds) { emitSample(ks, rect, Vector4(0.0f, 0.0f, d, 0.0f), centre); emitSample(ks, rect, Vector4(d, 0.0f, 0.0f, 0.0f), centre); }
        const Float3 top(0.5f, 0.5f, 0.95f);             // box (1, 2, 3), cdf (6, 9, 11): u[2] = 0.95 is the +z face, sampled point (0, 0, 3)
        // (3 + c rounds c away: the cosine is dz / distance with dz = 2^-21 above the face and the distance around 4, so that it crosses 2^-23 = FLT_EPSILON)
        Floats across; addNeighbourhood(across, 4.0f, 3);
        for (float d : across) { emitSample(ks, box, Vector4(d, 0.0f, 3.0f + 4.76837158203125e-7f, 0.0f), top); emitSample(ks, box, Vector4(0.0f, -d, 3.0f + 4.76837158203125e-7f, 0.0f), top); }
        for (float c : cs) emitSample(ks, box, Vector4(0.0f, 0.0f, 3.0f, 0.0f) + dirWithZ(c, 0.0), top);
        for (float d : ds) emitSample(ks, box, Vector4(0.0f, 0.0f, 3.0f + d, 0.0f), top);
        for (float a : unit) for (float b : unit) emitSample(ks, rect, Vector4(0.5f, -0.5f, 2.0f, 0.0f), Float3(a, b, 0.5f));
    }
    for (int i = 0; i < 64; ++i)
    {
        const EdgeShape* s = (i % 3 == 0) ? &sphere : (i % 3 == 1 ? &boxCdf : &rect);
        emitSample(ks, *s, Vector4(pick(g, { 0.0f, -0.0f, 1.0f, 3.0f }), g.range(-2.0f, 2.0f), pick(g, { 0.0f, FLT_EPSILON, 1.0f, ulpUp(1.0f), 1000.0f, kInf, kNaN }), 0.0f), Float3(pick(g, unit), pick(g, unit), pick(g, unit)));
    }
    // --- Pdf
    {
        const float flat = sphereFlatDistance(sphere);
        Floats dists = { 0.0f, 0.5f, 2.0f, 1.0e6f, FLT_MAX }; addAround(dists, 1.0f); addNeighbourhood(dists, flat, 1);
        for (float d : dists) for (float z : cosines) emitPdf(kp, sphere, Vector4(0.0f, 0.0f, d, 0.0f), dirWithZ(z));
        for (const EdgeShape* s : { &sphere, &box, &rect })
        {
            for (const Vector4& pt : { Vector4(0.0f, 0.0f, 1.0f, 0.0f), Vector4(1.0f, 0.0f, 0.0f, 0.0f), Vector4(0.0f, 0.0f, 0.0f, 0.0f) })
            {
                emitPdf(kp, *s, pt, pt);                                                               // point == ref
                emitPdf(kp, *s, Vector4(0.0f, 0.0f, 0.0f, 0.0f), pt); emitPdf(kp, *s, Vector4(kInf, 0.0f, 0.0f, 0.0f), pt); emitPdf(kp, *s, Vector4(0.0f, kNaN, 0.0f, 0.0f), pt);
                emitPdf(kp, *s, pt + Vector4(0.0f, 0.0f, kDenormal, 0.0f), pt);
            }
        }
        for (int i = 0; i < 64; ++i) emitPdf(kp, sphere, Vector4(pick(g, { 0.0f, 1.0f, 3.0f }), 0.0f, pick(g, dists), 0.0f), dirWithZ(pick(g, cosines), g.range(0.0f, 6.28f)));
    }
    // --- EvaluateIntersection
    {
        uint32_t redraws = 0;
        std::vector<std::pair<const EdgeShape*, Vector4>> recs;
        for (const EdgeShape* s : { &sphere, &sphere2 })
        {
            const float r = s->p[0];
            for (float pole : { r, -r }) for (float x : { 0.0f, -0.0f }) for (float z : { 0.0f, -0.0f }) recs.push_back({ s, Vector4(x, pole, z, 0.0f) });           // both poles
            for (float x : { 0.0f, -0.0f }) for (float y : { -r, -0.5f * r, -1.0e-3f }) recs.push_back({ s, Vector4(x, y, sqrtf(r * r - y * y), 0.0f) });   // the seam x = +-0, y < 0
            for (float x : { 0.0f, -0.0f }) for (float zs : { 1.0f, -1.0f }) recs.push_back({ s, Vector4(x, -0.0f, zs * r, 0.0f) });
            for (float ax : { r, -r }) { recs.push_back({ s, Vector4(ax, 0.0f, 0.0f, 0.0f) }); recs.push_back({ s, Vector4(0.0f, 0.0f, ax, 0.0f) }); recs.push_back({ s, Vector4(ax, -0.0f, -0.0f, 0.0f) }); }
            for (float z : cosines) recs.push_back({ s, dirWithZ(z, 1.0) * r });
            recs.push_back({ s, Vector4(0.0f, 0.0f, 0.0f, 0.0f) });                                           // zero-length vectors stay in: rsqrt(0) = inf both ways
            recs.push_back({ s, Vector4(1.0e-10f, r, 1.0e-10f, 0.0f) });
        }
        for (const EdgeShape* s : { &box, &cube })
        {
            const float* p = s->p;
            for (float sx : { 1.0f, -1.0f }) for (float sy : { 1.0f, -1.0f }) for (float sz : { 1.0f, -1.0f })
            {
                recs.push_back({ s, Vector4(sx * p[0], sy * p[1], sz * p[2], 0.0f) });                        // corners: which face wins
                recs.push_back({ s, Vector4(sx * p[0], sy * p[1], 0.25f * sz, 0.0f) }); recs.push_back({ s, Vector4(sx * p[0], 0.25f * sy, sz * p[2], 0.0f) }); recs.push_back({ s, Vector4(0.25f * sx, sy * p[1], sz * p[2], 0.0f) });   // edges
                recs.push_back({ s, Vector4(sx * ulpDown(p[0]), sy * p[1], sz * ulpDown(p[2]), 0.0f) });
            }
            for (float zero : { 0.0f, -0.0f }) { recs.push_back({ s, Vector4(zero, zero, zero, 0.0f) }); recs.push_back({ s, Vector4(p[0], zero, zero, 0.0f) }); recs.push_back({ s, Vector4(zero, -p[1], zero, 0.0f) }); recs.push_back({ s, Vector4(zero, zero, p[2], 0.0f) }); }
        }
        for (float sx : { 1.0f, -1.0f }) for (float sy : { 1.0f, -1.0f }) { recs.push_back({ &rect, Vector4(sx * 1.0f, sy * 2.0f, 0.0f, 0.0f) }); recs.push_back({ &rect, Vector4(sx * 0.0f, sy * 0.0f, -0.0f, 0.0f) }); }
        recs.push_back({ &rect, Vector4(kInf, kNaN, 0.0f, 0.0f) }); recs.push_back({ &rect, Vector4(kDenormal, -FLT_MAX, 1.0f, 0.0f) });
        for (int i = 0; i < 64; ++i)
        {
            const EdgeShape* s = (i % 3 == 0) ? &sphere : (i % 3 == 1 ? &box : &rect);
            recs.push_back({ s, s->kind == RT_SHAPE_SPHERE ? dirWithZ(pick(g, cosines), (i & 1) ? g.range(0.0f, 6.28f) : 1.5707963267948966 * (double)(g.u32() % 4))
                                                           : Vector4(pick(g, { 1.0f, -1.0f, 0.0f, -0.0f, 0.5f }), pick(g, { 2.0f, -2.0f, 0.0f, -0.0f, 0.5f }), pick(g, { 3.0f, -3.0f, 0.0f, -0.0f }), 0.0f) });
        }
        for (auto& rec : recs)
        {
            for (uint32_t attempt = 0; !emitEval(ke, *rec.first, rec.second); ++attempt)
            {
                if (attempt >= kMaxRedraws || ++redraws > kMaxRedraws) { fprintf(stderr, "genEdges: shape_eval needs more than %u redraws\n", kMaxRedraws); exit(1); }
                rec.second = g.dir() * rec.first->p[0];
            }
        }
        printf("edges/shape_eval.kat: %u records redrawn (squared length of a FastNormalize3 operand denormal)\n", redraws);
    }
    ki.finish(); ks.finish(); kp.finish(); ke.finish();
}

// ---- lights ------------------------------------------------------------------------------------------
struct EdgeLight
{
    std::unique_ptr<ILight> light; RtLight L; Matrix4 xf; int type;
};
static Matrix4 translation(float x, float y, float z) { Matrix4 m = Matrix4::Identity(); m.rows[3] = Vector4(x, y, z, 1.0f); return m; }
static Matrix4 quarterTurnAboutX(float x, float y, float z) { Matrix4 m = translation(x, y, z); m.rows[1] = Vector4(0.0f, 0.0f, 1.0f, 0.0f); m.rows[2] = Vector4(0.0f, -1.0f, 0.0f, 0.0f); return m; }
// type 0: area (shape), 1: background, 2: directional (angle), 3: point, 4: spot (angle)
static EdgeLight edgeLight(int type, const Matrix4& xf, const Vector4& color, float angle = 0.0f, EdgeShape* shape = nullptr)
{
    EdgeLight e; e.type = type; e.xf = xf;
    float p[4] = { 0, 0, 0, 0 }, p2[4] = { 0, 0, 0, 0 }; uint32_t shapeKind = 0; float cosAngle = 0.0f; uint32_t isDelta = 0;
    if (type == 0) { shapeKind = shape->kind; memcpy(p, shape->p, 16); memcpy(p2, shape->p2, 16); e.light = std::make_unique<AreaLight>(ShapePtr(std::move(shape->shape)), color); }
    else if (type == 1) e.light = std::make_unique<BackgroundLight>(color);
    else if (type == 2) { auto dl = std::make_unique<DirectionalLight>(color, angle); cosAngle = dl->mCosAngle; isDelta = dl->mIsDelta ? 1u : 0u; e.light = std::move(dl); }
    else if (type == 3) e.light = std::make_unique<PointLight>(color);
    else { auto sl = std::make_unique<SpotLight>(color, angle); cosAngle = sl->mCosAngle; isDelta = sl->mIsDelta ? 1u : 0u; e.light = std::move(sl); }
    fillLight(e.L, *e.light, xf, shapeKind, p, p2);
    e.L.cosAngle = cosAngle; e.L.isDelta = isDelta;
    return e;
}

static void edgeLights()
{
    const uint32_t LW = sizeof(RtLight) / 4;
    const Floats unit = unitSpecials(), cosines = cosineSpecials();
    EdgeWriter ki("light_illuminate", KAT_LIGHT_ILLUMINATE, LW + 16 + 3, 11), kr("light_radiance", KAT_LIGHT_RADIANCE, LW + 13, 5);
    EdgeWriter ke("light_emit", KAT_LIGHT_EMIT, LW + 5, 15), kib("light_illuminate_bidir", KAT_LIGHT_ILLUMINATE_BIDIR, LW + 16 + 3, 12), krb("light_radiance_bidir", KAT_LIGHT_RADIANCE_BIDIR, LW + 13, 6);
    RenderingContext* ctx = new RenderingContext();
    Lcg g(240);

    auto illuminate = [&](const EdgeLight& e, const Vector4& position, const Float3& u)
    {
        IntersectionData isect;
        isect.frame[0] = VECTOR_X; isect.frame[1] = VECTOR_Y; isect.frame[2] = VECTOR_Z; isect.frame[3] = position;
        {
            float* in = ki.addIn(); memcpy(in, &e.L, sizeof(e.L)); putM(in + LW, isect.frame); in[LW + 16] = u.x; in[LW + 17] = u.y; in[LW + 18] = u.z;
            const ILight::IlluminateParam param = { e.xf.Inverse(), e.xf, isect, ctx->wavelength, u };
            ILight::IlluminateResult res;
            const RayColor rad = e.light->Illuminate(param, res);
            float* out = ki.addOut(); put4(out, rad.value);
            const bool zero = rad.AlmostZero() && e.type == 0;   // area light early-out leaves the result untouched
            if (!zero) { put4(out + 4, res.directionToLight); out[8] = res.distance; out[9] = res.directPdfW; out[10] = res.cosAtLight; }
            else { put4(out + 4, Vector4::Zero()); out[8] = -1.0f; out[9] = -1.0f; out[10] = -1.0f; }
        }
        {
            float* in = kib.addIn(); memcpy(in, &e.L, sizeof(e.L)); putM(in + LW, isect.frame); in[LW + 16] = u.x; in[LW + 17] = u.y; in[LW + 18] = u.z;
            const ILight::IlluminateParam param = { e.xf.Inverse(), e.xf, isect, ctx->wavelength, u, false };
            ILight::IlluminateResult res;      // (the area light's early-out returns before it writes the pdfs: they keep the struct's defaults, -1)
            const RayColor rad = e.light->Illuminate(param, res);
            float* out = kib.addOut(); put4(out, rad.value);
            put4(out + 4, res.directionToLight); out[8] = res.distance; out[9] = res.directPdfW; out[10] = res.emissionPdfW; out[11] = res.cosAtLight;
        }
    };
    auto radiance = [&](const EdgeLight& e, const Vector4& origin, const Vector4& dir, const Vector4& hit, float cosAtLight)
    {
        if (e.type > 2) return;
        const Ray lray(origin, dir);
        {
            float* in = kr.addIn(); memcpy(in, &e.L, sizeof(e.L)); put4(in + LW, lray.origin); put4(in + LW + 4, lray.dir); put4(in + LW + 8, hit); in[LW + 12] = cosAtLight;
            const ILight::RadianceParam param = { *ctx, lray, hit, cosAtLight };
            float pdf = 0.0f;
            const RayColor rad = e.light->GetRadiance(param, &pdf);
            float* out = kr.addOut(); put4(out, rad.value); out[4] = rad.AlmostZero() ? 0.0f : pdf;
        }
        {
            float* in = krb.addIn(); memcpy(in, &e.L, sizeof(e.L)); put4(in + LW, lray.origin); put4(in + LW + 4, lray.dir); put4(in + LW + 8, hit); in[LW + 12] = cosAtLight;
            const ILight::RadianceParam param = { *ctx, lray, hit, cosAtLight, false };
            float pdfA = 0.0f, pdfW = 0.0f;
            const RayColor rad = e.light->GetRadiance(param, &pdfA, &pdfW);
            float* out = krb.addOut(); put4(out, rad.value); out[4] = rad.AlmostZero() ? 0.0f : pdfA; out[5] = rad.AlmostZero() ? 0.0f : pdfW;
        }
    };
    auto emit = [&](const EdgeLight& e, const Float3& up, const Float2& ud)
    {
        float* in = ke.addIn(); memcpy(in, &e.L, sizeof(e.L)); in[LW] = up.x; in[LW + 1] = up.y; in[LW + 2] = up.z; in[LW + 3] = ud.x; in[LW + 4] = ud.y;
        const ILight::EmitParam param = { e.xf, ctx->wavelength, up, ud };
        ILight::EmitResult res; memset(&res, 0, sizeof(res));
        const RayColor c = e.light->Emit(param, res);
        float* out = ke.addOut(); put4(out, c.value); put4(out + 4, res.position); put4(out + 8, res.direction);
        out[12] = res.directPdfA; out[13] = res.emissionPdfW; out[14] = res.cosAtLight;
    };

    const Vector4 white(1.0f, 2.0f, 3.0f, 0.0f);
    const Matrix4 places[3] = { Matrix4::Identity(), translation(1.0f, -2.0f, 3.0f), quarterTurnAboutX(0.0f, 0.0f, 0.0f) };      // (an array: Matrix4 is aligned to 32 bytes)
    Floats epsCos; addNeighbourhood(epsCos, RT_EPSILON, 3); addNeighbourhood(epsCos, FLT_EPSILON, 3); for (float c : { 0.0f, -0.0f, -RT_EPSILON, -1.0f, 1.0f, 0.5f }) epsCos.push_back(c);

    // --- area lights: the shading point in the light's plane and behind it, cosAtLight at RT_EPSILON (no solid-angle sampling) and FLT_EPSILON (with it)
    for (const Matrix4& xf : places)
    {
        for (int shapeIndex = 0; shapeIndex < 4; ++shapeIndex)
        {
            EdgeShape s = shapeIndex == 0 ? edgeRect(1.0f, 2.0f) : (shapeIndex == 1 ? edgeBox(1.0f, 1.0f, 0.5f) : (shapeIndex == 2 ? edgeSphere(1.0f) : edgeSphere(0.25f)));
            const float radius = s.p[0];
            const uint32_t kind = s.kind;
            const EdgeLight e = edgeLight(0, xf, white, 0.0f, &s);
            // the sampled point: the rect's centre (u = 0.5, 0.5); the box's +z face centre (u[2] = 0.75 .. 1); the sphere's cone axis
            const Float3 u(0.5f, 0.5f, 0.9f);
            const Vector4 localPoint = kind == RT_SHAPE_RECT ? Vector4(0.0f, 0.0f, 0.0f, 0.0f) : (kind == RT_SHAPE_BOX ? Vector4(0.0f, 0.0f, 0.5f, 0.0f) : Vector4(0.0f, 0.0f, 0.0f, 0.0f));
            for (float c : epsCos)
                for (float dist : { 1.0f, 3.0f })
                    illuminate(e, xf.TransformPoint(localPoint + dirWithZ(c, 0.0) * dist), u);
            for (float d : { 0.0f, kDenormal, ulpDown(FLT_EPSILON), FLT_EPSILON, ulpUp(FLT_EPSILON), -1.0f }) illuminate(e, xf.TransformPoint(localPoint + Vector4(0.0f, 0.0f, d, 0.0f)), u);
            if (kind == RT_SHAPE_SPHERE)
            {
                const EdgeShape probe = edgeSphere(radius);
                const float flat = sphereFlatDistance(probe);
                Floats dists = { 0.0f }; addAround(dists, radius); addNeighbourhood(dists, flat, 1);
                for (float d : dists) for (float a : { 0.0f, 0.5f, 0.99999994f }) for (float b : { 0.0f, 0.25f, 0.99999994f }) illuminate(e, xf.TransformPoint(Vector4(0.0f, 0.0f, d, 0.0f)), Float3(a, b, 0.5f));
            }
            for (float a : unit) illuminate(e, xf.TransformPoint(Vector4(0.5f, -0.25f, 4.0f, 0.0f)), Float3(a, 0.75f, a));
            for (float c : epsCos) { radiance(e, xf.TransformPoint(Vector4(0.0f, 0.0f, 4.0f, 0.0f)), xf.TransformVector(Vector4(0.0f, 0.0f, -1.0f, 0.0f)), Vector4(0.0f, 0.0f, radius, 0.0f), c); }
            radiance(e, Vector4(0.0f, 0.0f, radius, 0.0f), VECTOR_Z, Vector4(0.0f, 0.0f, radius, 0.0f), 1.0f);                  // the ray's origin on the hit point
            for (float a : unit) { emit(e, Float3(a, 0.5f, 0.9f), Float2(0.25f, 0.75f)); emit(e, Float3(0.25f, a, a), Float2(a, 0.5f)); emit(e, Float3(0.25f, 0.75f, 0.1f), Float2(0.5f, a)); emit(e, Float3(a, a, a), Float2(a, a)); }
        }
    }
    // --- background: directions at the poles and on the +-pi seam of its mapping
    for (const Vector4& color : { white, Vector4(0.0f, 0.0f, 0.0f, 0.0f), Vector4(0.0f, 0.0f, 0.0f, 1.0f) })
    {
        const EdgeLight e = edgeLight(1, Matrix4::Identity(), color);
        for (float s : { 1.0f, -1.0f })
        {
            radiance(e, Vector4(0.0f, 0.0f, 0.0f, 0.0f), Vector4(0.0f, s, 0.0f, 0.0f), Vector4(0.0f, 0.0f, 0.0f, 0.0f), 1.0f);
            radiance(e, Vector4(0.0f, 0.0f, 0.0f, 0.0f), Vector4(-0.0f, s, -0.0f, 0.0f), Vector4(0.0f, 0.0f, 0.0f, 0.0f), 1.0f);
            for (float zero : { 0.0f, -0.0f }) { radiance(e, Vector4(1.0f, 2.0f, 3.0f, 0.0f), Vector4(zero, 0.0f, s, 0.0f), Vector4(0.0f, 0.0f, 0.0f, 0.0f), 0.5f); radiance(e, Vector4(1.0f, 2.0f, 3.0f, 0.0f), Vector4(s, zero, zero, 0.0f), Vector4(0.0f, 0.0f, 0.0f, 0.0f), 0.5f);
                                                 radiance(e, Vector4(1.0f, 2.0f, 3.0f, 0.0f), Vector4(zero, -0.6f, s * 0.8f, 0.0f), Vector4(0.0f, 0.0f, 0.0f, 0.0f), 0.5f); }
        }
        for (float a : unit) for (float b : { 0.0f, 0.5f, 0.99999994f }) { illuminate(e, Vector4(1.0f, 2.0f, 3.0f, 0.0f), Float3(a, b, 0.5f)); illuminate(e, Vector4(0.0f, 0.0f, 0.0f, 0.0f), Float3(b, a, 0.5f)); emit(e, Float3(a, b, 0.5f), Float2(b, a)); emit(e, Float3(b, a, 0.5f), Float2(a, b)); }
    }
    // --- directional: angle 0; around the angle at which the light stops being a delta light (cos = 0.9999, Light.h:25); the smallest angles whose cap pdf is finite
    {
        const float deltaAngle = acosf(ILight::CosEpsilon);
        // the largest angle whose cosine is still 1: SphereCapPdf divides by 1 - cos = 0 there; a delta light never evaluates it
        const float capAngle = firstTrue(1.0e-6f, 0.01f, [](float a) { return cosf(a) < 1.0f; });
        Floats angles = { 0.0f, 0.5f, 1.5707963f }; addNeighbourhood(angles, deltaAngle, 2); addAround(angles, capAngle);
        for (float angle : angles) for (const Matrix4& xf : { places[0], places[2] })
        {
            const EdgeLight e = edgeLight(2, xf, white, angle);
            const float cosAngle = e.L.cosAngle;
            for (float a : { 0.0f, 0.5f, 0.99999994f }) for (float b : { 0.0f, 0.25f, 0.99999994f }) { illuminate(e, Vector4(1.0f, 2.0f, 3.0f, 0.0f), Float3(a, b, 0.5f)); emit(e, Float3(a, b, 0.5f), Float2(b, a)); emit(e, Float3(b, a, 0.5f), Float2(a, b)); }
            Floats zs; addAround(zs, -cosAngle); zs.push_back(-1.0f); zs.push_back(1.0f); zs.push_back(0.0f);       // the ray's direction on the cone
            for (float z : zs) radiance(e, Vector4(0.0f, 0.0f, 0.0f, 0.0f), dirWithZ(z, 1.0), Vector4(0.0f, 0.0f, 0.0f, 0.0f), 1.0f);
        }
    }
    // --- point: the shading point at the light
    for (const Matrix4& xf : places)
    {
        const EdgeLight e = edgeLight(3, xf, white);
        const Vector4 at = xf.GetTranslation();
        for (const Vector4& p : { at, at + Vector4(0.0f, 0.0f, kDenormal, 0.0f), at + Vector4(FLT_EPSILON, 0.0f, 0.0f, 0.0f), at + Vector4(0.0f, 1.0e-19f, 0.0f, 0.0f), at + Vector4(1.0e19f, 0.0f, 0.0f, 0.0f), at + Vector4(0.0f, 0.0f, 1.0f, 0.0f), at + Vector4(kInf, 0.0f, 0.0f, 0.0f) })
            illuminate(e, p & Vector4::MakeMask<1, 1, 1, 0>(), Float3(0.5f, 0.5f, 0.5f));
        for (float a : unit) for (float b : { 0.0f, 0.5f, 0.99999994f }) { emit(e, Float3(0.5f, 0.5f, 0.5f), Float2(a, b)); emit(e, Float3(a, b, a), Float2(b, a)); }
    }
    // --- spot: the direction at the cone's cosine with both neighbours, and on the axis
    {
        const float deltaAngle = acosf(ILight::CosEpsilon);
        Floats angles = { 0.0f, 0.5f, 1.0471976f /* cos = 0.5 */, 1.5707963f }; addAround(angles, deltaAngle);
        for (float angle : angles) for (const Matrix4& xf : { places[0], places[1] })
        {
            const EdgeLight e = edgeLight(4, xf, white, angle);
            const float cosAngle = e.L.cosAngle;
            Floats zs; addNeighbourhood(zs, cosAngle, 2); zs.push_back(1.0f); zs.push_back(-1.0f); zs.push_back(0.0f); zs.push_back(ulpDown(1.0f));
            // the light looks along +z: a shading point at distance 1 along dirWithZ(z) sees it under cosine z
            for (float z : zs) for (float dist : { 1.0f, 2.0f }) illuminate(e, (xf.GetTranslation() + dirWithZ(z, 0.0) * dist) & Vector4::MakeMask<1, 1, 1, 0>(), Float3(0.5f, 0.5f, 0.5f));
            illuminate(e, xf.GetTranslation() & Vector4::MakeMask<1, 1, 1, 0>(), Float3(0.5f, 0.5f, 0.5f));           // at the light
            for (float a : { 0.0f, 0.5f, 0.99999994f }) for (float b : { 0.0f, 0.25f, 0.99999994f }) { emit(e, Float3(0.5f, 0.5f, 0.5f), Float2(a, b)); emit(e, Float3(a, b, a), Float2(b, a)); }
        }
    }
    // --- seeded mixes over all five types
    for (int i = 0; i < 64; ++i)
    {
        const int type = i % 5;
        EdgeShape s = (i / 5) % 3 == 0 ? edgeSphere(1.0f) : ((i / 5) % 3 == 1 ? edgeBox(1.0f, 1.0f, 0.5f) : edgeRect(1.0f, 2.0f));
        const EdgeLight e = edgeLight(type, places[g.u32() % 3u], Vector4(g.range(0.0f, 6.0f), g.range(0.0f, 6.0f), g.range(0.0f, 6.0f), (i % 7 == 0) ? 1.0f : 0.0f), pick(g, { 0.0f, 0.005f, 0.5f, 0.014142f }), &s);
        illuminate(e, Vector4(pick(g, { 0.0f, -0.0f, 1.0f, 3.0f }), g.range(-4.0f, 4.0f), pick(g, { 0.0f, 0.5f, 1.0f, ulpUp(1.0f), 3.0f, 5.0f }), 0.0f), Float3(pick(g, unit), pick(g, unit), pick(g, unit)));
        radiance(e, g.vec(-6.0f, 6.0f), dirWithZ(pick(g, cosines), g.range(0.0f, 6.28f)), Vector4(pick(g, { 0.0f, 1.0f }), 0.0f, 1.0f, 0.0f), pick(g, epsCos));
        emit(e, Float3(pick(g, unit), pick(g, unit), pick(g, unit)), Float2(pick(g, unit), pick(g, unit)));
    }
    ki.finish(); kr.finish(); ke.finish(); kib.finish(); krb.finish();
}

// ---- BSDFs -------------------------------------------------------------------------------------------
struct EdgeMaterial
{
    Material mat; RtMaterial M; SampledMaterialParameters mp;
    EdgeMaterial(uint32_t kind, float roughness, float ior, float K, const Vector4& baseColor)
    {
        mat.SetBsdf(kBsdfNames[kind]);
        mat.baseColor = baseColor; mat.emission = Vector4::Zero(); mat.roughness = roughness; mat.metalness = 0.0f; mat.IoR = ior; mat.K = K;
        mat.Compile();
        memset(&M, 0, sizeof(M));
        memcpy(M.emission, &mat.emission.baseValue, 16); memcpy(M.baseColor, &mat.baseColor.baseValue, 16);
        M.roughness = mat.roughness.baseValue; M.metalness = mat.metalness.baseValue; M.IoR = mat.IoR; M.K = mat.K; M.bsdf = kind;
        mp.baseColor = RayColor(mat.baseColor.baseValue); mp.emissionColor = RayColor(mat.emission.baseValue);
        mp.roughness = M.roughness; mp.metalness = M.metalness; mp.IoR = M.IoR;
    }
};

static void edgeBsdf()
{
    const Floats unit = unitSpecials(), cosines = cosineSpecials();
    EdgeWriter ks("bsdf_sample", KAT_BSDF_SAMPLE, 23, 11), ke("bsdf_evaluate", KAT_BSDF_EVALUATE, 24, 5), kp("bsdf_pdfs", KAT_BSDF_PDFS, 24, 8);
    Wavelength wavelength;
    Lcg g(250);
    const float threshold = BSDF::SpecularEventRoughnessTreshold;
    const Floats roughnesses = { 0.0f, ulpDown(threshold), threshold, ulpUp(threshold), 1.0f };
    const Vector4 colour(0.8f, 0.6f, 0.4f, 0.0f);

    auto sample = [&](EdgeMaterial& m, const Vector4& outgoing, const Float3& u)
    {
        float* in = ks.addIn(); memcpy(in, &m.M, 64); put4(in + 16, outgoing); in[20] = u.x; in[21] = u.y; in[22] = u.z;
        BSDF::SamplingContext sc = { m.mat, m.mp, u, outgoing, wavelength };
        const bool ok = m.mat.GetBSDF()->Sample(sc);
        float* out = ks.addOut(); out[0] = bitsf(ok ? 1u : 0u);
        if (ok) { put4(out + 1, sc.outColor.value); put4(out + 5, sc.outIncomingDir); out[9] = sc.outPdf; out[10] = bitsf((uint32_t)sc.outEventType); }
    };
    auto evaluate = [&](EdgeMaterial& m, const Vector4& outgoing, const Vector4& incoming)
    {
        const BSDF::EvaluationContext ec = { m.mat, m.mp, wavelength, outgoing, incoming };
        {
            float* in = ke.addIn(); memcpy(in, &m.M, 64); put4(in + 16, outgoing); put4(in + 20, incoming);
            float pdf = 0.0f;
            const RayColor c = m.mat.GetBSDF()->Evaluate(ec, &pdf);
            float* out = ke.addOut(); put4(out, c.value); out[4] = c.AlmostZero() ? 0.0f : pdf;
        }
        // rough metal / rough plastic below the specular threshold leave *outReversePdfW unwritten (RoughMetalBSDF.cpp:71-75, RoughPlasticBSDF.cpp:95-98):
        // the reference has no defined answer there, so those materials enter bsdf_pdfs only at and above the threshold
        if ((m.M.bsdf == 6u || m.M.bsdf == 8u) && m.M.roughness < threshold) return;
        {
            float* in = kp.addIn(); memcpy(in, &m.M, 64); put4(in + 16, outgoing); put4(in + 20, incoming);
            float pdf = 0.0f, rev = 0.0f;
            const RayColor c = m.mat.GetBSDF()->Evaluate(ec, &pdf, &rev);
            float* out = kp.addOut(); put4(out, c.value); out[4] = c.AlmostZero() ? 0.0f : pdf; out[5] = c.AlmostZero() ? 0.0f : rev;
            out[6] = m.mat.GetBSDF()->Pdf(ec, BSDF::ForwardPdf); out[7] = m.mat.GetBSDF()->Pdf(ec, BSDF::ReversePdf);
        }
    };

    for (uint32_t kind = 0; kind < 9; ++kind)
    {
        const float ior = 1.5f, K = 2.0f;
        for (float roughness : roughnesses)
        {
            EdgeMaterial m(kind, roughness, ior, K, colour);
            // outgoing z over the cosine specials, both hemispheres
            for (float z : cosines) sample(m, dirWithZ(z), Float3(0.25f, 0.75f, 0.5f));
            sample(m, dirWithZ(0.6f), Float3(0.25f, 0.75f, 0.0f));      // u[2] = 0 takes the specular / glossy lobe on both sides of the roughness threshold
            // incoming: NdotL = -incoming.z over the same specials; incoming = -outgoing; incoming the mirror of outgoing
            const Vector4 out1 = dirWithZ(0.6f);
            for (float z : cosines) evaluate(m, out1, dirWithZ(-z, 2.1));
            if (roughness != roughnesses[1] && roughness != roughnesses[3]) for (float oz : { 0.6f, -0.6f }) { const Vector4 o = dirWithZ(oz); evaluate(m, o, -o); evaluate(m, o, Vector4(o.x, o.y, -o.z, 0.0f)); evaluate(m, o, Vector4(-o.x, -o.y, -o.z, 0.0f) * Vector4(1.0f, 1.0f, -1.0f, 0.0f)); }
        }
        for (float roughness : { ulpDown(threshold), 1.0f })
        {
            EdgeMaterial m(kind, roughness, ior, K, colour);
            for (float z : cosines) evaluate(m, dirWithZ(z), dirWithZ(-0.6f, 2.1));
            // VdotH and the half vector's z at CosEpsilon: outgoing and the reversed incoming direction mirrored about the normal, grazing
            if (roughness == 1.0f) for (float c : { ulpUp(BSDF::CosEpsilon), 2.0e-5f, 1.0e-4f }) { const Vector4 o = dirWithZ(c, 0.0); evaluate(m, o, Vector4(o.x, 0.0f, -c, 0.0f)); evaluate(m, o, Vector4(-o.x, 0.0f, -c, 0.0f)); evaluate(m, o, Vector4(-o.x, 0.0f, c, 0.0f)); }
        }
        // the unit specials in each sample dimension
        {
            EdgeMaterial rough(kind, 0.5f, ior, K, colour), smooth(kind, 0.0f, ior, K, colour);
            for (float a : unit)
            {
                sample(rough, dirWithZ(0.8f), Float3(a, 0.5f, 0.5f)); sample(rough, dirWithZ(0.8f), Float3(0.5f, a, 0.5f)); sample(rough, dirWithZ(0.8f), Float3(0.5f, 0.5f, a)); sample(rough, dirWithZ(-0.8f), Float3(a, a, a));
                sample(smooth, dirWithZ(0.8f), Float3(a, 0.5f, a)); sample(smooth, dirWithZ(-0.8f), Float3(a, a, a));
            }
        }
        // baseColor 0 and 1
        for (const Vector4& c : { Vector4(0.0f, 0.0f, 0.0f, 0.0f), Vector4(1.0f, 1.0f, 1.0f, 0.0f) }) for (float roughness : { 0.0f, 0.5f })
        {
            EdgeMaterial m(kind, roughness, ior, K, c);
            sample(m, dirWithZ(0.8f), Float3(0.25f, 0.75f, 0.5f)); sample(m, dirWithZ(0.8f), Float3(0.25f, 0.75f, 0.99999994f)); evaluate(m, dirWithZ(0.8f), dirWithZ(-0.5f, 2.1));
        }
    }
    // IoR 1 and 1 + ulp (dielectrics, plastics); a metal with IoR = 0, K = 0
    for (uint32_t kind : { 3u, 4u, 7u, 8u }) for (float ior : { 1.0f, ulpUp(1.0f) }) for (float roughness : { 0.0f, 0.5f })
    {
        EdgeMaterial m(kind, roughness, ior, 0.0f, colour);
        for (float z : { 0.8f, -0.8f, 0.3f, ulpUp(BSDF::CosEpsilon), 1.0f }) { sample(m, dirWithZ(z), Float3(0.25f, 0.75f, 0.5f)); sample(m, dirWithZ(z), Float3(0.99999994f, 0.75f, 0.99999994f)); evaluate(m, dirWithZ(z), dirWithZ(z > 0.5f ? -0.5f : 0.5f, 2.1)); }
    }
    for (uint32_t kind : { 5u, 6u }) for (float roughness : { 0.0f, threshold, 0.5f })
    {
        EdgeMaterial m(kind, roughness, 0.0f, 0.0f, colour);
        for (float z : { 1.0f, 0.5f, ulpUp(BSDF::CosEpsilon), BSDF::CosEpsilon, -0.5f }) { sample(m, dirWithZ(z), Float3(0.25f, 0.75f, 0.5f)); evaluate(m, dirWithZ(z), dirWithZ(-0.5f, 2.1)); evaluate(m, dirWithZ(z), Vector4(dirWithZ(z).x, dirWithZ(z).y, -z, 0.0f)); }
    }
    // the sample that decides between the two events equal to the reflection probability, with both neighbours: the probability is computed
    // here from the reference's own Fresnel value the way DielectricBSDF.cpp:46-55 (sample.x) and PlasticBSDF.cpp:25-38 (sample.z) compute it
    for (float ior : { 1.5f, 1.05f }) for (float z : { 0.8f, 0.3f, -0.8f, -0.3f })
    {
        const float F = FresnelDielectric(z, ior);
        const float reflectionProbability = 0.25f + (1.0f - 0.25f) * F;
        for (uint32_t kind : { 3u, 4u }) { EdgeMaterial m(kind, 0.0f, ior, 0.0f, colour); for (float p : { ulpDown(reflectionProbability), reflectionProbability, ulpUp(reflectionProbability) }) if (p < 1.0f) sample(m, dirWithZ(z), Float3(p, 0.75f, p)); }
        if (z > 0.0f)
        {
            const float specularWeight = 0.25f + F * (1.0f - 0.25f);
            const float diffuseWeight = (1.0f - F) * 0.8f;     // baseColor.Max()
            const float specularProbability = specularWeight / (specularWeight + diffuseWeight);
            for (uint32_t kind : { 7u, 8u }) { EdgeMaterial m(kind, 0.0f, ior, 0.0f, colour); for (float p : { ulpDown(specularProbability), specularProbability, ulpUp(specularProbability) }) if (p < 1.0f) sample(m, dirWithZ(z), Float3(p, 0.75f, p)); }
        }
        // rough dielectric: sample.z against the Fresnel value at the sampled half vector (RoughDielectricBSDF.cpp:55-62)
        {
            EdgeMaterial m(4u, 0.5f, ior, 0.0f, colour);
            const Microfacet microfacet(0.5f * 0.5f);
            const Vector4 h = microfacet.Sample(Float2(0.25f, 0.75f));
            const float Fh = FresnelDielectric(Vector4::Dot3(h, dirWithZ(z)), ior);
            for (float p : { ulpDown(Fh), Fh, ulpUp(Fh) }) if (p < 1.0f && p >= 0.0f) sample(m, dirWithZ(z), Float3(0.25f, 0.75f, p));
        }
    }
    // seeded mixes
    for (int i = 0; i < 64; ++i)
    {
        const uint32_t kind = (uint32_t)(i % 9);
        EdgeMaterial m(kind, pick(g, roughnesses), (kind == 5 || kind == 6) ? pick(g, { 0.0f, 0.2f, 2.0f }) : pick(g, { 1.0f, ulpUp(1.0f), 1.5f }), pick(g, { 0.0f, 3.0f }),
                       Vector4(pick(g, { 0.0f, 1.0f, 0.5f }), pick(g, { 0.0f, 1.0f, 0.5f }), g.range(0.0f, 1.0f), (i % 11 == 0) ? 1.0f : 0.0f));
        const Vector4 o = dirWithZ(pick(g, cosines), g.range(0.0f, 6.28f));
        sample(m, o, Float3(pick(g, unit), pick(g, unit), pick(g, unit)));
        evaluate(m, o, dirWithZ(pick(g, cosines), g.range(0.0f, 6.28f)));
    }
    ks.finish(); ke.finish(); kp.finish();
}

// ---- camera, film, photons, debug colours ------------------------------------------------------------
static void edgeCameraFilm()
{
    const uint32_t CW = sizeof(RtCamera) / 4;
    const Floats unit = unitSpecials();
    RenderingContext* ctx = new RenderingContext();
    Lcg g(260);
    auto fill = [](const Camera& cam, RtCamera& C)
    {
        memset(&C, 0, sizeof(C));
        memcpy(C.localToWorld, &cam.mLocalToWorld, 64);
        C.aspectRatio = cam.mAspectRatio; C.tanHalfFoV = cam.mTanHalfFoV; C.dofEnable = cam.mDOF.enable ? 1u : 0u;
        C.focalPlaneDistance = cam.mDOF.focalPlaneDistance; C.aperture = cam.mDOF.aperture;
        C.bokehShape = (uint32_t)cam.mDOF.bokehShape;
        C.barrelDistortionConstFactor = cam.barrelDistortionConstFactor; C.barrelDistortionVariableFactor = cam.barrelDistortionVariableFactor;
    };
    // the sampler words whose GetFloat is a unit special (GetFloat = min(0.99999994, u / 2^32): FLT_MIN is not reachable, 2^-32 stands in)
    const uint32_t seedWords[9] = { 0u, 1u, 0x100u, 0x40000000u, 0x7FFFFF80u, 0x80000000u, 0x80000100u, 0xC0000000u, 0xFFFFFFFFu };
    {
        EdgeWriter k("camera_ray", KAT_CAMERA_RAY, CW + 8, 16);
        const Floats film = { 0.0f, -0.0f, 1.0f, 0.5f, ulpDown(1.0f), FLT_MIN, 0.25f };
        struct Setup { bool dof; float aperture; int bokeh; float barrelVariable, barrelConst; bool rotated; };
        std::vector<Setup> setups = { { false, 0.1f, 0, 0.0f, 0.01f, false }, { false, 0.1f, 0, 0.0f, 0.01f, true }, { false, 0.1f, 0, 0.02f, 0.0f, false }, { false, 0.1f, 0, 0.02f, 0.01f, true },
            { true, 0.0f, 0, 0.0f, 0.01f, false }, { true, 0.0f, 1, 0.0f, 0.01f, true }, { true, 0.0f, 2, 0.02f, 0.01f, false } };
        auto run = [&](const Setup& s, float x, float y, uint32_t s0, uint32_t s1)
        {
            Camera cam;
            cam.SetTransform(s.rotated ? Transform(Vector4(1.0f, -2.0f, 3.0f, 0.0f), Quaternion::FromEulerAngles(Float3(0.3f, -1.2f, 0.1f))) : Transform(Vector4(0.0f, 0.0f, 0.0f, 0.0f), Quaternion::Identity()));
            cam.SetPerspective(1.5f, 1.0f);
            cam.mDOF.enable = s.dof; cam.mDOF.focalPlaneDistance = 4.0f; cam.mDOF.aperture = s.aperture; cam.mDOF.bokehShape = (BokehShape)s.bokeh;
            cam.barrelDistortionVariableFactor = s.barrelVariable; cam.barrelDistortionConstFactor = s.barrelConst;
            RtCamera C; fill(cam, C);
            const Vector4 coords(x, y, 0.0f, 0.0f);
            DynArray<uint32> seed; seed.PushBack(s0); seed.PushBack(s1);
            ctx->sampler.ResetFrame(seed, false);
            ctx->sampler.mBlueNoisePixelX = 0; ctx->sampler.mBlueNoisePixelY = 0; ctx->sampler.mSalt = 0; ctx->sampler.mSamplesGenerated = 0;
            ctx->randomGenerator.mSeed[0] = ((uint64)g.u32() << 32) | g.u32(); ctx->randomGenerator.mSeed[1] = ((uint64)g.u32() << 32) | g.u32() | 1u;
            float* in = k.addIn(); memcpy(in, &C, sizeof(C)); in[CW] = coords.x; in[CW + 1] = coords.y; in[CW + 2] = bitsf(s0); in[CW + 3] = bitsf(s1);
            memcpy(in + CW + 4, &ctx->randomGenerator.mSeed[0], 8); memcpy(in + CW + 6, &ctx->randomGenerator.mSeed[1], 8);
            const Ray r = cam.GenerateRay(coords, *ctx);
            float* out = k.addOut(); put4(out, r.origin); put4(out + 4, r.dir); put4(out + 8, r.invDir); put4(out + 12, r.originDivDir);
        };
        for (const Setup& s : setups) for (float x : film) for (float y : film) run(s, x, y, 0x40000000u, 0xC0000000u);
        for (int bokeh = 0; bokeh < 3; ++bokeh) for (float aperture : { 0.0f, 0.25f }) for (uint32_t s0 : seedWords) for (uint32_t s1 : seedWords) run({ true, aperture, bokeh, 0.0f, 0.01f, bokeh == 1 }, 0.25f, 0.75f, s0, s1);
        for (int i = 0; i < 64; ++i) run(setups[g.u32() % setups.size()], pick(g, film), pick(g, film), seedWords[g.u32() % 9], seedWords[g.u32() % 9]);
        k.finish();
    }
    {
        EdgeWriter k("camera_film", KAT_CAMERA_FILM, CW + 8, 6);
        for (int rotated = 0; rotated < 2; ++rotated) for (const auto& lens : { Float2(1.5f, 1.0f), Float2(1.0f, 1.5707963f) /* aspect 1, tan(fov / 2) ~ 1 */ })
        {
            Camera cam;
            cam.SetTransform(rotated ? Transform(Vector4(1.0f, -2.0f, 3.0f, 0.0f), Quaternion::FromEulerAngles(Float3(0.3f, -1.2f, 0.1f))) : Transform(Vector4(0.0f, 0.0f, 0.0f, 0.0f), Quaternion::Identity()));
            cam.SetPerspective(lens.x, lens.y);
            RtCamera C; fill(cam, C);
            memcpy(C.worldToScreen, &cam.mWorldToScreen, 64);
            C.dofEnable = 0; C.focalPlaneDistance = 0.0f; C.aperture = 0.0f; C.bokehShape = 0; C.barrelDistortionConstFactor = 0.0f; C.barrelDistortionVariableFactor = 0.0f;   // as the interior generator leaves them
            std::vector<Vector4> locals;
            const float ex = cam.mAspectRatio * cam.mTanHalfFoV, ey = cam.mTanHalfFoV;     // the film's borders at depth 1
            for (float z : { 1.0f, 4.0f }) for (float bx : { -1.0f, 0.0f, 1.0f, ulpDown(1.0f), ulpUp(1.0f), -ulpUp(1.0f) }) for (float by : { -1.0f, 0.0f, 1.0f, ulpUp(1.0f), -ulpDown(1.0f) })
                locals.push_back(Vector4(bx * ex * z, by * ey * z, z, 0.0f));
            for (float z : { 0.0f, -0.0f, kDenormal, -kDenormal, FLT_MIN, -1.0f, 0.005f, FLT_MAX, 1.0e-20f }) for (const auto& xy : { Float2(0.0f, 0.0f), Float2(0.5f, -0.25f) }) locals.push_back(Vector4(xy.x, xy.y, z, 0.0f));   // on the camera plane, behind it
            for (int i = 0; i < 16; ++i) locals.push_back(Vector4(pick(g, { 0.0f, ex, -ex, 1.0e19f }), pick(g, { 0.0f, ey, -ey, -0.0f }), pick(g, { 0.0f, 1.0f, -1.0f, kDenormal, 1.0e-19f }), 0.0f));
            for (const Vector4& local : locals)
            {
                const Vector4 world = cam.mLocalToWorld.TransformPoint(local);
                for (int which = 0; which < 2; ++which)
                {
                    const Vector4 toPoint = world - cam.mLocalToWorld.GetTranslation();
                    const Vector4 dir = which == 0 ? (toPoint.SqrLength3() > 0.0f ? toPoint.Normalized3() : Vector4(0.0f, 0.0f, 0.0f, 0.0f)) : cam.mLocalToWorld.TransformVector(dirWithZ(pick(g, cosineSpecials()), 1.0));
                    float* in = k.addIn(); memcpy(in, &C, sizeof(C)); put4(in + CW, world); put4(in + CW + 4, dir);
                    Vector4 film = Vector4::Zero();
                    const bool ok = cam.WorldToFilm(world, film);
                    float* out = k.addOut(); out[0] = bitsf(ok ? 1u : 0u);
                    if (ok) { out[1] = film.x; out[2] = film.y; out[3] = film.z; out[4] = film.w; }
                    out[5] = cam.PdfW(dir);
                }
            }
        }
        k.finish();
    }
    {
        EdgeWriter k("film_splat", KAT_FILM_SPLAT, 4 + 8, 2 + 8);
        auto run = [&](float x, float y, uint32_t w, uint32_t h)
        {
            Bitmap sum;
            Bitmap::InitData id; id.width = w; id.height = h; id.format = Bitmap::Format::R32G32B32_Float;
            sum.Init(id);
            memset(sum.GetData(), 0, (size_t)w * h * 12);
            Film film(sum, nullptr);
            const Vector4 pos(x, y, 0.0f, 0.0f);
            Random rng;
            for (int s = 0; s < 2; ++s) { rng.mSeedSimd4[s] = VectorInt4((int32)g.u32(), (int32)g.u32(), (int32)g.u32(), (int32)g.u32()); }
            float* in = k.addIn(); in[0] = pos.x; in[1] = pos.y; in[2] = bitsf(w); in[3] = bitsf(h);
            memcpy(in + 4, &rng.mSeedSimd4[0], 16); memcpy(in + 8, &rng.mSeedSimd4[1], 16);
            film.AccumulateColor(pos, Vector4(1.0f, 2.0f, 3.0f, 0.0f), rng);
            uint32_t px = 0xFFFFFFFFu, py = 0xFFFFFFFFu;
            const float* data = reinterpret_cast<const float*>(sum.GetData());
            for (uint32_t yy = 0; yy < h; ++yy) for (uint32_t xx = 0; xx < w; ++xx) if (data[3 * ((size_t)yy * w + xx)] != 0.0f) { px = xx; py = yy; }
            float* out = k.addOut(); out[0] = bitsf(px); out[1] = bitsf(py);
            memcpy(out + 2, &rng.mSeedSimd4[0], 16); memcpy(out + 6, &rng.mSeedSimd4[1], 16);
        };
        const uint32_t sizes[][2] = { { 1, 1 }, { 2, 1 }, { 1, 2 }, { 7, 5 }, { 96, 64 } };
        for (const auto& s : sizes)
        {
            const float w = (float)s[0], h = (float)s[1];
            Floats xs = { 0.0f, -0.0f, 1.0f, ulpDown(1.0f), ulpUp(1.0f), 0.5f, -kDenormal, -0.01f, -1.0f, kNaN, kInf, -kInf, 1.0e10f, FLT_MIN };
            // the first value that rounds to width / height: x * width is an integer's lower neighbour rounding up
            xs.push_back(firstTrue(0.5f, 1.0f, [&](float v) { return v * w >= w; })); xs.push_back(ulpDown(xs.back()));
            xs.push_back(firstTrue(0.25f, 1.0f, [&](float v) { return v * w + 0.5f >= w; })); xs.push_back(ulpDown(xs.back()));
            Floats ys = xs;
            ys.push_back(firstTrue(0.5f, 1.0f, [&](float v) { return v * h >= h; })); ys.push_back(ulpDown(ys.back()));
            ys.push_back(firstTrue(0.25f, 1.0f, [&](float v) { return v * h + 0.5f >= h; })); ys.push_back(ulpDown(ys.back()));
            for (float x : xs) { run(x, 0.5f, s[0], s[1]); run(x, x, s[0], s[1]); }
            for (float y : ys) { run(0.5f, y, s[0], s[1]); run(0.25f, y, s[0], s[1]); }
            for (uint32_t px = 0; px <= s[0] && px < 8; ++px) run((float)px / w, (float)(px % (s[1] + 1)) / h, s[0], s[1]);      // pixel borders
        }
        for (int i = 0; i < 64; ++i) { const auto& s = sizes[g.u32() % 5]; run(pick(g, { 0.0f, 1.0f, 0.5f, ulpDown(1.0f), -0.0f, kNaN, 0.999f }), g.range(-0.1f, 1.1f), s[0], s[1]); }
        k.finish();
    }
    {
        EdgeWriter k("packed_photon", KAT_PACKED_PHOTON, 8, 11);
        std::vector<std::array<Vector4, 2>> xs;
        std::vector<Vector4> dirs;
        for (float s : { 1.0f, -1.0f }) for (float zero : { 0.0f, -0.0f }) { dirs.push_back(Vector4(s, zero, zero, 0.0f)); dirs.push_back(Vector4(zero, s, zero, 0.0f)); dirs.push_back(Vector4(zero, zero, s, 0.0f)); }
        for (float z : cosineSpecials()) dirs.push_back(dirWithZ(z, 1.0));
        dirs.push_back(Vector4(0.0f, 0.0f, 0.0f, 0.0f)); dirs.push_back(Vector4(0.57735026f, 0.57735026f, 0.57735026f, 0.0f)); dirs.push_back(Vector4(-0.57735026f, 0.57735026f, -0.57735026f, 0.0f));
        std::vector<Vector4> colours = { Vector4(0.0f, 0.0f, 0.0f, 0.0f), Vector4(1.0f, 1.0f, 1.0f, 0.0f), Vector4(FLT_MAX, 1.0f, 0.5f, 0.0f), Vector4(1.0f, FLT_MAX, 0.5f, 0.0f), Vector4(0.5f, 1.0f, FLT_MAX, 0.0f),
            Vector4(kDenormal, 1.0f, 0.5f, 0.0f), Vector4(1.0f, kDenormal, 0.0f, 0.0f), Vector4(kDenormal, kDenormal, kDenormal, 0.0f), Vector4(FLT_MIN, 0.0f, 0.0f, 0.0f), Vector4(65504.0f, 65536.0f, 1.0e-8f, 0.0f),
            Vector4(0.0f, 0.0f, 1.0f, 0.0f), Vector4(1000.0f, 0.001f, 1.0f, 0.0f) };
        for (const Vector4& d : dirs) for (const Vector4& c : colours) xs.push_back({ d, c });
        for (int i = 0; i < 64; ++i) xs.push_back({ dirWithZ(pick(g, cosineSpecials()), g.range(0.0f, 6.28f)), Vector4(pick(g, { 0.0f, 1.0f, FLT_MAX, kDenormal }), g.range(0.0f, 2.0f), pick(g, { 0.0f, 1000.0f, 1.0e-30f }), 0.0f) });
        for (const auto& x : xs)
        {
            float* in = k.addIn(); put4(in, x[0]); put4(in + 4, x[1]);
            PackedUnitVector3 pd; pd.FromVector(x[0]);
            PackedColorRgbHdr pc; pc.FromVector(x[1]);
            float* out = k.addOut();
            memcpy(out, &pd, 4); memcpy(out + 1, &pc, 8);
            put4(out + 3, pd.ToVector()); put4(out + 7, pc.ToVector());
        }
        k.finish();
    }
    {
        EdgeWriter k("debug_triangle_id", KAT_HSV_TO_RGB, 2, 4);
        const uint32_t ids[] = { 0u, 1u, 2u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu, 63u, 64u, 299999u };
        for (uint32_t objectId : ids) for (uint32_t subObjectId : ids)
        {
            float* in = k.addIn(); in[0] = bitsf(objectId); in[1] = bitsf(subObjectId);
            const uint64 hash = Hash((uint64)objectId | ((uint64)subObjectId << 32));
            const float hue = (float)(uint32)hash / (float)UINT32_MAX;
            const float saturation = 0.5f + 0.5f * (float)(uint32)(hash >> 32) / (float)UINT32_MAX;
            put4(k.addOut(), HSVtoRGB(hue, saturation, 1.0f));
        }
        k.finish();
    }
}

static void genEdges()
{
    mkdir((gOutDir + "/edges").c_str(), 0777);
    edgeMath();
    edgeGeometry();
    edgeShapes();
    edgeLights();
    edgeBsdf();
    edgeCameraFilm();
}
