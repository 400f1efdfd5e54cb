// rt_denoise.inl -- kernels behind rtgpu_filter_atrous / rtgpu_denoise (include/rtgpu.h; host side: rt_runtime_denoise.inl).  Included by rt_trace.hip.
// An edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) guided by the first-hit planes of rtgpu_render_aovs.  The definition -- every operation and
// its order -- stands in include/rtgpu.h and DESIGN.md section 5; tests/denoise_ref.py is the same text in NumPy float32, and the kernels are held to it bit for
// bit (the unit is compiled with -ffp-contract=off: every a * b + c below is a rounded multiply and a rounded add).
//
//   k_denoise_prepare   planes -> three 16-byte records per pixel: {n.xyz, valid}, {p.xyz, 0}, {c.rgb, 0} with c = colour * colorScale (/ albedo)
//   k_atrous<kLast>     one level: one lane per pixel, a wave = 64 consecutive x of one row, so each of a tap's three 16-byte loads is one coalesced
//                       kilobyte per wave at every step; 25 taps unrolled, no branch inside (a tap outside the frame or on an invalid pixel loads a
//                       clamped address and is dropped by a select).  kLast: remodulates and writes the float3 image instead of the next level's records.
//   k_atrous_tiled<kLast, kStep>   the same level for steps 1 and 2 from LDS: a block of 8 rows x 32 columns stages its tile and the 2 * step halo (three
//                       records per pixel, 30 KB at step 2) and takes its taps from there.  The per-pixel operations and their order are k_atrous's
//                       (atrousTap, atrousStore), so both give the same bits.
// The variance-guided variant (rtgpu_filter_atrous_var / rtgpu_denoise_var) is the kVar instantiation of the same three: k_denoise_prepare_var also reads the
// half-sample sum and leaves v = (lum(c) - lum(b))^2 in the colour record's fourth lane, where it travels through the ping-pong buffers at no extra load;
// a level first takes g, the 3 x 3 (undilated) Gaussian of v around the pixel -- the tiled kernels from the halo they hold anyway, k_atrous with nine
// 4-byte gathers of v and of the valid flag beside the centre -- and then weighs its 25 taps by the luminance distance over g * sigmaLum^2 + varianceFloor.

// d_k of the definition: the albedo channel the colour is divided by before and multiplied with after the filter
RT_DEV float denoiseAlbedoDivisor(const float* __restrict__ albedo, size_t pixels, uint32_t i, uint32_t k)
{
    if (!albedo) return 1.0f;
    const float a = albedo[(size_t)k * pixels + i];
    return a > 1e-3f ? a : 1.0f;
}

// lum(c) of the variance-guided definition
RT_DEV float denoiseLum(float c0, float c1, float c2) { return ((c0 + 2.0f * c1) + c2) * 0.25f; }

// pixel i of k_denoise_prepare (kVar: of k_denoise_prepare_var, whose colour record carries the variance of the mean's luminance; kPrepared: of
// k_denoise_prepare_accumulated, RT_DENOISE_INPUT_PREPARED: colour and colorHalf are c and b themselves -- no scale, no doubling, no division)
template <bool kVar, bool kPrepared = false>
RT_DEV void denoisePrepare(uint32_t i, const float* __restrict__ color, const float* __restrict__ colorHalf, const float* __restrict__ depth, const float* __restrict__ normal,
                           const float* __restrict__ position, const float* __restrict__ albedo, uint32_t pixels, float colorScale,
                           float4* __restrict__ recN, float4* __restrict__ recP, float4* __restrict__ recC)
{
    const size_t n = pixels;
    const bool valid = (__float_as_uint(depth[i]) & 0x7F800000u) != 0x7F800000u;   // finite: a miss has +inf
    recN[i] = make_float4(normal[i], normal[n + i], normal[2 * n + i], valid ? 1.0f : 0.0f);
    recP[i] = make_float4(position[i], position[n + i], position[2 * n + i], 0.0f);
    float c[3], b[3];
    for (uint32_t k = 0; k < 3u; ++k)
    {
        if (kPrepared)
        {
            c[k] = color[3 * (size_t)i + k];
            b[k] = colorHalf[3 * (size_t)i + k];
            continue;
        }
        c[k] = color[3 * (size_t)i + k] * colorScale;
        if (kVar) b[k] = colorHalf[3 * (size_t)i + k] * (2.0f * colorScale);
        if (albedo)
        {
            const float d = denoiseAlbedoDivisor(albedo, n, i, k);
            c[k] = c[k] / d;
            if (kVar) b[k] = b[k] / d;
        }
    }
    float v = 0.0f;
    if (kVar && valid)
    {
        const float e = denoiseLum(c[0], c[1], c[2]) - denoiseLum(b[0], b[1], b[2]);
        v = e * e;
    }
    recC[i] = make_float4(c[0], c[1], c[2], v);
}

__global__ void __launch_bounds__(RT_BLOCK) k_denoise_prepare(const float* __restrict__ color, const float* __restrict__ depth, const float* __restrict__ normal,
                                                              const float* __restrict__ position, const float* __restrict__ albedo, uint32_t pixels, float colorScale,
                                                              float4* __restrict__ recN, float4* __restrict__ recP, float4* __restrict__ recC)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pixels) return;
    denoisePrepare<false>(i, color, nullptr, depth, normal, position, albedo, pixels, colorScale, recN, recP, recC);
}

__global__ void __launch_bounds__(RT_BLOCK) k_denoise_prepare_var(const float* __restrict__ color, const float* __restrict__ colorHalf, const float* __restrict__ depth,
                                                                  const float* __restrict__ normal, const float* __restrict__ position, const float* __restrict__ albedo,
                                                                  uint32_t pixels, float colorScale, float4* __restrict__ recN, float4* __restrict__ recP, float4* __restrict__ recC)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pixels) return;
    denoisePrepare<true>(i, color, colorHalf, depth, normal, position, albedo, pixels, colorScale, recN, recP, recC);
}

__global__ void __launch_bounds__(RT_BLOCK) k_denoise_prepare_accumulated(const float* __restrict__ color, const float* __restrict__ colorHalf, const float* __restrict__ depth,
                                                                          const float* __restrict__ normal, const float* __restrict__ position, uint32_t pixels,
                                                                          float4* __restrict__ recN, float4* __restrict__ recP, float4* __restrict__ recC)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pixels) return;
    denoisePrepare<true, true>(i, color, colorHalf, depth, normal, position, nullptr, pixels, 1.0f, recN, recP, recC);
}

// one tap of the definition: its weight from the three distances, then acc += w * c_q and wsum += w -- unless the tap is skipped (`take` false).
// kVar: the colour distance is the luminance one over `denom` (lumP = lum(c_p)), and vacc += w^2 * v_q with v in the colour records' fourth lane
template <bool kVar>
RT_DEV void atrousTap(const float4& np, const float4& pp, const float4& cp, const float4& nq, const float4& pq, const float4& cq, bool take, float kernelWeight,
                      const AtrousLevel& level, float lumP, float denom, float& acc0, float& acc1, float& acc2, float& vacc, float& wsum)
{
    const float dnx = np.x - nq.x, dny = np.y - nq.y, dnz = np.z - nq.z;
    const float dpx = pq.x - pp.x, dpy = pq.y - pp.y, dpz = pq.z - pp.z;
    const float xn = (dnx * dnx + dny * dny) + dnz * dnz;
    const float t = (np.x * dpx + np.y * dpy) + np.z * dpz;
    const float xp = t * t;
    float xs;
    if (kVar)
    {
        const float dl = lumP - denoiseLum(cq.x, cq.y, cq.z);
        const float xc = (dl * dl) / denom;
        xs = (xn * level.invN + xp * level.invP) + xc;
    }
    else
    {
        const float dcx = cp.x - cq.x, dcy = cp.y - cq.y, dcz = cp.z - cq.z;
        const float xc = (dcx * dcx + dcy * dcy) + dcz * dcz;
        xs = (xn * level.invN + xp * level.invP) + xc * level.invC;
    }
    float u = fmaxf(0.0f, 1.0f - xs * 0.0625f);   // (1 - x / 16)^16: exactly 0 from x = 16 on, and for a NaN x
    u = u * u; u = u * u; u = u * u; u = u * u;
    const float wt = kernelWeight * u;
    acc0 = take ? acc0 + wt * cq.x : acc0;
    acc1 = take ? acc1 + wt * cq.y : acc1;
    acc2 = take ? acc2 + wt * cq.z : acc2;
    if (kVar) vacc = take ? vacc + (wt * wt) * cq.w : vacc;
    wsum = take ? wsum + wt : wsum;
}

// a colour record of the variance-guided kernels, all four lanes in one 16-byte load (left to itself the compiler fetches c and v apart)
typedef float AtrousLanes __attribute__((ext_vector_type(4)));
template <bool kVar>
RT_DEV float4 atrousColour(const float4* __restrict__ src, uint32_t q)
{
    if (!kVar) return src[q];
    const AtrousLanes lanes = *reinterpret_cast<const AtrousLanes*>(src + q);
    return make_float4(lanes.x, lanes.y, lanes.z, lanes.w);
}

// one tap of the 3 x 3 window behind g, the local variance: gsum += k * v_q and gw += k, unless skipped
RT_DEV void atrousWindowTap(float vq, bool take, float k, float& gsum, float& gw)
{
    gsum = take ? gsum + k * vq : gsum;
    gw = take ? gw + k : gw;
}

// the denominator of the luminance distance from the window's sums
RT_DEV float atrousDenominator(float gsum, float gw, const AtrousLevel& level) { return (gsum / gw) * level.invC + level.varianceFloor; }   // (invC holds sigmaLum^2 here)

// what a level leaves for pixel p: the next level's colour record, or (kLast) the remodulated float3 pixel (kVar: and the variance, where the caller wants it)
template <bool kLast, bool kVar>
RT_DEV void atrousStore(uint32_t p, float r0, float r1, float r2, float v, float4* __restrict__ dst, const float* __restrict__ albedo, float* __restrict__ out,
                        float* __restrict__ outVariance, uint32_t width, uint32_t height)
{
    if (kLast)
    {
        const size_t pixels = (size_t)width * height;
        out[3 * (size_t)p + 0] = r0 * denoiseAlbedoDivisor(albedo, pixels, p, 0u);
        out[3 * (size_t)p + 1] = r1 * denoiseAlbedoDivisor(albedo, pixels, p, 1u);
        out[3 * (size_t)p + 2] = r2 * denoiseAlbedoDivisor(albedo, pixels, p, 2u);
        if (kVar && outVariance) outVariance[p] = v;
    }
    else dst[p] = make_float4(r0, r1, r2, kVar ? v : 0.0f);
}

template <bool kLast, bool kVar>
__global__ void RT_ATROUS_ATTR k_atrous RT_K_ATROUS_ARGS
{
    // the blocks of a frame are numbered row by row along grid.x (a tall, narrow image has more block rows than grid.y may hold)
    const uint32_t blocksX = (width + RT_DENOISE_BLOCK_X - 1u) / RT_DENOISE_BLOCK_X, blockY = blockIdx.x / blocksX, blockX = blockIdx.x - blockY * blocksX;
    const int32_t x = (int32_t)(blockX * RT_DENOISE_BLOCK_X + threadIdx.x), y = (int32_t)(blockY * RT_DENOISE_BLOCK_Y + threadIdx.y);
    if (x >= (int32_t)width || y >= (int32_t)height) return;
    const int32_t w = (int32_t)width, h = (int32_t)height;
    const uint32_t p = (uint32_t)y * width + (uint32_t)x;
    const float4 np = recN[p], pp = recP[p], cp = src[p];
    float r0 = cp.x, r1 = cp.y, r2 = cp.z, rv = cp.w;   // an invalid pixel copies its colour (and variance)
    if (np.w != 0.0f)
    {
        const float kernelWeights[3] = { 0.375f, 0.25f, 0.0625f };
        float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f, vacc = 0.0f, wsum = 0.0f, lumP = 0.0f, denom = 0.0f;
        if (kVar)
        {
            // g from the pixel's eight neighbours and itself: the fourth lanes of their colour and normal records, 4 bytes of each
            const float gaussWeights[2] = { 0.5f, 0.25f };
            float gsum = 0.0f, gw = 0.0f;
#pragma unroll
            for (int32_t j = -1; j <= 1; ++j)
            {
#pragma unroll
                for (int32_t i = -1; i <= 1; ++i)
                {
                    const int32_t qx = x + i, qy = y + j;
                    const bool inside = qx >= 0 && qx < w && qy >= 0 && qy < h;
                    const uint32_t q = inside ? (uint32_t)qy * width + (uint32_t)qx : p;
                    atrousWindowTap(src[q].w, inside && recN[q].w != 0.0f, gaussWeights[i < 0 ? -i : i] * gaussWeights[j < 0 ? -j : j], gsum, gw);
                }
            }
            denom = atrousDenominator(gsum, gw, level);
            lumP = denoiseLum(cp.x, cp.y, cp.z);
        }
#pragma unroll
        for (int32_t j = -2; j <= 2; ++j)
        {
#pragma unroll
            for (int32_t i = -2; i <= 2; ++i)
            {
                const int32_t qx = x + level.step * i, qy = y + level.step * j;
                const bool inside = qx >= 0 && qx < w && qy >= 0 && qy < h;
                const uint32_t q = inside ? (uint32_t)qy * width + (uint32_t)qx : p;
                const float4 nq = recN[q], pq = recP[q], cq = atrousColour<kVar>(src, q);
                atrousTap<kVar>(np, pp, cp, nq, pq, cq, inside && nq.w != 0.0f, kernelWeights[i < 0 ? -i : i] * kernelWeights[j < 0 ? -j : j], level, lumP, denom,
                                acc0, acc1, acc2, vacc, wsum);
            }
        }
        if (wsum != 0.0f)
        {
            r0 = acc0 / wsum; r1 = acc1 / wsum; r2 = acc2 / wsum;
            if (kVar) rv = vacc / (wsum * wsum);
        }
    }
    atrousStore<kLast, kVar>(p, r0, r1, r2, rv, dst, albedo, out, outVariance, width, height);
}
#define RT_X(L, V) template __global__ void RT_ATROUS_ATTR k_atrous<L, V> RT_K_ATROUS_ARGS;
RT_X(false, false) RT_X(true, false) RT_X(false, true) RT_X(true, true)
#undef RT_X

template <bool kLast, int kStep, bool kVar>
__global__ void RT_ATROUS_TILED_ATTR k_atrous_tiled RT_K_ATROUS_ARGS
{
    constexpr int32_t kHalo = 2 * kStep, kTileW = RT_DENOISE_TILE_X + 2 * kHalo, kTileH = RT_DENOISE_TILE_Y + 2 * kHalo;
    __shared__ float4 tileN[kTileH * kTileW], tileP[kTileH * kTileW], tileC[kTileH * kTileW];
    const int32_t w = (int32_t)width, h = (int32_t)height;
    const uint32_t blocksX = (width + RT_DENOISE_TILE_X - 1u) / RT_DENOISE_TILE_X, blockY = blockIdx.x / blocksX, blockX = blockIdx.x - blockY * blocksX;   // (as k_atrous numbers them)
    const int32_t x0 = (int32_t)(blockX * RT_DENOISE_TILE_X), y0 = (int32_t)(blockY * RT_DENOISE_TILE_Y);
    // the tile and its halo; a record outside the frame is invalid (n.w = 0), which is how its tap is skipped
    for (int32_t e = (int32_t)(threadIdx.y * RT_DENOISE_TILE_X + threadIdx.x); e < kTileH * kTileW; e += RT_DENOISE_TILE_X * RT_DENOISE_TILE_Y)
    {
        const int32_t ty = e / kTileW, tx = e - ty * kTileW;
        const int32_t gx = x0 - kHalo + tx, gy = y0 - kHalo + ty;
        const bool inside = gx >= 0 && gx < w && gy >= 0 && gy < h;
        float4 n = make_float4(0.0f, 0.0f, 0.0f, 0.0f), ps = n, c = n;
        if (inside)
        {
            const uint32_t g = (uint32_t)gy * width + (uint32_t)gx;
            n = recN[g]; ps = recP[g]; c = src[g];
        }
        tileN[e] = n; tileP[e] = ps; tileC[e] = c;
    }
    __syncthreads();
    const int32_t x = x0 + (int32_t)threadIdx.x, y = y0 + (int32_t)threadIdx.y;
    if (x >= w || y >= h) return;
    const uint32_t p = (uint32_t)y * width + (uint32_t)x;
    const int32_t centre = ((int32_t)threadIdx.y + kHalo) * kTileW + (int32_t)threadIdx.x + kHalo;
    const float4 np = tileN[centre], pp = tileP[centre], cp = tileC[centre];
    float r0 = cp.x, r1 = cp.y, r2 = cp.z, rv = cp.w;
    if (np.w != 0.0f)
    {
        const float kernelWeights[3] = { 0.375f, 0.25f, 0.0625f };
        float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f, vacc = 0.0f, wsum = 0.0f, lumP = 0.0f, denom = 0.0f;
        if (kVar)
        {
            // g from the tile: the halo is 2 * step >= 2 wide, so the undilated 3 x 3 window is inside it
            const float gaussWeights[2] = { 0.5f, 0.25f };
            float gsum = 0.0f, gw = 0.0f;
#pragma unroll
            for (int32_t j = -1; j <= 1; ++j)
            {
#pragma unroll
                for (int32_t i = -1; i <= 1; ++i)
                {
                    const int32_t q = centre + j * kTileW + i;
                    atrousWindowTap(tileC[q].w, tileN[q].w != 0.0f, gaussWeights[i < 0 ? -i : i] * gaussWeights[j < 0 ? -j : j], gsum, gw);
                }
            }
            denom = atrousDenominator(gsum, gw, level);
            lumP = denoiseLum(cp.x, cp.y, cp.z);
        }
#pragma unroll
        for (int32_t j = -2; j <= 2; ++j)
        {
#pragma unroll
            for (int32_t i = -2; i <= 2; ++i)
            {
                const int32_t q = centre + kStep * j * kTileW + kStep * i;
                const float4 nq = tileN[q], pq = tileP[q], cq = tileC[q];
                atrousTap<kVar>(np, pp, cp, nq, pq, cq, nq.w != 0.0f, kernelWeights[i < 0 ? -i : i] * kernelWeights[j < 0 ? -j : j], level, lumP, denom,
                                acc0, acc1, acc2, vacc, wsum);
            }
        }
        if (wsum != 0.0f)
        {
            r0 = acc0 / wsum; r1 = acc1 / wsum; r2 = acc2 / wsum;
            if (kVar) rv = vacc / (wsum * wsum);
        }
    }
    atrousStore<kLast, kVar>(p, r0, r1, r2, rv, dst, albedo, out, outVariance, width, height);
}
#define RT_X(L, S) template __global__ void RT_ATROUS_TILED_ATTR k_atrous_tiled<L, S, false> RT_K_ATROUS_ARGS; template __global__ void RT_ATROUS_TILED_ATTR k_atrous_tiled<L, S, true> RT_K_ATROUS_ARGS;
RT_X(false, 1) RT_X(true, 1) RT_X(false, 2) RT_X(true, 2)
#undef RT_X
