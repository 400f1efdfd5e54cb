// rt_temporal_moments_body.inl -- the colour statistics of history clipping.  rt_temporal.inl, which describes the kernel, includes it twice: as k_temporal_moments
// (RT_TEMPORAL_CHAIN 0: the blocks under that switch are not there) and as k_temporal_moments_chain (RT_TEMPORAL_CHAIN 1), rtgpu_temporal_accumulate_chain's variant
// over chain guides.  There chainDistance is staged where depth is -- both are +inf exactly on a miss -- so the plane tolerance scales with the unfolded path
// length, and the valid lane of {P.xyz, valid} holds chain length + 1 as a word (0: invalid): a window pixel counts only when it is valid and its chain is as
// long as the pixel's own, one integer compare in the place of the float one.
template <int kRadius>
__global__ void RT_TEMPORAL_MOMENTS_ATTR RT_TEMPORAL_MOMENTS_KERNEL
#if RT_TEMPORAL_CHAIN
    RT_K_TEMPORAL_MOMENTS_CHAIN_ARGS
#else
    RT_K_TEMPORAL_MOMENTS_ARGS
#endif
{
    constexpr int32_t kTileW = RT_DENOISE_TILE_X + 2 * kRadius, kTileH = RT_DENOISE_TILE_Y + 2 * kRadius;
    __shared__ float4 tileC[kTileH * kTileW], tileN[kTileH * kTileW], tileP[kTileH * kTileW];
    const int32_t w = (int32_t)width, h = (int32_t)height;
    const size_t pixels = (size_t)width * height;
    const uint32_t blocksX = (width + RT_DENOISE_TILE_X - 1u) / RT_DENOISE_TILE_X, blockY = blockIdx.x / blocksX, blockX = blockIdx.x - blockY * blocksX;   // (as k_atrous numbers them)
    const int32_t x0 = (int32_t)(blockX * RT_DENOISE_TILE_X), y0 = (int32_t)(blockY * RT_DENOISE_TILE_Y);
    for (int32_t e = (int32_t)(threadIdx.y * RT_DENOISE_TILE_X + threadIdx.x); e < kTileH * kTileW; e += RT_DENOISE_TILE_X * RT_DENOISE_TILE_Y)
    {
        const int32_t ty = e / kTileW, tx = e - ty * kTileW;
        const int32_t gx = x0 - kRadius + tx, gy = y0 - kRadius + ty;
        const bool inside = gx >= 0 && gx < w && gy >= 0 && gy < h;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), n = c, ps = c;
        if (inside)
        {
            const uint32_t g = (uint32_t)gy * width + (uint32_t)gx;
#if RT_TEMPORAL_CHAIN
            const float depth = chain.chainDistance[g];
#else
            const float depth = in.depth[g];
#endif
            const bool valid = (__float_as_uint(depth) & 0x7F800000u) != 0x7F800000u;
            float ck[3];
#pragma unroll
            for (uint32_t k = 0; k < 3u; ++k)
            {
                ck[k] = in.color[3 * (size_t)g + k] * frame.colorScale;
                if (in.albedo) ck[k] = ck[k] / denoiseAlbedoDivisor(in.albedo, pixels, g, k);
            }
            c = make_float4(ck[0], ck[1], ck[2], depth);
            n = make_float4(in.normal[g], in.normal[pixels + g], in.normal[2 * pixels + g], __uint_as_float(in.objectId ? in.objectId[g] : 0u));
#if RT_TEMPORAL_CHAIN
            ps = make_float4(in.position[g], in.position[pixels + g], in.position[2 * pixels + g], __uint_as_float(valid ? chain.chainLength[g] + 1u : 0u));
#else
            ps = make_float4(in.position[g], in.position[pixels + g], in.position[2 * pixels + g], valid ? 1.0f : 0.0f);
#endif
        }
        tileC[e] = c; tileN[e] = n; tileP[e] = ps;
    }
    __syncthreads();
    const int32_t x = x0 + (int32_t)threadIdx.x, y = y0 + (int32_t)threadIdx.y;
    if (x >= w || y >= h) return;
    const uint32_t p = (uint32_t)y * width + (uint32_t)x;
    const int32_t centre = ((int32_t)threadIdx.y + kRadius) * kTileW + (int32_t)threadIdx.x + kRadius;
    const float4 cp = tileC[centre], np = tileN[centre], pp = tileP[centre];
    const float limit = frame.planeTolerance * cp.w;
    float cnt = 0.0f, s10 = 0.0f, s11 = 0.0f, s12 = 0.0f, s20 = 0.0f, s21 = 0.0f, s22 = 0.0f;
#pragma unroll 1   // (see above)
    for (int32_t dy = -kRadius; dy <= kRadius; ++dy)
    {
#pragma unroll
        for (int32_t dx = -kRadius; dx <= kRadius; ++dx)
        {
            const int32_t q = centre + dy * kTileW + dx;
            const float4 cq = tileC[q], nq = tileN[q], pq = tileP[q];
            const float dpx = pq.x - pp.x, dpy = pq.y - pp.y, dpz = pq.z - pp.z;
            const float cosine = (np.x * nq.x + np.y * nq.y) + np.z * nq.z;
            const float offset = fabsf((np.x * dpx + np.y * dpy) + np.z * dpz);
#if RT_TEMPORAL_CHAIN
            const bool counts = __float_as_uint(pq.w) != 0u && __float_as_uint(pq.w) == __float_as_uint(pp.w) && __float_as_uint(nq.w) == __float_as_uint(np.w) &&
                                cosine >= frame.normalThreshold && offset <= limit;
#else
            const bool counts = pq.w != 0.0f && __float_as_uint(nq.w) == __float_as_uint(np.w) && cosine >= frame.normalThreshold && offset <= limit;
#endif
            cnt = counts ? cnt + 1.0f : cnt;
            s10 = counts ? s10 + cq.x : s10;
            s11 = counts ? s11 + cq.y : s11;
            s12 = counts ? s12 + cq.z : s12;
            s20 = counts ? s20 + cq.x * cq.x : s20;
            s21 = counts ? s21 + cq.y * cq.y : s21;
            s22 = counts ? s22 + cq.z * cq.z : s22;
        }
    }
    // (cnt == 0: not a number, and never read -- minCount is at least 1)
    const float mu0 = s10 / cnt, mu1 = s11 / cnt, mu2 = s12 / cnt;
    const float var0 = fmaxf(s20 / cnt - mu0 * mu0, 0.0f), var1 = fmaxf(s21 / cnt - mu1 * mu1, 0.0f), var2 = fmaxf(s22 / cnt - mu2 * mu2, 0.0f);
    outMu[p] = make_float4(mu0, mu1, mu2, cnt);
    outG[p] = make_float4(frame.gamma * sqrtf(var0), frame.gamma * sqrtf(var1), frame.gamma * sqrtf(var2), 0.0f);
}
