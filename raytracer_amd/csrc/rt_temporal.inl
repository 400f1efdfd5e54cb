// rt_temporal.inl -- kernels behind rtgpu_temporal_accumulate / rtgpu_denoise_temporal (include/rtgpu.h; host side: rt_runtime_temporal.inl).  Included by
// rt_trace.hip behind rt_denoise.inl, whose helpers it uses and whose -ffp-contract=off it shares: every a * b + c below is a rounded multiply and a rounded add.
// Temporal accumulation, the other half of SVGF: the world position of a pixel's first hit goes through the previous frame's worldToScreen, the previous
// frame's accumulated pair (A, B) and history length are fetched bilinearly from the four pixels around that point -- each tap tested against the pixel's own
// surface -- and blended with this frame's pair.  The definition stands in include/rtgpu.h; tests/temporal_ref.py is the same text in NumPy float32.
//
//   k_temporal_pack   planar history of a caller (the pure entries) -> the four 16-byte records per pixel the context keeps its own history in:
//                     {A.rgb, length}, {B.rgb, object id}, {N.xyz, valid}, {P.xyz, 0}
//   k_temporal        one lane per pixel, a wave = 64 consecutive x of one row.  The current planes are coalesced loads; a tap is four 16-byte gathers, no
//                     branch around it (a tap outside the frame loads the pixel's own address and is dropped by a select, as atrousTap does).  Neighbours
//                     share three of their four taps under coherent motion: the caches do what an LDS tile would.  It writes the planar outputs and,
//                     where asked, the records of the next frame's history and the remodulated image; every per-pixel operation exists once.
//   k_temporal<true>  the scene's objects moved between the two frames (rtgpu_update_objects): the pixel's object id selects an 80-byte record of the motion
//                     table -- one lane-indexed gather of five 16-byte loads; the table holds some hundred objects and neighbours share their object, so it
//                     is served from the caches, mostly as a broadcast -- whose matrix takes position and normal to where that surface point was in the
//                     previous frame.  Projection and the tap tests use the moved pair and the id the object had then; the stored history keeps this
//                     frame's own.  An unmoved object selects its own position and normal: the bits of k_temporal<false>.
//   k_temporal_moments<r>   history clipping: mean and gamma standard deviations of this frame's prepared colours over the (2r + 1)^2 window pixels on the pixel's
//                     own surface, from an LDS tile; two 16-byte records per pixel
//   k_temporal<., true>   the same kernel reading those records (coalesced): the reprojected A is clipped to mu +- g, B shifted along, the history length cut by how
//                     far A was pulled.  A compile-time variant: the two instantiations without it are what they were.

__global__ void __launch_bounds__(RT_BLOCK) k_temporal_pack(const float* __restrict__ prevA, const float* __restrict__ prevB, const float* __restrict__ prevLength,
                                                            const float* __restrict__ prevDepth, const float* __restrict__ prevNormal, const float* __restrict__ prevPosition,
                                                            const uint32_t* __restrict__ prevObjectId, uint32_t pixels, float4* __restrict__ recA, float4* __restrict__ recB,
                                                            float4* __restrict__ recN, float4* __restrict__ recP)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pixels) return;
    const size_t n = pixels;
    const bool valid = (__float_as_uint(prevDepth[i]) & 0x7F800000u) != 0x7F800000u;
    recA[i] = make_float4(prevA[3 * (size_t)i], prevA[3 * (size_t)i + 1], prevA[3 * (size_t)i + 2], prevLength[i]);
    recB[i] = make_float4(prevB[3 * (size_t)i], prevB[3 * (size_t)i + 1], prevB[3 * (size_t)i + 2], __uint_as_float(prevObjectId ? prevObjectId[i] : 0u));
    recN[i] = make_float4(prevNormal[i], prevNormal[n + i], prevNormal[2 * n + i], valid ? 1.0f : 0.0f);
    recP[i] = make_float4(prevPosition[i], prevPosition[n + i], prevPosition[2 * n + i], 0.0f);
}

// a history record in one 16-byte load (as atrousColour)
RT_DEV float4 temporalRecord(const float4* __restrict__ src, uint32_t q)
{
    const AtrousLanes lanes = *reinterpret_cast<const AtrousLanes*>(src + q);
    return make_float4(lanes.x, lanes.y, lanes.z, lanes.w);
}

// The colour statistics of history clipping ("Clipping the history", include/rtgpu.h): per pixel the mean and gamma standard deviations of the prepared colours
// over the window pixels that lie on the pixel's own surface.  A block stages its tile and a halo of kRadius into LDS as three 16-byte records -- {c.rgb, depth},
// {N.xyz, id bits}, {P.xyz, valid} -- with the prepare step done once per staged pixel; a record outside the frame is invalid, which is how its window pixel is
// skipped.  Each lane then walks its (2 kRadius + 1)^2 window row by row from LDS with no branch around a neighbour (selects, as atrousTap) and writes
// {mu.rgb, cnt} and {g.rgb, 0}.  Consecutive lanes read consecutive 16-byte records: no bank conflicts.  The window's columns are unrolled, its rows are not:
// with all 49 taps of radius 3 in one basic block the scheduler hoists every LDS load (218 VGPRs, two waves per SIMD) and the kernel takes twice as long
// (profiles/temporal_clip_resources.txt); a row at a time it holds 50 VGPRs, and the 25.5 KB tile lets six blocks -- six waves per SIMD -- share a CU.
template <int kRadius>
__global__ void RT_TEMPORAL_MOMENTS_ATTR k_temporal_moments RT_K_TEMPORAL_MOMENTS_ARGS
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
            const float depth = in.depth[g];
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
            ps = make_float4(in.position[g], in.position[pixels + g], in.position[2 * pixels + g], valid ? 1.0f : 0.0f);
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
            const bool counts = pq.w != 0.0f && __float_as_uint(nq.w) == __float_as_uint(np.w) && cosine >= frame.normalThreshold && offset <= limit;
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
template __global__ void RT_TEMPORAL_MOMENTS_ATTR k_temporal_moments<1> RT_K_TEMPORAL_MOMENTS_ARGS;
template __global__ void RT_TEMPORAL_MOMENTS_ATTR k_temporal_moments<2> RT_K_TEMPORAL_MOMENTS_ARGS;
template __global__ void RT_TEMPORAL_MOMENTS_ATTR k_temporal_moments<3> RT_K_TEMPORAL_MOMENTS_ARGS;

template <bool kMoving, bool kClip> __global__ void RT_ATROUS_ATTR k_temporal RT_K_TEMPORAL_ARGS
{
    // (blocks numbered row by row along grid.x, as k_atrous numbers them)
    const uint32_t blocksX = (width + RT_DENOISE_BLOCK_X - 1u) / RT_DENOISE_BLOCK_X, blockY = blockIdx.x / blocksX, blockX = blockIdx.x - blockY * blocksX;
    const int32_t x = (int32_t)(blockX * RT_DENOISE_BLOCK_X + threadIdx.x), y = (int32_t)(blockY * RT_DENOISE_BLOCK_Y + threadIdx.y);
    if (x >= (int32_t)width || y >= (int32_t)height) return;
    const int32_t w = (int32_t)width, h = (int32_t)height;
    const uint32_t p = (uint32_t)y * width + (uint32_t)x;
    const size_t pixels = (size_t)width * height;
    const float depthP = in.depth[p];
    const bool valid = (__float_as_uint(depthP) & 0x7F800000u) != 0x7F800000u;
    const float4 np = make_float4(in.normal[p], in.normal[pixels + p], in.normal[2 * pixels + p], valid ? 1.0f : 0.0f);
    const float4 pp = make_float4(in.position[p], in.position[pixels + p], in.position[2 * pixels + p], 0.0f);
    const uint32_t idP = in.objectId ? in.objectId[p] : 0u;
    // prepare
    float c[3], b[3], d[3];
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k)
    {
        c[k] = in.color[3 * (size_t)p + k] * frame.colorScale;
        b[k] = in.colorHalf[3 * (size_t)p + k] * (2.0f * frame.colorScale);
        d[k] = denoiseAlbedoDivisor(in.albedo, pixels, p, k);
        if (in.albedo)
        {
            c[k] = c[k] / d[k];
            b[k] = b[k] / d[k];
        }
    }
    float a0 = c[0], a1 = c[1], a2 = c[2], b0 = b[0], b1 = b[1], b2 = b[2], length = 1.0f, motionX = 0.0f, motionY = 0.0f;   // a pixel that starts
    [[maybe_unused]] float confidence = 1.0f;
    if (in.recA)   // (uniform: NULL without history)
    {
        [[maybe_unused]] float4 mu, g;   // (k_temporal_moments' records of this pixel: two coalesced 16-byte loads, in flight beside the taps)
        if constexpr (kClip) { mu = temporalRecord(frame.momentMu, p); g = temporalRecord(frame.momentG, p); }
        // where the pixel's surface point was in the previous frame (pm, nm) and the id its object had there: its own, unless objects moved
        float4 pm = pp, nm = np;
        uint32_t idThen = idP;
        bool known = true;
        if constexpr (kMoving)
        {
            known = idP < frame.numObjects;   // (a miss carries RT_INVALID_OBJECT; the table is never read out of range)
            const float4* const record = frame.objects + 5u * (size_t)(known ? idP : 0u);
            const float4 r0 = temporalRecord(record, 0u), r1 = temporalRecord(record, 1u), r2 = temporalRecord(record, 2u), r3 = temporalRecord(record, 3u);
            const float4 tail = temporalRecord(record, 4u);
            const bool moved = __float_as_uint(tail.y) != 0u;
            idThen = __float_as_uint(tail.x);
            const float rows[3][4] = { { r0.x, r1.x, r2.x, r3.x }, { r0.y, r1.y, r2.y, r3.y }, { r0.z, r1.z, r2.z, r3.z } };   // [lane j] = m[0][j], m[1][j], m[2][j], m[3][j]
            float pj[3], nj[3];
#pragma unroll
            for (uint32_t j = 0; j < 3u; ++j)
            {
                pj[j] = pp.x * rows[j][0] + rows[j][3];
                pj[j] = pp.y * rows[j][1] + pj[j];
                pj[j] = pp.z * rows[j][2] + pj[j];
                nj[j] = np.x * rows[j][0];
                nj[j] = np.y * rows[j][1] + nj[j];
                nj[j] = np.z * rows[j][2] + nj[j];
            }
            pm = make_float4(moved ? pj[0] : pp.x, moved ? pj[1] : pp.y, moved ? pj[2] : pp.z, 0.0f);
            nm = make_float4(moved ? nj[0] : np.x, moved ? nj[1] : np.y, moved ? nj[2] : np.z, np.w);
        }
        // project: transformPoint's operations, lane by lane
        float t[4];
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j)
        {
            t[j] = pm.x * frame.m[j] + frame.m[12u + j];
            t[j] = pm.y * frame.m[4u + j] + t[j];
            t[j] = pm.z * frame.m[8u + j] + t[j];
        }
        const float u = (t[0] / t[3]) * 0.5f + 0.5f, v = (t[1] / t[3]) * 0.5f + 0.5f;
        const float fw = (float)w, fh = (float)h;
        const float fx = u * fw - frame.prevSampleOffset[0];
        const float fr = v * fh - frame.prevSampleOffset[1];
        const float fy = (float)(h - 1) - fr;
        const bool reaches = valid && known && t[2] > 0.0f && fx > -1.0f && fx < fw && fy > -1.0f && fy < fh;   // (false for a NaN; before any conversion to integer)
        // taps: a pixel that does not reach the previous frame takes them around (0, 0) and drops the lot
        const float sx = reaches ? fx : 0.0f, sy = reaches ? fy : 0.0f;
        const float flx = floorf(sx), fly = floorf(sy);
        const float tx = sx - flx, ty = sy - fly;
        const int32_t x0 = (int32_t)flx, y0 = (int32_t)fly;
        const float limit = frame.planeTolerance * depthP;
        float hA0 = 0.0f, hA1 = 0.0f, hA2 = 0.0f, hB0 = 0.0f, hB1 = 0.0f, hB2 = 0.0f, ln = 0.0f, ks = 0.0f;
#pragma unroll
        for (int32_t tb = 0; tb < 2; ++tb)
        {
#pragma unroll
            for (int32_t ta = 0; ta < 2; ++ta)
            {
                const int32_t qx = x0 + ta, qy = y0 + tb;
                const bool inside = qx >= 0 && qx < w && qy >= 0 && qy < h;
                const uint32_t q = inside ? (uint32_t)qy * width + (uint32_t)qx : p;
                const float4 aq = temporalRecord(in.recA, q), bq = temporalRecord(in.recB, q), nq = temporalRecord(in.recN, q), pq = temporalRecord(in.recP, q);
                const float k = (ta ? tx : 1.0f - tx) * (tb ? ty : 1.0f - ty);
                const float dpx = pq.x - pm.x, dpy = pq.y - pm.y, dpz = pq.z - pm.z;
                const float cosine = (nm.x * nq.x + nm.y * nq.y) + nm.z * nq.z;
                const float offset = fabsf((nm.x * dpx + nm.y * dpy) + nm.z * dpz);
                const bool sameObject = !frame.useIds || __float_as_uint(bq.w) == idThen;
                const bool take = reaches && inside && nq.w != 0.0f && sameObject && cosine >= frame.normalThreshold && offset <= limit;
                hA0 = take ? hA0 + k * aq.x : hA0;
                hA1 = take ? hA1 + k * aq.y : hA1;
                hA2 = take ? hA2 + k * aq.z : hA2;
                hB0 = take ? hB0 + k * bq.x : hB0;
                hB1 = take ? hB1 + k * bq.y : hB1;
                hB2 = take ? hB2 + k * bq.z : hB2;
                ln = take ? ln + k * aq.w : ln;
                ks = take ? ks + k : ks;
            }
        }
        if (ks > 0.0f)
        {
            // blend
            hA0 = hA0 / ks; hA1 = hA1 / ks; hA2 = hA2 / ks;
            hB0 = hB0 / ks; hB1 = hB1 / ks; hB2 = hB2 / ks;
            float n;
            if constexpr (kClip)
            {
                // clip A into mu +- g, shift B by what A moved, and cut the history length by how far that was against the box's width; a pixel whose
                // window holds too few of its surface keeps every value (selects), and with e == 0 the factor is exactly 1: the bits of the call without
                const bool clips = mu.w >= frame.minCount;
                const float c0 = fminf(fmaxf(hA0, mu.x - g.x), mu.x + g.x), c1 = fminf(fmaxf(hA1, mu.y - g.y), mu.y + g.y), c2 = fminf(fmaxf(hA2, mu.z - g.z), mu.z + g.z);
                const float s0 = c0 - hA0, s1 = c1 - hA1, s2 = c2 - hA2;
                const float e = (fabsf(s0) + fabsf(s1)) + fabsf(s2);
                const float wd = (g.x + g.y) + g.z;
                hB0 = clips ? hB0 + s0 : hB0; hB1 = clips ? hB1 + s1 : hB1; hB2 = clips ? hB2 + s2 : hB2;
                hA0 = clips ? c0 : hA0; hA1 = clips ? c1 : hA1; hA2 = clips ? c2 : hA2;
                confidence = clips && e > 0.0f ? wd / (wd + e) : 1.0f;
                n = fminf((ln / ks) * confidence + 1.0f, frame.maxHistory);
            }
            else n = fminf(ln / ks + 1.0f, frame.maxHistory);
            const float alpha = fmaxf(1.0f / n, frame.alphaMin);
            a0 = hA0 + alpha * (c[0] - hA0); a1 = hA1 + alpha * (c[1] - hA1); a2 = hA2 + alpha * (c[2] - hA2);
            b0 = hB0 + alpha * (b[0] - hB0); b1 = hB1 + alpha * (b[1] - hB1); b2 = hB2 + alpha * (b[2] - hB2);
            length = n;
            motionX = fx - (float)x; motionY = fy - (float)y;
        }
    }
    out.a[3 * (size_t)p + 0] = a0; out.a[3 * (size_t)p + 1] = a1; out.a[3 * (size_t)p + 2] = a2;
    out.b[3 * (size_t)p + 0] = b0; out.b[3 * (size_t)p + 1] = b1; out.b[3 * (size_t)p + 2] = b2;
    out.length[p] = length;
    if (out.motion) { out.motion[p] = motionX; out.motion[pixels + p] = motionY; }
    if constexpr (kClip) { if (frame.confidence) frame.confidence[p] = confidence; }
    if (out.recA)   // the context's next history: this frame's pair beside this frame's guides
    {
        out.recA[p] = make_float4(a0, a1, a2, length);
        out.recB[p] = make_float4(b0, b1, b2, __uint_as_float(idP));
        out.recN[p] = np;
        out.recP[p] = pp;
    }
    if (out.image) { out.image[3 * (size_t)p + 0] = a0 * d[0]; out.image[3 * (size_t)p + 1] = a1 * d[1]; out.image[3 * (size_t)p + 2] = a2 * d[2]; }
}

template __global__ void RT_ATROUS_ATTR k_temporal<false, false>(const TemporalIn, const TemporalOut, uint32_t, uint32_t, const TemporalFrame);
template __global__ void RT_ATROUS_ATTR k_temporal<true, false>(const TemporalIn, const TemporalOut, uint32_t, uint32_t, const TemporalFrameMoving);
template __global__ void RT_ATROUS_ATTR k_temporal<false, true>(const TemporalIn, const TemporalOut, uint32_t, uint32_t, const TemporalFrameClip<TemporalFrame>);
template __global__ void RT_ATROUS_ATTR k_temporal<true, true>(const TemporalIn, const TemporalOut, uint32_t, uint32_t, const TemporalFrameClip<TemporalFrameMoving>);
