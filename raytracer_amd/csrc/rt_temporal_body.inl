// rt_temporal_body.inl -- the temporal accumulation kernel.  rt_temporal.inl, which describes it, includes it twice: as k_temporal (RT_TEMPORAL_CHAIN 0: the blocks
// under that switch are not there) and as k_temporal_chain (RT_TEMPORAL_CHAIN 1), rtgpu_temporal_accumulate_chain's variant over chain guides: three coalesced
// plane loads more (the chain length, the chain distance and -- static frames only -- the virtual position), one integer compare per tap against the chain
// length in the free lane of the {P.xyz, .} history record, and that lane written for the next frame.  With objects moved a pixel with a chain starts, so the
// moving variant projects the moved first-hit pair as ever and never loads the virtual position.
// k_temporal's third argument, kDeform (moving variants only; k_temporal_chain has none: a pixel with a chain starts when anything moved): an object whose
// motion record says RT_MOTION_DEFORMED takes its point of then from the triangle record its mesh had then.
#if RT_TEMPORAL_CHAIN
template <bool kMoving, bool kClip> __global__ void RT_ATROUS_ATTR RT_TEMPORAL_KERNEL RT_K_TEMPORAL_CHAIN_ARGS
#else
template <bool kMoving, bool kClip, bool kDeform> __global__ void RT_ATROUS_ATTR RT_TEMPORAL_KERNEL RT_K_TEMPORAL_ARGS
#endif
{
#if RT_TEMPORAL_CHAIN
    constexpr bool kDeform = false;
#endif
    static_assert(kMoving || !kDeform, "a deformed mesh is followed through the motion table");
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
#if RT_TEMPORAL_CHAIN
    const uint32_t chainP = chain.chainLength[p];
#endif
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
#if RT_TEMPORAL_CHAIN
            known = known && chainP == 0u;   // the virtual image of a scene in which something moved is not followed
#endif
            const float4* const record = frame.objects + 5u * (size_t)(known ? idP : 0u);
            const float4 r0 = temporalRecord(record, 0u), r1 = temporalRecord(record, 1u), r2 = temporalRecord(record, 2u), r3 = temporalRecord(record, 3u);
            const float4 tail = temporalRecord(record, 4u);
            const bool moved = __float_as_uint(tail.y) != 0u;
            idThen = __float_as_uint(tail.x);
            // the point the matrix takes: the pixel's own position, or -- on a deformed mesh -- where the old triangle record puts its barycentrics
            float4 from = pp;
            [[maybe_unused]] bool deformed = false;
            if constexpr (kDeform)
            {
                deformed = known && __float_as_uint(tail.y) == RT_MOTION_DEFORMED;
                const uint32_t first = __float_as_uint(tail.z), count = __float_as_uint(tail.w), t = frame.subObjectId[p];
                const float bu = frame.barycentrics[p], bv = frame.barycentrics[pixels + p];
                // (in 64 bits: first + t cannot wrap; a lane outside either range starts, and loads nothing)
                const bool inRange = t < count && (uint64_t)first + t < (uint64_t)frame.numPrevTriangles;
                known = known && (!deformed || inRange);
                if (deformed && inRange)
                {
                    const float* const tri = frame.prevTriangles + 9u * ((size_t)first + t);   // {v0, edge1, edge2}: nine dword loads
                    float l[3];
#pragma unroll
                    for (uint32_t k = 0; k < 3u; ++k)
                    {
                        l[k] = tri[3u + k] * bu + tri[k];
                        l[k] = tri[6u + k] * bv + l[k];
                    }
                    from = make_float4(l[0], l[1], l[2], 0.0f);
                }
            }
            const float rows[3][4] = { { r0.x, r1.x, r2.x, r3.x }, { r0.y, r1.y, r2.y, r3.y }, { r0.z, r1.z, r2.z, r3.z } };   // [lane j] = m[0][j], m[1][j], m[2][j], m[3][j]
            float pj[3], nj[3];
#pragma unroll
            for (uint32_t j = 0; j < 3u; ++j)
            {
                pj[j] = from.x * rows[j][0] + rows[j][3];
                pj[j] = from.y * rows[j][1] + pj[j];
                pj[j] = from.z * rows[j][2] + pj[j];
                nj[j] = np.x * rows[j][0];
                nj[j] = np.y * rows[j][1] + nj[j];
                nj[j] = np.z * rows[j][2] + nj[j];
            }
            pm = make_float4(moved ? pj[0] : pp.x, moved ? pj[1] : pp.y, moved ? pj[2] : pp.z, 0.0f);
            const bool turned = moved && !deformed;   // (a deformed surface keeps this frame's normal: normalThreshold takes what the deformation turned it by)
            nm = make_float4(turned ? nj[0] : np.x, turned ? nj[1] : np.y, turned ? nj[2] : np.z, np.w);
        }
        // project: transformPoint's operations, lane by lane
#if RT_TEMPORAL_CHAIN
        // (a static frame's chain guides: the virtual position in the position's place)
        if constexpr (!kMoving) pm = make_float4(chain.virtualPosition[p], chain.virtualPosition[pixels + p], chain.virtualPosition[2 * pixels + p], 0.0f);
#endif
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
#if RT_TEMPORAL_CHAIN
        if constexpr (!kMoving) pm = pp;   // (the surface tests compare the guide vertex's own position)
        const float limit = frame.planeTolerance * chain.chainDistance[p];   // the unfolded path length: inside a reflection the last segment's is the wrong scale
#else
        const float limit = frame.planeTolerance * depthP;
#endif
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
#if RT_TEMPORAL_CHAIN
                const bool take = reaches && inside && nq.w != 0.0f && sameObject && cosine >= frame.normalThreshold && offset <= limit && __float_as_uint(pq.w) == chainP;
#else
                const bool take = reaches && inside && nq.w != 0.0f && sameObject && cosine >= frame.normalThreshold && offset <= limit;
#endif
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
#if RT_TEMPORAL_CHAIN
        out.recP[p] = make_float4(pp.x, pp.y, pp.z, __uint_as_float(chainP));
#else
        out.recP[p] = pp;
#endif
    }
    if (out.image) { out.image[3 * (size_t)p + 0] = a0 * d[0]; out.image[3 * (size_t)p + 1] = a1 * d[1]; out.image[3 * (size_t)p + 2] = a2 * d[2]; }
}
