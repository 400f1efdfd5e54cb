// rt_raysource.inl -- the primary-ray sources (include/rtgpu.h): primary rays from a per-pixel table of the caller's in place of Camera::GenerateRay.
// Included LAST by rt_trace.hip (the slot-layout generate kernels, the two checks, the three exports) and, under RT_RAYSOURCE_DENSE, by rt_shade.hip (the dense
// generate kernels): the kernels in front of them keep the places in their code objects that they had before these existed.  Every generate kernel is
// generatePaths (rt_device_state.h), the body k_generate and k_generate_dense have, around its table's "ray of this pixel".
//
// The ray source (rtgpu_set_ray_source): width * height entries of 32 bytes, row-major in sum-buffer coordinates: entry y * width + x = {origin xyz, -,
// direction xyz, -} is the primary ray of pixel (x, y), the direction as Ray() takes it (not normalised).  A slot reads its entry as two 16-byte streaming loads
// -- the table is read once per pass -- and leaves the sampler and the per-pixel generator as resetPixel leaves them: a table ray is the ray of a camera that
// draws nothing.  Every consumer re-runs Ray() from the two records.
//
// The lens source (rtgpu_set_lens_source): a table of RECIPES -- a ray, its footprint per unit of the pass's sampleOffset, a thin lens.  An entry is RtLensRay:
// 128 bytes, eight float4, one aligned cache line per lane, read once per pass -- eight 16-byte streaming loads issued together (32 VGPRs in flight; the
// generate kernels hold little else, and the line is wholly consumed by the lane that fetched it, so nothing is read twice).
//   0 origin | aperture   1 direction | focalDistance   2, 3 dOrigin/dsx, /dsy   4, 5 dDirection/dsx, /dsy   6, 7 lensU, lensV   (w of 2..7: never read)

// the plain table as generatePaths' `rayOf`: the entry of pixel `pix` (x | y << 16)
struct TableRayOf
{
    static constexpr bool kFromFilm = false;
    const float4* __restrict__ rays;
    __device__ __forceinline__ void operator()(const DevPass& pass, uint32_t pix, V4, Sampler&, V4& origin, V4& direction) const
    {
        const size_t entry = (size_t)(pix >> 16) * pass.width + (pix & 0xFFFFu);
        const float4 o = ldStream(rays[2u * entry]), d = ldStream(rays[2u * entry + 1u]);
        origin = V4(o.x, o.y, o.z, 0.0f); direction = V4(d.x, d.y, d.z, 0.0f);
    }
};

// one component of the jitter step: (v + sx * dvdsx) + sy * dvdsy, every operation rounded on its own (tests/lens_source_ref.py is the same text)
RT_DEV float lensJitter(float v, float sx, float dvdsx, float sy, float dvdsy) { return __fadd_rn(__fadd_rn(v, __fmul_rn(sx, dvdsx)), __fmul_rn(sy, dvdsy)); }

// queryRayIsDegenerate (rt_trace_kernels.h) without its maxDistance, word for word: an origin word that is not finite, a direction whose squared length (dot3's
// sum, the one Ray() takes the root of) is 0 or not finite.  A COPY, kept on the compiler's evidence: with the guard calling the one rule (maxDistance 1, from a
// header both units see) k_generate_lens takes 76 VGPRs for its 72 and six waves for seven -- around its own loop as around generatePaths, through a V4 wrapper
// and with the rule force-inlined alike -- and a limit of seven waves makes it spill (profiles/source_unify_resources_diff.txt is taken with the copy).
// k_lens_source_check holds the stored rays to the original; the two must stay the same rule.
RT_DEV bool lensRayIsDegenerate(V4 o, V4 d)
{
    const float lengthSq = (d.x * d.x + d.y * d.y) + (d.z * d.z + 0.0f);
    const bool originFinite = isfinite(o.x) && isfinite(o.y) && isfinite(o.z);
    return !originFinite || !(lengthSq > 0.0f && lengthSq <= 3.402823466e+38f);
}

// The dofEnable branch of cameraGenerateRayParts (rt_device_core.h; Camera.cpp:104-114) with the entry's focal distance, aperture and lens axes in the places
// of the camera's and of its transform's rows 0 and 1.  It is a COPY, operation for operation: calling one shared function from the camera moved
// k_camera_rays by a scalar register, by value and by reference alike (profiles/lens_source_resources_diff.txt is taken with the camera's branch as it
// was), and cameraGenerateRayParts is inlined into the hottest shading kernels, whose generated code is held.  Whoever edits one edits the other:
// tests/test_gpu_lens_source.py holds the two together bit for bit in all three shapes.
RT_DEV void lensSourceThinLens(float focalDistance, uint32_t bokehShape, float aperture, V4 lensU, V4 lensV, Sampler& sampler, V4& origin, V4& direction)
{
    const V4 focusPoint = mulAdd(direction, focalDistance, origin);
    const float sx = sampler.getFloat(); const float sy = sampler.getFloat();
    // circle, hexagon (the third sample coordinate is always 0: its first rhombus, SamplingHelpers.cpp:40-57), square
    V4 bokeh;
    if (bokehShape == 1u) bokeh = V4(sx * -1.0f + sy * 0.5f, sx * 0.0f + sy * 0.8660254f, 0.0f, 0.0f);
    else if (bokehShape == 2u) bokeh = mulSub(V4(sx, sy, 0.0f, 0.0f), 2.0f, splat(1.0f));
    else bokeh = getCircle(sx, sy);
    const V4 randomPointOnCircle = bokeh * aperture;
    origin = mulAdd(splat(randomPointOnCircle.x), lensU, origin);
    origin = mulAdd(splat(randomPointOnCircle.y), lensV, origin);
    direction = focusPoint - origin;
}

// The ray of pixel `pix` (x | y << 16) of a frame `width` wide for a pass with sample offset (sx, sy) -- include/rtgpu.h defines it operation by operation:
// jitter (none at offset (0, 0): the stored words pass through, a -0.0 included), the camera's thin lens under `lens` (two draws from `sampler`, whatever the
// entry's aperture), and the guard: a final ray that is degenerate by queryRayIsDegenerate is replaced by the stored one, which the set call has checked.
RT_DEV void lensSourceRay(const float4* __restrict__ table, uint32_t pix, uint32_t width, float sx, float sy, uint32_t lens, uint32_t bokehShape, Sampler& sampler,
                          V4& origin, V4& direction)
{
    const float4* entry = table + 8u * ((size_t)(pix >> 16) * width + (pix & 0xFFFFu));
    const float4 q0 = ldStream(entry[0]), q1 = ldStream(entry[1]), q2 = ldStream(entry[2]), q3 = ldStream(entry[3]);
    const float4 q4 = ldStream(entry[4]), q5 = ldStream(entry[5]), q6 = ldStream(entry[6]), q7 = ldStream(entry[7]);
    origin = V4(q0.x, q0.y, q0.z, 0.0f); direction = V4(q1.x, q1.y, q1.z, 0.0f);
    if (!(sx == 0.0f && sy == 0.0f))
    {
        origin = V4(lensJitter(q0.x, sx, q2.x, sy, q3.x), lensJitter(q0.y, sx, q2.y, sy, q3.y), lensJitter(q0.z, sx, q2.z, sy, q3.z), 0.0f);
        direction = V4(lensJitter(q1.x, sx, q4.x, sy, q5.x), lensJitter(q1.y, sx, q4.y, sy, q5.y), lensJitter(q1.z, sx, q4.z, sy, q5.z), 0.0f);
    }
    if (lens) lensSourceThinLens(q1.w, bokehShape, q0.w, V4(q6.x, q6.y, q6.z, 0.0f), V4(q7.x, q7.y, q7.z, 0.0f), sampler, origin, direction);
    if (lensRayIsDegenerate(origin, direction))
    {
        origin = V4(q0.x, q0.y, q0.z, 0.0f); direction = V4(q1.x, q1.y, q1.z, 0.0f);
    }
}
// the lens table as generatePaths' `rayOf`: the sampler goes into the path's records where the lens left it
struct LensRayOf
{
    static constexpr bool kFromFilm = false;
    const float4* __restrict__ table; uint32_t lens, bokehShape;
    __device__ __forceinline__ void operator()(const DevPass& pass, uint32_t pix, V4, Sampler& sampler, V4& origin, V4& direction) const
    {
        lensSourceRay(table, pix, pass.width, pass.sampleOffset[0], pass.sampleOffset[1], lens, bokehShape, sampler, origin, direction);
    }
};

#ifndef RT_RAYSOURCE_DENSE
// k_generate (rt_generate.inl) fed from the table
__global__ void __launch_bounds__(RT_BLOCK) k_generate_rays(const RtSceneDesc scene, const DevPass* __restrict__ passes, uint32_t slotsPerPass,
                                                            const Paths paths, const uint32_t* __restrict__ slotPixel, uint32_t numSlots,
                                                            uint32_t* __restrict__ queue, uint32_t* __restrict__ queueCount,
                                                            unsigned long long* counters, const float4* __restrict__ rays)
{
    generatePaths<false>(RT_GRID_STRIDE, scene.blueNoise, passes, slotsPerPass, paths, slotPixel, numSlots, queue, TableRayOf{ rays });
    generateQueueCount(queueCount, counters, numSlots);
}

// The two checks' tally: a block adds what its lanes found in its LDS word `tally` and adds that to *outRefused (zeroed by the host) once.  (Two halves around
// the kernel's own loop: with the loop inside one shared body k_lens_source_check takes 38 VGPRs for its 13.)
RT_DEV void sourceTallyBegin(uint32_t& tally)
{
    if (threadIdx.x == 0) tally = 0u;
    __syncthreads();
}
RT_DEV void sourceTallyEnd(uint32_t& tally, uint32_t found, uint32_t* __restrict__ outRefused)
{
    if (found) atomicAdd(&tally, found);
    __syncthreads();
    if (threadIdx.x == 0 && tally != 0u) atomicAdd(outRefused, tally);
}

// The check of rtgpu_set_ray_source[_device]: one read-only pass over the context's copy of a table.  An entry is degenerate by the rule of the ray queries
// (queryRayIsDegenerate: a word of the origin or of the direction that is not finite, a direction whose squared length is 0 or not finite).
__global__ void __launch_bounds__(RT_BLOCK) k_ray_source_check(const float4* __restrict__ rays, uint32_t count, uint32_t* __restrict__ outDegenerate)
{
    __shared__ uint32_t sDegenerate;
    sourceTallyBegin(sDegenerate);
    uint32_t found = 0u;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride)
    {
        const float4 origin = ldStream(rays[2u * (size_t)i]), direction = ldStream(rays[2u * (size_t)i + 1u]);
        if (queryRayIsDegenerate(origin.x, origin.y, origin.z, 1.0f, direction.x, direction.y, direction.z)) found++;
    }
    sourceTallyEnd(sDegenerate, found, outDegenerate);
}

// rtgpu_read_camera_rays: what k_generate stores for every pixel of the frame -- cameraGenerateRayParts, written out in the table's layout and order.  The
// camera draws nothing (the host refuses depth of field and the variable barrel factor), so the sampler is never read.
__global__ void __launch_bounds__(RT_BLOCK) k_camera_rays(const RtCamera camera, float sampleOffsetX, float sampleOffsetY, uint32_t width, uint32_t height, float4* __restrict__ out)
{
    const uint32_t count = width * height, stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride)
    {
        const uint32_t y = i / width, x = i - y * width;
        const V4 coords = filmCoords(x, y, width, height, sampleOffsetX, sampleOffsetY);
        Sampler sampler;
        sampler.seed = nullptr; sampler.numDims = 0u; sampler.blueNoiseLayers = 0u; sampler.blueNoise = nullptr;
        sampler.resetPixel(x, y, 0ull, 0ull);
        V4 origin, direction;
        cameraGenerateRayParts(camera, coords, sampler, origin, direction);
        out[2u * (size_t)i] = f4(origin.x, origin.y, origin.z, 0.0f);
        out[2u * (size_t)i + 1u] = f4(direction.x, direction.y, direction.z, 0.0f);
    }
}

// k_generate fed from the lens table
__global__ void __launch_bounds__(RT_BLOCK) k_generate_lens(const RtSceneDesc scene, const DevPass* __restrict__ passes, uint32_t slotsPerPass,
                                                            const Paths paths, const uint32_t* __restrict__ slotPixel, uint32_t numSlots,
                                                            uint32_t* __restrict__ queue, uint32_t* __restrict__ queueCount,
                                                            unsigned long long* counters, const float4* __restrict__ table, uint32_t lens, uint32_t bokehShape)
{
    generatePaths<false>(RT_GRID_STRIDE, scene.blueNoise, passes, slotsPerPass, paths, slotPixel, numSlots, queue, LensRayOf{ table, lens, bokehShape });
    generateQueueCount(queueCount, counters, numSlots);
}

// The check of rtgpu_set_lens_source[_device]: one read-only pass over the context's copy of a table.  An entry is refused if one of its interpreted words is
// not finite (origin, direction, the four derivatives, the two lens axes, aperture, focalDistance), if its stored ray is degenerate by
// queryRayIsDegenerate, or -- under `lens` -- if its focalDistance is not > 0.  The w lanes of quads 2..7 are never tested.
__global__ void __launch_bounds__(RT_BLOCK) k_lens_source_check(const float4* __restrict__ table, uint32_t count, uint32_t lens, uint32_t* __restrict__ outRefused)
{
    __shared__ uint32_t sRefused;
    sourceTallyBegin(sRefused);
    uint32_t found = 0u;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride)
    {
        const float4* entry = table + 8u * (size_t)i;
        const float4 q0 = ldStream(entry[0]), q1 = ldStream(entry[1]);
        bool finite = isfinite(q0.x) && isfinite(q0.y) && isfinite(q0.z) && isfinite(q0.w) && isfinite(q1.x) && isfinite(q1.y) && isfinite(q1.z) && isfinite(q1.w);
        for (uint32_t k = 2u; k < 8u; ++k)
        {
            const float4 q = ldStream(entry[k]);
            finite = finite && isfinite(q.x) && isfinite(q.y) && isfinite(q.z);
        }
        if (!finite || queryRayIsDegenerate(q0.x, q0.y, q0.z, 1.0f, q1.x, q1.y, q1.z) || (lens && !(q1.w > 0.0f))) found++;
    }
    sourceTallyEnd(sRefused, found, outRefused);
}

// rtgpu_read_lens_source_rays: for every pixel of the frame the origin and direction a pass would start from under the lens table, the two lens draws
// included, in the plain table's layout and order (words 3 and 7 zero).  Not a pass: the sampler is rebuilt from the pass's constants, which arrive by value
// -- the lens draws are the sampler's first two, so two seed words are all of the seed array that can be read (numDims: the pass's, clipped to 2).
__global__ void __launch_bounds__(RT_BLOCK) k_lens_source_rays(const float4* __restrict__ table, uint32_t width, uint32_t height, float sx, float sy, uint32_t lens,
                                                               uint32_t bokehShape, uint32_t seed0, uint32_t seed1, uint32_t numDims, uint32_t blueNoiseLayers,
                                                               const uint16_t* __restrict__ blueNoise, unsigned long long rngKey0, unsigned long long rngKey1,
                                                               float4* __restrict__ out)
{
    __shared__ uint32_t seeds[2];   // (the sampler reads its seeds through a pointer)
    if (threadIdx.x == 0) { seeds[0] = seed0; seeds[1] = seed1; }
    __syncthreads();
    const uint32_t count = width * height, stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride)
    {
        const uint32_t y = i / width, x = i - y * width;
        Sampler sampler;
        sampler.seed = seeds; sampler.numDims = numDims; sampler.blueNoiseLayers = blueNoiseLayers; sampler.blueNoise = blueNoise;
        sampler.resetPixel(x, y, rngKey0, rngKey1);
        V4 origin, direction;
        lensSourceRay(table, x | (y << 16), width, sx, sy, lens, bokehShape, sampler, origin, direction);
        out[2u * (size_t)i] = f4(origin.x, origin.y, origin.z, 0.0f);
        out[2u * (size_t)i + 1u] = f4(direction.x, direction.y, direction.z, 0.0f);
    }
}

// rtgpu_read_camera_footprints: the camera as a lens table.  Origin and pinhole direction are cameraGenerateRayParts' at the pass's sample offset with the
// lens off (the host passes the camera with dofEnable cleared and refuses the variable barrel factor, so nothing is drawn); the direction's derivatives are
// analytic -- coords.x = (x + sx) / W enters the direction as r[0] * ((2 coords.x - 1) * aspectRatio * tanHalfFoV), and rows flip but realY + sy does not, so
// d/dsy keeps the camera's sign; a pinhole's origin does not move.  aperture, focalDistance and the lens axes are the camera's own.
__global__ void __launch_bounds__(RT_BLOCK) k_camera_footprints(const RtCamera camera, float sampleOffsetX, float sampleOffsetY, uint32_t width, uint32_t height, float4* __restrict__ out)
{
    const uint32_t count = width * height, stride = gridDim.x * blockDim.x;
    const M4 transform = loadM4(camera.localToWorld);
    const float invW = 1.0f / (float)(int32_t)width, invH = 1.0f / (float)(int32_t)height;
    const float scaleX = 2.0f * invW * camera.aspectRatio * camera.tanHalfFoV, scaleY = 2.0f * invH * camera.tanHalfFoV;
    const V4 ddx = transform.r[0] * scaleX, ddy = transform.r[1] * scaleY;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride)
    {
        const uint32_t y = i / width, x = i - y * width;
        const V4 coords = filmCoords(x, y, width, height, sampleOffsetX, sampleOffsetY);
        Sampler sampler;
        sampler.seed = nullptr; sampler.numDims = 0u; sampler.blueNoiseLayers = 0u; sampler.blueNoise = nullptr;
        sampler.resetPixel(x, y, 0ull, 0ull);
        V4 origin, direction;
        cameraGenerateRayParts(camera, coords, sampler, origin, direction);
        float4* entry = out + 8u * (size_t)i;
        entry[0] = f4(origin.x, origin.y, origin.z, camera.aperture);
        entry[1] = f4(direction.x, direction.y, direction.z, camera.focalPlaneDistance);
        entry[2] = f4(0.0f, 0.0f, 0.0f, 0.0f);
        entry[3] = f4(0.0f, 0.0f, 0.0f, 0.0f);
        entry[4] = f4(ddx.x, ddx.y, ddx.z, 0.0f);
        entry[5] = f4(ddy.x, ddy.y, ddy.z, 0.0f);
        entry[6] = f4(transform.r[0].x, transform.r[0].y, transform.r[0].z, 0.0f);
        entry[7] = f4(transform.r[1].x, transform.r[1].y, transform.r[1].z, 0.0f);
    }
}

#else   // RT_RAYSOURCE_DENSE
// k_generate_dense (rt_dense.inl) fed from the table: bounce 0's camera re-run (denseShadeVertex) leaves the sampler where resetPixel put it, because the host
// hands the batch a camera that draws nothing
__global__ void __launch_bounds__(RT_BLOCK) k_generate_dense_rays(const RtSceneDesc scene, const DevPass* __restrict__ passes, uint32_t slotsPerPass, const Paths paths,
                                                                  const uint32_t* __restrict__ slotPixel, uint32_t numSlots, uint32_t shardCapacity, uint32_t* __restrict__ counts,
                                                                  unsigned long long* counters, const float4* __restrict__ rays)
{
    generatePaths<true>(RT_GRID_STRIDE, scene.blueNoise, passes, slotsPerPass, paths, slotPixel, numSlots, nullptr, TableRayOf{ rays });
    generateShardCounts(counts, shardCapacity, counters, numSlots);
}

// k_generate_dense fed from the lens table: bounce 0's camera re-run takes the lens's two draws again from the same reset sampler, because the host hands the
// batch a zeroed camera whose dofEnable and bokehShape are the source's (makeDevPass): the sampler then stands where the draws here left it
__global__ void __launch_bounds__(RT_BLOCK) k_generate_dense_lens(const RtSceneDesc scene, const DevPass* __restrict__ passes, uint32_t slotsPerPass, const Paths paths,
                                                                  const uint32_t* __restrict__ slotPixel, uint32_t numSlots, uint32_t shardCapacity, uint32_t* __restrict__ counts,
                                                                  unsigned long long* counters, const float4* __restrict__ table, uint32_t lens, uint32_t bokehShape)
{
    generatePaths<true>(RT_GRID_STRIDE, scene.blueNoise, passes, slotsPerPass, paths, slotPixel, numSlots, nullptr, LensRayOf{ table, lens, bokehShape });
    generateShardCounts(counts, shardCapacity, counters, numSlots);
}
#endif
