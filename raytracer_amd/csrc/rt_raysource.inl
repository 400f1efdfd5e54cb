// rt_raysource.inl -- the ray source (include/rtgpu.h, rtgpu_set_ray_source): primary rays from a per-pixel table of the caller's in place of
// Camera::GenerateRay.  Included LAST by rt_trace.hip (k_generate_rays, k_ray_source_check, k_camera_rays) and, under RT_RAYSOURCE_DENSE, by rt_shade.hip
// (k_generate_dense_rays): the kernels in front of them keep the places in their code objects that they had before these existed.
//
// The table holds width * height entries of 32 bytes, row-major in sum-buffer coordinates: entry y * width + x = {origin xyz, -, direction xyz, -} is the
// primary ray of pixel (x, y), the direction as Ray() takes it (not normalised).  A slot reads its pixel from the slot -> pixel table and its entry as two
// 16-byte streaming loads -- the table is read once per pass -- and writes the records the camera kernels write, with the sampler and the per-pixel
// generator as resetPixel leaves them: a table ray is the ray of a camera that draws nothing.  Every consumer re-runs Ray() from the two records.

// the entry of pixel `pix` (x | y << 16) of a frame `width` wide
RT_DEV void raySourceLoad(const float4* __restrict__ rays, uint32_t pix, uint32_t width, float4& origin, float4& direction)
{
    const size_t entry = (size_t)(pix >> 16) * width + (pix & 0xFFFFu);
    origin = ldStream(rays[2u * entry]); direction = ldStream(rays[2u * entry + 1u]);
}

#ifndef RT_RAYSOURCE_DENSE
// k_generate (rt_generate.inl) fed from the table
__global__ void __launch_bounds__(RT_BLOCK) k_generate_rays(const RtSceneDesc scene, const DevPass* __restrict__ passes, uint32_t slotsPerPass,
                                                            const Paths paths, const uint32_t* __restrict__ slotPixel, uint32_t numSlots,
                                                            uint32_t* __restrict__ queue, uint32_t* __restrict__ queueCount,
                                                            unsigned long long* counters, const float4* __restrict__ rays)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < numSlots; slot += stride)
    {
        const uint32_t passInBatch = slot / slotsPerPass;
        const DevPass& pass = passes[passInBatch];
        const uint32_t pix = slotPixel[slot - passInBatch * slotsPerPass];
        Sampler sampler;
        sampler.seed = pass.seed; sampler.numDims = pass.numDimensions; sampler.blueNoiseLayers = pass.blueNoiseLayers; sampler.blueNoise = scene.blueNoise;
        sampler.resetPixel(pix & 0xFFFFu, pix >> 16, pass.rngKey[0], pass.rngKey[1]);
        float4 origin, direction;
        raySourceLoad(rays, pix, pass.width, origin, direction);
        prec(paths, R_ORIGIN, slot) = f4(origin.x, origin.y, origin.z, fbits(0x100u));   // depth 0, lastSpecular = true
        prec(paths, R_DIR, slot) = f4(direction.x, direction.y, direction.z, 1.0f);       // lastPdfW = 1
        prec(paths, R_TP, slot) = f4(1.0f, 1.0f, 1.0f, 1.0f);
        prec(paths, R_RESULT, slot) = f4(0.0f, 0.0f, 0.0f, fbits(pix));
        storeSampler(sampler, paths, slot, 0.0f, 0u);
        queue[slot] = slot;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
    {
        *queueCount = numSlots;
        atomicAdd(&counters[C_PRIMARY], (unsigned long long)numSlots);
    }
}

// The check of rtgpu_set_ray_source[_device]: one read-only pass over the context's copy of a table.  An entry is degenerate by the rule of the ray queries
// (queryRayIsDegenerate: a word of the origin or of the direction that is not finite, a direction whose squared length is 0 or not finite).  A block
// tallies in LDS and adds to *outDegenerate (zeroed by the host) once.
__global__ void __launch_bounds__(RT_BLOCK) k_ray_source_check(const float4* __restrict__ rays, uint32_t count, uint32_t* __restrict__ outDegenerate)
{
    __shared__ uint32_t sDegenerate;
    if (threadIdx.x == 0) sDegenerate = 0u;
    __syncthreads();
    uint32_t found = 0u;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride)
    {
        const float4 origin = ldStream(rays[2u * (size_t)i]), direction = ldStream(rays[2u * (size_t)i + 1u]);
        if (queryRayIsDegenerate(origin.x, origin.y, origin.z, 1.0f, direction.x, direction.y, direction.z)) found++;
    }
    if (found) atomicAdd(&sDegenerate, found);
    __syncthreads();
    if (threadIdx.x == 0 && sDegenerate != 0u) atomicAdd(outDegenerate, sDegenerate);
}

// rtgpu_read_camera_rays: what k_generate stores for every pixel of the frame -- cameraGenerateRayParts, written out in the table's layout and order.  The
// camera draws nothing (the host refuses depth of field and the variable barrel factor), so the sampler is never read.
__global__ void __launch_bounds__(RT_BLOCK) k_camera_rays(const RtCamera camera, float sampleOffsetX, float sampleOffsetY, uint32_t width, uint32_t height, float4* __restrict__ out)
{
    const uint32_t count = width * height, stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride)
    {
        const uint32_t y = i / width, x = i - y * width;
        const uint32_t realY = height - 1u - y;
        const float invW = 1.0f / (float)(int32_t)width, invH = 1.0f / (float)(int32_t)height;
        const V4 coords(((float)(int32_t)x + sampleOffsetX) * invW, ((float)(int32_t)realY + sampleOffsetY) * invH, 0.0f, 0.0f);
        Sampler sampler;
        sampler.seed = nullptr; sampler.numDims = 0u; sampler.blueNoiseLayers = 0u; sampler.blueNoise = nullptr;
        sampler.resetPixel(x, y, 0ull, 0ull);
        V4 origin, direction;
        cameraGenerateRayParts(camera, coords, sampler, origin, direction);
        out[2u * (size_t)i] = f4(origin.x, origin.y, origin.z, 0.0f);
        out[2u * (size_t)i + 1u] = f4(direction.x, direction.y, direction.z, 0.0f);
    }
}

#else   // RT_RAYSOURCE_DENSE
// k_generate_dense (rt_dense.inl) fed from the table: origin and direction only -- bounce 0's shade rebuilds the rest from the slot, and its camera re-run
// (denseShadeVertex) leaves the sampler where resetPixel put it, because the host hands the batch a camera that draws nothing
__global__ void __launch_bounds__(RT_BLOCK) k_generate_dense_rays(const RtSceneDesc scene, const DevPass* __restrict__ passes, uint32_t slotsPerPass, const Paths paths,
                                                                  const uint32_t* __restrict__ slotPixel, uint32_t numSlots, uint32_t shardCapacity, uint32_t* __restrict__ counts,
                                                                  unsigned long long* counters, const float4* __restrict__ rays)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < numSlots; slot += stride)
    {
        const uint32_t passInBatch = slot / slotsPerPass;
        const uint32_t pix = slotPixel[slot - passInBatch * slotsPerPass];
        float4 origin, direction;
        raySourceLoad(rays, pix, passes[passInBatch].width, origin, direction);
        stStream(prec(paths, R_ORIGIN, slot), f4(origin.x, origin.y, origin.z, fbits(0x100u)));   // depth 0, lastSpecular = true
        stStream(prec(paths, R_DIR, slot), f4(direction.x, direction.y, direction.z, 1.0f));       // lastPdfW = 1
    }
    if (blockIdx.x == 0 && threadIdx.x < RT_DENSE_SHARDS)
    {
        const uint32_t first = threadIdx.x * shardCapacity;
        counts[threadIdx.x] = first >= numSlots ? 0u : (numSlots - first < shardCapacity ? numSlots - first : shardCapacity);
        if (threadIdx.x == 0) atomicAdd(&counters[C_PRIMARY], (unsigned long long)numSlots);
    }
}
#endif
