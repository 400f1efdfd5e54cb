// rt_runtime_kat.inl -- the known-answer hooks of the test suite (rtgpu_kat*) and rtgpu_evaluate_textures.  Included by rt_runtime.hip.

// round trip of a host buffer through one of the KAT kernels (synchronous, lane 0's stream)
template <typename Launch>
static int katRoundTrip(RtgpuContext* c, const void* in, size_t inBytes, void* out, size_t outBytes, Launch launch)
{
    HIP_TRY(hipSetDevice(c->device));
    void* dIn = nullptr; void* dOut = nullptr;
    hipError_t e = hipMalloc(&dIn, inBytes ? inBytes : 4);
    if (e == hipSuccess) e = hipMalloc(&dOut, outBytes ? outBytes : 4);
    if (e == hipSuccess) e = rtMemcpy(dIn, in, inBytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemsetAsync(dOut, 0, outBytes, c->lanes[0].stream);   // on the kernel's stream: the lanes do not synchronise with the null stream
    if (e == hipSuccess)
    {
        launch(dIn, dOut, c->lanes[0].stream);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(c->lanes[0].stream);
    }
    if (e == hipSuccess) e = rtMemcpy(out, dOut, outBytes, hipMemcpyDeviceToHost);
    devFree(dIn, dOut);
    if (e != hipSuccess) return fail(RTGPU_ERR_DEVICE, std::string("rtgpu_kat: ") + hipGetErrorString(e));
    return RTGPU_OK;
}

RTGPU_API int rtgpu_kat(RtgpuContext* c, uint32_t func, const float* in, uint32_t inStride, float* out, uint32_t outStride, uint32_t n)
{
    if (!c || (n && (!in || !out))) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n == 0) return RTGPU_OK;
    static const struct { uint32_t func, minIn, minOut; } known[] = {
        { KAT_SIN_LANE, 1, 1 }, { KAT_SINCOS, 1, 4 }, { KAT_FASTLOG, 1, 1 }, { KAT_FASTACOS, 1, 1 }, { KAT_FASTATAN2, 2, 1 }, { KAT_FLOAT_NORMAL2, 2, 4 },
        { KAT_HEMISPHERE_COS, 2, 4 }, { KAT_SPHERE, 2, 4 }, { KAT_CIRCLE, 2, 4 }, { KAT_ORTHO_BASIS, 4, 8 }, { KAT_FRESNEL_DIELECTRIC, 2, 1 },
        { KAT_FRESNEL_METAL, 3, 1 }, { KAT_REFRACT3, 9, 4 }, { KAT_REFLECT3, 8, 4 }, { KAT_BOX_RAY, 14, 2 }, { KAT_BOX_RAY_TWOSIDED, 14, 3 },
        { KAT_TRIANGLE_RAY, 17, 4 }, { KAT_MAKE_RAY, 8, 12 }, { KAT_TRANSFORM_RAY, 24, 16 }, { KAT_FAST_INVERSE, 16, 16 }, { KAT_TRANSFORM_SCALED, 20, 12 }, { KAT_FRAME_COMPOSE, 40, 20 }, { KAT_SHAPE_INTERSECT, 13, 4 },
        { KAT_SHAPE_SAMPLE, 12, 8 }, { KAT_SHAPE_PDF, 13, 1 }, { KAT_SHAPE_EVAL, 13, 16 },
        { KAT_LIGHT_ILLUMINATE, (uint32_t)(sizeof(RtLight) / 4) + 19, 11 }, { KAT_LIGHT_RADIANCE, (uint32_t)(sizeof(RtLight) / 4) + 13, 5 },
        { KAT_LIGHT_EMIT, (uint32_t)(sizeof(RtLight) / 4) + 5, 15 }, { KAT_LIGHT_ILLUMINATE_BIDIR, (uint32_t)(sizeof(RtLight) / 4) + 19, 12 },
        { KAT_LIGHT_RADIANCE_BIDIR, (uint32_t)(sizeof(RtLight) / 4) + 13, 6 }, { KAT_BSDF_SAMPLE, 23, 11 }, { KAT_BSDF_EVALUATE, 24, 5 }, { KAT_BSDF_PDFS, 24, 8 },
        { KAT_CAMERA_RAY, (uint32_t)(sizeof(RtCamera) / 4) + 8, 16 }, { KAT_CAMERA_FILM, (uint32_t)(sizeof(RtCamera) / 4) + 8, 6 }, { KAT_FILM_SPLAT, 12, 10 },
        { KAT_PACKED_PHOTON, 8, 11 }, { KAT_HSV_TO_RGB, 2, 4 } };
    bool ok = false;
    for (const auto& k : known) if (k.func == func) { if (inStride < k.minIn || outStride < k.minOut) return fail(RTGPU_ERR_INVALID_ARGUMENT, "rtgpu_kat: record stride too small for this function"); ok = true; }
    if (!ok) return fail(RTGPU_ERR_INVALID_ARGUMENT, "rtgpu_kat: unknown function id");
    RtSceneDesc none; memset(&none, 0, sizeof(none));   // the fixtures' lights and materials carry no textures
    return katRoundTrip(c, in, (size_t)n * inStride * 4, out, (size_t)n * outStride * 4, [&](void* dIn, void* dOut, hipStream_t st) {
        hipLaunchKernelGGL(k_kat, dim3((n + 63u) / 64u), dim3(64), 0, st, none, func, (const float*)dIn, inStride, (float*)dOut, outStride, n);
    });
}

RTGPU_API int rtgpu_kat_sampler(RtgpuContext* c, const uint16_t* blueNoise, const uint32_t* in, uint32_t inStride, uint32_t count, uint32_t n, uint32_t* outInts, float* outFloats)
{
    if (!c || !in || !outInts || !outFloats || n == 0 || count == 0) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    for (uint32_t r = 0; r < n; ++r) if (inStride < 4u + in[(size_t)r * inStride + 3]) return fail(RTGPU_ERR_INVALID_ARGUMENT, "rtgpu_kat_sampler: record shorter than its seed table");
    HIP_TRY(hipSetDevice(c->device));
    uint16_t* dBlue = nullptr;
    if (blueNoise)
    {
        HIP_TRY(hipMalloc((void**)&dBlue, (size_t)128 * 128 * 4 * sizeof(uint16_t)));
        const hipError_t e = rtMemcpy(dBlue, blueNoise, (size_t)128 * 128 * 4 * sizeof(uint16_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(dBlue); return fail(RTGPU_ERR_DEVICE, hipGetErrorString(e)); }
    }
    std::vector<float> out((size_t)n * 2 * count);
    const int r = katRoundTrip(c, in, (size_t)n * inStride * 4, out.data(), out.size() * 4, [&](void* dIn, void* dOut, hipStream_t st) {
        hipLaunchKernelGGL(k_kat_sampler, dim3((n + 63u) / 64u), dim3(64), 0, st, dBlue, (const float*)dIn, inStride, (float*)dOut, count, n);
    });
    if (dBlue) (void)hipFree(dBlue);
    if (r) return r;
    for (uint32_t k = 0; k < n; ++k)
    {
        memcpy(outInts + (size_t)k * count, out.data() + (size_t)k * 2 * count, count * 4);
        memcpy(outFloats + (size_t)k * count, out.data() + (size_t)k * 2 * count + count, count * 4);
    }
    return RTGPU_OK;
}

RTGPU_API int rtgpu_kat_mesh(RtgpuContext* c, const float* rays, uint32_t n, uint32_t* out)
{
    if (!c || (n && (!rays || !out))) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!c->sceneReady) return fail(RTGPU_ERR_NOT_READY, "rtgpu_upload_scene has not been called");
    if (c->sceneDev.numObjects != 1u || c->sceneDev.numMeshes != 1u) return fail(RTGPU_ERR_INVALID_ARGUMENT, "rtgpu_kat_mesh needs a scene made of exactly one mesh object");
    if (c->traversalStackNeed > RT_KAT_MESH_STACK) return fail(RTGPU_ERR_UNSUPPORTED, "mesh BVH deeper than the KAT kernel's stack");
    if (n == 0) return RTGPU_OK;
    { int fr = flushQueued(c); if (fr) return fr; }
    return katRoundTrip(c, rays, (size_t)n * 7 * 4, out, (size_t)n * 19 * 4, [&](void* dIn, void* dOut, hipStream_t st) {
        hipLaunchKernelGGL(k_kat_mesh, dim3((n + 63u) / 64u), dim3(64), 0, st, c->sceneDev, (const float*)dIn, n, (uint32_t*)dOut);
    });
}

RTGPU_API int rtgpu_kat_postprocess(RtgpuContext* c, const RtPostprocessParams* params, const float* rgb, uint32_t n, uint32_t* outBGR, float* outToneMapped)
{
    if (!c || (n && (!params || !rgb || !outBGR))) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n == 0) return RTGPU_OK;
    std::vector<PostScale> scales(n);
    for (uint32_t i = 0; i < n; ++i)
    {
        if (params[i].tonemapper > RT_TONEMAPPER_ACES) return fail(RTGPU_ERR_INVALID_ARGUMENT, "unknown tonemapper");
        if (params[i].numPasses == 0) return fail(RTGPU_ERR_INVALID_ARGUMENT, "numPasses must be > 0");
        scales[i] = postScale(&params[i]);
    }
    HIP_TRY(hipSetDevice(c->device));
    RtPostprocessParams* dParams = nullptr; PostScale* dScales = nullptr; float* dRgb = nullptr; uint32_t* dBGR = nullptr; float* dTone = nullptr;
    hipError_t e = hipMalloc((void**)&dParams, (size_t)n * sizeof(RtPostprocessParams));
    if (e == hipSuccess) e = hipMalloc((void**)&dScales, (size_t)n * sizeof(PostScale));
    if (e == hipSuccess) e = hipMalloc((void**)&dRgb, (size_t)n * 3 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&dBGR, (size_t)n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&dTone, (size_t)n * 3 * sizeof(float));
    if (e == hipSuccess) e = rtMemcpy(dParams, params, (size_t)n * sizeof(RtPostprocessParams), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = rtMemcpy(dScales, scales.data(), (size_t)n * sizeof(PostScale), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = rtMemcpy(dRgb, rgb, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess)
    {
        hipLaunchKernelGGL(k_kat_postprocess, dim3((n + 63u) / 64u), dim3(64), 0, c->lanes[0].stream, dParams, dScales, dRgb, n, dBGR, dTone);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(c->lanes[0].stream);
    }
    if (e == hipSuccess) e = rtMemcpy(outBGR, dBGR, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && outToneMapped) e = rtMemcpy(outToneMapped, dTone, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost);
    devFree(dParams, dScales, dRgb, dBGR, dTone);
    if (e != hipSuccess) return fail(RTGPU_ERR_DEVICE, std::string("rtgpu_kat_postprocess: ") + hipGetErrorString(e));
    return RTGPU_OK;
}

RTGPU_API int rtgpu_kat_blur(RtgpuContext* c, float* rgbHost, uint32_t width, uint32_t height, float sigma)
{
    if (!c || !rgbHost) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    if (width == 0 || height == 0 || !(sigma > 0.0f)) return fail(RTGPU_ERR_INVALID_ARGUMENT, "rtgpu_kat_blur: empty image or sigma not positive");
    BlurPlan plan;
    { const int pr = blurPlanFor(sigma, width, height, &plan); if (pr) return pr; }
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t)width * height * 3 * sizeof(float);
    float* dImage = nullptr; float* dLines = nullptr;
    hipError_t e = hipMalloc((void**)&dImage, bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&dLines, bytes * 2);
    if (e == hipSuccess) e = rtMemcpy(dImage, rgbHost, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess)
    {
        blurImage(c->lanes[0].stream, dImage, width, height, plan, dLines);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(c->lanes[0].stream);
    }
    if (e == hipSuccess) e = rtMemcpy(rgbHost, dImage, bytes, hipMemcpyDeviceToHost);
    devFree(dImage, dLines);
    if (e != hipSuccess) return fail(RTGPU_ERR_DEVICE, std::string("rtgpu_kat_blur: ") + hipGetErrorString(e));
    return RTGPU_OK;
}

RTGPU_API int rtgpu_evaluate_textures(RtgpuContext* c, uint32_t count, const uint32_t* textureIndex, const float* uv, float* out)
{
    if (!c || (count && (!textureIndex || !uv || !out))) return fail(RTGPU_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!c->sceneReady) return fail(RTGPU_ERR_NOT_READY, "rtgpu_upload_scene has not been called");
    if (count == 0) return RTGPU_OK;
    HIP_TRY(hipSetDevice(c->device));
    for (uint32_t i = 0; i < count; ++i) if (textureIndex[i] >= c->sceneDev.numTextures) return fail(RTGPU_ERR_INVALID_ARGUMENT, "texture index out of range");
    uint32_t* dIndex = nullptr; float* dUv = nullptr; float* dOut = nullptr;
    hipError_t e = hipMalloc((void**)&dIndex, count * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&dUv, (size_t)count * 2 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&dOut, (size_t)count * 4 * sizeof(float));
    if (e == hipSuccess) e = rtMemcpy(dIndex, textureIndex, count * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = rtMemcpy(dUv, uv, (size_t)count * 2 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess)
    {
        hipLaunchKernelGGL(k_evaluate_textures, dim3((count + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, c->lanes[0].stream, c->sceneDev, count, dIndex, dUv, dOut);
        e = hipStreamSynchronize(c->lanes[0].stream);
    }
    if (e == hipSuccess) e = rtMemcpy(out, dOut, (size_t)count * 4 * sizeof(float), hipMemcpyDeviceToHost);
    devFree(dIndex, dUv, dOut);
    if (e != hipSuccess) return fail(RTGPU_ERR_DEVICE, std::string("rtgpu_evaluate_textures: ") + hipGetErrorString(e));
    return RTGPU_OK;
}
