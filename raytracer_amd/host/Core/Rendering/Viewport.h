// Viewport: progressive accumulation driver (reference: Core/Rendering/Viewport.h:37-58).
// Render() performs the pass prologue of Viewport::Render (Core/Rendering/Viewport.cpp:200-242) on the
// host -- Halton seeds, anti-aliasing offset -- then hands ONE pass to the renderer instead of fanning
// 32x32 tiles out to a thread pool.  GetFrontBuffer() runs Viewport::PostProcessTile (Viewport.cpp:495-550) on the device for the
// whole image (bloom included: the five blurred copies are rebuilt from the sum buffer on demand).  Adaptive rendering keeps the reference's block list logic (Viewport.cpp:552-700) on the host; the
// error estimates come from the device.
#pragma once

#include "Renderer.h"
#include "../Sampling/HaltonSampler.h"

namespace rt {

struct RenderingProgress
{
    uint32 passesFinished = 0;
    uint32 activePixels = 0;
    uint32 activeBlocks = 0;
    float converged = 0.0f;
    float averageError = std::numeric_limits<float>::infinity();
};

class RAYLIB_API Viewport
{
public:
    Viewport();
    ~Viewport();

    bool Resize(uint32 width, uint32 height);
    bool SetRenderingParams(const RenderingParams& params);
    const RenderingParams& GetRenderingParams() const { return mParams; }
    bool SetRenderer(const RendererPtr& renderer);
    bool Render(const Camera& camera);
    void Reset();
    bool UpdateScene();   // sends what Scene::UpdateBVH changed to the renderer's device (mirror-only, like UpdateBVH)

    // Synchronises with the device and returns the accumulated (not tone-mapped) image.
    const Bitmap& GetSumBuffer();
    const Bitmap& GetSecondarySumBuffer();
    // tone-mapped B8G8R8A8 image of the passes finished so far (reference: Viewport::GetFrontBuffer, Viewport.h:47)
    const Bitmap& GetFrontBuffer();
    bool SetPostprocessParams(const PostprocessParams& params);
    const PostprocessParams& GetPostprocessParams() const { return mPostprocessParams; }
    uint32 GetWidth() const { return mWidth; }
    uint32 GetHeight() const { return mHeight; }
    // averageError: with adaptive rendering off the reference recomputes it after every second pass; here it is evaluated when
    // asked for, at an even pass count (otherwise the value of the last evaluation is returned)
    const RenderingProgress& GetProgress();
    const std::vector<RtBlock>& GetBlocks() const { return mBlocks; }
    // known-answer hook: the list walk of UpdateBlocksList with the pass counter and the block errors supplied by the caller
    void UpdateBlocksListWithErrors(uint32 passesFinished, std::vector<float> errors);
    uint32 GetPassesFinished() const { return mProgress.passesFinished; }
    // counters of the LAST pass (synchronises), like the reference
    const RayTracingCounters& GetCounters();
    // totals since Reset (synchronises)
    RayTracingCounters GetTotalCounters();

    // Extension (the reference has no seed API): re-seed the Viewport's generators.
    void SetSeed(uint64 seed);
    void ClearAccumulation();   // sums, progress, counters, block list start over; the sample sequence goes on
    // Extension (rtgpu_set_ray_source): the passes that follow start at the caller's primary rays -- width * height entries, entry y * width + x the ray of
    // pixel (x, y) of the sum buffer -- instead of the camera's, whose part of Render()'s constants is then not read.  nullptr with count 0: the camera
    // again.  The table is copied.  Resize and SetRenderer drop it (a table is a frame's, and it lives in the renderer's device context).
    bool SetRaySource(const RtPrimaryRay* rays, size_t count);
    // Extension (rtgpu_set_lens_source): the same with a table of lens rays -- each entry a ray, its change per unit of the pass's sample offset and a thin
    // lens -- so that Render()'s anti-aliasing offsets and, with params.lens, depth of field apply to the caller's rays pass after pass without a new
    // table.  Of Render()'s constants the sample offset is then read, the camera is not.  Replaces a ray source; SetRaySource(nullptr, 0) clears it.
    bool SetLensSource(const RtLensRay* rays, size_t count, const RtLensSourceParams& params);

    // The per-pass constants Render() would use next; advances the Halton sequence and the generator
    // exactly like Render().  Exposed so parity tests can feed identical constants to the CPU oracle.
    bool NextPassParams(const Camera& camera, RtPassParams& outParams);
    void FinishPass();

private:
    RendererPtr mRenderer;
    math::Random mRandomGenerator;
    HaltonSequence mHaltonSequence;
    RenderingParams mParams;
    RenderingProgress mProgress;
    void BuildInitialBlocksList();
    bool UpdateBlocksList();
    void ApplyBlockErrors(std::vector<float>& errors);
    std::vector<RtBlock> mBlocks;
    uint32 mErrorEvaluatedAtPass = 0;
    Bitmap mSum, mSecondarySum, mFrontBuffer;
    PostprocessParams mPostprocessParams;
    uint32 mWidth = 0, mHeight = 0;
    bool mSumDirty = false, mSecondarySumDirty = false;   // the device holds passes the host bitmaps have not seen
    bool mSumPinned = false;
    void PinSumBuffers(bool pin);   // page-locks the two sum bitmaps for the read-back (IRenderer::PinHostBuffer)
    std::vector<uint32> mSeedStorage;
    uint64 mRngKey[2];
    RayTracingCounters mCounters, mTotalsAtLastPass, mTotalsBeforeLastPass;
};

} // namespace rt
