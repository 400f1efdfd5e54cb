// rt_generate.inl -- camera rays of the slot-per-pixel pipeline.  Included by rt_trace.hip.
// Viewport::RenderTile per-pixel prologue + Camera::GenerateRay (Viewport.cpp:305-331, Camera.cpp:81-118): generatePaths (rt_device_state.h) around the camera
__global__ void __launch_bounds__(RT_BLOCK) k_generate(const RtSceneDesc scene, const DevPass* __restrict__ passes, uint32_t slotsPerPass,
                                                       const Paths paths, const uint32_t* __restrict__ slotPixel, uint32_t numSlots,
                                                       uint32_t* __restrict__ queue, uint32_t* __restrict__ queueCount,
                                                       unsigned long long* counters)
{
    generatePaths<false>(RT_GRID_STRIDE, scene.blueNoise, passes, slotsPerPass, paths, slotPixel, numSlots, queue, CameraRayOf());
    generateQueueCount(queueCount, counters, numSlots);
}
