// rt_vcm_photons.h -- interface between the integrator kernels (rt_runtime.hip / rt_vcm.inl) and the photon hash-grid
// builder (rt_vcm_photons.hip, the one translation unit that uses hipCUB's device scan / radix sort).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// per-pass photon storage written by the light stage: up to `maxPerPixel` photons per path slot, two float4 per photon,
// photon-major (record r of photon k of slot s at raw[(k * 2 + r) * capacity + s])
struct VcmPhotonInput
{
    const float4* raw; const uint32_t* countPerSlot; const uint32_t* slotPixel;   // slot -> x | y << 16
    uint32_t numSlots, capacity, width, height, maxPerPixel;
};

// the merge set of a pass: photons in (pixel row-major, path vertex) order + the hash grid of Core/Utils/HashGrid.h
struct VcmPhotonGrid
{
    float4* photons = nullptr;       // 2 float4 per photon (32 bytes, VertexConnectionAndMerging::Photon)
    float4* sorted = nullptr;        // the same photons in mIndices order (what the range query reads)
    uint32_t* indices = nullptr;     // HashGrid::mIndices
    uint32_t* cellEnds = nullptr;    // HashGrid::mCellEnds (after Build: the END offset of every cell)
    float* boxMin = nullptr;         // 3 floats (device)
    uint32_t numPhotons = 0, hashTableMask = 0;
    float radiusSqr = 0.0f, invCellSize = 0.0f;
    // scratch
    uint32_t* pixelCounts = nullptr; uint32_t* pixelOffsets = nullptr; uint32_t* keys[2] = { nullptr, nullptr }; uint32_t* values[2] = { nullptr, nullptr };
    void* temp = nullptr; size_t tempBytes = 0; uint32_t* totalHost = nullptr;
    size_t photonCapacity = 0, pixelCapacity = 0, cellCapacity = 0;
};

// the cell of a photon, for the builder (k_photon_cells) and the range query (mergeCellRanges, rt_vcm.inl) alike
__device__ __forceinline__ int32_t cvtT(float f) { return (f >= 2147483648.0f || f < -2147483648.0f || f != f) ? (int32_t)0x80000000 : (int32_t)f; }   // _mm_cvttps_epi32
__device__ __forceinline__ uint32_t hashCellIndex(uint32_t x, uint32_t y, uint32_t z, uint32_t mask) { return ((x * 73856093u) ^ (y * 19349663u) ^ (z * 83492791u)) & mask; }   // HashGrid.h:148-152

// HashGrid::Build over the photons of `in` (radius = mMergingRadiusVM).  Synchronises the stream once (the photon count sizes
// the table).  Returns a hipError_t as int.
int vcmBuildPhotonGrid(const VcmPhotonInput& in, float radius, hipStream_t stream, VcmPhotonGrid& grid);
void vcmFreePhotonGrid(VcmPhotonGrid& grid);
