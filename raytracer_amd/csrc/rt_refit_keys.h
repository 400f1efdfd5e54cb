// rt_refit_keys.h -- floats as unsigned keys in the floats' own order, for k_refit_check (rt_runtime_refit.inl): integer atomicMin / atomicMax on the keys
// are a float minimum / maximum that no order of the blocks can change.  Plain C++ that host code includes too (tests/cpp/refit_keys_check.cpp holds it to its
// contract without a device).
//   refitKey    strictly monotone over every float that is not a NaN: -inf < -FLT_MAX < ... < -denormals < -0 < +0 < +denormals < ... < +inf.  A negative
//               float's bits grow as the float falls, so they are inverted; a non-negative one only takes the top bit.
//   refitUnkey  the float a key came from, bit for bit (the sign of a zero included).
// -0 sorts below +0, where `a < b ? a : b` keeps whichever zero the fold met last: the sign of a zero bound is the one place a minimum over keys can differ
// from a fold of the floats.  A NaN's key is above +inf's or below -inf's, by its sign bit: k_refit_check counts non-finite floats apart and its caller then
// ignores the box.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define RT_KEY_HD __host__ __device__
#else
#define RT_KEY_HD
#endif

#define RT_REFIT_KEY_HIGHEST 0xFFFFFFFFu   // the identities of a minimum and of a maximum over keys
#define RT_REFIT_KEY_LOWEST 0u

RT_KEY_HD static inline uint32_t refitKey(float f)
{
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
RT_KEY_HD static inline float refitUnkey(uint32_t k)
{
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
RT_KEY_HD static inline bool refitBitsFinite(uint32_t u) { return (u & 0x7F800000u) != 0x7F800000u; }   // neither an infinity nor a NaN

// What k_refit_check leaves on the device, 32 bytes: keys of the box over the positions the triangles refer to (the identities where there is no triangle) and
// the number of blocks that met a float that is not finite among ALL positions
struct RefitCheckRecord { uint32_t lo[3], hi[3], nonFinite, pad; };
