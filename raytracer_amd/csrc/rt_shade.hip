// rt_shade.hip -- the shading kernels of the library, a translation unit of their own: PathTracerMIS / PathTracer / Debug shading over
// slot-per-pixel and dense path state (rt_shade.inl with rt_shade_body.inl, rt_dense.inl: two layouts around ONE set of vertex stages, the mis* functions
// of rt_shade.inl), the bidirectional integrator's kernels (rt_vcm.inl) and the
// resolve kernels of rtgpu_render_aovs and rtgpu_render_aovs_chain (rt_aov.inl).  The host side
// (rt_runtime.hip) launches them through the declarations of rt_shade_kernels.h.
//
// Why its own unit: it is compiled with -mllvm -simplifycfg-sink-common=false.  SimplifyCFG's common-code sinking merges the stores that
// different branches of the BSDF / shape / counter code make into ONE store through a pointer phi, which SROA cannot promote: the BSDF
// sample record, a pdf and two counters of the generic kernels then live in private (scratch) memory -- 48 ... 192 bytes per lane.  Without
// the sinking: none (generic shade -7 ... -11 %).  The traversal kernels are 0.6 % FASTER with it, hence two units
// (profiles/r03_shade_variants.txt).
#define RT_SHADE_DEFINITIONS 1
#include "rt_device_traverse.h"
#include "rt_vcm_state.h"
#include "rt_shade_kernels.h"

#include "rt_shade.inl"
#include "rt_dense.inl"
#include "rt_vcm.inl"
#include "rt_aov.inl"

// the instantiations the host side launches (the lists are in rt_shade_kernels.h)
#define RT_X(L, P, A) template __global__ void RT_SHADE_DENSE_ATTR(L, A) k_shade_dense<L, P, A, 0> RT_K_SHADE_DENSE_ARGS; \
                      template __global__ void RT_SHADE_DENSE_ATTR(L, A) k_shade_dense<L, P, A, 1> RT_K_SHADE_DENSE_ARGS; \
                      template __global__ void RT_SHADE_DENSE_ATTR(L, A) k_shade_dense<L, P, A, 2> RT_K_SHADE_DENSE_ARGS;
RT_K_SHADE_DENSE_INSTANCES(RT_X)
#undef RT_X
#define RT_X(L, P) template __global__ void __launch_bounds__(RT_BLOCK) k_shade<L, P> RT_K_SHADE_ARGS;
RT_K_SHADE_INSTANCES(RT_X)
#undef RT_X
template __global__ void __launch_bounds__(RT_BLOCK) k_shade_record<false, false> RT_K_SHADE_RECORD_ARGS;
template __global__ void __launch_bounds__(RT_BLOCK) k_shade_chain<false, false> RT_K_SHADE_CHAIN_ARGS;
#define RT_X(C) template __global__ void __launch_bounds__(RT_BLOCK) k_vcm_emit<C> RT_K_VCM_EMIT_ARGS; \
                template __global__ void __launch_bounds__(RT_BLOCK) k_vcm_light_shade<C> RT_K_VCM_LIGHT_SHADE_ARGS; \
                template __global__ void __launch_bounds__(RT_BLOCK) k_lt_shade<C> RT_K_VCM_LIGHT_SHADE_ARGS; \
                template __global__ void __launch_bounds__(RT_BLOCK) k_vcm_camera_shade<C> RT_K_VCM_CAMERA_SHADE_ARGS;
RT_VCM_CLASSES(RT_X)
#undef RT_X
#define RT_X(C) template __global__ void __launch_bounds__(RT_BLOCK) k_aov_resolve<C> RT_K_AOV_RESOLVE_ARGS;
RT_AOV_CLASSES(RT_X)
#undef RT_X
#define RT_X(C) template __global__ void __launch_bounds__(RT_BLOCK) k_aov_resolve_chain<C> RT_K_AOV_RESOLVE_CHAIN_ARGS;
RT_AOV_CLASSES(RT_X)
#undef RT_X

// (behind everything else: the kernels above keep their places in the code object) k_generate_dense fed from a table of rays, rtgpu_set_ray_source, and from a
// table of lens rays, rtgpu_set_lens_source
#define RT_RAYSOURCE_DENSE 1
#include "rt_raysource.inl"
