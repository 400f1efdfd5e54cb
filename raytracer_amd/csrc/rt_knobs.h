// rt_knobs.h -- every RTGPU_* environment variable the library reads, in one place, ordered by WHEN it is read.  Included by rt_runtime.hip behind
// rt_runtime_context.h.  DESIGN.md ("Environment knobs") lists them with their defaults; why a default is what it is stands next to the policy
// that uses it (launchTraceWide, launchRetrace, tailDepthFor, ...), not here.  A knob scales a policy or forces code that ships anyway (which is how the
// tests reach it); a path that lost its measurement has none -- it is deleted together with its option, and DESIGN.md keeps the finding.
//
//   1. per context   copied into the RtgpuContext by rtgpu_create / rtgpu_create_multi: a later change of the variable reaches new contexts only
//   2. per process   read once, by the first call that needs the value (a function-local static): a later change is never seen
//   3. per call      read on every launch (or every scene upload): the tests flip these between two renders of one process
#pragma once

namespace knobs {

static inline int envInt(const char* name, int fallback) { const char* e = getenv(name); return e ? atoi(e) : fallback; }
static inline bool envSet(const char* name) { return getenv(name) != nullptr; }

// ---- 1. per context --------------------------------------------------------------------------------------------------------------------------
// bytes RTGPU_LANE_BUDGET_MB asks for; 0: not set
static inline size_t laneBudgetBytes() { const char* e = getenv("RTGPU_LANE_BUDGET_MB"); return e ? (size_t)strtoull(e, nullptr, 10) << 20 : 0u; }

// the scheduling and layout knobs of a new context, with their clamps (performance only; results do not depend on them)
static inline void readContextKnobs(RtgpuContext* c)
{
    c->tune.refillMinIdle = (uint32_t)envInt("RTGPU_REFILL_MIN_IDLE", (int)c->tune.refillMinIdle);
    c->tune.otherMinLanes = (uint32_t)envInt("RTGPU_OTHER_MIN_LANES", (int)c->tune.otherMinLanes);
    c->travBlocksPerCU = (uint32_t)envInt("RTGPU_TRAV_BLOCKS_PER_CU", (int)c->travBlocksPerCU);
    c->wideAllowed = envInt("RTGPU_WIDE", 1) != 0;
    c->wide2Allowed = envInt("RTGPU_WIDE2", 1) != 0;
    c->denseAllowed = envInt("RTGPU_NO_DENSE", 0) == 0;
    c->countIntersections = envInt("RTGPU_INTERSECTION_COUNTERS", 0) != 0;
    if (envSet("RTGPU_PASS_BATCH")) { c->passBatch = (uint32_t)envInt("RTGPU_PASS_BATCH", 0); c->passBatchFromEnv = true; }
    if (c->passBatch < 1) c->passBatch = 1;
    if (c->passBatch > RT_SEED_RING / 2) c->passBatch = RT_SEED_RING / 2;
    if (envSet("RTGPU_LANES")) { c->numLanes = (uint32_t)envInt("RTGPU_LANES", 0); c->lanesChosen = true; }
    if (c->numLanes < 1) c->numLanes = 1;
    if (c->numLanes > RT_MAX_LANES) c->numLanes = RT_MAX_LANES;
    if (c->tune.refillMinIdle < 1) c->tune.refillMinIdle = 1;
    if (c->tune.otherMinLanes < 1) c->tune.otherMinLanes = 1;
}
// rtgpu_create_multi
static inline bool multiStaged() { return envInt("RTGPU_MULTI_STAGED", 0) != 0; }
static inline bool verbose() { return envInt("RTGPU_VERBOSE", 0) != 0; }

// ---- 2. per process --------------------------------------------------------------------------------------------------------------------------
#define RT_KNOB_ONCE(type, name, value) static inline type name() { static const type v = (value); return v; }
RT_KNOB_ONCE(uint32_t, passBatchBase, (uint32_t)envInt("RTGPU_PASS_BATCH_BASE", 5))
RT_KNOB_ONCE(uint32_t, smallFrameBatch, (uint32_t)envInt("RTGPU_SMALL_FRAME_BATCH", 20))
RT_KNOB_ONCE(uint32_t, maxStreamBatch, (uint32_t)envInt("RTGPU_MAX_STREAM_BATCH", 24))
RT_KNOB_ONCE(uint32_t, shadeBlocksPerCU, (uint32_t)envInt("RTGPU_SHADE_BLOCKS_PER_CU", 8))
RT_KNOB_ONCE(uint32_t, tailBlocksPerCU, (uint32_t)envInt("RTGPU_TAIL_BLOCKS_PER_CU", 4))
RT_KNOB_ONCE(uint32_t, packetBlocksPerCU, (uint32_t)envInt("RTGPU_PACKET_BLOCKS", 8))
RT_KNOB_ONCE(uint32_t, wideChunkMin, (uint32_t)envInt("RTGPU_WIDE_CHUNK_MIN", 64))
RT_KNOB_ONCE(bool, wideDiag, envSet("RTGPU_WIDE_DIAG"))                           // (its value is read per launch: wideDiagMode)
RT_KNOB_ONCE(uint32_t, retraceSplitAfter, (uint32_t)envInt("RTGPU_RETRACE_SPLIT_AFTER", 0))   // 0: RT_RETRACE_SPLIT_AFTER
RT_KNOB_ONCE(int, retraceFullGrid, envInt("RTGPU_RETRACE_FULL_GRID", -1))         // -1: policy
RT_KNOB_ONCE(int, abortClosestAfter, envInt("RTGPU_ABORT_CLOSEST_AFTER", -1))     // test hook; -1: the context's value
RT_KNOB_ONCE(bool, vcmClass, envInt("RTGPU_VCM_CLASS", 1) != 0)
RT_KNOB_ONCE(bool, vcmWide, envInt("RTGPU_VCM_WIDE", 0) != 0)
RT_KNOB_ONCE(uint32_t, vcmMergeCooperativeMin, (uint32_t)envInt("RTGPU_VCM_MERGE_COOP", RT_VCM_COOPERATIVE_MERGE_MIN))
RT_KNOB_ONCE(int, vcmBatch, envInt("RTGPU_VCM_BATCH", 0))                         // <= 0: policy
RT_KNOB_ONCE(bool, denoiseTiled, envInt("RTGPU_DENOISE_TILED", 1) != 0)           // the a-trous levels of steps 1 and 2 from LDS tiles (k_atrous_tiled); 0: every level gathers from memory (k_atrous); same bits either way
#undef RT_KNOB_ONCE

// ---- 3. per call -----------------------------------------------------------------------------------------------------------------------------
// every launch of a 4-wide walk
static inline uint32_t wideDrainAbort() { return (uint32_t)envInt("RTGPU_WIDE_DRAIN_ABORT", 0); }   // test hook; 0: off
static inline uint32_t wideDiagMode() { return (uint32_t)envInt("RTGPU_WIDE_DIAG", 0); }
static inline bool packets() { return envInt("RTGPU_PACKET", 1) != 0; }
// every dense batch: a still camera's packets take their leaves from per-tile lists (rt_beam_lists.h; beamListsFor); 0: they walk.  Same bits either way
static inline bool beamLists() { return envInt("RTGPU_BEAM_LISTS", 1) != 0; }
// test hook: entries a tile's list may hold, 1 .. RT_BEAM_MAX_CAPACITY (a tile with more leaves has no list and walks)
static inline uint32_t beamListCap() { const int v = envInt("RTGPU_BEAM_LIST_CAP", (int)RT_BEAM_MAX_CAPACITY); return v < 1 ? 1u : (v > (int)RT_BEAM_MAX_CAPACITY ? RT_BEAM_MAX_CAPACITY : (uint32_t)v); }
// every launch of k_shade_dense: the launch-uniform tables (objects, meshes, materials, lights, seed rows) from LDS copies; 0: everything from memory; same bits either way
static inline bool shadeStage() { return envInt("RTGPU_SHADE_STAGE", 1) != 0; }
// every rtgpu_render_aovs: pixels per chunk, 1 .. 4 M (the tests run a small frame in several chunks)
static inline uint32_t aovChunk() { const int v = envInt("RTGPU_AOV_CHUNK", 1 << 22); return v < 1 ? 1u : (v > (1 << 22) ? (1u << 22) : (uint32_t)v); }
// every rtgpu_upload_scene
static inline bool noLean() { return envInt("RTGPU_NO_LEAN", 0) != 0; }
static inline bool noSimpleTextures() { return envInt("RTGPU_NO_SIMPLE_TEXTURES", 0) != 0; }

} // namespace knobs
