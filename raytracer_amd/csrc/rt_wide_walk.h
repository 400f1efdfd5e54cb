// rt_wide_walk.h -- the device code the 4-wide walks share, each part once: k_trace_wide / k_tail (traceWideLoop, rt_trace_wide.inl), k_trace_wide2
// (rt_trace_wide2.inl) and k_trace_packet (rt_trace_packet.inl): the node record's slab test, the hand-over lists, the request ray, the fold, the interior
// step, the mesh leaf, the end of a ray and the tallies.  Included by rt_trace.hip and rt_tail.hip behind rt_wide_grid.inl (the exactness argument these
// parts carry out; the grid, the records and WideTuning are rt_wide_format.h) and before the walk files, which keep what is their own: the loops, the phase scheduling, the refill
// policy, the tolerance policy, the second level, the packet's uniform node.
//
// Form.  k_trace_wide and k_trace_wide2 sit on the 96-VGPR limit (five waves per SIMD, no scratch in the hot instantiation): a part is a force-inlined
// function with values in and out where that compiles to the registers, scratch and LDS of the hand-written copies it replaced, and a macro over the
// caller's names (as RT_WIDE_SLAB) where it does not -- the fold; profiles/wide_walk_parts_resources.txt has the table.

// ---- node records ----------------------------------------------------------------------------------------------------------------------
// slab test of one child record against the ray's folded constants; near is clamped to >= 0 (its bits then order like the float).
// Which of an axis's two planes the ray meets first is a property of the RAY (the sign of its direction), so three byte permutes with
// per-ray selectors (v_perm_b32) put {near plane, far plane} of every axis into one word and the six min / max of the textbook slab
// test disappear: 3 perm + 6 cvt (sub-word select) + 6 fma + max + max3 + min3 per child.
// Record words: w0 = minx | miny << 16, w1 = minz | maxx << 16, w2 = maxy | maxz << 16.  __builtin_amdgcn_perm(hi, lo, sel): byte i of
// the result is byte sel[i] of {lo = bytes 0-3, hi = bytes 4-7}.
#define RT_WIDE_SEL_X_POS 0x07060100u   // perm(w1, w0): minx (bytes 0,1) first, maxx (bytes 6,7) second
#define RT_WIDE_SEL_X_NEG 0x01000706u
#define RT_WIDE_SEL_Y_POS 0x05040302u   // perm(w2, w0): miny (bytes 2,3) first, maxy (bytes 4,5) second
#define RT_WIDE_SEL_Y_NEG 0x03020504u
#define RT_WIDE_SEL_Z_POS 0x07060100u   // perm(w2, w1): minz (bytes 0,1) first, maxz (bytes 6,7) second
#define RT_WIDE_SEL_Z_NEG 0x01000706u
#define RT_WIDE_SLAB(q, nearOut, farOut)                                                                                                          \
    {                                                                                                                                             \
        const uint32_t w0 = ubits(q.x), w1 = ubits(q.y), w2 = ubits(q.z);                                                                         \
        const uint32_t px = __builtin_amdgcn_perm(w1, w0, selX), py = __builtin_amdgcn_perm(w2, w0, selY), pz = __builtin_amdgcn_perm(w2, w1, selZ); \
        const float nx = __fmaf_rn((float)(px & 0xFFFFu), ax, bx), ny = __fmaf_rn((float)(py & 0xFFFFu), ay, by), nz = __fmaf_rn((float)(pz & 0xFFFFu), az, bz); \
        const float xx = __fmaf_rn((float)(px >> 16), ax, bx), xy = __fmaf_rn((float)(py >> 16), ay, by), xz = __fmaf_rn((float)(pz >> 16), az, bz);            \
        nearOut = fmaxf(fmaxf(nx, ny), fmaxf(nz, 0.0f));                                                                                           \
        farOut = fminf(fminf(xx, xy), xz);                                                                                                        \
    }
#define RT_WIDE_IS_LEAF(ref) ((((ref) >> RT_NODE_LEAVES_SHIFT) - 1u) < 2u)   // one or two triangles; not an interior node (0), not RT_WIDE_EMPTY / RT_QUANT_DONE (3)

// ---- hand-over ---------------------------------------------------------------------------------------------------------------------------
// The block's own list of the rays its walk does not decide (LDS): they are traced by the reference's walk (traceBinaryLoop) in the same launch
// when the block's 4-wide walk is done, instead of by a launch of their own behind this one (ten launches of 70 ... 1600 us per batch for 0.1 %
// of the rays, profiles/r03_timeline_serial_start_of_round.txt).  What does not fit the list goes to the launch's queues as before.
struct WideLocal
{
    uint32_t* exact; uint32_t* exactCount;       // closest-hit rays (path slots)
    uint32_t* shadow; uint32_t* shadowCount;     // any-hit requests (light * capacity + slot)
    uint32_t capacity;                           // entries per list; 0: no local lists
};
RT_DEV void widePushExact(const WideTuning& tune, const WideLocal& local, bool shadowRequest, uint32_t request)
{
    if (local.capacity != 0u)
    {
        const uint32_t i = atomicAdd(shadowRequest ? local.shadowCount : local.exactCount, 1u);   // (the consumer clamps the count to the capacity)
        if (i < local.capacity) { (shadowRequest ? local.shadow : local.exact)[i] = request; return; }
    }
    if (tune.exactQueue == nullptr) return;   // k_tail: its lists hold every request a chunk can produce (rt_tail.hip states the invariant)
    if (shadowRequest) tune.exactShadowQueue[atomicAdd(tune.exactShadowCount, 1u)] = request;
    else tune.exactQueue[atomicAdd(tune.exactCount, 1u)] = request;
}

// ---- request ray ------------------------------------------------------------------------------------------------------------------------
// The reference's world ray of a request from its records (closest-hit: R_ORIGIN, R_DIR; any-hit: the record shadowOriginRecord names and the light's shadow record): Ray::Ray
// normalises the direction (PathTracerMIS.cpp:86 / :392), then the origin moves along it -- shadowOffset (1e-4) for an any-hit ray, 1e-3 for a
// bounce, not at all for a primary ray (bounce 0: the origin record's low byte) -- and originDivDir stays what Ray::Ray made it, STALE by that
// offset (PathTracerMIS.cpp:392-393): that is what the reference's top-level box tests see, and what k_trace_wide2 parks for its top-level gates.
RT_DEV Ray wideWorldRay(float4 origin, float4 dir, bool shadow, float shadowOffset)
{
    const float offset = shadow ? shadowOffset : 0.001f;
    Ray world = makeRay(V4(origin.x, origin.y, origin.z, 0.0f), V4(dir.x, dir.y, dir.z, 0.0f));
    if (shadow || (ubits(origin.w) & 0xFFu) != 0u) world.origin = world.origin + world.dir * offset;
    return world;
}

// ---- fold -------------------------------------------------------------------------------------------------------------------------------
// The slab constants of `ray` folded onto a 16-bit grid (`grid`: a WideBvh or a WideLevel -- base, step, bound): t(q) = fma(q, a, b) with
// a = step * invDir, b = base * invDir - originDivDir.  RT_WIDE_FOLD_TEST declares mx, my, mz -- per axis, the largest magnitude a slab test of this ray
// can produce -- and `trusted`.  Not trusted -- the reference's walk only -- is a ray with a zero direction component (NaNs in the reference's slab
// test) or an origin so far outside the grid that the folded test's rounding, 2^-21 of that magnitude, could eat the spare grid step.
// RT_WIDE_FOLD_SET assigns the caller's ax .. bz.  The tolerance policy is the caller's; RT_WIDE_FOLD_TOL is its unit, 16 ulps of the largest slab term.
// (Macros over the caller's names: as functions -- one returning a struct, or a pair with reference parameters -- they cost k_trace_wide's diagnostic
// instantiation, which has no register to spare, 20 bytes of scratch.)
#define RT_WIDE_FOLD_TEST(ray, grid)                                                                                                              \
    const float mx = fabsf(ray.originDivDir.x) + grid.bound[0] * fabsf(ray.invDir.x);                                                             \
    const float my = fabsf(ray.originDivDir.y) + grid.bound[1] * fabsf(ray.invDir.y);                                                             \
    const float mz = fabsf(ray.originDivDir.z) + grid.bound[2] * fabsf(ray.invDir.z);                                                             \
    const float fold = 4.76837158203125e-07f;   /* 2^-21 */                                                                                       \
    const bool trusted = rayIsNaNFree(ray) &&                                                                                                     \
                         mx * fold < grid.step[0] * fabsf(ray.invDir.x) && my * fold < grid.step[1] * fabsf(ray.invDir.y) && mz * fold < grid.step[2] * fabsf(ray.invDir.z);
#define RT_WIDE_FOLD_SET(ray, grid)                                                                                                               \
    ax = grid.step[0] * ray.invDir.x; ay = grid.step[1] * ray.invDir.y; az = grid.step[2] * ray.invDir.z;                                         \
    bx = __fmaf_rn(grid.base[0], ray.invDir.x, -ray.originDivDir.x);                                                                              \
    by = __fmaf_rn(grid.base[1], ray.invDir.y, -ray.originDivDir.y);                                                                              \
    bz = __fmaf_rn(grid.base[2], ray.invDir.z, -ray.originDivDir.z);
#define RT_WIDE_FOLD_TOL (fmaxf(fmaxf(mx, my), mz) * 1.9073486328125e-06f)   // 2^-19

// ---- interior step --------------------------------------------------------------------------------------------------------------------
// One visit of the interior node at `node` (four child records) by the ray with the folded constants a, b, the byte selectors, `limit` (= best + 2 tol:
// box occlusion with the slack that keeps every candidate within tol of the final hit in the walk) and `tol`: four slab tests, the entered children
// sorted, all but one deferred on the lane's `stack` column from entry `sp` up; returns the reference to walk next and the new stack level.
// `floor` is the stack level the walk may not pop below (0, or where the mesh level of a two-level walk began).  The overflow check and the diagnostics
// are the caller's.
//
// Order.  (key, reference) pairs are sorted so that the children the ray enters come first and the ones it misses last (key = all ones); the first
// numHit - 1 references are deferred and the LAST entered one is walked next: the nearest child for a closest-hit ray (key = 0x7FFFFFFF ^ bits(entry
// distance): farthest first; the distance is >= 0, so its bits order like the float and there is no borrow), the FARTHEST for an any-hit ray
// (key = bits(entry distance): nearest first; round 6).  A closest-hit ray wants its nearest child (hits shorten it).
// An any-hit ray has nothing to shorten -- it ends with the first occluder, wherever that lies -- and nearest-first is the worst order for it: a
// next-event ray starts ON a surface, so the nearest boxes hold that surface's neighbours, which never occlude it; farthest first finds the walls
// and roofs that do (step model over the benchmark's rays, tools/wide8/walk_model.cpp, profiles/r06_wide8_step_model.txt: 9.9 interior + 1.5 leaf
// visits per any-hit ray instead of 16.0 + 2.6; 13.6 % end to end against nearest first, profiles/r06_anyhit_order_ab.txt -- that order is no
// longer selectable).  Occlusion is an OR over the same candidates: the result does not depend on the order.
// The flip is rebuilt in every visit from `tol` behind an optimisation barrier: as a loop-invariant value it would be one more vector register
// live across the loop -- the 97th: 20 bytes of scratch -- for three instructions per visit saved.
// INVARIANT the flip rests on: `tol == 0` stands for "any-hit ray".  Any-hit rays keep tol = 0 (they track no runner-up), and every trusted
// closest-hit ray has tol > 0: its tolerance is at least RT_WIDE_FOLD_TOL >= 2^-19 x (bound x |invDir|) of any axis, where invDir is finite and not zero
// (rayIsNaNFree; the folded ray may be an instance's local ray, which is not normalised) and bound > 0 (the trust test fails on a zero grid step).  A change that gives a closest-hit ray tol == 0, or an any-hit ray a slack, flips the
// visiting order (never the result of an any-hit ray; a closest-hit ray would only walk farther): derive the flip from the request's kind then.
// The three stack stores are unconditional: what lands above the new top is free space; the caller's overflow check keeps three entries in reserve.
#define RT_WIDE_CE(ka, ra, kb, rb) { const bool c_ = ka > kb; const uint32_t lo_ = min(ka, kb), hi_ = max(ka, kb), rl_ = c_ ? rb : ra, rh_ = c_ ? ra : rb; ka = lo_; kb = hi_; ra = rl_; rb = rh_; }
struct WideStep { uint32_t cur, sp; };
RT_DEV WideStep wideInteriorStep(const float4* node, uint32_t* stack, uint32_t floor, uint32_t sp, float ax, float ay, float az, float bx, float by, float bz,
                                 uint32_t selX, uint32_t selY, uint32_t selZ, float limit, float tol)
{
    const float4 q0 = node[0], q1 = node[1], q2 = node[2], q3 = node[3];
    float n0, f0, n1, f1, n2, f2, n3, f3;
    RT_WIDE_SLAB(q0, n0, f0); RT_WIDE_SLAB(q1, n1, f1); RT_WIDE_SLAB(q2, n2, f2); RT_WIDE_SLAB(q3, n3, f3);
    const bool h0 = f0 >= n0 && n0 < limit, h1 = f1 >= n1 && n1 < limit, h2 = f2 >= n2 && n2 < limit, h3 = f3 >= n3 && n3 < limit;
    float tolNow = tol;
    asm volatile("" : "+v"(tolNow));
    const uint32_t orderFlip = tolNow == 0.0f ? 0u : 0x7FFFFFFFu;
    uint32_t k0 = h0 ? orderFlip ^ ubits(n0) : 0xFFFFFFFFu, k1 = h1 ? orderFlip ^ ubits(n1) : 0xFFFFFFFFu;
    uint32_t k2 = h2 ? orderFlip ^ ubits(n2) : 0xFFFFFFFFu, k3 = h3 ? orderFlip ^ ubits(n3) : 0xFFFFFFFFu;
    uint32_t r0 = ubits(q0.w), r1 = ubits(q1.w), r2 = ubits(q2.w), r3 = ubits(q3.w);
    RT_WIDE_CE(k0, r0, k1, r1) RT_WIDE_CE(k2, r2, k3, r3) RT_WIDE_CE(k0, r0, k2, r2) RT_WIDE_CE(k1, r1, k3, r3) RT_WIDE_CE(k1, r1, k2, r2)
    const uint32_t numHit = (h0 ? 1u : 0u) + (h1 ? 1u : 0u) + (h2 ? 1u : 0u) + (h3 ? 1u : 0u);
    uint32_t* const top = stack + sp * RT_BLOCK;
    top[0] = r0; top[RT_BLOCK] = r1; top[2 * RT_BLOCK] = r2;
    uint32_t cur;
    if (numHit != 0u) { cur = numHit == 1u ? r0 : (numHit == 2u ? r1 : (numHit == 3u ? r2 : r3)); sp += numHit - 1u; }
    else if (sp == floor) cur = RT_QUANT_DONE;
    else { --sp; cur = stack[sp * RT_BLOCK]; }
    WideStep next; next.cur = cur; next.sp = sp;
    return next;
}
#undef RT_WIDE_CE

// ---- mesh leaf: MeshShape::Traverse_Leaf(_Shadow), MeshShape.cpp:134-207 -------------------------------------------------------------------
// The triangle pair of the leaf reference `leaf` (one or two triangles from `tris` on; the second rides in the same round trip): hit distances
// (inf: no hit) and barycentrics; returns lo = min(t0, t1).  A hit that matters (lo < best + tol) is the caller's test.
RT_DEV float wideLeafPair(const RtTriangle* tris, uint32_t leaf, const Ray& ray, float& t0, float& u0, float& v0_, float& t1, float& u1, float& v1)
{
    const float inf = __uint_as_float(0x7f800000u);
    const uint32_t numLeaves = leaf >> RT_NODE_LEAVES_SHIFT, first = leaf & RT_NODE_CHILD_MASK;
    V4 v0, e1, e2, nv0, ne1, ne2;
    loadTriangle(tris + first, v0, e1, e2);
    loadTriangle(tris + first + (numLeaves > 1u ? 1u : 0u), nv0, ne1, ne2);
    u1 = 0.0f; v1 = 0.0f; t1 = inf;
    if (!intersectTriangleRay(ray, v0, e1, e2, u0, v0_, t0)) t0 = inf;
    if (numLeaves > 1u && !intersectTriangleRay(ray, nv0, ne1, ne2, u1, v1, t1)) t1 = inf;
    return fminf(t0, t1);
}
// Such a hit counts only if the ray passes the leaf's exact box (gate[2 first], gate[2 first + 1]), as in the reference's walk -- any-hit rays: with
// its entry-distance test against the fixed ray length.  `gateRay`: the quotients transformRayUnsafe built, which the caller has parked or rebuilds.
// `entry`: the exact box's entry distance as the reference's walk computes it (what its own culling compares with the running hit distance).
RT_DEV bool wideLeafGate(const float4* gate, uint32_t first, const Ray& gateRay, bool shadow, float best, float& entry)
{
    const float4 gmin = gate[2u * first], gmax = gate[2u * first + 1u];
    return intersectBoxRayNoNaN(gateRay, gmin.x, gmin.y, gmin.z, gmax.x, gmax.y, gmax.z, entry) && (!shadow || entry < best);
}
// A candidate pair of a closest-hit ray behind its leaf's exact box: the running minimum, the runner-up and -- written through -- the HitPoint of
// the path in `slot` (an exact tie is retraced anyway).  True: a hit record was written.  (k_trace_packet calls this behind its scalar loads.)
// `entry`, `tol`: the leaf's exact entry distance (wideLeafGate) and the ray's tolerance.  A hit that lies more than tol IN FRONT of its own leaf box is one
// the reference's walk finds or culls depending on its order (rt_wide_grid.inl, "Hits in front of their box"): it becomes its own runner-up, so the ray is
// retraced if it ends with this hit.
RT_DEV bool wideAcceptPair(const Paths& paths, uint32_t slot, uint32_t objectId, uint32_t first, float t0, float u0, float v0, float t1, float u1, float v1,
                           float lo, float entry, float tol, float& best, float& second)
{
    const float hi = fmaxf(t0, t1);
    if (!(lo < best)) { second = fminf(second, lo); return false; }
    second = lo < entry - tol ? lo : fminf(best, hi);
    best = lo;
    const bool firstWins = t0 <= t1;
    prec(paths, R_HIT, slot) = f4(fbits(objectId), fbits(first + (firstWins ? 0u : 1u)), lo, firstWins ? u0 : u1);
    prec(paths, R_SAMPLER, slot).x = firstWins ? v0 : v1;
    return true;
}

// ---- finish, tallies ------------------------------------------------------------------------------------------------------------------
// The end of a ray's walk.  `handOver`: the walk gave up (stack overflow, drain abort, an untrusted level).  True: the request went to the
// reference's own walk (widePushExact); an any-hit request among those is counted by the kernel that resolves it, as are the unoccluded ones.
RT_DEV bool wideFinishRay(const Paths& paths, const WideTuning& tune, const WideLocal& lists, bool shadow, uint32_t light, uint32_t slot, bool handOver, bool occluded,
                          float best, float second, float tol)
{
    const float inf = __uint_as_float(0x7f800000u);
    if (handOver) { widePushExact(tune, lists, shadow, shadow ? light * paths.capacity + slot : slot); return true; }
    if (shadow) { if (occluded) pshadow(paths, light, verdictRecord(paths), slot).w = -1.0f; return false; }
    if (best == inf) { prec(paths, R_HIT, slot) = f4(fbits(RT_INVALID_OBJECT), fbits(0u), inf, 0.0f); return false; }   // HitPoint.h:14-51
    if (!(second <= best + tol)) return false;
    widePushExact(tune, lists, false, slot);   // a runner-up too close to call: the reference's own walk decides
    return true;
}
// A block's tallies -> sTally[0..3] (LDS; `zeroed`: already cleared behind a barrier) -> the launch's counters, one atomic per block and counter:
// 0 any-hit rays traced here (C_SHADOW), 1 rays handed to the reference's walk (RT_COUNTER_RETRACED), of which 2 untrusted at refill and 3 stack
// overflows (the two diagnostic counters behind it).  kMask: the tallies this kernel keeps; `diagnostics` false: 2 and 3 stay in LDS (the diagnostic kernel uses their counters).  `adds`: this lane holds tallies (one lane per wave for
// tallies kept per wave).  Block-uniform: it holds barriers.
template <uint32_t kMask>
RT_DEV void wideFlushTallies(uint32_t* sTally, bool zeroed, bool adds, uint32_t numShadowRays, uint32_t numRetraced, uint32_t numUntrusted, uint32_t numOverflow,
                             bool diagnostics, unsigned long long* counters)
{
    if (!zeroed)
    {
        if (threadIdx.x < (kMask > 3u ? 4u : 2u)) sTally[threadIdx.x] = 0u;
        __syncthreads();
    }
    if (adds)
    {
        if ((kMask & 1u) && numShadowRays) atomicAdd(&sTally[0], numShadowRays);
        if ((kMask & 2u) && numRetraced) atomicAdd(&sTally[1], numRetraced);
        if ((kMask & 4u) && numUntrusted) atomicAdd(&sTally[2], numUntrusted);
        if ((kMask & 8u) && numOverflow) atomicAdd(&sTally[3], numOverflow);
    }
    __syncthreads();
    if ((kMask & 1u) && threadIdx.x == 0u && sTally[0]) atomicAdd(&counters[C_SHADOW], (unsigned long long)sTally[0]);
    if ((kMask & 2u) && threadIdx.x == 1u && sTally[1]) atomicAdd(&counters[RT_COUNTER_RETRACED], (unsigned long long)sTally[1]);
    if (!diagnostics) return;
    if ((kMask & 4u) && threadIdx.x == 2u && sTally[2]) atomicAdd(&counters[RT_COUNTER_RETRACED + 1], (unsigned long long)sTally[2]);
    if ((kMask & 8u) && threadIdx.x == 3u && sTally[3]) atomicAdd(&counters[RT_COUNTER_RETRACED + 2], (unsigned long long)sTally[3]);
}
