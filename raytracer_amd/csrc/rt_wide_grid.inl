// rt_wide_grid.inl -- why the 4-wide walks (rt_trace_wide.inl, rt_trace_wide2.inl, rt_trace_packet.inl) return the reference's hits: the exactness argument
// over the 16-bit grid of conservative boxes and the per-leaf exact boxes ("gates").  Device only; included by rt_trace.hip and rt_tail.hip in front of
// rt_wide_walk.h, the device code the walks share (request ray, fold, interior step, mesh leaf, finish, tallies).  The format itself -- constants, node
// records, gates, WideBvh / WideLevel / WideScene, WideTuning -- is rt_wide_format.h; the host code that builds the trees and keeps the promise this
// argument starts from is rt_scene_prepare.h.
// (The argument was first written for k_trace_quant, a walk of the reference's BINARY tree over the same records: bit-exact and no faster than k_trace.
// The patch that restores it is profiles/r05_removed_optin_paths.patch.)
//
// The re-encoding:
//   * a child record is 16 bytes {min.xyz, max.xyz as 16-bit grid coordinates, child reference}; the grid spans the mesh's bounds, planes are
//     rounded OUTWARDS with a step to spare, so a stored box always contains the reference's box;
//   * the slab test needs no decode step: t = fma(float(q), step * invDir, base * invDir - origin * invDir), two constants per axis and ray;
//   * boxes that are only conservative cannot decide what the reference tests, so a leaf's triangles count only if the ray also passes the
//     leaf's EXACT box (the test the reference's walk performs before it reaches them) -- fetched only when a triangle was actually hit.
//
// Exactness.  Same argument as for any walk that visits a superset of the reference's leaves in another order: every candidate hit
// (a triangle the ray intersects inside a leaf whose exact box it passes) has the same (t, u, v) as in the reference's walk, because
// the triangle test and the exact box test are the reference's arithmetic; the slab test is monotone in the box planes, so passing a
// leaf's exact box implies passing every ancestor's box with a smaller entry distance, i.e. the reference's walk reaches exactly these
// candidates unless its running hit distance culls one -- which can only change the result when two candidates are closer together than
// the disagreement between a box's entry distance and its triangle's hit distance.  The walks cull with a slack (near < best + 2 tol),
// track the SECOND smallest candidate distance, and a ray whose runner-up lies within tol of its best (tol = 16 ulps of the largest
// term of its slab tests) is not trusted: it goes to the exact queue and is traced again by k_trace in the reference's order.  So do
// rays with a zero direction component (their slab tests produce NaNs, which the reference's min/max operand order resolves in its
// own way) and rays that start so far outside the mesh that the folded slab test's rounding could eat the spare grid step.  Any-hit rays
// need no runner-up: occlusion is an OR over the same candidate set (their leaf gate includes the reference's entry-distance test
// against the fixed ray length).  The reference's box / triangle test counters belong to its own walk: with the intersection
// counters on, k_trace runs alone.
//
// Hits in front of their box.  The argument above lets the running hit distance cull a candidate only where two candidates lie within the rounding of a SLAB test
// of each other.  It took for granted that a triangle's hit distance is not smaller than its leaf box's entry distance.  Exact arithmetic says so; the triangle
// test's own rounding does not: its error grows with 1 / cos of the angle between ray and triangle plane, and a ray 0.14 degrees off a sheet had t = 0.9755346 on
// a triangle whose leaf box it enters at 0.975574 -- 4e-5 apart, tol was 3.4e-6.  The reference's walk, with the neighbouring triangle's hit (0.97554296) found
// first, culls that leaf (entry >= best) and reports the neighbour; found in the other order it reports the nearer hit.  So a candidate with lo < entry - tol
// (entry: the exact box's entry distance, which the leaf gate computes anyway) is one whose fate depends on the reference's order: wideAcceptPair makes it its own
// runner-up, and a ray that ends with it is retraced.  Down to entry - tol the existing rule covers it (a hit that culls it lies within tol of it and is its
// runner-up).  NOT covered: the mirror case -- the walk culls such a leaf by its conservative entry (>= best + 2 tol) and never tests the triangle, while the
// reference, meeting it first, reports it.  That needs the two walks to visit the two leaves in opposite orders with the nearer box holding the farther hit; no
// constructed input has shown it (tests/test_gpu_wide_margins.py), DESIGN_PARITY.md "Margins" keeps it as an open finding.  Any-hit rays are not concerned: their
// candidate set does not depend on a running distance.
