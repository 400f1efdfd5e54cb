#!/usr/bin/env python3
"""Throughput of the batched ray queries (include/rtgpu.h: rtgpu_trace_rays_async through Viewport.trace_rays / occluded on torch tensors) on the
Sponza-class scene (raytracer_amd.scenes.sponza_class, 262 176 triangles), and -- in the same process -- the render pipeline's trace-class time per
traced ray, for the comparison of DESIGN.md ("Ray queries").  Prints one JSON line.

Ray sets: (a) coherent: the 1920 x 1080 pinhole camera rays of the scene's camera, computed in NumPy; (b) incoherent: cosine-hemisphere rays from
the first hits of (a), origins moved 1e-3 along the facing normal (the caller's offset).  Timing: device events around the query on the current
stream, after a warm-up of every shape, `--reps` repetitions (median, min, max).  The per-kernel split (load / trace / re-trace / store /
evaluate) comes from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_rays.py` run.

  python tools/bench_rays.py [--reps 30] [--render-passes 8]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def camera_rays(vp, camera, w, h):
    p = vp.next_pass_params(camera).camera
    m = np.array(p.localToWorld[:], dtype=np.float32).reshape(4, 4)
    x = ((np.arange(w, dtype=np.float32) + 0.5) / w * 2.0 - 1.0) * p.tanHalfFoV * p.aspectRatio
    y = ((np.arange(h, dtype=np.float32) + 0.5) / h * 2.0 - 1.0) * p.tanHalfFoV
    xx, yy = np.meshgrid(x, y)
    local = np.stack([xx.ravel(), yy.ravel(), np.ones(w * h, dtype=np.float32)], axis=1)
    d = local @ m[:3, :3]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.broadcast_to(m[3, :3], d.shape).copy()
    return o.astype(np.float32), d.astype(np.float32)


def hemisphere_rays(position, normal, direction, rng):
    n = normal.astype(np.float64)
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-12)
    flip = (n * direction).sum(axis=1) > 0.0
    n[flip] *= -1.0
    a = np.where(np.abs(n[:, :1]) > 0.9, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    t = np.cross(n, a)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(n, t)
    u1, u2 = rng.rand(len(n), 1), rng.rand(len(n), 1)
    r, phi = np.sqrt(u1), 2.0 * np.pi * u2
    d = t * (r * np.cos(phi)) + b * (r * np.sin(phi)) + n * np.sqrt(1.0 - u1)
    return (position + 1e-3 * n).astype(np.float32), d.astype(np.float32)


def time_query(torch, fn, reps):
    fn()   # warm-up of this shape (arena growth, code objects)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return np.array(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--render-passes", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    import torch
    import raytracer_amd as ra
    from raytracer_amd import scenes
    w, h = args.width, args.height
    scene, camera = scenes.sponza_class(w / h)
    vp = ra.Viewport(w, h, seed=1234, max_ray_depth=6)
    vp.set_renderer(scene)
    dev = torch.device("cuda:0")
    o_a, d_a = camera_rays(ra.Viewport(w, h), camera, w, h)
    first = vp.trace_rays(o_a, d_a, surfaces=True)
    hit = first.object_id != ra.RT_INVALID_OBJECT
    o_b, d_b = hemisphere_rays(first.position[hit], first.normal[hit], d_a[hit], np.random.RandomState(5))
    sets = {"coherent": (o_a, d_a), "incoherent": (o_b, d_b)}
    out = {"scene": "sponza_class", "triangles": int(scene.desc.contents.numTriangles), "reps": args.reps, "queries": {}}
    for label, (o, d) in sets.items():
        to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        n = len(o)
        for kind, fn in (("closest", lambda: vp.trace_rays(to, td)), ("closest_surfaces", lambda: vp.trace_rays(to, td, surfaces=True)),
                         ("any", lambda: vp.occluded(to, td))):
            ms = time_query(torch, fn, args.reps)
            med = float(np.median(ms))
            out["queries"]["%s_%s" % (label, kind)] = {"rays": n, "ms_median": med, "ms_min": float(ms.min()), "ms_max": float(ms.max()),
                                                       "mrays_per_s": n / med / 1e3, "ms_per_mray": med / (n / 1e6)}
    # the render pipeline's trace classes per traced ray (serial kernels: one batch lane, so that the classes' times do not overlap)
    lib = ra.rtgpu_lib()
    ctx = vp.device_context()
    lib.rtgpu_set_concurrency(ctx, 1)
    vp.render(camera, passes=2)   # warm-up
    vp.reset()
    lib.rtgpu_enable_timing(ctx, 1)
    vp.render(camera, passes=args.render_passes)
    ms, launches, names = (C.c_double * 8)(), (C.c_uint64 * 8)(), (C.c_char_p * 8)()
    lib.rtgpu_get_kernel_times(ctx, ms, launches, names)
    times = {names[i].decode(): ms[i] for i in range(8) if names[i]}
    cnt = ra.RtCounters()
    lib.rtgpu_get_counters(ctx, C.byref(cnt))
    traced = cnt.numRays + cnt.numShadowRays
    trace_ms = times.get("trace", 0.0) + times.get("retrace", 0.0) + times.get("tail", 0.0)
    out["render"] = {"passes": args.render_passes, "trace_ms": times.get("trace", 0.0), "retrace_ms": times.get("retrace", 0.0), "tail_ms": times.get("tail", 0.0),
                     "traced_rays": int(traced), "ms_per_mray": trace_ms / (traced / 1e6)}
    inc = out["queries"]["incoherent_closest"]["ms_per_mray"]
    out["incoherent_closest_vs_render_trace"] = inc / out["render"]["ms_per_mray"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
