#!/usr/bin/env python3
"""Time of one AOV call (include/rtgpu.h: rtgpu_render_aovs_async through Viewport.render_aovs(device=True)) on the Sponza-class 1920 x 1080 frame
(raytracer_amd.scenes.sponza_class, 262 176 triangles): every plane without the four cost planes (the walk the context renders with), every plane with
them (the counting binary walk), and -- for scale, in the same process -- one RT_INTEGRATOR_DEBUG pass of the same frame (renderer "Debug", mode
Normals: one quantity, squeezed into a colour, through the film).  Prints one JSON line.

Timing, after a warm-up (arena growth, code objects), `--reps` repetitions (median, min, max): every figure is HOST WALL TIME from the call to the end of
its device work (AOVs: the call, then a synchronise of its stream; Debug: render, then rtgpu_synchronize), so the three compare like for like, launch and
Python overhead included on every side.  The AOV calls also report `device_ms_median`: device events around the call on its stream, a second loop.

--chain N: instead, the guide-chain call (rtgpu_render_aovs_chain_async through Viewport.render_aovs(chain=N, device=True)) beside the first-hit call of the
same run and the same planes -- the denoiser's four guides, and every non-cost plane -- on the stock scene, which has no specular surface (every pixel stops at
its first hit: the cost of the early stop), and with --mirror on the scene with a smooth-metal rect and a glass sphere added (scenes.add_mirror_props).

  python tools/bench_aovs.py [--reps 20] [--chain 3 [--mirror]]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wall_time(fn, finish, reps):
    fn()
    finish()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        finish()
        ms.append(1e3 * (time.perf_counter() - t0))
    return np.array(ms)


def time_call(torch, fn, reps):
    fn()
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


def summary(ms, pixels):
    med = float(np.median(ms))
    return {"ms_median": med, "ms_min": float(ms.min()), "ms_max": float(ms.max()), "mpixels_per_s": pixels / med / 1e3}


def chain_beside_first_hit(args, torch, ra, scenes):
    w, h = args.width, args.height
    out = {"width": w, "height": h, "reps": args.reps, "max_chain": args.chain, "max_ray_depth": 6}
    guides = ("depth", "normal", "position", "base_color")
    non_cost = tuple(n for n in ra.AOV_PLANES if not n.endswith(("tests", "tests_passed")))
    stream = torch.cuda.Stream()
    for label in ("stock", "mirror") if args.mirror else ("stock",):
        scene, camera = scenes.sponza_class(w / h)
        if label == "mirror":
            scenes.add_mirror_props(scene)
        vp = ra.Viewport(w, h, seed=1234, max_ray_depth=6, min_russian_roulette_depth=args.chain)   # (roulette never cuts a chain)
        vp.set_renderer(scene)
        p = vp.next_pass_params(camera)
        res = {"triangles": int(scene.desc.contents.numTriangles)}
        with torch.cuda.stream(stream):
            length = vp.render_aovs(p, ("chain_length",), device=True, chain=args.chain)["chain_length"]
            res["pixels_with_chain"] = int((length >= 1).sum().item())
            for name, planes in (("guides", guides), ("all_non_cost", non_cost)):
                first = lambda: vp.render_aovs(p, planes, device=True)   # noqa: E731
                chain = lambda: vp.render_aovs(p, planes, device=True, chain=args.chain)   # noqa: E731
                a, b = np.median(time_call(torch, first, args.reps)), np.median(time_call(torch, chain, args.reps))
                res[name] = {"planes": len(planes), "first_hit_device_ms_median": float(a), "chain_device_ms_median": float(b), "chain_over_first_hit": float(b / a)}
        out[label] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--chain", type=int, default=None)
    ap.add_argument("--mirror", action="store_true")
    args = ap.parse_args()
    import torch
    import raytracer_amd as ra
    from raytracer_amd import scenes
    w, h = args.width, args.height
    if args.chain is not None:
        print(json.dumps(chain_beside_first_hit(args, torch, ra, scenes)))
        return
    scene, camera = scenes.sponza_class(w / h)
    vp = ra.Viewport(w, h, seed=1234, max_ray_depth=6)
    vp.set_renderer(scene)
    p = vp.next_pass_params(camera)
    cost = ("box_tests", "box_tests_passed", "triangle_tests", "triangle_tests_passed")
    every = tuple(ra.AOV_PLANES)
    without = tuple(n for n in every if n not in cost)
    out = {"scene": "sponza_class", "triangles": int(scene.desc.contents.numTriangles), "width": w, "height": h, "reps": args.reps}
    stream = torch.cuda.Stream()   # (the null stream would send the call through the wrapper's side stream)
    with torch.cuda.stream(stream):
        for label, planes in (("all_planes_without_cost", without), ("all_planes_with_cost", every), ("depth_only", ("depth",))):
            call = lambda: vp.render_aovs(p, planes, device=True)   # noqa: E731
            out[label] = dict(summary(wall_time(call, stream.synchronize, args.reps), w * h), planes=len(planes),
                              device_ms_median=float(np.median(time_call(torch, call, args.reps))))
    # one Debug pass of the same frame: a viewport of its own, so that the pass is a pass of that renderer from the start
    dbg = ra.Viewport(w, h, seed=1234, max_ray_depth=6)
    dbg.set_renderer(scene, name="Debug")
    dbg.set_debug_mode(4)
    lib, ctx = ra.rtgpu_lib(), dbg.device_context()
    out["debug_pass"] = summary(wall_time(lambda: dbg.render(camera, passes=1), lambda: lib.rtgpu_synchronize(ctx), args.reps), w * h)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
