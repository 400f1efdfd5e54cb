#!/usr/bin/env python3
"""Time of the denoiser (include/rtgpu.h: rtgpu_denoise_async through Viewport.denoise(device=True)) on the Sponza-class 1920 x 1080 frame
(raytracer_amd.scenes.sponza_class, 262 176 triangles) after 20 passes: one call with 1 .. 5 levels, the guide render alone (the four planes through
Viewport.render_aovs(device=True)), the filter alone on those planes (raytracer_amd.atrous_filter on tensors) and -- for scale, same context -- one render
pass; and the same two for the variance-guided filter (rtgpu_denoise_var_async through Viewport.denoise(variance=True, device=True), rtgpu_filter_atrous_var_async
through atrous_filter(color_half=...)), both with the variance plane written, interleaved with the plain ones level count by level count, with their
ratios to them (`var_over_plain`).  A build without the variance-guided filter reports the plain figures alone.  Prints one JSON line and, with --output,
writes it to a file.

Timing, after a warm-up of every shape (scratch growth, code objects), `--reps` repetitions (median, min, max): device events around the call on a
stream of the tool's own; the render pass: host wall time around a batch of passes that ends in rtgpu_synchronize, per pass.
`gbytes_per_s_compulsory`: the 64 bytes per pixel and level that a level cannot avoid (three 16-byte records read, one written) over the filter's time --
what the 25-tap gather achieves against the traffic a perfect cache would leave, not a share of peak.

The tiled / direct A/B: the same command under RTGPU_DENOISE_TILED=0 and =1 (the knob is read once per process), alternating.

--chain N: instead, what guide chains (Viewport.set_guide_chain(N)) do to the filtered frame: for --passes passes, the relative mean squared error
mean((x - r)^2 / (r^2 + 1e-2)) of the frame against the tool's converged render r (--converged passes of the same scene), over the pixels with
chain_length >= 1 and over the rest, unfiltered, filtered with first-hit guides and filtered with chain guides (five levels, the wrappers' default sigmas, plain
and variance-guided), and the time of one denoise call either way.  --mirror adds a smooth-metal rect and a glass sphere (scenes.add_mirror_props): the stock scene
has no specular surface.

  python tools/bench_denoise.py [--reps 20] [--output profiles/denoise_bench_1080p.json] [--chain 3 --mirror [--converged 1024]]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_call(torch, fn, reps):
    for _ in range(3):
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
    ms = np.array(ms)
    return {"ms_median": float(np.median(ms)), "ms_min": float(ms.min()), "ms_max": float(ms.max())}


def chain_quality(args, torch, ra, scenes):
    w, h = args.width, args.height
    scene, camera = scenes.sponza_class(w / h, args.triangles)
    if args.mirror:
        scenes.add_mirror_props(scene)
    vp = ra.Viewport(w, h, seed=1234, max_ray_depth=args.depth)
    vp.set_renderer(scene)
    vp.render(camera, passes=args.passes)
    guide = vp.next_pass_params(camera)
    # the guides' own params: the frame's, with roulette pushed behind the chain so that it never cuts one (include/rtgpu.h)
    guide.minRussianRouletteDepth = max(int(guide.minRussianRouletteDepth), args.chain)
    noisy = vp.sum_buffer() / np.float32(vp.passes_finished)
    length = vp.render_aovs(guide, ("chain_length",), chain=args.chain)["chain_length"]
    frames = {"unfiltered": noisy}
    times = {}
    stream = torch.cuda.Stream()
    for label, chain in (("first_hit", None), ("chain", args.chain)):
        vp.set_guide_chain(chain)
        frames[label] = vp.denoise(guide)
        frames[label + "_variance"] = vp.denoise(guide, variance=True)
        with torch.cuda.stream(stream):
            times[label] = time_call(torch, lambda: vp.denoise(guide, device=True), args.reps)
    vp.set_guide_chain(None)
    ref_vp = ra.Viewport(w, h, seed=4321, max_ray_depth=args.depth)
    ref_vp.set_renderer(scene)
    ref_vp.render(camera, passes=args.converged)
    ref = ref_vp.sum_buffer() / np.float32(ref_vp.passes_finished)
    inside = length >= 1
    # the chain pixels by what the primary ray hit: a metal (the mirror: one event per vertex) or a dielectric (the sphere: reflect or refract by the pass's draw)
    first_material = vp.render_aovs(guide, ("material",))["material"]
    desc = scene.desc.contents
    kind_of = np.array([desc.materials[m].bsdf for m in range(desc.numMaterials)] + [0], dtype=np.uint32)
    first_kind = kind_of[np.minimum(first_material, desc.numMaterials)]
    metal, glass = inside & (first_kind == ra.BSDF_NAMES.index("metal")), inside & (first_kind == ra.BSDF_NAMES.index("dielectric"))
    rel = lambda x, mask: float(np.mean(((x[mask] - ref[mask]) ** 2) / (ref[mask] ** 2 + 1e-2)))   # noqa: E731
    out = {"scene": "sponza_class" + ("+mirror_props" if args.mirror else ""), "width": w, "height": h, "passes": vp.passes_finished, "converged_passes": args.converged,
           "max_chain": args.chain, "depth": args.depth, "pixels_with_chain": int(inside.sum()), "metal_pixels": int(metal.sum()), "glass_pixels": int(glass.sum()), "denoise_ms": times, "relative_mse": {}}
    for label, x in frames.items():
        out["relative_mse"][label] = {"chain_pixels": rel(x, inside) if inside.any() else None, "metal_pixels": rel(x, metal) if metal.any() else None,
                                      "glass_pixels": rel(x, glass) if glass.any() else None, "other_pixels": rel(x, ~inside)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--triangles", type=int, default=262144)
    ap.add_argument("--output", default=None)
    ap.add_argument("--chain", type=int, default=None)
    ap.add_argument("--mirror", action="store_true")
    ap.add_argument("--converged", type=int, default=1024)
    args = ap.parse_args()
    import torch
    import raytracer_amd as ra
    from raytracer_amd import scenes
    w, h = args.width, args.height
    if args.chain is not None:
        line = json.dumps(chain_quality(args, torch, ra, scenes))
        print(line)
        if args.output:
            with open(args.output, "w") as f:
                f.write(line + "\n")
        return
    scene, camera = scenes.sponza_class(w / h, args.triangles)
    vp = ra.Viewport(w, h, seed=1234, max_ray_depth=args.depth)
    vp.set_renderer(scene)
    lib, ctx = ra.rtgpu_lib(), vp.device_context()
    vp.render(camera, passes=args.passes)
    assert lib.rtgpu_synchronize(ctx) == 0
    # a render pass of the same context, for scale: batches of `passes` passes, wall time to the end of the device work
    per_pass = []
    for _ in range(3):
        t0 = time.perf_counter()
        vp.render(camera, passes=args.passes)
        assert lib.rtgpu_synchronize(ctx) == 0
        per_pass.append(1e3 * (time.perf_counter() - t0) / args.passes)
    guide = vp.next_pass_params(camera)
    out = {"scene": "sponza_class", "triangles": int(scene.desc.contents.numTriangles), "width": w, "height": h, "passes": vp.passes_finished, "reps": args.reps,
           "RTGPU_DENOISE_TILED": os.environ.get("RTGPU_DENOISE_TILED"),   # None: the library's default
           "render_pass_ms": {"median": float(np.median(per_pass)), "min": float(min(per_pass)), "max": float(max(per_pass)), "passes_per_batch": args.passes}}
    names = ("depth", "normal", "position", "base_color")
    stream = torch.cuda.Stream()   # (the null stream would send the calls through the wrappers' side stream)
    with torch.cuda.stream(stream):
        out["guide_render"] = time_call(torch, lambda: vp.render_aovs(guide, names, device=True), args.reps)
        planes = vp.render_aovs(guide, names, device=True)
        has_var = hasattr(lib, "rtgpu_denoise_var_async")
        sums = vp.sum_buffer(secondary=True)
        color, color_half = torch.from_numpy(sums[0]).cuda(), torch.from_numpy(sums[1]).cuda()
        stream.synchronize()
        out["denoise"], out["filter_alone"] = {}, {}
        if has_var:
            out["denoise_var"], out["filter_var_alone"], out["var_over_plain"] = {}, {}, {}
        for iterations in range(1, 6):
            out["denoise"][str(iterations)] = time_call(torch, lambda: vp.denoise(guide, iterations=iterations, device=True), args.reps)
            t = time_call(torch, lambda: ra.atrous_filter(color, planes["depth"], planes["normal"], planes["position"], planes["base_color"], iterations=iterations,
                                                          color_scale=1.0 / vp.passes_finished, ctx=ctx), args.reps)
            t["compulsory_bytes"] = 64 * w * h * iterations
            t["gbytes_per_s_compulsory"] = t["compulsory_bytes"] / t["ms_median"] / 1e6
            out["filter_alone"][str(iterations)] = t
            if has_var:
                out["denoise_var"][str(iterations)] = time_call(torch, lambda: vp.denoise(guide, iterations=iterations, device=True, variance=True, return_variance=True), args.reps)
                tv = time_call(torch, lambda: ra.atrous_filter(color, planes["depth"], planes["normal"], planes["position"], planes["base_color"], iterations=iterations,
                                                               color_scale=1.0 / vp.passes_finished, ctx=ctx, color_half=color_half, return_variance=True), args.reps)
                tv["compulsory_bytes"] = 64 * w * h * iterations
                tv["gbytes_per_s_compulsory"] = tv["compulsory_bytes"] / tv["ms_median"] / 1e6
                out["filter_var_alone"][str(iterations)] = tv
                out["var_over_plain"][str(iterations)] = {"denoise": out["denoise_var"][str(iterations)]["ms_median"] / out["denoise"][str(iterations)]["ms_median"],
                                                          "filter_alone": tv["ms_median"] / t["ms_median"]}
    line = json.dumps(out)
    print(line)
    if args.output:
        with open(args.output, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
