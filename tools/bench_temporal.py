#!/usr/bin/env python3
"""Cost and worth of temporal accumulation (include/rtgpu.h: rtgpu_denoise_temporal_async through Viewport.denoise(temporal=True, device=True)) on the
Sponza-class 1920 x 1080 frame (raytracer_amd.scenes.sponza_class, 262 176 triangles) as the interactive caller drives it: a camera that yaws by `--yaw`
degrees per frame, `--passes` passes per frame, the film reset between frames.

Times, after a warm-up of every shape, `--reps` repetitions (median, min, max), device events around the call on a stream of the tool's own:
  accumulate_pure        raytracer_amd.temporal_accumulate on tensors with a history: k_temporal_pack + k_temporal (the pack is the pure entry's alone)
  accumulate_pure_start  the same without a history: k_temporal alone, every pixel starting (no taps)
  temporal_unfiltered    the context-level call with variance=False: guide render + k_temporal on the context's own records
  temporal_call          the whole call: guide render + k_temporal + five levels of the variance-guided filter
  denoise_var            rtgpu_denoise_var alone on the same film, and guide_render, the five planes alone
  render_pass_ms         one render pass of the same context, for scale (host wall time around a batch that ends in rtgpu_synchronize, per pass)
`k_temporal_in_call_ms` is temporal_unfiltered minus guide_render: the kernel where it runs, on the context's records.  `bytes_per_pixel`: what that kernel
cannot avoid moving -- 68 bytes of this frame's planes, 64 of history records (each read once by a perfect cache), 28 of planar results, 64 of new
records and the unfiltered call's 12 of image -- and `share_of_hbm_peak` the time those bytes take at 8 TB/s over the kernel's time.

Worth: the relative MSE, mean((x - ref)^2 / (ref^2 + 0.01)), against a render of `--reference-passes` passes at the last camera, of (a) rtgpu_denoise_var on
the last frame alone and (b) the temporal call after `--frames` frames; beside them the raw frame and the accumulated frame without the spatial filter.
Prints one JSON line and, with --output, writes it to a file.

--clip adds, per gamma of --clip-gammas at radius 3, minCount 9: `rel_mse` of the same sequence with the history clipped (Viewport.denoise(temporal=True,
clip=...)) filtered and unfiltered, the share of the last frame's pixels whose confidence fell below 0.5 and below 1, and for the first gamma the times
`temporal_call_clipped`, `temporal_unfiltered_clipped` and `accumulate_pure_clipped` beside their unclipped twins (k_temporal_moments + the clipping k_temporal).

--diagnose adds `starts_by_the_model`: the NumPy model (tests/temporal_ref.py) over the guides of the last two frames, with the defaults and with one
surface test relaxed at a time -- how many pixels start and why.

--chain N [--mirror]: another report altogether -- reflections in the history (rtgpu_denoise_temporal_chain through Viewport.denoise(temporal=True, chain=N)).
--mirror adds scenes.add_mirror_props, as tools/bench_denoise.py --mirror does.  Under the yawing camera, after --frames frames, for the pixels with a chain and
for the rest separately: the relative MSE against the converged render of (a) denoise(temporal=True) with first-hit guides, (b) denoise(temporal=True, chain=N)
and (c) denoise(variance=True) under set_guide_chain(N), no history; (a) and (b) also without the spatial filter (variance=False), and with the clip of --clip-gammas' first gamma when --clip is given; the mean
history length inside the chain pixels, by the pure entry; and the times: the pure entry with a history over chain planes against the entry without on the
same planes (k_temporal_pack + k_temporal[_chain], with the clip k_temporal_moments[_chain] in front), and the whole context call against
rtgpu_denoise_temporal[_clip].  These are times of calls: no kernel is timed alone.  `clip_adds_to_pure_ms` is the clipped pure entry minus the unclipped one,
with and without chain planes: the moments kernel and the clipping variant's extra work.  Without --mirror every k is 0: the kChain kernels' cost where they change nothing.

  python tools/bench_temporal.py [--reps 20] [--diagnose] [--output profiles/temporal_bench_1080p.json]
  python tools/bench_temporal.py --chain 3 --mirror --clip [--output profiles/temporal_chain_bench_1080p_mirror.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_denoise import time_call   # noqa: E402

HBM_PEAK = 8.0e12
BYTES_PER_PIXEL = {"current planes": 68, "history records": 64, "planar results": 28, "new records": 64, "image (the unfiltered call, which is the one timed)": 12}


def chain_report(args, torch, ra, scenes):
    w, h = args.width, args.height
    scene, camera = scenes.sponza_class(w / h, args.triangles)
    if args.mirror:
        scenes.add_mirror_props(scene)
    translation, orientation = camera.settings["translation"], camera.settings["orientation_deg"]

    def look(frame):
        camera.set_transform(translation, (orientation[0], orientation[1] + args.yaw * frame, orientation[2]))
        camera.set_perspective(camera.settings["aspect"], camera.settings["fov_rad"])
    vp = ra.Viewport(w, h, seed=1234, max_ray_depth=args.depth)
    vp.set_renderer(scene)
    ctx = vp.device_context()
    last = args.frames - 1
    look(last)
    vp.render(camera, passes=args.reference_passes)
    reference = (vp.sum_buffer() / np.float32(args.reference_passes)).astype(np.float64)
    out = {"scene": "sponza_class" + ("+mirror_props" if args.mirror else ""), "width": w, "height": h, "passes_per_frame": args.passes, "frames": args.frames,
           "yaw_deg_per_frame": args.yaw, "reference_passes": args.reference_passes, "reps": args.reps, "max_chain": args.chain, "max_ray_depth": args.depth}
    guides = ("depth", "normal", "position", "base_color", "object_id")
    chain_guides = guides + ("chain_length", "chain_distance", "virtual_position")
    clips = [("", None)] + ([("_clipped", dict(radius=3, gamma=float(args.clip_gammas.split(",")[0]), min_count=9))] if args.clip else [])
    scale = float(np.float32(1.0 / args.passes))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        def sequence(call):
            """the frames the caller drives; call(guide params) per frame; returns the last one's result"""
            vp.reset_history()
            result = None
            for frame in range(args.frames):
                look(frame)
                vp.reset()
                vp.render(camera, passes=args.passes)
                result = call(vp.next_pass_params(camera))
            return result
        images = {}
        for suffix, clip in clips:
            images["a_temporal_first_hit" + suffix] = sequence(lambda p: vp.denoise(p, temporal=True, variance=True, device=True, clip=clip))
            images["b_temporal_chain" + suffix] = sequence(lambda p: vp.denoise(p, temporal=True, variance=True, device=True, clip=clip, chain=args.chain))
            # the accumulated frames without the spatial filter: what the reprojection alone is worth, apart from what chain guides do to the filter
            images["a_temporal_first_hit_unfiltered" + suffix] = sequence(lambda p: vp.denoise(p, temporal=True, variance=False, device=True, clip=clip))
            images["b_temporal_chain_unfiltered" + suffix] = sequence(lambda p: vp.denoise(p, temporal=True, variance=False, device=True, clip=clip, chain=args.chain))
        vp.set_guide_chain(args.chain)
        images["c_variance_chain_guides_no_history"] = vp.denoise(vp.next_pass_params(camera), variance=True, device=True)
        vp.set_guide_chain(None)
        # the same sequence through the pure entry, which returns the history lengths
        state = dict(history=None, previous=None)

        def pure_step(p):
            g = vp.render_aovs(p, chain_guides, device=True, chain=args.chain)
            s = vp.sum_buffer(secondary=True)
            kw = {} if state["previous"] is None else dict(prev_world_to_screen=list(state["previous"].camera.worldToScreen), prev_sample_offset=tuple(state["previous"].sampleOffset))
            state["before"] = (state["history"], state["previous"])
            state["history"] = ra.temporal_accumulate(torch.from_numpy(s[0]).cuda(), torch.from_numpy(s[1]).cuda(), g["depth"], g["normal"], g["position"], g["base_color"], g["object_id"],
                                                      history=state["history"], color_scale=scale, ctx=ctx, chain={k: g[k] for k in ra.CHAIN_KEYS}, **kw)
            state["previous"], state["planes"], state["sums"] = p, g, s
            return state["history"]
        pure = sequence(pure_step)
        stream.synchronize()
        g = state["planes"]
        inside = (g["chain_length"] >= 1).cpu().numpy()
        hit = torch.isfinite(g["depth"]).cpu().numpy()
        length = pure["length"].cpu().numpy()
        # the chain pixels by what the primary ray hit: a metal (the mirror: one event per vertex) or a dielectric (the sphere: reflect or refract by the pass's draw)
        first_material = vp.render_aovs(state["previous"], ("material",))["material"]
        desc = scene.desc.contents
        kind_of = np.array([desc.materials[m].bsdf for m in range(desc.numMaterials)] + [0], dtype=np.uint32)
        first_kind = kind_of[np.minimum(first_material, desc.numMaterials)]
        metal, glass = inside & (first_kind == ra.BSDF_NAMES.index("metal")), inside & (first_kind == ra.BSDF_NAMES.index("dielectric"))
        out["metal_pixels"] = {"share": float(metal.mean()), "length_mean": float(length[metal & hit].mean()) if (metal & hit).any() else None,
                               "share_started_in_the_last_frame": float((length[metal & hit] == 1.0).mean()) if (metal & hit).any() else None}
        out["glass_pixels"] = {"share": float(glass.mean()), "length_mean": float(length[glass & hit].mean()) if (glass & hit).any() else None,
                               "share_started_in_the_last_frame": float((length[glass & hit] == 1.0).mean()) if (glass & hit).any() else None}
        out["chain_pixels"] = {"share": float(inside.mean()), "share_with_a_surface_guide": float((inside & hit).mean()),
                               "length_mean": float(length[inside & hit].mean()) if (inside & hit).any() else None,
                               "share_started_in_the_last_frame": float((length[inside & hit] == 1.0).mean()) if (inside & hit).any() else None}
        out["other_pixels"] = {"length_mean": float(length[~inside & hit].mean()), "share_started_in_the_last_frame": float((length[~inside & hit] == 1.0).mean())}
        error = lambda image: (image.cpu().numpy().astype(np.float64) - reference) ** 2 / (reference ** 2 + 0.01)   # noqa: E731
        out["rel_mse"] = {}
        for name, image in images.items():
            e = error(image).mean(axis=-1)
            out["rel_mse"][name] = {"chain_pixels": float(e[inside].mean()) if inside.any() else None, "metal_pixels": float(e[metal].mean()) if metal.any() else None,
                                    "glass_pixels": float(e[glass].mean()) if glass.any() else None, "other_pixels": float(e[~inside].mean()), "frame": float(e.mean())}
        # times: the film holds the last frame and the pure sequence's history of the frame before it
        history, previous = state["before"]
        color, color_half = torch.from_numpy(state["sums"][0]).cuda(), torch.from_numpy(state["sums"][1]).cuda()
        kw = dict(depth=g["depth"], normal=g["normal"], position=g["position"], albedo=g["base_color"], object_id=g["object_id"].to(torch.int32), color_scale=scale, ctx=ctx,
                  prev_world_to_screen=list(previous.camera.worldToScreen), prev_sample_offset=tuple(previous.sampleOffset))
        chain = {k: (g[k].to(torch.int32) if k == "chain_length" else g[k]) for k in ra.CHAIN_KEYS}
        plain_history = {k: v for k, v in history.items() if k != "chain_length"}
        guide = state["previous"]
        for suffix, clip in clips:
            out["accumulate_pure" + suffix] = time_call(torch, lambda: ra.temporal_accumulate(color, color_half, history=plain_history, clip=clip, **kw), args.reps)
            out["accumulate_pure_chain" + suffix] = time_call(torch, lambda: ra.temporal_accumulate(color, color_half, history=history, clip=clip, chain=chain, **kw), args.reps)
            out["temporal_call" + suffix] = time_call(torch, lambda: vp.denoise(guide, temporal=True, variance=True, device=True, clip=clip), args.reps)
            out["temporal_call_chain" + suffix] = time_call(torch, lambda: vp.denoise(guide, temporal=True, variance=True, device=True, clip=clip, chain=args.chain), args.reps)
        # what the clip adds to the pure entry: k_temporal_moments[_chain] and the clipping variant of k_temporal[_chain] in the unclipped one's place -- the nearest this
        # tool comes to the kernels themselves; it times calls, never a kernel alone
        if args.clip:
            out["clip_adds_to_pure_ms"] = {"without_chain": out["accumulate_pure_clipped"]["ms_median"] - out["accumulate_pure"]["ms_median"],
                                           "with_chain": out["accumulate_pure_chain_clipped"]["ms_median"] - out["accumulate_pure_chain"]["ms_median"]}
    line = json.dumps(out)
    print(line)
    if args.output:
        with open(args.output, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--yaw", type=float, default=0.25)
    ap.add_argument("--reference-passes", type=int, default=512)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--triangles", type=int, default=262144)
    ap.add_argument("--diagnose", action="store_true", help="also count, by the NumPy model on the last two frames' guides, why pixels start")
    ap.add_argument("--clip", action="store_true", help="add the clipped columns: the same sequence with the history clipped, once per gamma")
    ap.add_argument("--clip-gammas", default="1,2,4,8")
    ap.add_argument("--chain", type=int, default=None, help="the report on reflections in the history instead: denoise(temporal=True, chain=N) beside the calls that exist")
    ap.add_argument("--mirror", action="store_true", help="with --chain: add a mirror and a glass sphere (scenes.add_mirror_props)")
    ap.add_argument("--output", default=None)
    args = ap.parse_args()
    if args.frames < 2:
        ap.error("--frames must be at least 2")
    if args.mirror and args.chain is None:
        ap.error("--mirror goes with --chain N")
    import torch
    import raytracer_amd as ra
    from raytracer_amd import scenes
    if args.chain is not None:
        return chain_report(args, torch, ra, scenes)
    w, h = args.width, args.height
    scene, camera = scenes.sponza_class(w / h, args.triangles)
    translation, orientation = camera.settings["translation"], camera.settings["orientation_deg"]

    def look(frame):
        camera.set_transform(translation, (orientation[0], orientation[1] + args.yaw * frame, orientation[2]))
        # (worldToScreen is what set_perspective computes from the transform of the moment, as in the reference: a moved camera has to be given it again)
        camera.set_perspective(camera.settings["aspect"], camera.settings["fov_rad"])
    vp = ra.Viewport(w, h, seed=1234, max_ray_depth=args.depth)
    vp.set_renderer(scene)
    lib, ctx = ra.rtgpu_lib(), vp.device_context()
    last = args.frames - 1
    # the reference: the last camera, converged
    look(last)
    vp.render(camera, passes=args.reference_passes)
    reference = vp.sum_buffer() / np.float32(args.reference_passes)
    per_pass = []
    for _ in range(3):
        t0 = time.perf_counter()
        vp.render(camera, passes=20)
        assert lib.rtgpu_synchronize(ctx) == 0
        per_pass.append(1e3 * (time.perf_counter() - t0) / 20)
    out = {"scene": "sponza_class", "triangles": int(scene.desc.contents.numTriangles), "width": w, "height": h, "passes_per_frame": args.passes, "frames": args.frames,
           "yaw_deg_per_frame": args.yaw, "reference_passes": args.reference_passes, "reps": args.reps,
           "render_pass_ms": {"median": float(np.median(per_pass)), "min": float(min(per_pass)), "max": float(max(per_pass)), "passes_per_batch": 20}}
    rel_mse = lambda image: float(np.mean((image.astype(np.float64) - reference) ** 2 / (reference.astype(np.float64) ** 2 + 0.01)))   # noqa: E731
    names = ("depth", "normal", "position", "base_color", "object_id")
    builds_still = vp.beam_list_info()["builds"]   # the reference render and the timed batches above: one camera, so its beam lists are built (include/rtgpu.h)
    stream = torch.cuda.Stream()   # (the null stream would send the calls through the wrappers' side stream)
    with torch.cuda.stream(stream):
        # the sequence the caller drives
        vp.reset_history()
        previous = None
        for frame in range(args.frames):
            look(frame)
            vp.reset()
            vp.render(camera, passes=args.passes)
            guide = vp.next_pass_params(camera)
            if frame == last:
                planes = vp.render_aovs(guide, names, device=True)
                history_before = previous
            temporal = vp.denoise(guide, temporal=True, variance=True, device=True)
            previous = guide
        stream.synchronize()
        # a camera that turns with every frame must never pay for a build of beam lists: the sequence adds none
        out["beam_list_builds"] = {"still_reference_and_timed_batches": int(builds_still), "in_the_turning_sequence": int(vp.beam_list_info()["builds"] - builds_still)}
        sums = vp.sum_buffer(secondary=True)
        scale = np.float32(1.0 / args.passes)
        alone = vp.denoise(guide, variance=True, device=True)
        vp.reset_history()
        out["rel_mse"] = {"raw_frame": rel_mse(sums[0] * scale), "a_denoise_var_last_frame_alone": rel_mse(alone.cpu().numpy()),
                          "b_temporal_after_%d_frames" % args.frames: rel_mse(temporal.cpu().numpy())}
        # the accumulated frame without the spatial filter: the sequence again
        # beside it the same chain through the pure entry, which also returns the history lengths: how much of the frame finds its history
        pure, previous = None, None
        for frame in range(args.frames):
            look(frame)
            vp.reset()
            vp.render(camera, passes=args.passes)
            step = vp.next_pass_params(camera)
            g = vp.render_aovs(step, names, device=True)
            s = vp.sum_buffer(secondary=True)
            camera_kw = {} if previous is None else dict(prev_world_to_screen=list(previous.camera.worldToScreen), prev_sample_offset=tuple(previous.sampleOffset))
            pure = ra.temporal_accumulate(torch.from_numpy(s[0]).cuda(), torch.from_numpy(s[1]).cuda(), g["depth"], g["normal"], g["position"], g["base_color"], g["object_id"],
                                          history=pure, color_scale=float(scale), ctx=ctx, **camera_kw)
            unfiltered = vp.denoise(step, temporal=True, variance=False, device=True)
            if frame == last - 1:
                guides_before = {k: v.cpu().numpy() for k, v in g.items()}
            previous_step, previous = previous, step
        out["rel_mse"]["temporal_unfiltered_after_%d_frames" % args.frames] = rel_mse(unfiltered.cpu().numpy())
        albedo = g["base_color"].permute(1, 2, 0)
        remodulated = pure["a"] * torch.where(albedo > 1e-3, albedo, torch.ones_like(albedo))
        hit = torch.isfinite(g["depth"])
        length = pure["length"][hit]
        out["history"] = {"pure_chain_equals_context_call": bool(torch.equal(remodulated.view(torch.int32), unfiltered.view(torch.int32))),
                          "hit_share": float(hit.float().mean()), "length_mean_of_hits": float(length.mean()),
                          "share_of_hits_that_started_in_the_last_frame": float((length == 1.0).float().mean()),
                          "share_of_hits_with_length_at_least_8": float((length >= 8.0).float().mean())}
        # the same sequence with the history clipped, filtered and not
        gammas = [float(g) for g in args.clip_gammas.split(",")] if args.clip else []
        for gamma in gammas:
            clip = dict(radius=3, gamma=gamma, min_count=9)
            for variance, label in ((True, "b_temporal_clipped_gamma_%g"), (False, "temporal_unfiltered_clipped_gamma_%g")):
                vp.reset_history()
                for frame in range(args.frames):
                    look(frame)
                    vp.reset()
                    vp.render(camera, passes=args.passes)
                    image, confidence = vp.denoise(vp.next_pass_params(camera), temporal=True, variance=variance, device=True, clip=clip, return_confidence=True)
                out["rel_mse"][label % gamma] = rel_mse(image.cpu().numpy())
            out.setdefault("clip_confidence", {})["gamma_%g" % gamma] = {"share_below_0.5": float((confidence < 0.5).float().mean()), "share_below_1": float((confidence < 1.0).float().mean())}
        if gammas:   # (leave the film and the history as the timed calls below expect them: the last frame, unclipped)
            vp.reset_history()
            look(last)
            vp.reset()
            vp.render(camera, passes=args.passes)
            guide = vp.next_pass_params(camera)
            vp.denoise(guide, temporal=True, variance=True, device=True)
        # times: the film holds the last frame; every timed temporal call sees a full history (the call before it stored one at the same camera)
        # (the five planes through the raw entry, into tensors made once: what the temporal call itself does, without the wrapper's id conversion)
        raw = [torch.empty((ra.AOV_PLANES[name][1], h, w), dtype=torch.float32 if ra.AOV_PLANES[name][2] is np.float32 else torch.int32, device=temporal.device) for name in names]
        plane_ids, plane_ptrs = (C.c_uint32 * 5)(*[ra.AOV_PLANES[name][0] for name in names]), (C.c_void_p * 5)(*[t.data_ptr() for t in raw])
        out["guide_render"] = time_call(torch, lambda: lib.rtgpu_render_aovs_async(ctx, C.byref(guide), plane_ids, C.c_uint32(5), plane_ptrs, C.c_void_p(stream.cuda_stream)), args.reps)
        out["denoise_var"] = time_call(torch, lambda: vp.denoise(guide, variance=True, device=True), args.reps)
        out["temporal_call"] = time_call(torch, lambda: vp.denoise(guide, temporal=True, variance=True, device=True), args.reps)
        out["temporal_unfiltered"] = time_call(torch, lambda: vp.denoise(guide, temporal=True, variance=False, device=True), args.reps)
        color, color_half = torch.from_numpy(sums[0]).cuda(), torch.from_numpy(sums[1]).cuda()
        kw = dict(depth=planes["depth"], normal=planes["normal"], position=planes["position"], albedo=planes["base_color"], object_id=planes["object_id"].to(torch.int32),
                  color_scale=float(scale), ctx=ctx)
        first = ra.temporal_accumulate(color, color_half, **kw)
        camera_kw = dict(prev_world_to_screen=list(history_before.camera.worldToScreen), prev_sample_offset=tuple(history_before.sampleOffset))
        out["accumulate_pure"] = time_call(torch, lambda: ra.temporal_accumulate(color, color_half, history=first, **camera_kw, **kw), args.reps)
        out["accumulate_pure_start"] = time_call(torch, lambda: ra.temporal_accumulate(color, color_half, **kw), args.reps)
        if gammas:
            clip = dict(radius=3, gamma=gammas[0], min_count=9)
            out["temporal_call_clipped"] = time_call(torch, lambda: vp.denoise(guide, temporal=True, variance=True, device=True, clip=clip), args.reps)
            out["temporal_unfiltered_clipped"] = time_call(torch, lambda: vp.denoise(guide, temporal=True, variance=False, device=True, clip=clip), args.reps)
            out["accumulate_pure_clipped"] = time_call(torch, lambda: ra.temporal_accumulate(color, color_half, history=first, clip=clip, **camera_kw, **kw), args.reps)
            out["temporal_call_again"] = time_call(torch, lambda: vp.denoise(guide, temporal=True, variance=True, device=True), args.reps)
            out["temporal_unfiltered_again"] = time_call(torch, lambda: vp.denoise(guide, temporal=True, variance=False, device=True), args.reps)
    # why pixels start, by the model (tests/temporal_ref.py) on the guides of the last two frames: the defaults, then one test relaxed at a time
    if args.diagnose:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import temporal_ref as ref
        cur = {k: v.cpu().numpy() for k, v in g.items()}
        ones = np.ones((h, w, 3), dtype=np.float32)
        model = lambda guides, history=None, **kw: ref.accumulate(ones, ones, guides["depth"], guides["normal"], guides["position"], None,   # noqa: E731
                                                                  guides["object_id"].astype(np.uint32), history=history, demodulate=False, **kw)
        before = model(guides_before)[0]
        camera_kw = dict(prev_world_to_screen=list(previous_step.camera.worldToScreen), prev_sample_offset=tuple(previous_step.sampleOffset))
        out["starts_by_the_model"] = {}
        for label, kw in (("defaults", {}), ("normal test off", dict(normal_threshold=-1.0)), ("plane test off", dict(plane_tolerance=1e30)),
                          ("plane tolerance 0.1", dict(plane_tolerance=0.1))):
            _, motion, taken, why = model(cur, before, **camera_kw, **kw)
            out["starts_by_the_model"][label] = {"invalid": float((why == ref.START_INVALID).mean()), "behind_or_outside": float((why == ref.START_OFF_SCREEN).mean()),
                                                 "no_tap_taken": float((why == ref.START_NO_TAP).mean()), "four_taps": float((taken == 4).mean()),
                                                 "one_to_three_taps": float(((taken > 0) & (taken < 4)).mean()),
                                                 "mean_abs_motion_x": float(np.abs(motion[0][why == ref.BLENDED]).mean()) if (why == ref.BLENDED).any() else None}
    kernel_ms = out["temporal_unfiltered"]["ms_median"] - out["guide_render"]["ms_median"]
    total = sum(BYTES_PER_PIXEL.values())
    out["k_temporal_in_call_ms"] = kernel_ms
    out["bytes_per_pixel"] = dict(BYTES_PER_PIXEL, total=total)
    out["share_of_hbm_peak"] = (total * w * h / HBM_PEAK) / (kernel_ms * 1e-3) if kernel_ms > 0 else None
    line = json.dumps(out)
    print(line)
    if args.output:
        with open(args.output, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
