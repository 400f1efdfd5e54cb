#!/usr/bin/env python3
"""What a ray source costs (include/rtgpu.h: rtgpu_set_ray_source, rtgpu_read_camera_rays) on the Sponza-class 1920 x 1080 frame bench.py times: the
262 176-triangle mesh (raytracer_amd.scenes.sponza_class), depth 8, the library's defaults.  Everything in ONE run, `--reps` repetitions each (at least
10): median, min, max.

  pass_camera          ms per pass over `--passes` (20) passes from the camera: queued back to back, then read back (host wall time, synchronised)
  pass_table           the same passes from the table exported from that camera (Viewport.camera_rays -> set_ray_source), alternating with the camera's
                       repetition by repetition; the two frames must have the same bits, or the tool stops
  set_ray_source_device  rtgpu_set_ray_source_device alone on a device tensor: the device-to-device copy and k_ray_source_check (host wall time; the call
                       returns synchronised)
  read_camera_rays_async rtgpu_read_camera_rays_async alone: k_camera_rays into a device tensor (device events)
  pass_table_set_per_pass  `--passes` passes with a new table set before each pass -- what anti-aliasing under a source costs, because every set call ends
                       the batch of passes in flight (ms per pass, the set calls included)
The yardstick is the camera's passes of the same run; `table_over_camera` and `set_per_pass_over_camera` are the ratios of the medians.  The table kernels
read 32 bytes per pixel and pass where the camera kernels read none.  Prints one JSON line and, with --output, writes it to a file.

  python tools/bench_ray_source.py [--reps 12] [--output profiles/ray_source_bench_1080p.json]

--lens: what a LENS source costs (rtgpu_set_lens_source), on the same frame, in one run; every row is ms per pass over `--passes` passes queued back to back
and read back, `--reps` repetitions, median with min .. max:

  a_camera_jittered      the camera at the viewport's anti-aliasing spread 0.5: a new sample offset every pass
  b_lens_table           the same passes, the same offsets, under the camera's exported lens table (Viewport.camera_footprints at offset 0, set once);
                         alternates with (a) repetition by repetition
  c_plain_set_per_pass   the plain source's route to the same picture: a finished table per pass (Viewport.lens_source_rays, made beforehand on the device),
                         set before every pass -- every set call ends the batch in flight
  d_dof_camera / d_dof_lens_table   a camera with depth of field against its lens table set with lens=True, alternating
  e_set_lens_source_device          rtgpu_set_lens_source_device alone on a device tensor: the copy and k_lens_source_check (host wall time)
The lens kernels read 128 bytes per pixel and pass.  `lens_minus_camera_ms` is (b) - (a) of the medians, `camera_spread_ms` (a)'s max - min; where the
first exceeds the second it is reported as `table_cost_ms`, else that is null.  (b) must beat (c) or the tool stops: that is what the feature is for.

  python tools/bench_ray_source.py --lens [--reps 12] [--output profiles/lens_source_bench_1080p.json]"""
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


def stats(ms):
    ms = np.array(ms, dtype=np.float64)
    return {"ms_median": float(np.median(ms)), "ms_min": float(ms.min()), "ms_max": float(ms.max())}


def lens_block(args, torch, ra, scenes):
    w, h = args.width, args.height
    lib = ra.rtgpu_lib()
    scene, camera = scenes.sponza_class(w / h, args.triangles)
    vp = ra.Viewport(w, h, seed=1234, max_ray_depth=args.depth, anti_aliasing_spread=0.5)
    vp.set_renderer(scene)
    ctx = vp.device_context()

    def passes_of(cam):
        params = [vp.next_pass_params(cam) for _ in range(args.passes)]
        for i, p in enumerate(params):
            p.passIndex = i
        return params

    def at_zero(p):
        q = ra.RtPassParams.from_buffer_copy(p)
        q._seed_keepalive = p._seed_keepalive
        q.sampleOffset[0] = q.sampleOffset[1] = 0.0
        return q

    def frame(params, source):
        """`params` from the camera (source None) or under the lens table `source` = (table, lens, bokeh shape): ms per pass, the frame"""
        if source is None:
            vp.set_ray_source(None)
        else:
            vp.set_lens_source(source[0], lens=source[1], bokeh_shape=source[2])
        vp.reset()
        vp.sum_buffer()
        t0 = time.perf_counter()
        for p in params:
            vp.render_pass_with(p)
        film = vp.sum_buffer()
        return 1e3 * (time.perf_counter() - t0) / args.passes, film

    def alternate(params, source):
        frame(params, None), frame(params, source)   # warm-up
        camera_ms, lens_ms, worst = [], [], 0.0
        for _ in range(args.reps):   # alternating: both see the same clocks
            ms, want = frame(params, None)
            camera_ms.append(ms)
            ms, got = frame(params, source)
            lens_ms.append(ms)
            worst = max(worst, float(np.abs(got.mean(axis=(0, 1)) - want.mean(axis=(0, 1))).max() / want.mean()))
        return camera_ms, lens_ms, worst

    params = passes_of(camera)
    table = vp.camera_footprints(at_zero(params[0]), device=True)
    torch.cuda.synchronize()
    a_ms, b_ms, ab_mean = alternate(params, (table, False, 0))

    # (c) the plain source, a finished table per pass: the rays the lens table gives each pass, exported beforehand
    vp.set_lens_source(table)
    plain = [vp.lens_source_rays(p, device=True) for p in params]
    torch.cuda.synchronize()

    def per_pass():
        vp.reset()
        vp.sum_buffer()
        t0 = time.perf_counter()
        for p, t in zip(params, plain):
            vp.set_ray_source(t)
            vp.render_pass_with(p)
        vp.sum_buffer()
        return 1e3 * (time.perf_counter() - t0) / args.passes
    per_pass()
    c_ms = [per_pass() for _ in range(args.reps)]
    del plain

    # (d) depth of field: the camera's own lens against the table's
    camera.set_dof(True, 6.0, 0.05)
    camera.set_lens(bokeh_shape=1)
    dof_params = passes_of(camera)
    dof_table = vp.camera_footprints(at_zero(dof_params[0]), device=True)
    torch.cuda.synchronize()
    d_camera_ms, d_lens_ms, d_mean = alternate(dof_params, (dof_table, True, 1))

    # (e) the set call alone
    stream = torch.cuda.Stream()
    handle = C.c_void_p(stream.cuda_stream)
    settings = ra.RtLensSourceParams(1, 1)
    e_ms = []
    with torch.cuda.stream(stream):
        for i in range(3 + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = lib.rtgpu_set_lens_source_device(ctx, C.c_void_p(dof_table.data_ptr()), C.c_uint64(w * h), C.byref(settings), handle)
            if r != 0:
                raise SystemExit("rtgpu_set_lens_source_device: %s" % (lib.rtgpu_last_error() or b"").decode())
            if i >= 3:
                e_ms.append(1e3 * (time.perf_counter() - t0))
    torch.cuda.synchronize()

    result = {
        "tool": "bench_ray_source --lens", "width": w, "height": h, "triangles": args.triangles, "depth": args.depth, "passes": args.passes, "reps": args.reps,
        "device": torch.cuda.get_device_name(0), "anti_aliasing_spread": 0.5, "table_bytes": int(w) * int(h) * 128,
        "a_camera_jittered": stats(a_ms), "b_lens_table": stats(b_ms), "c_plain_set_per_pass": stats(c_ms),
        "d_dof_camera": stats(d_camera_ms), "d_dof_lens_table": stats(d_lens_ms), "e_set_lens_source_device": stats(e_ms),
        # the frames are the same estimate, not the same bits (the table's jitter rounds each step on its own): relative difference of the channel means
        "b_mean_differs_from_a_by": ab_mean, "d_lens_mean_differs_from_camera_by": d_mean,
    }
    a, b, c = result["a_camera_jittered"], result["b_lens_table"], result["c_plain_set_per_pass"]
    result["lens_over_camera"] = b["ms_median"] / a["ms_median"]
    result["plain_set_per_pass_over_lens"] = c["ms_median"] / b["ms_median"]
    result["lens_minus_camera_ms"] = b["ms_median"] - a["ms_median"]
    result["camera_spread_ms"] = a["ms_max"] - a["ms_min"]
    result["table_cost_ms"] = result["lens_minus_camera_ms"] if result["lens_minus_camera_ms"] > result["camera_spread_ms"] else None
    result["dof_lens_over_dof_camera"] = result["d_dof_lens_table"]["ms_median"] / result["d_dof_camera"]["ms_median"]
    print(json.dumps(result))
    if args.output:
        with open(args.output, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    if not b["ms_median"] < c["ms_median"]:
        raise SystemExit("the lens table (%.3f ms per pass) does not beat a plain table per pass (%.3f)" % (b["ms_median"], c["ms_median"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--triangles", type=int, default=262144)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--output", default=None)
    ap.add_argument("--lens", action="store_true", help="the lens source's block instead (rtgpu_set_lens_source)")
    args = ap.parse_args()
    if args.reps < 10:
        ap.error("--reps must be at least 10")

    import torch
    import __graft_entry__ as g
    g.build()
    import raytracer_amd as ra
    from raytracer_amd import scenes

    if args.lens:
        return lens_block(args, torch, ra, scenes)
    w, h = args.width, args.height
    lib = ra.rtgpu_lib()
    scene, camera = scenes.sponza_class(w / h, args.triangles)
    vp = ra.Viewport(w, h, seed=1234, max_ray_depth=args.depth, anti_aliasing_spread=0.0)   # spread 0: one table serves every pass
    vp.set_renderer(scene)
    ctx = vp.device_context()
    params = [vp.next_pass_params(camera) for _ in range(args.passes)]
    for i, p in enumerate(params):
        p.passIndex = i
    table = vp.camera_rays(params[0], device=True)
    torch.cuda.synchronize()

    def frame(source):
        """the passes from the camera (source None) or from `source`; ms per pass and the frame's two sum buffers"""
        vp.set_ray_source(source)
        vp.reset()
        vp.sum_buffer()
        t0 = time.perf_counter()
        for p in params:
            vp.render_pass_with(p)
        sums = vp.sum_buffer(secondary=True)
        return 1e3 * (time.perf_counter() - t0) / args.passes, sums

    frame(None), frame(table)   # warm-up: the scene's upload, the lanes' arenas, both sets of kernels
    camera_ms, table_ms = [], []
    for _ in range(args.reps):   # alternating: both see the same clocks
        ms, want = frame(None)
        camera_ms.append(ms)
        ms, got = frame(table)
        table_ms.append(ms)
        for a, b in zip(got, want):
            if not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
                raise SystemExit("the table's frame differs from the camera's: %d words" % int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32))))

    def per_pass():
        vp.reset()
        vp.sum_buffer()
        t0 = time.perf_counter()
        for p in params:
            vp.set_ray_source(table)
            vp.render_pass_with(p)
        vp.sum_buffer()
        return 1e3 * (time.perf_counter() - t0) / args.passes
    per_pass()
    set_per_pass_ms = [per_pass() for _ in range(args.reps)]

    stream = torch.cuda.Stream()
    handle = C.c_void_p(stream.cuda_stream)
    out = torch.empty_like(table)
    set_ms = []
    with torch.cuda.stream(stream):
        for i in range(3 + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = lib.rtgpu_set_ray_source_device(ctx, C.c_void_p(table.data_ptr()), C.c_uint64(w * h), handle)
            if r != 0:
                raise SystemExit("rtgpu_set_ray_source_device: %s" % (lib.rtgpu_last_error() or b"").decode())
            if i >= 3:
                set_ms.append(1e3 * (time.perf_counter() - t0))
        export = time_call(torch, lambda: lib.rtgpu_read_camera_rays_async(ctx, C.byref(params[0]), C.c_void_p(out.data_ptr()), handle), args.reps)
    torch.cuda.synchronize()
    if not torch.equal(out.view(torch.int32), table.view(torch.int32)):
        raise SystemExit("the export differs from run to run")

    result = {
        "tool": "bench_ray_source", "width": w, "height": h, "triangles": args.triangles, "depth": args.depth, "passes": args.passes, "reps": args.reps,
        "device": torch.cuda.get_device_name(0), "frames_have_the_same_bits": True, "table_bytes": int(w) * int(h) * 32,
        "pass_camera": stats(camera_ms), "pass_table": stats(table_ms), "pass_table_set_per_pass": stats(set_per_pass_ms),
        "set_ray_source_device": stats(set_ms), "read_camera_rays_async": export,
    }
    result["table_over_camera"] = result["pass_table"]["ms_median"] / result["pass_camera"]["ms_median"]
    result["set_per_pass_over_camera"] = result["pass_table_set_per_pass"]["ms_median"] / result["pass_camera"]["ms_median"]
    line = json.dumps(result)
    print(line)
    if args.output:
        with open(args.output, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
