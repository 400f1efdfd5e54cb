#!/usr/bin/env python3
"""Cost and worth of moving objects between frames (include/rtgpu.h: rtgpu_update_objects, temporal accumulation that follows moving objects) on the
Sponza-class 1920 x 1080 frame: the 262 176-triangle mesh (raytracer_amd.scenes.sponza_class_mesh) plus a handful of objects that orbit in front of the camera
-- two spheres, a box and a small mesh (12 triangles) -- so that the scene takes the two-level 4-wide walk.  `--passes` passes per frame, the film reset
between frames, the orbit advanced by `--step` degrees per frame.

Times (after a warm-up; `--reps` repetitions: median, min, max):
  host_update            Scene.update(): the top-level tree rebuilt over the objects' boxes, the flat objects rewritten (host wall time)
  update_objects         Viewport.update_scene() -> rtgpu_update_objects of that update (host wall time; the call synchronises as rtgpu_upload_scene does)
  upload_scene           rtgpu_upload_scene of the same scene, for comparison (host wall time), and `bytes_uploaded` by the update (rtgpu_get_update_info)
  k_temporal_static      rtgpu_temporal_accumulate_async on device tensors with a history: k_temporal_pack + k_temporal<false> (device events)
  k_temporal_moving      rtgpu_temporal_accumulate_moving_async on the same tensors and a device table: k_temporal_pack + k_temporal<true>
`k_temporal_motion_table_ms` is the difference of the two medians: what the table costs the kernel.

Worth: the relative MSE, mean((x - ref)^2 / (ref^2 + 0.01)), against a render of `--reference-passes` passes of the scene as it stands after `--frames` frames,
over the whole frame and over the pixels of the orbiting objects alone, of
  a  this feature: update_scene() + Viewport.denoise(temporal=True) every frame, the history kept across the moves
  b  the history dropped at every move (what a caller had to do: every move was a new scene)
  c  rtgpu_denoise_var on the last frame alone
  d  (--clip) a with the history clipped to each frame's local colour statistics (Viewport.denoise(temporal=True, clip=...)), once per gamma of --clip-gammas at
     radius 3, minCount 9; beside each the share of the last frame's pixels whose confidence fell below 0.5 (where the history was pulled far) and below 1
The history follows surfaces, not light: where a moved object's shadow was, and on a surface that turned towards or away from a light, it lags by what alphaMin
allows.  Under the scene's sun (20 000 units through a one-degree cone) that lag dominates a RELATIVE error; --no-sun measures the same frames under the sky alone.
Prints one JSON line and, with --output, writes it to a file.

  python tools/bench_update.py [--reps 20] [--output profiles/update_bench_1080p.json]

--deform: cost and worth of DEFORMING the mesh between frames instead (rtgpu_update_mesh).  The Sponza-class mesh alone (a single-mesh scene, bench.py's) under a
travelling sine: every vertex is displaced along y by amplitude * sin(2 pi (x + z) / wavelength + phase), amplitude = `--amplitude` times the largest extent of
the mesh's box (default 0.002: 6 cm on the 30 m hall), the wave one tenth of that extent long, the phase advanced by 0.4 rad per frame.  Times:
  host_update            Scene.set_mesh_vertices() + Scene.update(): the mirror's own refit (host wall time)
  update_mesh            Viewport.update_scene() -> rtgpu_update_mesh (host wall time; the call synchronises) and `bytes_uploaded` by it
  upload_scene           rtgpu_upload_scene of the same deformed scene in the same run: the only way to do this before
  pass_ms                ms per pass (wall, `--bench-passes` passes, synchronised) on the REFIT tree and on the same vertices built and uploaded AFRESH, at the
                         amplitude and at four times it: the price of the kept topology and the kept collapse
  rel_mse                after `--frames` frames against `--reference-passes` passes of the last frame's mesh: the history kept across the updates (every pixel of
                         the deformed mesh starts anew at each: tracking is off) and dropped at every update
--deform --track: what following the deformation costs and buys (rtgpu_set_deform_tracking, Viewport.track_deformation).  Both sides of every comparison in this run:
  rel_mse                at the amplitude and at four times it, each against its own reference: `history_tracked` beside the two figures above
  update_mesh_tracked    rtgpu_update_mesh with the snapshot copy against `update_mesh_untracked`: a temporal call between the updates in both (only the first
                         update after a history takes a snapshot), host wall time of Viewport.update_scene()
  denoise_temporal       the whole call after an update, Viewport.denoise(temporal=True, variance=True, device=True) synchronised (host wall time): tracked -- two
                         guide planes more and k_temporal<true, false, true> -- against untracked
  k_temporal_moving / k_temporal_deform   the pure _async entries on the same device planes and a one-record table (device events): k_temporal_pack +
                         k_temporal<true> against k_temporal_pack + k_temporal<true, false, true> with the mesh's old triangle records
--deform --device: deforming from positions that are on the device already (rtgpu_update_mesh_device, Viewport.update_mesh_device), in the same run and
interleaved with its yardstick.  Every row: median, min, max and `spread` = max - min over `--reps`:
  entry_host / entry_device      rtgpu_update_mesh on host positions against rtgpu_update_mesh_device on the same positions in a device tensor, alternating
                         call by call (host wall time; both return synchronised).  `device_entry_below_host_entry_by_more_than_its_spread` is the one
                         condition under which "faster" may be written
  k_refit_check          the check alone (rtgpu_refit_check_async: init + k_refit_check; device events)
  route_host / route_device      from a device-resident tensor to an updated scene: .cpu().numpy() -> set_mesh_vertices -> update -> update_scene against
                         update_mesh_device -> update -> update_scene (host wall time), in alternating blocks; the second round is kept
  pass_ms_by_route       ms per pass on the tables either route refitted from the same positions: the same bits, so one timing of each"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_denoise import time_call   # noqa: E402

ORBIT_CENTRE, ORBIT_RADIUS = (-6.0, 2.0, 0.6), 2.2
NAMES = ("color", "color_half", "depth", "normal", "position", "albedo", "object_id", "prev_a", "prev_b", "prev_length", "prev_depth", "prev_normal", "prev_position",
         "prev_object_id")


def wall(fn, reps):
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    ms = np.array(ms)
    return {"ms_median": float(np.median(ms)), "ms_min": float(ms.min()), "ms_max": float(ms.max())}


def track_costs(args, ra, lib, ctx, scene, vp, camera, wave, out):
    """--deform --track: the update with and without the snapshot copy, the whole temporal call with and without the two planes, the kernel with and without the gather"""
    import torch
    w, h = args.width, args.height
    stats = lambda ms: {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}   # noqa: E731
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for track in (False, True, False, True):      # interleaved: both see the same clocks; the second round is the one kept
            vp.track_deformation(track)
            vp.reset_history()
            update, call = [], []
            for frame in range(2 + args.reps):
                vp.reset()
                vp.render(camera, passes=args.passes)
                guide = vp.next_pass_params(camera)
                torch.cuda.synchronize()
                t0 = time.perf_counter(); vp.denoise(guide, temporal=True, variance=True, device=True); torch.cuda.synchronize(); t1 = time.perf_counter()
                scene.set_mesh_vertices(0, wave(20 + frame, args.amplitude)); scene.update()
                t2 = time.perf_counter(); vp.update_scene(); t3 = time.perf_counter()
                if frame >= 2:      # (the first call has no history, the second builds the scratch)
                    call.append(1e3 * (t1 - t0)); update.append(1e3 * (t3 - t2))
            key = "tracked" if track else "untracked"
            out["update_mesh_" + key], out["denoise_temporal_" + key] = stats(update), stats(call)
        vp.track_deformation(False)
        # the pure entries on planes made once: the mesh one step on, its records of a step ago, a one-record table
        d = scene.desc.contents
        triangles = torch.from_numpy(ra.read_mesh(ctx, 0, int(d.meshes[0].numNodes), int(d.meshes[0].numTriangles))[1]).cuda()
        scene.set_mesh_vertices(0, wave(60, args.amplitude)); scene.update(); vp.update_scene()
        vp.reset()
        vp.render(camera, passes=args.passes)
        guide = vp.next_pass_params(camera)
        sums = vp.sum_buffer(secondary=True)
        planes = vp.render_aovs(guide, ("depth", "normal", "position", "base_color", "object_id", "sub_object_id", "barycentrics"), device=True)
        scale = 1.0 / args.passes
        t = dict(color=torch.from_numpy(sums[0]).cuda(), color_half=torch.from_numpy(sums[1]).cuda(), depth=planes["depth"], normal=planes["normal"], position=planes["position"],
                 albedo=planes["base_color"], object_id=planes["object_id"].to(torch.int32))
        first = ra.temporal_accumulate(t["color"], t["color_half"], t["depth"], t["normal"], t["position"], t["albedo"], t["object_id"], color_scale=scale, ctx=ctx)
        t.update(prev_a=first["a"], prev_b=first["b"], prev_length=first["length"], prev_depth=t["depth"], prev_normal=t["normal"], prev_position=t["position"],
                 prev_object_id=t["object_id"])
        outputs = [torch.empty((h, w, 3), dtype=torch.float32, device="cuda"), torch.empty((h, w, 3), dtype=torch.float32, device="cuda"),
                   torch.empty((h, w), dtype=torch.float32, device="cuda"), torch.empty((2, h, w), dtype=torch.float32, device="cuda")]
        p = ra.temporal_params(color_scale=scale, prev_world_to_screen=list(guide.camera.worldToScreen), prev_sample_offset=tuple(guide.sampleOffset))
        pointers = [C.c_void_p(t[name].data_ptr()) for name in NAMES] + [C.c_void_p(o.data_ptr()) for o in outputs]
        n = int(d.numObjects)
        transform = np.array([[d.objects[i].transform[k] for k in range(16)] for i in range(n)], dtype=np.float32).reshape(n, 4, 4)
        rigid = torch.from_numpy(ra.object_motion_table((transform, np.arange(n), np.ones(n))).view(np.int32)).cuda()      # (moved = 1: the matrix is used)
        deformed = torch.from_numpy(ra.object_motion_table((transform, np.arange(n), np.full(n, ra.RT_MOTION_DEFORMED)),
                                                           dict(first_triangle=np.zeros(n), num_triangles=np.full(n, triangles.shape[0]))).view(np.int32)).cuda()
        sub, bary = planes["sub_object_id"].to(torch.int32), planes["barycentrics"]
        block = ra.RtTemporalDeform(sub.data_ptr(), bary.data_ptr(), triangles.data_ptr(), int(triangles.shape[0]), 0)
        handle = C.c_void_p(stream.cuda_stream)
        head = [ctx, C.byref(p), C.c_uint32(w), C.c_uint32(h)] + pointers
        moving = lambda: lib.rtgpu_temporal_accumulate_moving_async(*(head + [C.c_void_p(rigid.data_ptr()), C.c_uint32(n), handle]))   # noqa: E731
        deform = lambda: lib.rtgpu_temporal_accumulate_deform_async(*(head + [C.c_void_p(deformed.data_ptr()), C.c_uint32(n), None, None, C.byref(block), handle]))   # noqa: E731
        assert moving() == 0 and deform() == 0, lib.rtgpu_last_error()
        out["k_temporal_moving"] = time_call(torch, moving, args.reps)
        out["k_temporal_deform"] = time_call(torch, deform, args.reps)
        out["k_temporal_moving_again"] = time_call(torch, moving, args.reps)
        assert deform() == 0
        torch.cuda.synchronize()
        out["history_length_mean_with_the_triangles"] = float(outputs[2].cpu().numpy().mean())


def device_costs(args, ra, lib, ctx, scene, vp, wave, pass_ms, out):
    """--deform --device: the device entry beside the host entry on the same positions, the check alone, the two whole routes, a pass after either"""
    import torch

    def stats(ms):
        return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "spread": float(max(ms) - min(ms))}
    count = len(wave(0, args.amplitude))
    frames = [np.ascontiguousarray(wave(30 + k, args.amplitude)) for k in range(4)]
    tensors = [torch.from_numpy(f).cuda() for f in frames]
    torch.cuda.synchronize()
    # the two entries, call by call on the same positions (the mirror is not told: this part measures the C calls alone, as README's figures do)
    host, device, bytes_host, bytes_device = [], [], 0, 0
    for rep in range(2 + args.reps):
        f, t = frames[rep % 4], tensors[rep % 4]
        u = ra.RtMeshUpdate(3, 0, count, 0, f.ctypes.data_as(C.POINTER(C.c_float)), None)
        t0 = time.perf_counter(); r = lib.rtgpu_update_mesh(ctx, C.byref(u)); t1 = time.perf_counter()
        assert r == 0, lib.rtgpu_last_error()
        bytes_host = ra.update_info(ctx)["bytesUploaded"]
        t2 = time.perf_counter(); r, box = ra.update_mesh_device(ctx, 0, count, t.data_ptr()); t3 = time.perf_counter()
        assert r == 0, lib.rtgpu_last_error()
        bytes_device = ra.update_info(ctx)["bytesUploaded"]
        if rep >= 2:
            host.append(1e3 * (t1 - t0)); device.append(1e3 * (t3 - t2))
    out["entry_host"], out["entry_device"] = dict(stats(host), bytes_uploaded=bytes_host), dict(stats(device), bytes_uploaded=bytes_device)
    out["device_entry_below_host_entry_by_more_than_its_spread"] = bool(out["entry_device"]["ms_median"] < out["entry_host"]["ms_median"] - out["entry_host"]["spread"])
    # the check alone, on a stream of torch's
    stream = torch.cuda.Stream()
    record = torch.empty(8, dtype=torch.int32, device="cuda")
    with torch.cuda.stream(stream):
        check = lambda: ra.refit_check(ctx, 0, tensors[0], C.c_void_p(stream.cuda_stream), record)   # noqa: E731
        assert check() == 0, lib.rtgpu_last_error()
        out["k_refit_check"] = dict(time_call(torch, check, args.reps), bytes_read=int(12 * count + 16 * scene.desc.contents.numTriangles + 36 * scene.desc.contents.numTriangles))
    out["k_refit_check"]["spread"] = out["k_refit_check"]["ms_max"] - out["k_refit_check"]["ms_min"]

    # the two whole routes from a device-resident tensor, in alternating blocks (a host-route call after a device-route call also takes the mesh back, with
    # its normals and tangents: the first calls of a block are not kept)
    def route_host(t):
        scene.set_mesh_vertices(0, t.cpu().numpy()); scene.update(); vp.update_scene()

    def route_device(t):
        vp.update_mesh_device(0, t); scene.update(); vp.update_scene()
    scene.set_mesh_vertices(0, frames[0]); scene.update(); vp.update_scene()      # (the mirror in step with the device again)
    for name, route in (("route_host", route_host), ("route_device", route_device)) * 2:
        ms = []
        for rep in range(2 + args.reps):
            t = tensors[rep % 4]
            t0 = time.perf_counter(); route(t); t1 = time.perf_counter()
            if rep >= 2:
                ms.append(1e3 * (t1 - t0))
        out[name] = stats(ms)
    out["device_route_below_host_route_by_more_than_its_spread"] = bool(out["route_device"]["ms_median"] < out["route_host"]["ms_median"] - out["route_host"]["spread"])
    # a pass on the tables of either route, the same positions
    route_device(tensors[1])
    by_device = pass_ms(vp)
    route_host(tensors[1])
    out["pass_ms_by_route"] = {"device": by_device, "host": pass_ms(vp)}


def deform_main(args):
    import raytracer_amd as ra
    from raytracer_amd import scenes
    w, h = args.width, args.height
    pos, idx, nrm, tan, uv, mat = scenes.sponza_class_mesh(args.triangles, 7, refine=True)
    pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
    extent = float((pos.max(axis=0) - pos.min(axis=0)).max())
    blue_noise = ra.load_blue_noise()

    def wave(frame, amplitude):
        p = pos.astype(np.float64)
        p[:, 1] += amplitude * extent * np.sin(2.0 * math.pi * (p[:, 0] + p[:, 2]) / (0.1 * extent) + 0.4 * frame)
        return p.astype(np.float32)

    def build(positions):
        scene = ra.Scene()
        mats = [scene.add_material("diffuse", c) for _, c in scenes.SPONZA_MATERIALS]
        scene.add_mesh(positions, idx, nrm, tan, uv, mat, mats)
        scene.add_background_light((1.0, 1.5, 2.0))
        if not args.no_sun:
            scene.add_directional_light((20000.0, 19000.0, 18000.0), np.float32(1.0) / np.float32(180.0) * np.float32(3.14159265359),
                                        ra.transform_from_euler((0.0, 0.0, 0.0), scenes.SPONZA_LIGHT_ORIENTATION))
        scene.build()
        scene.desc.contents.blueNoise = blue_noise.ctypes.data
        vp = ra.Viewport(w, h, seed=1234, max_ray_depth=args.depth)
        vp.set_renderer(scene)
        return scene, vp
    camera = ra.Camera((-12.5, 2.2, 0.6), (4.0, 82.0, 0.0), w / h, 65.0)
    scene, vp = build(pos)
    lib, ctx = ra.rtgpu_lib(), vp.device_context()
    vp.render(camera, passes=1)
    assert lib.rtgpu_synchronize(ctx) == 0
    out = {"scene": "sponza_class, deforming", "triangles": int(scene.desc.contents.numTriangles), "vertices": int(len(pos)), "width": w, "height": h,
           "amplitude_share_of_extent": args.amplitude, "extent": extent, "passes_per_frame": args.passes, "frames": args.frames, "sun": not args.no_sun,
           "reference_passes": args.reference_passes, "reps": args.reps}

    def deform_to(frame, amplitude):
        scene.set_mesh_vertices(0, wave(frame, amplitude))
        scene.update()
        vp.update_scene()
    for frame in range(3):
        deform_to(frame, args.amplitude)
    host, device = [], []
    for frame in range(3, 3 + args.reps):
        new = wave(frame, args.amplitude)
        t0 = time.perf_counter(); scene.set_mesh_vertices(0, new); scene.update(); t1 = time.perf_counter(); vp.update_scene(); t2 = time.perf_counter()
        host.append(1e3 * (t1 - t0)); device.append(1e3 * (t2 - t1))
    stats = lambda ms: {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}   # noqa: E731
    out["host_update"], out["update_mesh"] = stats(host), stats(device)
    info = ra.update_info(ctx)
    out["bytes_uploaded"], out["walk"], out["mesh_updates"] = info["bytesUploaded"], info["walk"], info["numMeshUpdates"]

    def pass_ms(viewport):
        context = viewport.device_context()
        viewport.reset(); viewport.render(camera, passes=2); assert lib.rtgpu_synchronize(context) == 0
        ms = []
        for _ in range(3):
            viewport.reset()
            t0 = time.perf_counter(); viewport.render(camera, passes=args.bench_passes); assert lib.rtgpu_synchronize(context) == 0
            ms.append(1e3 * (time.perf_counter() - t0) / args.bench_passes)
        return float(np.median(ms))
    if args.device:
        device_costs(args, ra, lib, ctx, scene, vp, wave, pass_ms, out)
    out["pass_ms"] = {}
    for factor in (1.0, 4.0):
        deform_to(7, factor * args.amplitude)
        refit = pass_ms(vp)
        fresh_scene, fresh_vp = build(wave(7, factor * args.amplitude))
        out["pass_ms"]["amplitude_x%g" % factor] = {"refit_tree": refit, "uploaded_afresh": pass_ms(fresh_vp)}
        del fresh_vp, fresh_scene
    deform_to(0, 0.0)
    out["pass_ms"]["undeformed"] = pass_ms(vp)
    # the upload of the same deformed scene, in the same run (after the timings above: an upload chooses the collapse anew)
    deform_to(7, args.amplitude)
    upload = lambda: lib.rtgpu_upload_scene(ctx, scene.desc)   # noqa: E731
    assert upload() == 0
    out["upload_scene"] = wall(upload, max(3, args.reps // 4))
    out["update_share_of_upload"] = out["update_mesh"]["ms_median"] / out["upload_scene"]["ms_median"]

    # ---- worth: the history kept across the updates against dropped at each (and, with --track, followed through them) ------------------------------------
    def chain(drop_history, amplitude, track=False):
        vp.track_deformation(track)
        vp.reset_history()
        for frame in range(args.frames):
            deform_to(frame, amplitude)
            vp.reset()
            vp.render(camera, passes=args.passes)
            guide = vp.next_pass_params(camera)
            if drop_history:
                vp.reset_history()
            image = vp.denoise(guide, temporal=True, variance=True)
        vp.track_deformation(False)
        return np.asarray(image)

    def worth(amplitude):
        kept = chain(False, amplitude)
        raw = vp.sum_buffer() * np.float32(1.0 / args.passes)
        dropped = chain(True, amplitude)
        tracked = chain(False, amplitude, track=True) if args.track else None
        vp.reset()
        vp.render(camera, passes=args.reference_passes)
        reference = (vp.sum_buffer() / np.float32(args.reference_passes)).astype(np.float64)
        rel_mse = lambda image: float(((image.astype(np.float64) - reference) ** 2 / (reference ** 2 + 0.01)).mean())   # noqa: E731
        figures = {"raw_frame": rel_mse(raw), "history_kept": rel_mse(kept), "history_dropped_at_every_update": rel_mse(dropped)}
        if tracked is not None:
            figures["history_tracked"] = rel_mse(tracked)
        return figures
    out["rel_mse"] = worth(args.amplitude)
    if args.track:
        out["rel_mse_amplitude_x4"] = worth(4.0 * args.amplitude)
        track_costs(args, ra, lib, ctx, scene, vp, camera, wave, out)
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
    ap.add_argument("--step", type=float, default=3.0, help="degrees of orbit per frame")
    ap.add_argument("--reference-passes", type=int, default=512)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--triangles", type=int, default=262144)
    ap.add_argument("--no-sun", action="store_true", help="leave the directional light out: under the sky alone nothing casts a hard shadow that moves with the objects")
    ap.add_argument("--clip", action="store_true", help="add the clipped columns: the same frames with the history clipped, once per gamma")
    ap.add_argument("--clip-gammas", default="1,2,4,8")
    ap.add_argument("--output", default=None)
    ap.add_argument("--deform", action="store_true", help="measure rtgpu_update_mesh instead: the Sponza-class mesh under a travelling sine (see above)")
    ap.add_argument("--amplitude", type=float, default=0.002, help="--deform: the wave's amplitude as a share of the mesh's largest extent")
    ap.add_argument("--bench-passes", type=int, default=16, help="--deform: passes per timing of a pass")
    ap.add_argument("--device", action="store_true", help="--deform: also rtgpu_update_mesh_device on positions that are on the device already, beside rtgpu_update_mesh in the same run")
    ap.add_argument("--track", action="store_true", help="--deform: also with the deformation followed (Viewport.track_deformation), at the amplitude and four times it, and what following costs")
    args = ap.parse_args()
    if args.deform:
        return deform_main(args)
    import torch
    import raytracer_amd as ra
    from raytracer_amd import scenes
    w, h = args.width, args.height
    pos, idx, nrm, tan, uv, mat = scenes.sponza_class_mesh(args.triangles, 7, refine=True)
    scene = ra.Scene()
    mats = [scene.add_material("diffuse", c) for _, c in scenes.SPONZA_MATERIALS]
    scene.add_mesh(pos, idx, nrm, tan, uv, mat, mats)
    orbiters = []      # (object index, phase in degrees, height)

    def pose(k, frame):
        _, phase, lift = orbiters[k]
        a = math.radians(phase + args.step * frame)
        return ra.transform_from_euler((ORBIT_CENTRE[0] + ORBIT_RADIUS * math.cos(a), ORBIT_CENTRE[1] + lift, ORBIT_CENTRE[2] + ORBIT_RADIUS * math.sin(a)),
                                       (0.0, 2.0 * args.step * frame + phase, 0.0))
    red, gold = scene.add_material("diffuse", (0.8, 0.15, 0.1)), scene.add_material("roughMetal", (1.0, 0.7, 0.2), roughness=0.3)
    for phase, lift, add in ((0.0, 0.0, lambda t: scene.add_sphere(0.5, t, red)), (90.0, 0.6, lambda t: scene.add_sphere(0.35, t, gold)),
                             (180.0, -0.4, lambda t: scene.add_box((0.4, 0.6, 0.4), t, red)),
                             (270.0, 0.3, lambda t: scene.add_mesh(*scenes.box_mesh(0.45), materials=[gold, red], transform=t))):
        orbiters.append((scene.object_count(), phase, lift))
        add(pose(len(orbiters) - 1, 0))
    scene.add_background_light((1.0, 1.5, 2.0))
    if not args.no_sun:
        scene.add_directional_light((20000.0, 19000.0, 18000.0), np.float32(1.0) / np.float32(180.0) * np.float32(3.14159265359),
                                    ra.transform_from_euler((0.0, 0.0, 0.0), scenes.SPONZA_LIGHT_ORIENTATION))
    scene.build()
    camera = ra.Camera((-12.5, 2.2, 0.6), (4.0, 82.0, 0.0), w / h, 65.0)
    vp = ra.Viewport(w, h, seed=1234, max_ray_depth=args.depth)
    vp.set_renderer(scene)
    lib, ctx = ra.rtgpu_lib(), vp.device_context()

    def move_to(frame):
        for k, (index, _, _) in enumerate(orbiters):
            scene.set_object_transform(index, pose(k, frame))
        scene.update()
        vp.update_scene()
    vp.render(camera, passes=1)
    assert lib.rtgpu_synchronize(ctx) == 0
    out = {"scene": "sponza_class + %d orbiting objects" % len(orbiters), "triangles": int(scene.desc.contents.numTriangles), "objects": int(scene.desc.contents.numObjects),
           "width": w, "height": h, "passes_per_frame": args.passes, "frames": args.frames, "orbit_deg_per_frame": args.step, "sun": not args.no_sun, "reference_passes": args.reference_passes,
           "reps": args.reps}
    # ---- the update against the upload ---------------------------------------------------------------------------------------------------------------
    counter = [0]

    def advance():
        counter[0] += 1
        for k, (index, _, _) in enumerate(orbiters):
            scene.set_object_transform(index, pose(k, counter[0]))
    for _ in range(3):
        advance(); scene.update(); vp.update_scene()
    host, device = [], []
    for _ in range(args.reps):
        advance()
        t0 = time.perf_counter(); scene.update(); t1 = time.perf_counter(); vp.update_scene(); t2 = time.perf_counter()
        host.append(1e3 * (t1 - t0)); device.append(1e3 * (t2 - t1))
    stats = lambda ms: {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}   # noqa: E731
    out["host_update"], out["update_objects"] = stats(host), stats(device)
    info = ra.update_info(ctx)
    out["bytes_uploaded"], out["walk"], out["top_depth"] = info["bytesUploaded"], info["walk"], info["topDepth"]
    blue_noise = ra.load_blue_noise()                           # (the renderer uploads the scene with the sampler's table: so does this)
    scene.desc.contents.blueNoise = blue_noise.ctypes.data
    upload = lambda: lib.rtgpu_upload_scene(ctx, scene.desc)   # noqa: E731  (the same flat scene; the viewport's renderer already holds it)
    assert upload() == 0
    out["upload_scene"] = wall(upload, max(3, args.reps // 4))
    out["update_share_of_upload"] = out["update_objects"]["ms_median"] / out["upload_scene"]["ms_median"]

    # ---- worth: three ways through the same sixteen frames ---------------------------------------------------------------------------------------------
    names = ("depth", "normal", "position", "base_color", "object_id")
    stream = torch.cuda.Stream()
    scale = np.float32(1.0 / args.passes)
    last = args.frames - 1
    with torch.cuda.stream(stream):
        def chain(drop_history, clip=None):
            vp.reset_history()
            for frame in range(args.frames):
                move_to(frame)
                vp.reset()
                vp.render(camera, passes=args.passes)
                guide = vp.next_pass_params(camera)
                if drop_history:
                    vp.reset_history()
                if clip is None:
                    image = vp.denoise(guide, temporal=True, variance=True, device=True)
                else:
                    image, confidence = vp.denoise(guide, temporal=True, variance=True, device=True, clip=clip, return_confidence=True)
            stream.synchronize()
            return (image.cpu().numpy(), guide) if clip is None else (image.cpu().numpy(), confidence.cpu().numpy())
        followed, guide = chain(False)
        alone = vp.denoise(guide, variance=True, device=True).cpu().numpy()
        raw = vp.sum_buffer() * scale
        planes = vp.render_aovs(guide, names, device=True)
        dropped, _ = chain(True)
        clipped = {}
        if args.clip:
            for gamma in (float(g) for g in args.clip_gammas.split(",")):
                clipped[gamma] = chain(False, clip=dict(radius=3, gamma=gamma, min_count=9))
        # the reference: the scene as it stands now, converged
        vp.reset()
        vp.render(camera, passes=args.reference_passes)
        reference = (vp.sum_buffer() / np.float32(args.reference_passes)).astype(np.float64)
        ids = planes["object_id"].cpu().numpy().reshape(h, w)
        d = scene.desc.contents
        moving_ids = [i for i in range(d.numObjects) if d.objects[i].objectKind == 0 and not (d.objects[i].shapeKind == 3 and d.meshes[d.objects[i].meshIndex].numTriangles > 1000)]
        on_orbiters = np.isin(ids, moving_ids)

        def rel_mse(image, mask=None):
            e = (image.astype(np.float64) - reference) ** 2 / (reference ** 2 + 0.01)
            return float(e.mean() if mask is None else e[mask].mean())
        out["orbiter_pixels"] = int(on_orbiters.sum())
        out["rel_mse"] = {"raw_frame": rel_mse(raw), "a_update_and_temporal": rel_mse(followed), "b_history_dropped_at_every_move": rel_mse(dropped),
                          "c_denoise_var_last_frame_alone": rel_mse(alone)}
        out["rel_mse_on_orbiters"] = {"raw_frame": rel_mse(raw, on_orbiters), "a_update_and_temporal": rel_mse(followed, on_orbiters),
                                      "b_history_dropped_at_every_move": rel_mse(dropped, on_orbiters), "c_denoise_var_last_frame_alone": rel_mse(alone, on_orbiters)}

        for gamma, (image, confidence) in clipped.items():
            key = "d_clipped_gamma_%g" % gamma
            out["rel_mse"][key], out["rel_mse_on_orbiters"][key] = rel_mse(image), rel_mse(image, on_orbiters)
            out.setdefault("clip_confidence", {})[key] = {"share_below_0.5": float((confidence < 0.5).mean()), "share_below_1": float((confidence < 1.0).mean())}

        # ---- the kernel with and without the table: the raw _async entries on tensors made once ----------------------------------------------------------
        vp.reset()
        vp.render(camera, passes=args.passes)
        sums = vp.sum_buffer(secondary=True)
        t = dict(color=torch.from_numpy(sums[0]).cuda(), color_half=torch.from_numpy(sums[1]).cuda(), depth=planes["depth"], normal=planes["normal"], position=planes["position"],
                 albedo=planes["base_color"], object_id=planes["object_id"].to(torch.int32))
        first = ra.temporal_accumulate(t["color"], t["color_half"], t["depth"], t["normal"], t["position"], t["albedo"], t["object_id"], color_scale=float(scale), ctx=ctx)
        t.update(prev_a=first["a"], prev_b=first["b"], prev_length=first["length"], prev_depth=t["depth"], prev_normal=t["normal"], prev_position=t["position"],
                 prev_object_id=t["object_id"])
        outputs = [torch.empty((h, w, 3), dtype=torch.float32, device="cuda"), torch.empty((h, w, 3), dtype=torch.float32, device="cuda"),
                   torch.empty((h, w), dtype=torch.float32, device="cuda"), torch.empty((2, h, w), dtype=torch.float32, device="cuda")]
        p = ra.temporal_params(color_scale=float(scale), prev_world_to_screen=list(guide.camera.worldToScreen), prev_sample_offset=tuple(guide.sampleOffset))
        pointers = [C.c_void_p(t[name].data_ptr()) for name in NAMES] + [C.c_void_p(o.data_ptr()) for o in outputs]
        n = int(d.numObjects)
        # every orbiter "moved" by the step of one frame (a rigid motion about the orbit's axis): the table's matrices are used, the ids stand still
        a = math.radians(args.step)
        turn = np.array([[math.cos(a), 0.0, -math.sin(a), 0.0], [0.0, 1.0, 0.0, 0.0], [math.sin(a), 0.0, math.cos(a), 0.0], [0.0, 0.0, 0.0, 1.0]])
        shift = np.eye(4); shift[3, :3] = ORBIT_CENTRE
        back = np.eye(4); back[3, :3] = [-c for c in ORBIT_CENTRE]
        matrices = np.stack([(back @ turn @ shift) if i in moving_ids else np.eye(4) for i in range(n)]).astype(np.float32)
        table = torch.from_numpy(ra.object_motion_table((matrices, np.arange(n), [1 if i in moving_ids else 0 for i in range(n)])).view(np.int32)).cuda()
        handle = C.c_void_p(stream.cuda_stream)
        static = lambda: lib.rtgpu_temporal_accumulate_async(ctx, C.byref(p), C.c_uint32(w), C.c_uint32(h), *(pointers + [handle]))   # noqa: E731
        moving = lambda: lib.rtgpu_temporal_accumulate_moving_async(ctx, C.byref(p), C.c_uint32(w), C.c_uint32(h), *(pointers + [C.c_void_p(table.data_ptr()), C.c_uint32(n), handle]))   # noqa: E731
        assert static() == 0 and moving() == 0, lib.rtgpu_last_error()
        # interleaved, so that both see the same clocks
        out["k_temporal_static"] = time_call(torch, static, args.reps)
        out["k_temporal_moving"] = time_call(torch, moving, args.reps)
        out["k_temporal_static_again"] = time_call(torch, static, args.reps)
        out["k_temporal_motion_table_ms"] = out["k_temporal_moving"]["ms_median"] - 0.5 * (out["k_temporal_static"]["ms_median"] + out["k_temporal_static_again"]["ms_median"])
        out["history_length_mean_on_orbiters_with_the_table"] = float(outputs[2].cpu().numpy()[on_orbiters].mean()) if on_orbiters.any() else None
    line = json.dumps(out)
    print(line)
    if args.output:
        with open(args.output, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
