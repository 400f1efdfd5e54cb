#!/usr/bin/env python3
"""The kernel launches of the host launch sequences, in order: the check that a change of the host runtime (raytracer_amd/csrc/rt_runtime_*) launches what
its parent launched.

  rocprofv3 --kernel-trace -d OUT/<case> -o r -- python tools/launch_order.py --case <case>    # one process per case (CASES below)
  python tools/launch_order.py --list OUT                                                      # the launches of every case under OUT

--list prints, per case and per stream (streams in order of first use), every launch as `kernel  grid  block  LDS bytes` in submission order.  Two libraries
launch the same when the two listings are equal; a listing holds no times, so it does not differ from run to run."""
import argparse
import glob
import os
import sqlite3
import sys

# case -> (environment, scene, light sampling all, depth, intersection counters, renderer, what runs)
CASES = {
    "default": ({}, "sponza", False, 3, False, "Path Tracer MIS", "passes"),
    "no_dense": ({"RTGPU_NO_DENSE": "1"}, "sponza", False, 3, False, "Path Tracer MIS", "passes"),
    "binary": ({"RTGPU_WIDE": "0"}, "sponza", False, 3, False, "Path Tracer MIS", "passes"),
    "counters": ({}, "sponza", False, 3, True, "Path Tracer MIS", "passes"),
    "all_lights": ({}, "sponza", True, 3, False, "Path Tracer MIS", "passes"),
    "cornell": ({}, "cornell", False, 3, False, "Path Tracer MIS", "passes"),
    "tail": ({}, "sponza", False, 6, False, "Path Tracer MIS", "passes"),
    "vcm": ({}, "sponza", False, 3, False, "VCM", "passes"),
    "vcm_wide": ({"RTGPU_VCM_WIDE": "1"}, "sponza", False, 3, False, "VCM", "passes"),
    "query_closest": ({}, "sponza", False, 3, False, "Path Tracer MIS", "closest"),
    "query_any": ({}, "sponza", False, 3, False, "Path Tracer MIS", "any"),
    "aov_cost": ({}, "sponza", False, 3, False, "Path Tracer MIS", "aov_cost"),
    "aov": ({}, "sponza", False, 3, False, "Path Tracer MIS", "aov"),
    "record": ({}, "sponza", False, 3, False, "Path Tracer MIS", "record"),
}


def run_case(name):
    env, scene_name, sampling_all, depth, counting, renderer, what = CASES[name]
    os.environ.update(env)   # before the library loads: some knobs are read once per process
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import raytracer_amd as ra
    from raytracer_amd import scenes
    w, h = (64, 48) if scene_name == "cornell" else (96, 54)
    scene, camera = scenes.cornell_box(w / h) if scene_name == "cornell" else scenes.sponza_class(w / h, 6000)
    vp = ra.Viewport(w, h, seed=1234, max_ray_depth=depth, light_sampling_all=sampling_all, dimensions=128 if sampling_all else 64)
    vp.set_renderer(scene, name=renderer, intersection_counters=counting)
    if renderer == "VCM":
        vp.set_vcm(max_path_length=4)
    if what == "passes":
        vp.render(camera, 2)
        print(name, "mean", float(vp.sum_buffer().mean()))
        return
    p = vp.next_pass_params(camera)
    if what in ("closest", "any"):
        rng = np.random.default_rng(7)
        origins = np.tile(np.asarray((-12.5, 2.2, 0.6), np.float32), (4096, 1))   # (inside the hall)
        directions = rng.normal(size=(4096, 3)).astype(np.float32)
        out = vp.trace_rays(origins, directions) if what == "closest" else vp.occluded(origins, directions, max_distance=5.0)
        print(name, "answers", len(out.distance if what == "closest" else out))
    elif what in ("aov", "aov_cost"):
        out = vp.render_aovs(p, planes=("depth", "normal") + (("box_tests",) if what == "aov_cost" else ()))
        print(name, "planes", sorted(out))
    else:
        print(name, "paths", len(vp.record_paths(p, [(x, y) for y in range(h) for x in range(w)])))


def list_launches(out):
    for name in CASES:
        dbs = sorted(glob.glob(os.path.join(out, name, "**", "*.db"), recursive=True))
        print("== %s%s" % (name, "" if dbs else ": no trace"))
        for db in dbs:
            rows = sqlite3.connect(db).execute("select stream_id, queue_id, name, grid_x, grid_y, grid_z, workgroup_x, workgroup_y, workgroup_z, lds_size "
                                               "from kernels order by dispatch_id").fetchall()
            streams = {}
            for r in rows:
                streams.setdefault((r[0], r[1]), []).append(r[2:])
            for k, launches in enumerate(streams.values()):   # (a dict keeps the order of first use)
                print("-- stream %d: %d launches" % (k, len(launches)))
                for kernel, gx, gy, gz, bx, by, bz, lds in launches:
                    print("%s  grid %d,%d,%d  block %d,%d,%d  lds %d" % (kernel.split("(")[0], gx, gy, gz, bx, by, bz, lds))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--list", metavar="OUT")
    args = ap.parse_args()
    if args.case:
        run_case(args.case)
    if args.list:
        list_launches(args.list)
