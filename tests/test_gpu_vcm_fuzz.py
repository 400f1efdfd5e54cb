"""The bidirectional integrator (renderer "VCM") and the light tracer on the device against the oracle, on the pinned slice of tools/vcm_fuzz_replay.py's case
stream (tests/vcm_fuzz_cases.py; tests/test_vcm_fuzz_cases.py says what the slice covers): random scenes, every BSDF and light type, path lengths 1 ... 16,
both estimators toggled, sampling weights of 0.5 and 0, frames from one pixel up, merge sets of 0, 1 and 2 photons, streamed and synchronised passes.
Leg A (camera_connecting_weight = 0): both sum buffers bit-identical, every compared counter and every synchronised photon count equal.  Leg B (the full image):
counters equal, pixels within the float-atomic bound of tests/test_gpu_vcm.py wherever no pixel receives more than 80 splats.  Then the limits of the settings
through the C ABI and the mirror, and the process-wide knobs DESIGN.md promises not to change any result."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib
import scene_zoo
import raytracer_amd as ra
import vcm_fuzz_cases as pinned

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.parametrize("entry", pinned.CASES, ids=pinned.case_id)
def test_pinned_case_against_the_oracle(built, entry):
    import vcm_fuzz_replay as replay
    same, report = replay.render(pinned.resolve(entry), quiet=True)
    print(pinned.case_id(entry), report)
    assert same, report["problems"]


def test_limits_of_the_settings(built):
    """rtgpu_set_integrator refuses what the device code has no room for (RT_VCM_MAX_PATH_LENGTH, the per-vertex request budget of 64) or what makes no sense
    (radii, multiplier); the mirror hands the refusal on as a failed pass; the largest accepted configuration renders the oracle's frame."""
    import vcm_fuzz_replay as replay
    INVALID, UNSUPPORTED = -1, -6
    lib = ra.rtgpu_lib()
    w, h = 16, 12
    scene, camera = replay.two_estimator_scene(w / h)
    vp = ra.Viewport(w, h, seed=3)
    vp.set_renderer(scene, name="VCM")
    ctx = vp.device_context()

    def status(**settings):
        words = oracle_lib.Vcm(**settings).settings      # the 28 words of RtVcmParams
        return lib.rtgpu_set_integrator(ctx, C.c_uint32(1), words.ctypes.data_as(C.c_void_p))
    refused = (dict(max_path_length=0), dict(max_path_length=17), dict(initial_merging_radius=0.1, min_merging_radius=0.2), dict(merging_radius_multiplier=0.0),
               dict(merging_radius_multiplier=1.5))
    for settings in refused:
        assert status(**settings) == INVALID, settings
    for settings in (dict(max_path_length=1), dict(max_path_length=16), dict(initial_merging_radius=0.2, min_merging_radius=0.2, merging_radius_multiplier=1.0)):
        assert status(**settings) == 0, settings
    for settings in refused:      # the mirror: the setter stores, the pass fails
        vp.set_vcm(**settings)
        with pytest.raises(RuntimeError):
            vp.render_pass_with(vp.next_pass_params(camera))
    # lights + light vertices per camera vertex: 64 fit.  Path length 16 keeps 15 light vertices, so 49 lights are accepted and 50 are not
    case = dict(pinned.resolve("two_streamed_shrinking"), w=w, h=h, passes=3, streamed=False, counting=True)
    case["renderer"] = dict(case["renderer"], vcm=dict(case["renderer"]["vcm"], max_path_length=16))
    many, many_camera = scene_zoo.many_lights_scene(w / h, num_point_lights=47)
    assert many.desc.contents.numLights == 49
    out = replay.accumulate(case, (many, many_camera), True, camera_connecting_weight=0.0)
    assert out["ref"].any() and out["ref_photons"][-1] > 0
    assert replay.leg_a_problems(case, out) == []
    too_many, too_many_camera = scene_zoo.many_lights_scene(w / h, num_point_lights=48)
    assert too_many.desc.contents.numLights == 50
    vp2 = ra.Viewport(w, h, seed=3)
    vp2.set_renderer(too_many, name="VCM")
    vp2.set_vcm(max_path_length=16)
    p = vp2.next_pass_params(too_many_camera)
    with pytest.raises(RuntimeError):
        vp2.render_pass_with(p)
    assert lib.rtgpu_render_pass(vp2.device_context(), C.byref(p)) == UNSUPPORTED      # (the scene is uploaded by now: the status itself, through the C ABI)
    vp2.set_vcm(max_path_length=15)
    vp2.render_pass_with(vp2.next_pass_params(too_many_camera))
    # the light tracer keeps maxRayDepth + 2 counter planes: 18 is the deepest
    vp3 = ra.Viewport(w, h, seed=3, max_ray_depth=19)
    vp3.set_renderer(scene, name="Light Tracer")
    p = vp3.next_pass_params(camera)
    with pytest.raises(RuntimeError):
        vp3.render_pass_with(p)
    assert lib.rtgpu_render_pass(vp3.device_context(), C.byref(p)) == UNSUPPORTED


KNOB_CHILD = r'''
import sys
sys.path.insert(0, "tests"); sys.path.insert(0, "tools")
import vcm_fuzz_cases as pinned, vcm_fuzz_replay as replay
for entry in pinned.KNOB_CASES:
    same, report = replay.render(pinned.resolve(entry), quiet=True, legs="a")
    assert same, (entry, report["problems"])
print("OK")
'''


@pytest.mark.parametrize("knob,value", [("RTGPU_VCM_CLASS", "0"), ("RTGPU_VCM_MERGE_COOP", "1"), ("RTGPU_VCM_MERGE_COOP", "1073741824"), ("RTGPU_VCM_BATCH", "1"),
                                        ("RTGPU_VCM_BATCH", "3"), ("RTGPU_VCM_WIDE", "1")])
def test_results_do_not_depend_on_the_knob(built, knob, value):
    """DESIGN.md's "results do not depend on it" knobs are read once per process, so every setting gets a child process of its own: the generic kernels for
    every scene, every non-empty cell merged cooperatively, none merged cooperatively, one pass per launch sequence, three (11 streamed passes = 3 + 3 + 3 + 2:
    batches whose first merge set comes from the batch before), and the 4-wide walks in front.  Each renders leg A of the three knob cases against the oracle."""
    r = subprocess.run([sys.executable, "-c", KNOB_CHILD], cwd=ROOT, env=dict(os.environ, **{knob: value}), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
