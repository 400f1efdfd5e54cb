"""The record layout of the dense path-state arenas (raytracer_amd/csrc/rt_dense.inl, rt_device_state.h): the home index packed with the
pending-request count in R_SAMPLER.w, R_SH_TP carried only while a request is pending, any-hit origins read from R_ORIGIN (zombies
store their shading point there), the occlusion verdict in the contribution record.

Bar: as tests/test_gpu_parity.py -- BIT-EXACT sum buffers and IDENTICAL ray counters against the CPU oracle.  Every case renders a
small frame; a scene's oracle image is computed once and shared by the launch-sequence variants of that scene.  The fused tail is switched
on through rtgpu_set_schedule, per context."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import raytracer_amd as ra
from raytracer_amd import scenes
import test_gpu_parity as parity

pytestmark = pytest.mark.gpu

# launch-sequence variants: dense arenas, slot-per-pixel state (the first layout, R_SH_P and all), the fused tail from bounce 1 (in-place arena)
VARIANTS = ("dense", "slot-per-pixel", "tail-from-1")


def viewport(scene, w, h, variant, monkeypatch, seed, **vp_args):
    monkeypatch.setenv("RTGPU_NO_DENSE", "1" if variant == "slot-per-pixel" else "0")
    vp = ra.Viewport(w, h, seed=seed, **vp_args)
    vp.set_renderer(scene)
    lib = ra.rtgpu_lib()
    assert lib.rtgpu_set_intersection_counters(vp.device_context(), 0) == 0
    assert lib.rtgpu_set_schedule(vp.device_context(), C.c_uint32(0), C.c_int32(1 if variant == "tail-from-1" else 0)) == 0
    return vp


def check_variants(scene, camera, w, h, passes, monkeypatch, variants=VARIANTS, seed=515, env=(), **vp_args):
    """Renders `passes` passes per variant with the same per-pass constants (same seed); the first variant's passes also go through the
    oracle.  Returns the oracle's counters."""
    desc = scene.desc
    bn = ra.load_blue_noise()
    desc.contents.blueNoise = bn.ctypes.data
    for name, value in env:
        monkeypatch.setenv(name, value)
    reference = None
    for variant in variants:
        vp = viewport(scene, w, h, variant, monkeypatch, seed, **vp_args)
        if reference is None:
            ref = np.zeros((h, w, 3), dtype=np.float32); ref2 = np.zeros((h, w, 3), dtype=np.float32)
            cnt = np.zeros(16, dtype=np.uint64)
            for _ in range(passes):
                p = vp.next_pass_params(camera)
                vp.render_pass_with(p)
                oracle_lib.render_pass(desc, p, w, h, ref, ref2, cnt, threads=8)
            reference = (ref, ref2, {n: int(cnt[i]) for i, n in enumerate(ra.COUNTER_NAMES)})
        else:
            vp.render(camera, passes)
        img, img2 = vp.sum_buffer(secondary=True)
        parity.assert_quant_identical(img, img2, vp.counters(), *reference)
    return reference[2]


_small_sponza = {}


def small_sponza(aspect):
    """A few hundred triangles of the benchmark's scene class: one mesh, background + directional light (two lights under `Single`)."""
    if aspect not in _small_sponza:
        _small_sponza[aspect] = scenes.sponza_class(aspect, 600)
    return _small_sponza[aspect]


@pytest.mark.parametrize("depth", [1, 2])
def test_zombies_everywhere(built, monkeypatch, depth):
    """max_ray_depth 1 and 2: most paths end with their last next-event request still pending, i.e. as zombies whose any-hit ray starts at
    the point they stored into R_ORIGIN.  67 x 45: odd rows, a partial last block."""
    w, h = 67, 45
    scene, camera = small_sponza(w / h)
    counters = check_variants(scene, camera, w, h, 3, monkeypatch, max_ray_depth=depth)
    assert counters["numShadowRays"] > w * h and 0 < counters["numShadowRaysHit"] < counters["numShadowRays"]


def test_frame_smaller_than_one_block(built, monkeypatch):
    """8 x 8 pixels: fewer vertices than one block of k_shade_dense at every bounce, depth 8."""
    w, h = 8, 8
    scene, camera = small_sponza(w / h)
    counters = check_variants(scene, camera, w, h, 3, monkeypatch, max_ray_depth=8)
    assert counters["numShadowRays"] > 0


def inward_box(half):
    """box_mesh with the faces turned inwards: a closed room"""
    mb = scenes.MeshBuilder()
    h = half
    faces = [((-h, -h, h), (2 * h, 0, 0), (0, 2 * h, 0)), ((h, -h, -h), (-2 * h, 0, 0), (0, 2 * h, 0)),
             ((h, -h, h), (0, 0, -2 * h), (0, 2 * h, 0)), ((-h, -h, -h), (0, 0, 2 * h), (0, 2 * h, 0)),
             ((-h, h, h), (2 * h, 0, 0), (0, 0, -2 * h)), ((-h, -h, -h), (2 * h, 0, 0), (0, 0, 2 * h))]
    for f, (o, eu, ev) in enumerate(faces):
        mb.add_grid(np.asarray(o) + np.asarray(eu), -np.asarray(eu, dtype=np.float64), ev, 2, 2, f % 2)
    return mb.arrays()


SUN = ra.transform_from_euler((0.0, 0.0, 0.0), (70.0, 20.0, 0.0))


def closed_room(aspect, with_sphere):
    """Every next-event ray is occluded: the camera sits in a closed box, the only light is a directional light outside.  `with_sphere`: an
    analytic sphere in the room makes the scene two-level (k_trace_wide2 or the binary walk)."""
    pos, idx, nrm, tan, uv, mat = inward_box(3.0)
    scene = ra.Scene()
    scene.add_mesh(pos, idx, nrm, tan, uv, mat, [scene.add_material("diffuse", (0.8, 0.3, 0.2)), scene.add_material("diffuse", (0.3, 0.8, 0.2))])
    if with_sphere:
        scene.add_sphere(0.5, ra.transform_from_euler((0.5, -1.0, -1.5)), scene.add_material("diffuse", (0.7, 0.7, 0.7)))
    scene.add_directional_light((5.0, 5.0, 5.0), 0.02, SUN)
    scene.build()
    return scene, ra.Camera((0.0, 0.0, 2.0), (10.0, 180.0, 0.0), aspect, 60.0)


def open_ground(aspect):
    """No next-event ray is occluded: one ground quad under a background light and a directional light."""
    mb = scenes.MeshBuilder()
    mb.add_grid((-20.0, 0.0, 20.0), (40.0, 0.0, 0.0), (0.0, 0.0, -40.0), 3, 3, 0)   # normal = +y
    pos, idx, nrm, tan, uv, mat = mb.arrays()
    scene = ra.Scene()
    scene.add_mesh(pos, idx, nrm, tan, uv, mat, [scene.add_material("diffuse", (0.6, 0.6, 0.5))])
    scene.add_background_light((1.0, 1.5, 2.0))
    scene.add_directional_light((5.0, 5.0, 5.0), 0.02, SUN)
    scene.build()
    return scene, ra.Camera((0.0, 2.0, 6.0), (25.0, 180.0, 0.0), aspect, 50.0)


@pytest.mark.parametrize("case", ["occluded-wide", "occluded-binary", "occluded-wide2", "occluded-two-level-binary", "open-wide", "open-binary"])
def test_verdict_extremes(built, monkeypatch, case):
    """All next-event rays occluded / none occluded, through the 4-wide walk, the two-level 4-wide walk and the reference's binary walk, each
    with the dense arenas, the first layout and (single mesh, 4-wide walk) the fused tail."""
    w, h = 67, 45
    occluded = case.startswith("occluded")
    scene, camera = closed_room(w / h, "wide2" in case or "two-level" in case) if occluded else open_ground(w / h)
    wide = case.endswith("wide") or case.endswith("wide2")
    env = (("RTGPU_WIDE", "1" if wide else "0"), ("RTGPU_WIDE2", "1" if wide else "0"))
    variants = VARIANTS if case.endswith("-wide") else VARIANTS[:2]   # (the tail runs behind the single-mesh 4-wide walk only)
    counters = check_variants(scene, camera, w, h, 2, monkeypatch, variants=variants, env=env, max_ray_depth=3)
    assert counters["numShadowRays"] > w * h
    if occluded:
        assert counters["numShadowRaysHit"] == 0
    else:
        # (the ground is convex, so nothing can shadow it; a ray that leaves it at a grazing angle may still meet it again within rounding: one in 5494 does)
        assert counters["numShadowRaysHit"] >= 0.99 * counters["numShadowRays"]


def test_seven_lights_under_all(built, monkeypatch):
    """LightSamplingStrategy::All with RT_DENSE_MAX_LIGHTS = 7 lights: the largest request count the packed field holds.  Narrow spot
    lights need no ray at most vertices: requests created without a ray, marked as the walks mark an occluded one."""
    w, h = 64, 48
    pos, idx, nrm, tan, uv, mat = scenes.sponza_class_mesh(600, 7, refine=True)
    scene = ra.Scene()
    scene.add_mesh(pos, idx, nrm, tan, uv, mat, [scene.add_material("diffuse", c) for _, c in scenes.SPONZA_MATERIALS])
    scene.add_background_light((1.0, 1.5, 2.0))
    scene.add_directional_light((20.0, 19.0, 18.0), 0.02, SUN)
    scene.add_point_light((30.0, 20.0, 10.0), ra.transform_from_euler((-8.0, 3.0, 0.5)))
    scene.add_point_light((10.0, 20.0, 30.0), ra.transform_from_euler((-4.0, 1.5, -0.5)))
    for k, angle in enumerate((0.08, 0.15, 0.3)):
        scene.add_spot_light((200.0, 150.0 + 50.0 * k, 100.0), angle, ra.transform_from_euler((-10.0 + 2.0 * k, 4.0, 0.6), (80.0, 30.0 * k, 0.0)))
    scene.build()
    camera = ra.Camera((-12.5, 2.2, 0.6), (4.0, 82.0, 0.0), w / h, 65.0)
    counters = check_variants(scene, camera, w, h, 2, monkeypatch, variants=VARIANTS[:2], max_ray_depth=4, light_sampling_all=True, dimensions=128)
    assert counters["numShadowRays"] > 2 * w * h and counters["numShadowRaysHit"] > 0


@pytest.mark.parametrize("batch", ["1", "5"])
def test_home_indices_across_pass_batches(built, monkeypatch, batch):
    """RTGPU_PASS_BATCH 1 and 5 on the zombie scene: with five passes in one batch the home indices reach five times the pixel count."""
    w, h = 67, 45
    scene, camera = small_sponza(w / h)
    check_variants(scene, camera, w, h, 5, monkeypatch, variants=("dense", "tail-from-1"), env=(("RTGPU_PASS_BATCH", batch),), max_ray_depth=2)
