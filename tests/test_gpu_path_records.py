"""Path records on the device (rtgpu_record_paths, Viewport.record_paths) -- the reference's PathDebugData hook -- against the oracle's recording of the
same pass (oracle_lib.render_pixel_paths, which tests/test_reference_paths.py holds to the reference's own recordings vertex by vertex).

Bar: the same vertex count and every word of every vertex BIT-EQUAL, except the fields the reference leaves as an earlier vertex wrote them, where
the device writes zero (path_records_ref.stale_mask: exactly the list in include/rtgpu.h); radiance bit-equal to the oracle's pixel and to the
rendered pass.  Both sides evaluate the reference's arithmetic in its order with IEEE operations: there is no tolerance to state."""
import ctypes as C
import time

import numpy as np
import pytest

import oracle_lib
import path_records_ref as ref
import raytracer_amd as ra
from raytracer_amd import scenes

pytestmark = pytest.mark.gpu

HIT_BACKGROUND, HIT_LIGHT, DEPTH, THROUGHPUT, NO_SAMPLED_EVENT, RUSSIAN_ROULETTE = 1, 2, 3, 4, 5, 6
OK, INVALID_ARGUMENT, NOT_READY, UNSUPPORTED = 0, -1, -5, -6


def viewport(name, walk, **kwargs):
    scene, camera, w, h, args = ref.fixture(name)
    vp = ra.Viewport(w, h, **args)
    vp.set_renderer(scene, intersection_counters=(walk == "counting"), **kwargs)
    return vp, scene, camera, w, h


def same_words(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def assert_same_records(a, b):
    assert len(a) == len(b)
    for (va, ra_, ca), (vb, rb, cb) in zip(a, b):
        assert va.shape == vb.shape and same_words(va, vb) and ra_ == rb and same_words(ca, cb)


def reason_agrees_with_last_record(vertices, reason):
    last = vertices[-1, 6:8].view(np.uint32)
    return (reason == HIT_BACKGROUND) == (last[0] == ref.INVALID_OBJECT) and (reason == HIT_LIGHT) == (last[0] != ref.INVALID_OBJECT and last[1] == ref.LIGHT_OBJECT)


# ---- 1. device against oracle --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.FIXTURE_NAMES)
def test_device_records_equal_the_oracles(built, walk, name):
    vp, scene, _, w, h = viewport(name, walk)
    p = ref.first_pass_params(name)
    expected = ref.oracle_frame(name)
    t0 = time.perf_counter()
    got = vp.record_paths(p, ref.all_pixels(w, h))
    print("%s [%s]: whole-frame record_paths call, %d pixels: %.1f ms" % (name, walk, w * h, 1e3 * (time.perf_counter() - t0)))
    assert len(got) == len(expected) == w * h
    desc = scene.desc.contents
    compared = masked = 0
    for i, ((v, reason, radiance), (ov, oradiance)) in enumerate(zip(got, expected)):
        where = "pixel (%d, %d)" % (i % w, i // w)
        assert len(v) == len(ov), "%s: %d vertices, the oracle has %d" % (where, len(v), len(ov))
        mask = ref.stale_mask(ov, desc)
        differs = (v.view(np.uint32) != ov.view(np.uint32)) & ~mask
        assert not differs.any(), "%s: vertex %d word %d differs: %r, the oracle has %r" % (
            (where,) + tuple(int(k) for k in np.argwhere(differs)[0]) + (v[differs][0], ov[differs][0]))
        assert not v[mask].view(np.uint32).any(), "%s: a stale field is not zero" % where
        assert same_words(radiance, oradiance), "%s: radiance %r, the oracle's pixel is %r" % (where, radiance, oradiance)
        assert 1 <= reason <= 6 and reason_agrees_with_last_record(v, reason), "%s: reason %d" % (where, reason)
        compared += v.size
        masked += int(mask.sum())
    assert masked * 2 < compared, "the mask covers %d of %d words" % (masked, compared)


@pytest.mark.parametrize("name", ["sponza_class", "cornell_box"])
def test_device_records_equal_the_oracles_on_the_binary_walk_without_counters(built, monkeypatch, name):
    """RTGPU_WIDE=0 / RTGPU_WIDE2=0 with the intersection counters off: the recorder's trace steps take the reference's binary walk (k_trace) without the
    counting code -- the one walk the `walk` cases above do not reach (they take the 4-wide walks or the counting k_trace).  Two passes, every pixel, depth 3;
    the bar of the test above."""
    monkeypatch.setenv("RTGPU_WIDE", "0")
    monkeypatch.setenv("RTGPU_WIDE2", "0")
    w, h = (96, 54) if name == "sponza_class" else (64, 48)
    scene, camera = scenes.sponza_class(w / h, 6000) if name == "sponza_class" else scenes.cornell_box(w / h)
    bn = ra.load_blue_noise()
    scene.desc.contents.blueNoise = bn.ctypes.data
    vp = ra.Viewport(w, h, seed=4242, max_ray_depth=3)
    vp.set_renderer(scene)
    desc = scene.desc.contents
    pixels = ref.all_pixels(w, h)
    for _ in range(2):
        p = vp.next_pass_params(camera)
        got = vp.record_paths(p, pixels)
        assert len(got) == w * h
        for (x, y), (v, reason, radiance) in zip(pixels, got):
            ov = oracle_lib.render_pixel_paths(scene.desc, p, w, h, x, y, capacity=5)
            assert len(v) == len(ov), "pixel (%d, %d): %d vertices, the oracle has %d" % (x, y, len(v), len(ov))
            mask = ref.stale_mask(ov, desc)
            assert not ((v.view(np.uint32) != ov.view(np.uint32)) & ~mask).any(), "pixel (%d, %d): a record differs from the oracle's" % (x, y)
            assert not v[mask].view(np.uint32).any(), "pixel (%d, %d): a stale field is not zero" % (x, y)
            assert same_words(radiance, oracle_lib.render_pixel(scene.desc, p, w, h, x, y)[:3]), "pixel (%d, %d): radiance" % (x, y)
            assert 1 <= reason <= 6 and reason_agrees_with_last_record(v, reason), "pixel (%d, %d): reason %d" % (x, y, reason)


# ---- 2. recording against rendering --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "mesh_single"])
def test_recorded_radiance_is_the_rendered_pass(built, walk, name):
    """the slot-layout recorder against the default pipeline (dense path state, batches): one pass, the same params"""
    vp, _, camera, w, h = viewport(name, walk)
    vp.reset()
    p = vp.next_pass_params(camera)
    vp.render_pass_with(p)
    image = vp.sum_buffer()
    got = vp.record_paths(p, ref.all_pixels(w, h))
    radiance = np.array([c for _, _, c in got], dtype=np.float32).reshape(h, w, 3)
    nbad = int(np.count_nonzero(radiance.view(np.uint32) != image.view(np.uint32)))
    assert nbad == 0, "%d of %d channel words differ from the one-pass sum buffer" % (nbad, image.size)


# ---- 3. isolation --------------------------------------------------------------------------------------------------------------------------
def test_a_recording_leaves_the_render_state_alone(built, walk):
    def four_passes(record):
        vp, _, camera, w, h = viewport("cornell", walk)
        recorded = None
        for k in range(4):
            p = vp.next_pass_params(camera)
            if record and k == 2:
                before = vp.passes_finished
                recorded = vp.record_paths(p, [(5, 7), (40, 20), (5, 7)])   # between the 2nd and the 3rd pass, while they are still queued
                assert vp.passes_finished == before
            vp.render_pass_with(p)
        s, s2 = vp.sum_buffer(secondary=True)
        raw = ra.RtCounters()
        assert ra.rtgpu_lib().rtgpu_get_counters(vp.device_context(), C.byref(raw)) == 0
        return s, s2, vp.counters(), bytes(raw), vp.passes_finished, recorded
    plain, with_recording = four_passes(False), four_passes(True)
    assert same_words(plain[0], with_recording[0]) and same_words(plain[1], with_recording[1])
    assert plain[2] == with_recording[2] and plain[3] == with_recording[3]
    assert plain[4] == with_recording[4] == 4
    assert_same_records(with_recording[5][0:1], with_recording[5][2:3])   # a pixel that repeats in the list


def test_one_pixel_equals_its_entry_of_the_whole_frame(built, walk):
    """the schedule-independence the feature rests on"""
    vp, _, _, w, h = viewport("mesh_single", walk)
    p = ref.first_pass_params("mesh_single")
    frame = vp.record_paths(p, ref.all_pixels(w, h))
    for x, y in ((0, 0), (w - 1, h - 1), (17, 23), (40, 11)):
        assert_same_records(vp.record_paths(p, [(x, y)]), frame[y * w + x:y * w + x + 1])


# ---- 4. truncation -------------------------------------------------------------------------------------------------------------------------
def test_truncation_keeps_the_count_and_the_buffer_beyond(built, walk):
    vp, _, _, w, h = viewport("cornell", walk)
    p = ref.first_pass_params("cornell")
    pixels = ref.all_pixels(w, h)
    full = vp.record_paths(p, pixels)
    assert max(len(v) for v, _, _ in full) > 2 and min(len(v) for v, _, _ in full) < 2
    n = len(pixels)
    guard = np.float32(-77.25)
    vertices = np.full(n * 2 * 28 + 1, guard, dtype=np.float32)   # maxVertices = 2, and one word behind the last pixel's two records
    infos = np.zeros((n, 8), dtype=np.uint32)
    xy = np.array(pixels, dtype=np.uint32)
    r = ra.rtgpu_lib().rtgpu_record_paths(vp.device_context(), C.byref(p), xy.ctypes.data_as(C.c_void_p), C.c_uint32(n), C.c_uint32(2),
                                          vertices.ctypes.data_as(C.c_void_p), infos.ctypes.data_as(C.c_void_p))
    assert r == OK, ra.rtgpu_lib().rtgpu_last_error()
    assert vertices[-1] == guard
    stored = vertices[:-1].reshape(n, 2, 28)
    for i, (v, reason, radiance) in enumerate(full):
        assert infos[i, 0] == len(v) and infos[i, 1] == reason and same_words(infos[i, 2:5], radiance)
        k = min(len(v), 2)
        assert same_words(stored[i, :k], v[:k])
        assert (stored[i, k:] == guard).all()   # records the path does not have are not written


# ---- 5. termination reasons on built scenes ------------------------------------------------------------------------------------------------
def reasons_scene(floor_bsdf="diffuse", floor_color=(0.7, 0.7, 0.7), box_color=None, light=False, camera=((0.0, 2.0, 6.0), (40.0, 180.0, 0.0))):
    s = ra.Scene()
    floor = s.add_material(floor_bsdf, floor_color)
    s.add_rect((8.0, 8.0), ra.transform_from_euler((0.0, -2.0, 0.0), (-90.0, 0.0, 0.0)), floor)
    s.add_sphere(0.8, ra.transform_from_euler((-2.0, -1.2, 0.0)), floor)
    if box_color is not None:
        s.add_box((1.0, 1.0, 1.0), ra.transform_from_euler((1.0, -0.5, 0.0), (0.0, 30.0, 0.0)), s.add_material("diffuse", box_color))
    if light:
        s.add_area_light("rect", [1.0, 1.0], (12.0, 11.0, 10.0), ra.transform_from_euler((0.0, 4.0, 0.0), (90.0, 0.0, 0.0)))
    s.add_background_light((1.0, 1.5, 2.0))
    s.build()
    return s, ra.Camera(camera[0], camera[1], 1.0, 50.0)


def record_reasons(walk, scene, camera, **vp_args):
    vp = ra.Viewport(16, 16, seed=7, **vp_args)
    vp.set_renderer(scene, intersection_counters=(walk == "counting"))
    p = vp.next_pass_params(camera)
    got = vp.record_paths(p, ref.all_pixels(16, 16))
    for v, reason, _ in got:
        assert 1 <= reason <= 6 and reason_agrees_with_last_record(v, reason)
    surface = [(v, reason) for v, reason, _ in got if reason not in (HIT_BACKGROUND, HIT_LIGHT)]
    return got, surface, int(p.maxRayDepth)


def test_reason_depth(built, walk):
    scene, camera = reasons_scene()
    got, surface, _ = record_reasons(walk, scene, camera, max_ray_depth=0)
    assert surface and all(reason == DEPTH and len(v) == 1 for v, reason in surface)
    assert all(len(v) == 1 for v, _, _ in got)


def test_reason_hit_background(built, walk):
    scene, camera = reasons_scene(camera=((0.0, 2.0, 6.0), (-60.0, 180.0, 0.0)))   # looking at the sky
    got, surface, _ = record_reasons(walk, scene, camera, max_ray_depth=4)
    assert not surface and all(reason == HIT_BACKGROUND and len(v) == 1 for v, reason, _ in got)


def test_reason_hit_light(built, walk):
    scene, camera = reasons_scene(light=True, camera=((0.0, 0.0, 0.0), (-90.0, 180.0, 0.0)))   # below the rect light, looking straight up at it
    got, _, _ = record_reasons(walk, scene, camera, max_ray_depth=4)
    first_hit_light = [reason for v, reason, _ in got if len(v) == 1 and v[0, 7:8].view(np.uint32)[0] == ref.LIGHT_OBJECT]
    assert first_hit_light and all(reason == HIT_LIGHT for reason in first_hit_light)
    assert any(reason == HIT_BACKGROUND for _, reason, _ in got)   # the light does not fill the view


def test_reason_no_sampled_event(built, walk):
    scene, camera = reasons_scene(floor_bsdf="null")
    _, surface, _ = record_reasons(walk, scene, camera, max_ray_depth=4, min_russian_roulette_depth=10)
    assert surface and all(reason == NO_SAMPLED_EVENT and len(v) == 1 for v, reason in surface)


def test_reason_throughput(built, walk):
    scene, camera = reasons_scene(floor_color=(0.0, 0.0, 0.0))   # black: the sampled BSDF value takes the throughput to zero
    _, surface, _ = record_reasons(walk, scene, camera, max_ray_depth=4, min_russian_roulette_depth=10)   # Russian roulette out of reach
    assert surface and all(reason == THROUGHPUT and len(v) == 1 for v, reason in surface)


def test_reason_russian_roulette(built, walk):
    scene, camera = reasons_scene(floor_color=(0.15, 0.15, 0.15), box_color=(0.1, 0.12, 0.1))
    _, surface, depth = record_reasons(walk, scene, camera, max_ray_depth=8, min_russian_roulette_depth=0)
    below_limit = [reason for v, reason in surface if len(v) <= depth]   # a path that ends at the limit has depth + 1 vertices
    assert below_limit and all(reason == RUSSIAN_ROULETTE for reason in below_limit)
    assert all(reason == DEPTH for v, reason in surface if len(v) == depth + 1)


# ---- 6. errors -----------------------------------------------------------------------------------------------------------------------------
def raw_call(ctx, p, pixels, max_vertices=4, vertices=True, infos=True, count=None):
    xy = np.array(pixels, dtype=np.uint32).reshape(-1, 2)
    n = len(xy) if count is None else count
    v = np.zeros((max(len(xy), 1), max(max_vertices, 1), 28), dtype=np.float32)
    info = np.zeros((max(len(xy), 1), 8), dtype=np.uint32)
    return ra.rtgpu_lib().rtgpu_record_paths(ctx, C.byref(p) if p is not None else None, xy.ctypes.data_as(C.c_void_p) if len(xy) else None, C.c_uint32(n),
                                             C.c_uint32(max_vertices), v.ctypes.data_as(C.c_void_p) if vertices else None, info.ctypes.data_as(C.c_void_p) if infos else None)


def changed(p, **fields):
    q = ra.RtPassParams.from_buffer_copy(p)
    q._seed_keepalive = p._seed_keepalive
    for k, v in fields.items():
        setattr(q, k, v)
    return q


def test_errors(built):
    lib = ra.rtgpu_lib()
    scene, camera, w, h, args = ref.fixture("cornell")
    p = ref.first_pass_params("cornell")
    # before rtgpu_upload_scene, then before rtgpu_resize
    ctx = C.c_void_p()
    assert lib.rtgpu_create(0, C.byref(ctx)) == OK
    try:
        assert raw_call(ctx, p, [(0, 0)]) == NOT_READY
        assert lib.rtgpu_upload_scene(ctx, scene.desc) == OK
        assert raw_call(ctx, p, [(0, 0)]) == NOT_READY
        assert raw_call(ctx, p, [], count=0) == OK   # nothing to do
    finally:
        lib.rtgpu_destroy(ctx)

    vp = ra.Viewport(w, h, **args)
    vp.set_renderer(scene)
    ctx = vp.device_context()
    assert len(vp.record_paths(p, [(0, 0)])) == 1   # (the renderer uploads its scene on first use: the wrapper sees to it)
    assert raw_call(ctx, p, [(0, 0)]) == OK
    assert raw_call(ctx, p, [], count=0) == OK and raw_call(ctx, p, [], count=0, vertices=False, infos=False) == OK
    assert raw_call(ctx, None, [(0, 0)]) == INVALID_ARGUMENT
    assert raw_call(ctx, p, [(0, 0)], vertices=False) == INVALID_ARGUMENT and raw_call(ctx, p, [(0, 0)], infos=False) == INVALID_ARGUMENT
    assert raw_call(ctx, p, [], count=1) == INVALID_ARGUMENT   # no pixel list
    assert raw_call(ctx, p, [(w, 0)]) == INVALID_ARGUMENT and raw_call(ctx, p, [(0, 0), (0, h)]) == INVALID_ARGUMENT
    assert b"outside the frame" in lib.rtgpu_last_error()
    assert raw_call(ctx, p, [(0, 0)], max_vertices=0) == INVALID_ARGUMENT
    # what rtgpu_render_pass refuses in the params
    assert raw_call(ctx, changed(p, numDimensions=4097), [(0, 0)]) == INVALID_ARGUMENT
    assert raw_call(ctx, changed(p, seed=C.POINTER(C.c_uint32)()), [(0, 0)]) == INVALID_ARGUMENT
    assert raw_call(ctx, changed(p, maxRayDepth=255), [(0, 0)]) == INVALID_ARGUMENT
    bokeh = changed(p)
    bokeh.camera.dofEnable, bokeh.camera.bokehShape = 1, 3
    assert raw_call(ctx, bokeh, [(0, 0)]) == lib.rtgpu_render_pass(ctx, C.byref(bokeh)) == UNSUPPORTED
    with pytest.raises(ValueError):
        vp.record_paths(changed(p, maxRayDepth=255), [(0, 0)])
    # every integrator but PathTracerMIS
    for integrator in (2, 3, 4, 1):   # Path Tracer, Debug, Light Tracer, VCM
        assert lib.rtgpu_set_integrator(ctx, C.c_uint32(integrator), None) == OK
        assert raw_call(ctx, p, [(0, 0)]) == UNSUPPORTED
    assert lib.rtgpu_set_integrator(ctx, C.c_uint32(0), None) == OK
    assert raw_call(ctx, p, [(0, 0)]) == OK


def test_a_vcm_renderer_is_refused(built):
    scene, camera = scenes.sphere_area_light(1.0)
    vp = ra.Viewport(16, 16, seed=3, max_ray_depth=3)
    vp.set_renderer(scene, name="VCM")
    p = vp.next_pass_params(camera)
    vp.render_pass_with(p)   # (the renderer selects its integrator with its first pass)
    with pytest.raises(RuntimeError, match="-6"):
        vp.record_paths(p, [(3, 4)])


def test_a_multi_device_context_answers_like_a_single_one(built):
    """one device index, repeated: two shards, and the call is not restricted to the first one's tiles"""
    name = "box_mesh"
    single, _, _, w, h = viewport(name, "default")
    multi, _, _, _, _ = viewport(name, "default", devices=[0, 0])
    p = ref.first_pass_params(name)
    pixels = ref.all_pixels(w, h)[::7]
    assert_same_records(multi.record_paths(p, pixels), single.record_paths(p, pixels))


# ---- the headless demo ---------------------------------------------------------------------------------------------------------------------
def test_rt_demo_prints_the_path_of_a_pixel(built, tmp_path):
    """rt_demo --debug-pixel X,Y: the path of that pixel of pass 0, one line per vertex, and the reason's name"""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    scene = os.path.join(root, "tests", "golden", "obj", "scene.json")
    r = subprocess.run([os.path.join(root, "raytracer_amd", "lib", "rt_demo"), "-s", scene, "--data", os.path.dirname(scene) + "/", "--width", "64", "--height", "48",
                        "--passes", "1", "--depth", "5", "--seed", "11", "--output", str(tmp_path / "out.bmp"), "--debug-pixel", "30,20"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    head = re.search(r"pixel \(30, 20\), pass 0: (\d+) vertices, (\w+), radiance", r.stdout)
    assert head and head.group(2) in ra.PATH_TERMINATION_REASONS[1:], r.stdout
    lines = re.findall(r"^  (\d+): origin .* throughput .* event \d+$", r.stdout, flags=re.M)
    assert [int(k) for k in lines] == list(range(int(head.group(1)))), r.stdout
    assert "1 passes of 64x48" in r.stdout   # the pass still renders
