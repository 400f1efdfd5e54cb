"""The a-trous filter on the device (rtgpu_filter_atrous, rtgpu_denoise, rtgpu_postprocess_from; raytracer_amd.atrous_filter, Viewport.denoise,
Viewport.front_buffer_from) against its NumPy float32 model (tests/denoise_ref.py).

Bar: BIT-EQUAL words.  The filter is defined operation by operation (include/rtgpu.h), the model performs those operations in that order in IEEE
float32, and the device library is compiled without contraction: there is no tolerance to state."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as ref
import raytracer_amd as ra
from raytracer_amd import scenes

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, NOT_READY, UNSUPPORTED = 0, -1, -5, -6
# (W, H): one pixel; one row, wider than a wave; a column of many blocks; a frame the reach of step 16 (32 pixels) exceeds; several workgroups both ways
SHAPES = [(1, 1), (70, 1), (3, 200), (37, 23), (130, 70)]
SIGMAS = dict(sigma_color=3.0, sigma_normal=0.5, sigma_plane=0.15)

_frames = {}


def frame(w, h):
    if (w, h) not in _frames:
        _frames[w, h] = ref.random_frame(w, h, seed=1000 * w + h)
    return _frames[w, h]


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_image(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    bad = np.argwhere(words(got) != words(want))
    assert len(bad) == 0, "%s: %d of %d channel words differ, first at %r: %r, the model has %r" % (
        what, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


# ---- 1. the filter on random inputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("demodulate", [True, False], ids=["demodulated", "plain"])
@pytest.mark.parametrize("w, h", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_the_filter_equals_the_model(built, w, h, demodulate):
    f = frame(w, h)
    if w * h > 500:
        miss = ~np.isfinite(f["depth"])
        assert 0.05 < miss.mean() < 0.2 and (f["albedo"][:, ~miss] < 1e-3).any()
        assert abs(float((f["normal"][:, ~miss] ** 2).sum(axis=0).mean()) - 1.0) < 1e-5
    for iterations in (1, 2, 5):
        want = ref.atrous(iterations=iterations, color_scale=0.25, demodulate=demodulate, **f, **SIGMAS)
        got = ra.atrous_filter(f["color"], f["depth"], f["normal"], f["position"], f["albedo"] if demodulate else None, iterations=iterations, color_scale=0.25,
                               demodulate=demodulate, **SIGMAS)
        assert_same_image(got, want, "%d x %d, %d levels" % (w, h, iterations))
        if w * h > 500:
            assert not np.array_equal(words(got), words(f["color"] * np.float32(0.25)))   # (it filters)


def test_eight_levels_reach_across_the_frame(built):
    f = frame(130, 70)
    want = ref.atrous(iterations=8, demodulate=True, **f, **SIGMAS)
    assert_same_image(ra.atrous_filter(iterations=8, **f, **SIGMAS), want, "eight levels")


def test_a_column_taller_than_a_grid_dimension(built):
    """1 x 262200: more rows of blocks than grid.y may hold (4 x 65535 = 262140 rows); the blocks are numbered along grid.x"""
    w, h = 1, 262200
    f = ref.random_frame(w, h, seed=3)
    want = ref.atrous(iterations=3, demodulate=True, **f, **SIGMAS)
    assert_same_image(ra.atrous_filter(iterations=3, **f, **SIGMAS), want, "1 x 262200")
    ra.release_filter_contexts()   # (its scratch is not kept for the rest of the session)


# ---- 1b. the two kernel variants ------------------------------------------------------------------------------------------------------------------
VARIANT_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import denoise_ref as ref
import raytracer_amd as ra
out = {}
for w, h in ((37, 23), (130, 70)):
    f = ref.random_frame(w, h, seed=1000 * w + h)
    for iterations in (1, 2, 5):
        for demodulate in (True, False):
            out["%d_%d_%d_%d" % (w, h, iterations, demodulate)] = ra.atrous_filter(f["color"], f["depth"], f["normal"], f["position"], f["albedo"] if demodulate else None,
                iterations=iterations, color_scale=0.25, demodulate=demodulate, sigma_color=3.0, sigma_normal=0.5, sigma_plane=0.15)
np.savez(sys.argv[2], **out)
"""


def test_both_kernel_variants_give_the_models_bits(built, tmp_path):
    """RTGPU_DENOISE_TILED is read once per process: a child per value filters 37 x 23 and 130 x 70 (1, 2 and 5 levels: the tiled kernels serve steps 1 and 2,
    as a middle and as the last level), and both equal the model, hence each other"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    results = {}
    for value in ("0", "1"):
        path = str(tmp_path / ("variant%s.npz" % value))
        r = subprocess.run([sys.executable, "-c", VARIANT_CHILD, root, path], env=dict(os.environ, RTGPU_DENOISE_TILED=value), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        results[value] = dict(np.load(path))
    assert len(results["0"]) == 12
    for key, direct in results["0"].items():
        w, h, iterations, demodulate = (int(v) for v in key.split("_"))
        f = frame(w, h)
        want = ref.atrous(iterations=iterations, color_scale=0.25, demodulate=bool(demodulate), **f, **SIGMAS)
        assert_same_image(direct, want, "direct, " + key)
        assert_same_image(results["1"][key], want, "tiled, " + key)


# ---- 2. device tensors on a stream of the caller's ------------------------------------------------------------------------------------------------
def test_tensors_on_a_side_stream_equal_the_host_call(built):
    import torch
    f = frame(130, 70)
    host = ra.atrous_filter(iterations=5, **f, **SIGMAS)
    plain = ra.atrous_filter(f["color"], f["depth"], f["normal"], f["position"], iterations=3, demodulate=False, **SIGMAS)
    t = {k: torch.from_numpy(v).cuda() for k, v in f.items()}
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        a = ra.atrous_filter(iterations=5, **t, **SIGMAS)
        b = ra.atrous_filter(t["color"], t["depth"], t["normal"], t["position"], iterations=3, demodulate=False, **SIGMAS)   # the scratch is shared: ordered behind a
    on_default = ra.atrous_filter(iterations=5, **t, **SIGMAS)   # torch's null stream: the wrapper's side stream
    stream.synchronize()
    assert a.is_cuda and a.dtype == torch.float32 and tuple(a.shape) == (70, 130, 3)
    assert_same_image(a.cpu().numpy(), host, "side stream")
    assert_same_image(b.cpu().numpy(), plain, "side stream, second call")
    assert_same_image(on_default.cpu().numpy(), host, "default stream")
    with pytest.raises(ValueError):
        ra.atrous_filter(t["color"], f["depth"], t["normal"], t["position"], demodulate=False)   # arrays and tensors mixed


# ---- 3. a rendered frame --------------------------------------------------------------------------------------------------------------------------
W, H, PASSES = 48, 32, 4


def rendered(denoise):
    """four passes of the sphere under its rect light (misses around it), a fifth after the call under test: what the frame holds then"""
    scene, camera = scenes.sphere_area_light(W / H)
    vp = ra.Viewport(W, H, seed=4321, max_ray_depth=3)
    vp.set_renderer(scene)
    params = [vp.next_pass_params(camera) for _ in range(PASSES + 1)]
    for p in params[:PASSES]:
        vp.render_pass_with(p)
    out = None
    if denoise:
        out = dict(host=vp.denoise(params[PASSES], **SIGMAS), device=vp.denoise(params[PASSES], device=True, **SIGMAS).cpu().numpy(),
                   plain=vp.denoise(params[PASSES], iterations=2, demodulate=False, color_scale=0.5, **SIGMAS),
                   sums=vp.sum_buffer(secondary=True), counters=vp.counters(), passes=vp.passes_finished,
                   guides=vp.render_aovs(params[PASSES], ("depth", "normal", "position", "base_color")))
    vp.render_pass_with(params[PASSES])
    return out, vp.sum_buffer(secondary=True), vp.counters(), vp.passes_finished


def test_a_rendered_frame_equals_the_model_and_the_call_is_not_a_pass(built):
    out, sums, counters, passes = rendered(True)
    _, plain_sums, plain_counters, plain_passes = rendered(False)
    g, (s, s2) = out["guides"], out["sums"]
    miss = ~np.isfinite(g["depth"])
    assert miss.sum() > 100 and (~miss).sum() > 100 and s[~miss].any() and out["passes"] == PASSES
    want = ref.atrous(s, g["depth"], g["normal"], g["position"], g["base_color"], iterations=5, color_scale=1.0 / PASSES, demodulate=True, **SIGMAS)
    assert_same_image(out["host"], want, "Viewport.denoise")
    assert_same_image(out["device"], want, "Viewport.denoise(device=True)")
    assert_same_image(out["plain"], ref.atrous(s, g["depth"], g["normal"], g["position"], iterations=2, color_scale=0.5, demodulate=False, **SIGMAS), "two levels, not demodulated")
    assert not np.array_equal(words(want), words(s * np.float32(1.0 / PASSES)))
    # the render state: the fifth pass lands on the same film, the counters count the same rays
    assert np.array_equal(words(sums[0]), words(plain_sums[0])) and np.array_equal(words(sums[1]), words(plain_sums[1]))
    assert counters == plain_counters and passes == plain_passes == PASSES + 1
    assert not np.array_equal(words(sums[0]), words(s))


# ---- 4. statuses through the raw ABI --------------------------------------------------------------------------------------------------------------
def raw_filter(ctx, p, w, h, null=(), entry="rtgpu_filter_atrous", pointers=None):
    n = max(1, min(w * h, 4096))
    keep = {name: np.zeros(3 * n, dtype=np.float32) for name in ("color", "depth", "normal", "position", "albedo", "out")}
    ptr = {name: a.ctypes.data_as(C.c_void_p) for name, a in keep.items()}
    ptr.update(pointers or {})
    ptr.update({name: None for name in null})
    args = (ctx, C.byref(p) if p is not None else None, C.c_uint32(w), C.c_uint32(h), ptr["color"], ptr["depth"], ptr["normal"], ptr["position"], ptr["albedo"], ptr["out"])
    if entry.endswith("_async"):
        args += (None,)
    return getattr(ra.rtgpu_lib(), entry)(*args)


def test_statuses(built):
    import torch
    lib = ra.rtgpu_lib()
    ctx = C.c_void_p()
    assert lib.rtgpu_create(0, C.byref(ctx)) == OK
    try:
        good, plain = ra.denoise_params(), ra.denoise_params(demodulate=False)
        dev = torch.zeros(16 * 64 + 4, dtype=torch.float32, device="cuda")
        at = lambda k: C.c_void_p(dev.data_ptr() + 64 * 4 * k)   # noqa: E731
        device_pointers = dict(color=at(0), depth=at(3), normal=at(4), position=at(7), albedo=at(10), out=at(13))
        for entry, pointers in (("rtgpu_filter_atrous", None), ("rtgpu_filter_atrous_async", device_pointers)):
            call = lambda p, w=4, h=4, null=(), extra=None: raw_filter(ctx, p, w, h, null, entry, dict(pointers or {}, **(extra or {})))   # noqa: E731
            assert call(good) == OK                                   # a pure image filter: no scene, no rtgpu_resize
            assert call(None) == INVALID_ARGUMENT
            for name in ("color", "depth", "normal", "position", "out", "albedo"):
                assert call(good, null=(name,)) == INVALID_ARGUMENT, name
            assert call(plain, null=("albedo",)) == OK                # albedo may be NULL without RT_DENOISE_DEMODULATE
            for iterations in (0, 9, 0xFFFFFFFF):
                assert call(ra.denoise_params(iterations=iterations)) == INVALID_ARGUMENT
            assert call(ra.denoise_params(iterations=8)) == OK
            for field in ("sigma_color", "sigma_normal", "sigma_plane", "color_scale"):
                for value in (0.0, -1.0, float("inf"), float("nan")):
                    assert call(ra.denoise_params(**{field: value})) == INVALID_ARGUMENT, (field, value)
            assert call(good, w=0) == INVALID_ARGUMENT and call(good, h=0) == INVALID_ARGUMENT
            assert call(good, w=4097, h=4096) == UNSUPPORTED          # > 16 Mi pixels: refused before a buffer is read
            assert call(good, w=65536, h=65536) == UNSUPPORTED
        # the async entry: 16-byte aligned device memory, and an output that overlaps no input
        assert raw_filter(ctx, good, 4, 4, (), "rtgpu_filter_atrous_async", dict(device_pointers, out=C.c_void_p(dev.data_ptr() + 64 * 4 * 13 + 4))) == INVALID_ARGUMENT
        assert raw_filter(ctx, good, 4, 4, (), "rtgpu_filter_atrous_async", dict(device_pointers, depth=C.c_void_p(dev.data_ptr() + 64 * 4 * 3 + 8))) == INVALID_ARGUMENT
        assert raw_filter(ctx, good, 4, 4, (), "rtgpu_filter_atrous_async", dict(device_pointers, out=C.c_void_p(dev.data_ptr() + 4 * 32))) == INVALID_ARGUMENT
        assert b"overlap" in lib.rtgpu_last_error()
        # the checker is the variance-guided and the temporal entries' too: an output inside an input that is not the colour, a misaligned input that is not the colour
        inside_position = C.c_void_p(dev.data_ptr() + 64 * 4 * 7 + 4 * 32)
        assert raw_filter(ctx, good, 4, 4, (), "rtgpu_filter_atrous_async", dict(device_pointers, out=inside_position)) == INVALID_ARGUMENT and b"overlap" in lib.rtgpu_last_error()
        assert raw_filter(ctx, good, 4, 4, (), "rtgpu_filter_atrous_async", dict(device_pointers, normal=C.c_void_p(dev.data_ptr() + 64 * 4 * 4 + 4))) == INVALID_ARGUMENT
        assert b"aligned" in lib.rtgpu_last_error()
        assert lib.rtgpu_synchronize(ctx) == OK
        torch.cuda.synchronize()
        # rtgpu_denoise before rtgpu_upload_scene, then before rtgpu_resize
        scene, camera = scenes.sphere_area_light(1.5)
        probe = ra.Viewport(48, 32, seed=1, max_ray_depth=2)
        pp = probe.next_pass_params(camera)
        out = np.zeros((32, 48, 3), dtype=np.float32)
        optr = out.ctypes.data_as(C.c_void_p)
        assert lib.rtgpu_denoise(ctx, C.byref(good), C.byref(pp), optr) == NOT_READY
        assert lib.rtgpu_denoise_async(ctx, C.byref(good), C.byref(pp), at(0), None) == NOT_READY
        assert lib.rtgpu_upload_scene(ctx, scene.desc) == OK
        assert lib.rtgpu_denoise(ctx, C.byref(good), C.byref(pp), optr) == NOT_READY
        assert lib.rtgpu_postprocess_from(ctx, C.byref(ra.RtPostprocessParams()), optr, optr) == NOT_READY
        assert lib.rtgpu_resize(ctx, 48, 32) == OK
        assert lib.rtgpu_denoise(ctx, C.byref(good), C.byref(pp), optr) == OK   # (an empty film: zeros in, zeros out)
        assert not out.any()
        assert lib.rtgpu_denoise(ctx, None, C.byref(pp), optr) == INVALID_ARGUMENT and lib.rtgpu_denoise(ctx, C.byref(good), None, optr) == INVALID_ARGUMENT
        assert lib.rtgpu_denoise(ctx, C.byref(good), C.byref(pp), None) == INVALID_ARGUMENT
        assert lib.rtgpu_denoise(ctx, C.byref(ra.denoise_params(iterations=0)), C.byref(pp), optr) == INVALID_ARGUMENT
        assert lib.rtgpu_denoise(ctx, C.byref(ra.denoise_params(sigma_plane=0.0)), C.byref(pp), optr) == INVALID_ARGUMENT
        assert lib.rtgpu_denoise_async(ctx, C.byref(good), C.byref(pp), C.c_void_p(dev.data_ptr() + 4), None) == INVALID_ARGUMENT
        # what rtgpu_render_aovs refuses in the guide params gets the status it gets there
        deep = ra.RtPassParams.from_buffer_copy(pp)
        deep.maxRayDepth = 255
        planes, outputs = (C.c_uint32 * 1)(0), (C.c_void_p * 1)(out.ctypes.data)
        assert lib.rtgpu_denoise(ctx, C.byref(good), C.byref(deep), optr) == lib.rtgpu_render_aovs(ctx, C.byref(deep), planes, C.c_uint32(1), outputs) == INVALID_ARGUMENT
        bokeh = ra.RtPassParams.from_buffer_copy(pp)
        bokeh.camera.dofEnable, bokeh.camera.bokehShape = 1, 3
        assert lib.rtgpu_denoise(ctx, C.byref(good), C.byref(bokeh), optr) == lib.rtgpu_render_aovs(ctx, C.byref(bokeh), planes, C.c_uint32(1), outputs) == UNSUPPORTED
        assert lib.rtgpu_denoise_async(ctx, C.byref(good), C.byref(bokeh), at(0), None) == UNSUPPORTED
    finally:
        lib.rtgpu_destroy(ctx)


# ---- 5. the post-process over a caller's image -----------------------------------------------------------------------------------------------------
def test_postprocess_from_the_sum_buffer_equals_postprocess(built):
    w, h = 208, 200   # bloom: a multiple of 4 wide, larger than the widest blur window (195)
    scene, camera = scenes.sphere_area_light(w / h)
    vp = ra.Viewport(w, h, seed=99, max_ray_depth=2)
    vp.set_renderer(scene)
    for _ in range(3):
        vp.render_pass_with(vp.next_pass_params(camera))
    s = vp.sum_buffer()
    for bloom in (0.0, 0.3):
        want = vp.front_buffer(bloom=bloom, dither_seed=5)
        got = vp.front_buffer_from(s, bloom=bloom, dither_seed=5, num_passes=vp.passes_finished)
        assert want.any() and np.array_equal(got, want), "bloom %g" % bloom
    assert not np.array_equal(vp.front_buffer_from(s * np.float32(0.5), num_passes=vp.passes_finished), vp.front_buffer())
    # the same restrictions
    small = ra.Viewport(50, 32, seed=99)
    small.set_renderer(scene)
    with pytest.raises(RuntimeError, match="bloom"):
        small.front_buffer_from(np.zeros((32, 50, 3), dtype=np.float32), bloom=0.3)
    with pytest.raises(RuntimeError, match="bloom"):
        small.front_buffer(bloom=0.3)


# ---- 6. the headless demo --------------------------------------------------------------------------------------------------------------------------
def test_rt_demo_writes_the_denoised_frame(built, tmp_path):
    """rt_demo --denoise [N]: the same passes, the frame through rtgpu_denoise and rtgpu_postprocess_from before it is written"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    scene = os.path.join(root, "tests", "golden", "obj", "scene.json")
    images = {}
    for label, extra in (("plain", []), ("three", ["--denoise", "3"]), ("default", ["--denoise"])):
        path = str(tmp_path / (label + ".bmp"))
        r = subprocess.run([os.path.join(root, "raytracer_amd", "lib", "rt_demo"), "-s", scene, "--data", os.path.dirname(scene) + "/", "--width", "64", "--height", "48",
                            "--passes", "2", "--depth", "3", "--seed", "11"] + extra + ["--output", path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("denoised: %d levels" % (3 if label == "three" else 5) in r.stdout) == (label != "plain"), r.stdout
        assert "2 passes of 64x48" in r.stdout
        images[label] = open(path, "rb").read()
    assert len(images["plain"]) == len(images["three"]) == len(images["default"]) == 54 + 64 * 48 * 3
    assert images["plain"][:54] == images["three"][:54] and images["plain"] != images["three"] and images["three"] != images["default"]
    r = subprocess.run([os.path.join(root, "raytracer_amd", "lib", "rt_demo"), "-s", scene, "--denoise", "9"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "1..8" in r.stderr
