"""The variance-guided a-trous filter on the device (rtgpu_filter_atrous_var, rtgpu_denoise_var; raytracer_amd.atrous_filter(color_half=...),
Viewport.denoise(variance=True), rt_demo --denoise-variance) against its NumPy float32 model (tests/denoise_var_ref.py).

Bar: BIT-EQUAL words, image and variance.  The filter is defined operation by operation (include/rtgpu.h), the model performs those operations in that
order in IEEE float32, and the device library is compiled without contraction: there is no tolerance to state."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_var_ref as ref
import raytracer_amd as ra
from raytracer_amd import scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARGUMENT, NOT_READY, UNSUPPORTED = 0, -1, -5, -6
# (W, H): one pixel; one row, wider than a wave; a column of many blocks; a frame the reach of step 16 exceeds and whose 3 x 3 windows are clipped at
# every border; several workgroups and tiles both ways
SHAPES = [(1, 1), (70, 1), (3, 200), (37, 23), (130, 70)]
SIGMAS = dict(sigma_lum=3.0, sigma_normal=0.5, sigma_plane=0.15)

_frames = {}
_models = {}


def frame(w, h):
    if (w, h) not in _frames:
        _frames[w, h] = ref.random_frame_var(w, h, seed=1000 * w + h)
    return _frames[w, h]


def model(w, h, iterations, demodulate):
    """(image, variance) of the model for frame(w, h), colorScale 0.25: computed once, shared, never written"""
    key = (w, h, iterations, demodulate)
    if key not in _models:
        _models[key] = ref.atrous_var(iterations=iterations, color_scale=0.25, demodulate=demodulate, **frame(w, h), **SIGMAS)
        for a in _models[key]:
            a.setflags(write=False)
    return _models[key]


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    bad = np.argwhere(words(got) != words(want))
    assert len(bad) == 0, "%s: %d of %d words differ, first at %r: %r, the model has %r" % (
        what, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def device_filter(f, iterations, demodulate, return_variance=True):
    return ra.atrous_filter(f["color"], f["depth"], f["normal"], f["position"], f["albedo"] if demodulate else None, iterations=iterations, color_scale=0.25,
                            demodulate=demodulate, color_half=f["color_half"], return_variance=return_variance, **SIGMAS)


# ---- 1. the filter on random inputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("demodulate", [True, False], ids=["demodulated", "plain"])
@pytest.mark.parametrize("w, h", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_the_filter_equals_the_model(built, w, h, demodulate):
    f = frame(w, h)
    if w * h > 500:
        miss = ~np.isfinite(f["depth"])
        agree = (words(f["color_half"] * np.float32(2.0)) == words(f["color"])).all(axis=-1)
        assert 0.05 < miss.mean() < 0.2 and 0.05 < agree.mean() < 0.2 and (f["color"] > 1e3).any()
    for iterations in (1, 2, 5):
        want, want_v = model(w, h, iterations, demodulate)
        got, got_v = device_filter(f, iterations, demodulate)
        assert_same(got, want, "%d x %d, %d levels" % (w, h, iterations))
        assert_same(got_v, want_v, "%d x %d, %d levels, variance" % (w, h, iterations))
        if w * h > 500:
            assert not np.array_equal(words(got), words(f["color"] * np.float32(0.25))) and got_v.any()   # (it filters)
    # outVariance == NULL: the same image
    assert_same(device_filter(f, 2, demodulate, return_variance=False), model(w, h, 2, demodulate)[0], "%d x %d, no variance asked for" % (w, h))


def test_eight_levels_reach_across_the_frame(built):
    for w, h, demodulate in ((37, 23, True), (37, 23, False), (130, 70, True), (130, 70, False)):
        want, want_v = model(w, h, 8, demodulate)
        got, got_v = device_filter(frame(w, h), 8, demodulate)
        assert_same(got, want, "eight levels, %d x %d, demodulate %r" % (w, h, demodulate))
        assert_same(got_v, want_v, "eight levels, %d x %d, demodulate %r, variance" % (w, h, demodulate))


def test_the_plain_filter_is_what_it_was_beside_the_new_one(built):
    """the kernels are shared by template parameter: the existing instantiations still give the existing model's bits, interleaved with variance calls
    on the same context's scratch (whose fourth colour lane the variance calls leave non-zero)"""
    import denoise_ref
    f = frame(130, 70)
    plain = {k: f[k] for k in ("color", "depth", "normal", "position", "albedo")}
    want = denoise_ref.atrous(iterations=5, sigma_color=3.0, sigma_normal=0.5, sigma_plane=0.15, **plain)
    device_filter(f, 5, True)
    assert_same(ra.atrous_filter(iterations=5, sigma_color=3.0, sigma_normal=0.5, sigma_plane=0.15, **plain), want, "the plain filter after a variance call")


# ---- 1b. the two kernel variants ------------------------------------------------------------------------------------------------------------------
VARIANT_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import denoise_var_ref as ref
import raytracer_amd as ra
out = {}
for w, h in ((37, 23), (130, 70)):
    f = ref.random_frame_var(w, h, seed=1000 * w + h)
    for iterations in (1, 2, 5):
        for demodulate in (True, False):
            image, variance = ra.atrous_filter(f["color"], f["depth"], f["normal"], f["position"], f["albedo"] if demodulate else None, iterations=iterations,
                color_scale=0.25, demodulate=demodulate, color_half=f["color_half"], return_variance=True, sigma_lum=3.0, sigma_normal=0.5, sigma_plane=0.15)
            out["i_%d_%d_%d_%d" % (w, h, iterations, demodulate)] = image
            out["v_%d_%d_%d_%d" % (w, h, iterations, demodulate)] = variance
np.savez(sys.argv[2], **out)
"""


def test_both_kernel_variants_give_the_models_bits(built, tmp_path):
    """RTGPU_DENOISE_TILED is read once per process: a child per value filters 37 x 23 and 130 x 70 (1, 2 and 5 levels: the tiled variance kernels serve
    steps 1 and 2, each as a middle and as the last level), and both equal the model, hence each other"""
    results = {}
    for value in ("0", "1"):
        path = str(tmp_path / ("variant%s.npz" % value))
        r = subprocess.run([sys.executable, "-c", VARIANT_CHILD, ROOT, path], env=dict(os.environ, RTGPU_DENOISE_TILED=value), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        results[value] = dict(np.load(path))
    assert len(results["0"]) == len(results["1"]) == 24
    for key, direct in results["0"].items():
        kind, w, h, iterations, demodulate = key.split("_")
        want = model(int(w), int(h), int(iterations), bool(int(demodulate)))[0 if kind == "i" else 1]
        assert_same(direct, want, "direct, " + key)
        assert_same(results["1"][key], want, "tiled, " + key)


# ---- 2. device tensors on a stream of the caller's ------------------------------------------------------------------------------------------------
def test_tensors_on_a_side_stream_and_on_the_default_stream(built):
    import torch
    f = frame(130, 70)
    want, want_v = model(130, 70, 5, True)
    plain, plain_v = model(130, 70, 2, False)
    t = {k: torch.from_numpy(v).cuda() for k, v in f.items()}
    call = lambda iterations, demodulate, **kw: ra.atrous_filter(t["color"], t["depth"], t["normal"], t["position"], t["albedo"] if demodulate else None,   # noqa: E731
                                                                 iterations=iterations, color_scale=0.25, demodulate=demodulate, color_half=t["color_half"], **SIGMAS, **kw)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        a, av = call(5, True, return_variance=True)
        b, bv = call(2, False, return_variance=True)   # the scratch is shared: ordered behind a
        c = call(5, True)
    on_default, on_default_v = call(5, True, return_variance=True)   # torch's null stream: the wrapper's side stream
    stream.synchronize()
    assert a.is_cuda and a.dtype == av.dtype == torch.float32 and tuple(a.shape) == (70, 130, 3) and tuple(av.shape) == (70, 130) and av.device == a.device
    assert_same(a.cpu().numpy(), want, "side stream")
    assert_same(av.cpu().numpy(), want_v, "side stream, variance")
    assert_same(b.cpu().numpy(), plain, "side stream, second call")
    assert_same(bv.cpu().numpy(), plain_v, "side stream, second call, variance")
    assert_same(c.cpu().numpy(), want, "side stream, no variance asked for")
    assert_same(on_default.cpu().numpy(), want, "default stream")
    assert_same(on_default_v.cpu().numpy(), want_v, "default stream, variance")
    with pytest.raises(ValueError):
        ra.atrous_filter(t["color"], t["depth"], t["normal"], t["position"], demodulate=False, color_half=f["color_half"])   # arrays and tensors mixed


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
        out = dict(host=vp.denoise(params[PASSES], variance=True, return_variance=True, **SIGMAS),
                   device=tuple(t.cpu().numpy() for t in vp.denoise(params[PASSES], variance=True, return_variance=True, device=True, **SIGMAS)),
                   image_only=vp.denoise(params[PASSES], variance=True, **SIGMAS),
                   plain=vp.denoise(params[PASSES], variance=True, return_variance=True, iterations=2, demodulate=False, color_scale=0.5, **SIGMAS),
                   sums=vp.sum_buffer(secondary=True), counters=vp.counters(), passes=vp.passes_finished,
                   guides=vp.render_aovs(params[PASSES], ("depth", "normal", "position", "base_color")))
    vp.render_pass_with(params[PASSES])
    return out, vp.sum_buffer(secondary=True), vp.counters(), vp.passes_finished


def test_a_rendered_frame_equals_the_model_and_the_call_is_not_a_pass(built):
    out, sums, counters, passes = rendered(True)
    _, plain_sums, plain_counters, plain_passes = rendered(False)
    g, (s, s2) = out["guides"], out["sums"]
    miss = ~np.isfinite(g["depth"])
    assert miss.sum() > 100 and (~miss).sum() > 100 and s[~miss].any() and s2[~miss].any() and out["passes"] == PASSES
    want, want_v = ref.atrous_var(s, s2, g["depth"], g["normal"], g["position"], g["base_color"], iterations=5, color_scale=1.0 / PASSES, demodulate=True, **SIGMAS)
    assert_same(out["host"][0], want, "Viewport.denoise(variance=True)")
    assert_same(out["host"][1], want_v, "Viewport.denoise(variance=True), variance")
    assert_same(out["device"][0], want, "Viewport.denoise(variance=True, device=True)")
    assert_same(out["device"][1], want_v, "Viewport.denoise(variance=True, device=True), variance")
    assert_same(out["image_only"], want, "Viewport.denoise(variance=True), no variance asked for")
    two, two_v = ref.atrous_var(s, s2, g["depth"], g["normal"], g["position"], iterations=2, color_scale=0.5, demodulate=False, **SIGMAS)
    assert_same(out["plain"][0], two, "two levels, not demodulated")
    assert_same(out["plain"][1], two_v, "two levels, not demodulated, variance")
    assert not np.array_equal(words(want), words(s * np.float32(1.0 / PASSES))) and want_v[~miss].any() and not want_v[miss].any()
    # the render state: the fifth pass lands on the same film, the counters count the same rays
    assert np.array_equal(words(sums[0]), words(plain_sums[0])) and np.array_equal(words(sums[1]), words(plain_sums[1]))
    assert counters == plain_counters and passes == plain_passes == PASSES + 1
    assert not np.array_equal(words(sums[0]), words(s))


# ---- 4. statuses through the raw ABI --------------------------------------------------------------------------------------------------------------
NAMES = ("color", "half", "depth", "normal", "position", "albedo", "out", "variance")


def raw_filter(ctx, p, w, h, null=(), entry="rtgpu_filter_atrous_var", pointers=None):
    n = max(1, min(w * h, 4096))
    keep = {name: np.zeros(3 * n, dtype=np.float32) for name in NAMES}
    ptr = {name: a.ctypes.data_as(C.c_void_p) for name, a in keep.items()}
    ptr.update(pointers or {})
    ptr.update({name: None for name in null})
    args = (ctx, C.byref(p) if p is not None else None, C.c_uint32(w), C.c_uint32(h)) + tuple(ptr[name] for name in NAMES)
    if entry.endswith("_async"):
        args += (None,)
    return getattr(ra.rtgpu_lib(), entry)(*args)


def test_statuses(built):
    import torch
    lib = ra.rtgpu_lib()
    ctx = C.c_void_p()
    assert lib.rtgpu_create(0, C.byref(ctx)) == OK
    try:
        good, plain = ra.denoise_var_params(), ra.denoise_var_params(demodulate=False)
        dev = torch.zeros(20 * 64 + 4, dtype=torch.float32, device="cuda")
        at = lambda k: C.c_void_p(dev.data_ptr() + 64 * 4 * k)   # noqa: E731
        device_pointers = dict(color=at(0), half=at(3), depth=at(6), normal=at(7), position=at(10), albedo=at(13), out=at(16), variance=at(19))
        for entry, pointers in (("rtgpu_filter_atrous_var", None), ("rtgpu_filter_atrous_var_async", device_pointers)):
            call = lambda p, w=4, h=4, null=(), extra=None: raw_filter(ctx, p, w, h, null, entry, dict(pointers or {}, **(extra or {})))   # noqa: E731
            assert call(good) == OK                                   # a pure image filter: no scene, no rtgpu_resize
            assert call(None) == INVALID_ARGUMENT
            for name in ("color", "half", "depth", "normal", "position", "out", "albedo"):
                assert call(good, null=(name,)) == INVALID_ARGUMENT, name
            assert call(good, null=("variance",)) == OK               # outVariance is optional
            assert call(plain, null=("albedo",)) == OK                # albedo may be NULL without RT_DENOISE_DEMODULATE
            assert call(plain, null=("albedo", "half")) == INVALID_ARGUMENT
            for iterations in (0, 9, 0xFFFFFFFF):
                assert call(ra.denoise_var_params(iterations=iterations)) == INVALID_ARGUMENT
            assert call(ra.denoise_var_params(iterations=8)) == OK
            for field in ("sigma_lum", "variance_floor", "sigma_normal", "sigma_plane", "color_scale"):
                for value in (0.0, -1.0, float("inf"), float("nan")):
                    assert call(ra.denoise_var_params(**{field: value})) == INVALID_ARGUMENT, (field, value)
            assert call(good, w=0) == INVALID_ARGUMENT and call(good, h=0) == INVALID_ARGUMENT
            assert call(good, w=4097, h=4096) == UNSUPPORTED          # > 16 Mi pixels: refused before a buffer is read
            assert call(good, w=65536, h=65536) == UNSUPPORTED
        # the async entry: 16-byte aligned device memory, and outputs that overlap no input and not each other
        async_call = lambda **extra: raw_filter(ctx, good, 4, 4, (), "rtgpu_filter_atrous_var_async", dict(device_pointers, **extra))   # noqa: E731
        base = dev.data_ptr()
        assert async_call(out=C.c_void_p(base + 64 * 4 * 16 + 4)) == INVALID_ARGUMENT
        assert async_call(variance=C.c_void_p(base + 64 * 4 * 19 + 4)) == INVALID_ARGUMENT
        assert async_call(half=C.c_void_p(base + 64 * 4 * 3 + 8)) == INVALID_ARGUMENT
        assert async_call(out=C.c_void_p(base + 4 * 32)) == INVALID_ARGUMENT and b"overlap" in lib.rtgpu_last_error()          # over the colour
        assert async_call(out=at(3)) == INVALID_ARGUMENT and b"overlap" in lib.rtgpu_last_error()                              # the half buffer itself
        assert async_call(variance=at(6)) == INVALID_ARGUMENT and b"overlap" in lib.rtgpu_last_error()                         # over the depth plane
        assert async_call(variance=C.c_void_p(base + 64 * 4 * 16 + 4 * 32)) == INVALID_ARGUMENT and b"overlap" in lib.rtgpu_last_error()   # inside outRGB
        assert lib.rtgpu_synchronize(ctx) == OK
        torch.cuda.synchronize()
        # rtgpu_denoise_var before rtgpu_upload_scene, then before rtgpu_resize
        scene, camera = scenes.sphere_area_light(1.5)
        probe = ra.Viewport(48, 32, seed=1, max_ray_depth=2)
        pp = probe.next_pass_params(camera)
        out, var = np.ones((32, 48, 3), dtype=np.float32), np.ones((32, 48), dtype=np.float32)
        optr, vptr = out.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p)
        big = torch.zeros(48 * 32 * 4 + 8, dtype=torch.float32, device="cuda")
        dout, dvar = C.c_void_p(big.data_ptr()), C.c_void_p(big.data_ptr() + 48 * 32 * 3 * 4)
        assert lib.rtgpu_denoise_var(ctx, C.byref(good), C.byref(pp), optr, vptr) == NOT_READY
        assert lib.rtgpu_denoise_var_async(ctx, C.byref(good), C.byref(pp), dout, dvar, None) == NOT_READY
        assert lib.rtgpu_upload_scene(ctx, scene.desc) == OK
        assert lib.rtgpu_denoise_var(ctx, C.byref(good), C.byref(pp), optr, vptr) == NOT_READY
        assert lib.rtgpu_resize(ctx, 48, 32) == OK
        assert lib.rtgpu_denoise_var(ctx, C.byref(good), C.byref(pp), optr, vptr) == OK   # (an empty film: zeros in, zeros out)
        assert not out.any() and not var.any()
        assert lib.rtgpu_denoise_var(ctx, C.byref(good), C.byref(pp), optr, None) == OK
        assert lib.rtgpu_denoise_var_async(ctx, C.byref(good), C.byref(pp), dout, dvar, None) == OK
        assert lib.rtgpu_denoise_var_async(ctx, C.byref(good), C.byref(pp), dout, None, None) == OK
        assert lib.rtgpu_synchronize(ctx) == OK
        assert lib.rtgpu_denoise_var(ctx, None, C.byref(pp), optr, vptr) == INVALID_ARGUMENT and lib.rtgpu_denoise_var(ctx, C.byref(good), None, optr, vptr) == INVALID_ARGUMENT
        assert lib.rtgpu_denoise_var(ctx, C.byref(good), C.byref(pp), None, vptr) == INVALID_ARGUMENT
        assert lib.rtgpu_denoise_var(ctx, C.byref(ra.denoise_var_params(iterations=0)), C.byref(pp), optr, vptr) == INVALID_ARGUMENT
        assert lib.rtgpu_denoise_var(ctx, C.byref(ra.denoise_var_params(sigma_lum=0.0)), C.byref(pp), optr, vptr) == INVALID_ARGUMENT
        assert lib.rtgpu_denoise_var(ctx, C.byref(ra.denoise_var_params(variance_floor=float("nan"))), C.byref(pp), optr, vptr) == INVALID_ARGUMENT
        assert lib.rtgpu_denoise_var_async(ctx, C.byref(good), C.byref(pp), C.c_void_p(big.data_ptr() + 4), dvar, None) == INVALID_ARGUMENT
        assert lib.rtgpu_denoise_var_async(ctx, C.byref(good), C.byref(pp), dout, C.c_void_p(big.data_ptr() + 48 * 32 * 3 * 4 + 4), None) == INVALID_ARGUMENT
        assert lib.rtgpu_denoise_var_async(ctx, C.byref(good), C.byref(pp), dout, C.c_void_p(big.data_ptr() + 64), None) == INVALID_ARGUMENT and b"overlap" in lib.rtgpu_last_error()
        # what rtgpu_render_aovs refuses in the guide params gets the status it gets there
        deep = ra.RtPassParams.from_buffer_copy(pp)
        deep.maxRayDepth = 255
        planes, outputs = (C.c_uint32 * 1)(0), (C.c_void_p * 1)(out.ctypes.data)
        assert lib.rtgpu_denoise_var(ctx, C.byref(good), C.byref(deep), optr, vptr) == lib.rtgpu_render_aovs(ctx, C.byref(deep), planes, C.c_uint32(1), outputs) == INVALID_ARGUMENT
        bokeh = ra.RtPassParams.from_buffer_copy(pp)
        bokeh.camera.dofEnable, bokeh.camera.bokehShape = 1, 3
        assert lib.rtgpu_denoise_var(ctx, C.byref(good), C.byref(bokeh), optr, vptr) == lib.rtgpu_render_aovs(ctx, C.byref(bokeh), planes, C.c_uint32(1), outputs) == UNSUPPORTED
        assert lib.rtgpu_denoise_var_async(ctx, C.byref(good), C.byref(bokeh), dout, dvar, None) == UNSUPPORTED
    finally:
        lib.rtgpu_destroy(ctx)


# ---- 5. the headless demo --------------------------------------------------------------------------------------------------------------------------
def test_rt_demo_writes_the_variance_guided_frame(built, tmp_path):
    """rt_demo --denoise-variance [N]: the same passes, the frame through rtgpu_denoise_var and rtgpu_postprocess_from before it is written"""
    scene = os.path.join(ROOT, "tests", "golden", "obj", "scene.json")
    demo = os.path.join(ROOT, "raytracer_amd", "lib", "rt_demo")
    images = {}
    for label, extra in (("plain", []), ("colour", ["--denoise", "3"]), ("three", ["--denoise-variance", "3"]), ("default", ["--denoise-variance"])):
        path = str(tmp_path / (label + ".bmp"))
        r = subprocess.run([demo, "-s", scene, "--data", os.path.dirname(scene) + "/", "--width", "64", "--height", "48", "--passes", "2", "--depth", "3", "--seed", "11"] +
                           extra + ["--output", path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("denoised: %d levels of the variance-guided a-trous filter" % (5 if label == "default" else 3) in r.stdout) == (label in ("three", "default")), r.stdout
        assert "2 passes of 64x48" in r.stdout
        images[label] = open(path, "rb").read()
    assert all(len(image) == 54 + 64 * 48 * 3 for image in images.values())
    assert images["plain"][:54] == images["three"][:54] and len(set(images.values())) == 4
    r = subprocess.run([demo, "-s", scene, "--denoise-variance", "9"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "1..8" in r.stderr
