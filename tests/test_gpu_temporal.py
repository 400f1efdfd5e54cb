"""Temporal accumulation on the device (rtgpu_temporal_accumulate, rtgpu_denoise_temporal, RT_DENOISE_INPUT_PREPARED; raytracer_amd.temporal_accumulate,
atrous_filter(prepared=True), Viewport.denoise(temporal=True)) against its NumPy float32 model (tests/temporal_ref.py).

Bar: BIT-EQUAL words in outA, outB, outLength and outMotion, and in the filtered image and variance behind them.  The operation is defined step by step
(include/rtgpu.h), the model performs those steps in that order in IEEE float32, and the device library is compiled without contraction: there is no
tolerance to state.  What the random frames cover is asserted by tests/test_temporal_model.py."""
import ctypes as C

import numpy as np
import pytest

import denoise_var_ref
import temporal_ref as ref
import raytracer_amd as ra
from raytracer_amd import scenes

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, NOT_READY, UNSUPPORTED = 0, -1, -5, -6
# (W, H), the filter's shapes for the filter's reasons: one pixel; one row, wider than a wave; a column of many blocks; clipped borders; several workgroups both ways
SHAPES = [(1, 1), (70, 1), (3, 200), (37, 23), (130, 70)]
PARAMS = dict(alpha_min=0.05, max_history=48.0, color_scale=0.25)   # (the two thresholds at their defaults, as the coverage test runs the frames)
SIGMAS = dict(sigma_lum=3.0, sigma_normal=0.5, sigma_plane=0.15)
OUTPUTS = ("a", "b", "length")

_frames = {}
_models = {}


def frame(w, h):
    if (w, h) not in _frames:
        _frames[w, h] = ref.random_temporal_frame(w, h, seed=1000 * w + h)
    return _frames[w, h]


def inputs(w, h, demodulate, ids, history):
    """the keyword arguments model and device take alike for one case of frame(w, h)"""
    f = frame(w, h)
    cur = dict(f["current"])
    if not demodulate:
        del cur["albedo"]
    if not ids:
        del cur["object_id"]
    kw = dict(cur, demodulate=demodulate, **PARAMS)
    if history:
        kw.update(history=dict(f["history"], object_id=f["history"]["object_id"] if ids else None), prev_world_to_screen=f["prev_world_to_screen"],
                  prev_sample_offset=f["prev_sample_offset"])
    return kw


def model(w, h, demodulate, ids, history):
    """(history dict, motion) of the model: computed once, shared, never written"""
    key = (w, h, demodulate, ids, history)
    if key not in _models:
        out, motion, _, _ = ref.accumulate(**inputs(w, h, demodulate, ids, history))
        for a in [out[k] for k in OUTPUTS] + [motion]:
            a.setflags(write=False)
        _models[key] = (out, motion)
    return _models[key]


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    bad = np.argwhere(words(got) != words(want))
    assert len(bad) == 0, "%s: %d of %d words differ, first at %r: %r, the model has %r" % (
        what, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def assert_history(got, got_motion, want, want_motion, what):
    for k in OUTPUTS:
        assert_same(got[k], want[k], "%s, %s" % (what, k))
    assert_same(got_motion, want_motion, what + ", motion")


# ---- 1. the pure entry on random inputs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("demodulate", [True, False], ids=["demodulated", "plain"])
@pytest.mark.parametrize("w, h", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_the_pure_entry_equals_the_model(built, w, h, demodulate):
    for ids in (True, False):
        for history in (True, False):
            kw = inputs(w, h, demodulate, ids, history)
            want, want_motion = model(w, h, demodulate, ids, history)
            got, got_motion = ra.temporal_accumulate(return_motion=True, **kw)
            what = "%d x %d, ids %r, history %r" % (w, h, ids, history)
            assert_history(got, got_motion, want, want_motion, what)
            assert got["depth"] is not None and (got["object_id"] is None) == (not ids)
            if history and w * h > 500:
                assert (want["length"] > 1.0).mean() > 0.3 and (want["length"] == 1.0).mean() > 0.15 and want_motion.any()   # (it accumulates, and it starts)
            # outMotion == NULL: the same history
            alone = ra.temporal_accumulate(**kw)
            for k in OUTPUTS:
                assert_same(alone[k], want[k], what + ", no motion asked for, " + k)


def test_the_returned_history_goes_back_in(built):
    """three frames over the same guides through the wrapper's own dict, against the model's chain"""
    w, h = 37, 23
    kw = inputs(w, h, True, True, True)
    got, want = kw["history"], kw["history"]
    for _ in range(3):
        step = dict(kw, history=got)
        got = ra.temporal_accumulate(**step)
        want, _, _, _ = ref.accumulate(**dict(kw, history=want))
        for k in OUTPUTS:
            assert_same(got[k], want[k], k)
    assert want["length"].max() > 3.0


# ---- 2. device tensors on a stream of the caller's --------------------------------------------------------------------------------------------------
def test_tensors_on_a_side_stream_and_on_the_default_stream(built):
    import torch
    w, h = 130, 70
    cases = [(True, True, True), (False, False, True), (True, True, False)]

    def on_device(kw):
        t = {}
        for k, v in kw.items():
            if isinstance(v, np.ndarray) and k != "prev_world_to_screen":
                t[k] = torch.from_numpy(v.astype(np.int32) if v.dtype == np.uint32 else v).cuda()
            elif k == "history":
                t[k] = {name: None if a is None else torch.from_numpy(a.astype(np.int32) if a.dtype == np.uint32 else a).cuda() for name, a in v.items()}
            else:
                t[k] = v
        return t
    tensors = [on_device(inputs(w, h, *case)) for case in cases]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        on_side = [ra.temporal_accumulate(return_motion=True, **t) for t in tensors]   # the record scratch is shared: each ordered behind the one before
    on_default = ra.temporal_accumulate(return_motion=True, **tensors[0])   # torch's null stream: the wrapper's side stream
    stream.synchronize()
    for case, (got, motion) in zip(cases, on_side):
        assert got["a"].is_cuda and got["a"].dtype == torch.float32 and tuple(got["a"].shape) == (h, w, 3) and tuple(motion.shape) == (2, h, w)
        want, want_motion = model(w, h, *case)
        assert_history({k: got[k].cpu().numpy() for k in OUTPUTS}, motion.cpu().numpy(), want, want_motion, "side stream, %r" % (case,))
    want, want_motion = model(w, h, *cases[0])
    assert_history({k: on_default[0][k].cpu().numpy() for k in OUTPUTS}, on_default[1].cpu().numpy(), want, want_motion, "default stream")
    # ids as render_aovs(device=True) returns them: int64
    wide = dict(tensors[0], object_id=tensors[0]["object_id"].to(torch.int64), history=dict(tensors[0]["history"], object_id=tensors[0]["history"]["object_id"].to(torch.int64)))
    got = ra.temporal_accumulate(**wide)
    for k in OUTPUTS:
        assert_same(got[k].cpu().numpy(), want[k], "int64 ids, " + k)
    with pytest.raises(ValueError):
        ra.temporal_accumulate(**dict(tensors[0], depth=inputs(w, h, *cases[0])["depth"]))   # arrays and tensors mixed


# ---- 3. the accumulated pair through the filter: RT_DENOISE_INPUT_PREPARED ---------------------------------------------------------------------------
@pytest.mark.parametrize("w, h", [(37, 23), (130, 70)], ids=["37x23", "130x70"])
def test_the_prepared_filter_equals_the_model_and_the_plain_one_is_what_it_was(built, w, h):
    f = frame(w, h)["current"]
    for demodulate in (True, False):
        acc, _ = model(w, h, demodulate, True, True)
        for iterations in (1, 2, 5):
            want, want_v = ref.atrous_var_prepared(acc["a"], acc["b"], f["depth"], f["normal"], f["position"], f["albedo"] if demodulate else None, iterations=iterations,
                                                   demodulate=demodulate, **SIGMAS)
            got, got_v = ra.atrous_filter(acc["a"], f["depth"], f["normal"], f["position"], f["albedo"] if demodulate else None, iterations=iterations, demodulate=demodulate,
                                          color_half=acc["b"], return_variance=True, prepared=True, color_scale=0.125, **SIGMAS)   # (the scale is not applied)
            assert_same(got, want, "%d x %d, %d levels, demodulate %r" % (w, h, iterations, demodulate))
            assert_same(got_v, want_v, "%d x %d, %d levels, demodulate %r, variance" % (w, h, iterations, demodulate))
    # without the flag the filter is what the existing model says, on the existing frame
    g = denoise_var_ref.random_frame_var(37, 23, seed=1000 * 37 + 23)
    want, want_v = denoise_var_ref.atrous_var(iterations=5, color_scale=0.25, demodulate=True, **g, **SIGMAS)
    got, got_v = ra.atrous_filter(g["color"], g["depth"], g["normal"], g["position"], g["albedo"], iterations=5, color_scale=0.25, demodulate=True, color_half=g["color_half"],
                                  return_variance=True, **SIGMAS)
    assert_same(got, want, "the filter without the flag")
    assert_same(got_v, want_v, "the filter without the flag, variance")


# ---- 4. rendered frames ------------------------------------------------------------------------------------------------------------------------------
W, H = 64, 48
GUIDES = ("depth", "normal", "position", "base_color", "object_id")
# normals within 8 degrees: on a sphere eleven pixels in radius, a lone convex body that a 2 degree turn of the camera disoccludes nowhere, the pixels at the
# limb then find their reprojected neighbourhood turned away and start, as a disoccluded pixel does; the body of the sphere keeps its four taps
TEMPORAL = dict(normal_threshold=0.99)


def cameras():
    a = ra.Camera((0.0, 0.0, 6.0), (0.0, 180.0, 0.0), W / H, 40.0)
    b = ra.Camera((0.0, 0.0, 6.0), (0.0, 182.0, 0.0), W / H, 40.0)
    return a, b


def render_frame(vp, camera, passes=2):
    """`passes` passes of a fresh film; returns the params of the pass after them (the guides') and the read-backs the model chain starts from"""
    vp.reset()
    params = [vp.next_pass_params(camera) for _ in range(passes + 1)]
    for p in params[:passes]:
        vp.render_pass_with(p)
    s, s2 = vp.sum_buffer(secondary=True)
    return params[passes], dict(color=s, color_half=s2), vp.render_aovs(params[passes], GUIDES)


def model_step(sums, g, history, prev, demodulate=True, color_scale=0.5, **kw):
    return ref.accumulate(sums["color"], sums["color_half"], g["depth"], g["normal"], g["position"], g["base_color"] if demodulate else None, g["object_id"], history=history,
                          prev_world_to_screen=None if prev is None else list(prev.camera.worldToScreen), prev_sample_offset=(0.0, 0.0) if prev is None else tuple(prev.sampleOffset),
                          color_scale=color_scale, demodulate=demodulate, **kw)


def test_two_rendered_frames_equal_the_model_chain_and_the_calls_are_not_passes(built):
    scene, _ = scenes.sphere_area_light(W / H)
    cam_a, cam_b = cameras()
    vp = ra.Viewport(W, H, seed=4321, max_ray_depth=3)
    vp.set_renderer(scene)
    results, chain, history, prev = [], [], None, None
    for camera in (cam_a, cam_b):
        p, sums, g = render_frame(vp, camera)
        before = (vp.sum_buffer(secondary=True), vp.counters(), vp.passes_finished)
        results.append(vp.denoise(p, temporal=True, variance=True, return_variance=True, **TEMPORAL, **SIGMAS))
        after = (vp.sum_buffer(secondary=True), vp.counters(), vp.passes_finished)
        # film, both sum buffers and counters are unchanged by the call
        assert np.array_equal(words(before[0][0]), words(after[0][0])) and np.array_equal(words(before[0][1]), words(after[0][1])) and before[1:] == after[1:]
        assert np.array_equal(words(sums["color"]), words(after[0][0])) and after[2] == 2 and sums["color"].any() and sums["color_half"].any()
        history, motion, taken, why = model_step(sums, g, history, prev, **TEMPORAL)
        chain.append((ref.atrous_var_prepared(history["a"], history["b"], g["depth"], g["normal"], g["position"], g["base_color"], iterations=5, **SIGMAS), taken, why, g))
        prev = p
    for i, ((got, got_v), ((want, want_v), _, _, _)) in enumerate(zip(results, chain)):
        assert_same(got, want, "frame %d" % (i + 1))
        assert_same(got_v, want_v, "frame %d, variance" % (i + 1))
    _, taken, why, g = chain[1]
    valid = np.isfinite(g["depth"])
    assert valid.sum() > 300 and (~valid).sum() > 300
    assert (taken[valid] == 4).sum() * 3 >= valid.sum(), ((taken[valid] == 4).sum(), valid.sum())   # at least a third of the valid pixels take four taps
    assert (why == ref.START_NO_TAP).sum() >= 1                                                        # and at least one starts as a disoccluded pixel does
    assert not np.array_equal(words(results[0][0]), words(results[1][0]))


def test_the_device_entry_and_the_unfiltered_call_on_rendered_frames(built):
    """device=True on torch's stream gives the host call's bits; variance=False returns outA * d, and on the first call of a plain history sum_buffer() * color_scale"""
    scene, _ = scenes.sphere_area_light(W / H)
    cam_a, cam_b = cameras()
    twins = []
    for device in (False, True):
        vp = ra.Viewport(W, H, seed=4321, max_ray_depth=3)
        vp.set_renderer(scene)
        out = []
        for camera in (cam_a, cam_b):
            p, sums, g = render_frame(vp, camera)
            image, variance = vp.denoise(p, temporal=True, variance=True, return_variance=True, device=device, **TEMPORAL, **SIGMAS)
            out.append((image.cpu().numpy(), variance.cpu().numpy()) if device else (image, variance))
        twins.append(out)
    for (a, av), (b, bv) in zip(*twins):
        assert_same(b, a, "device=True")
        assert_same(bv, av, "device=True, variance")
    # no filter: the first call starts every pixel, the second blends
    vp = ra.Viewport(W, H, seed=4321, max_ray_depth=3)
    vp.set_renderer(scene)
    p, sums, g = render_frame(vp, cam_a)
    first = vp.denoise(p, temporal=True, variance=False, demodulate=False)
    assert_same(first, sums["color"] * np.float32(0.5), "the first call, plain: sum_buffer() * color_scale")
    history, _, _, _ = model_step(sums, g, None, None, demodulate=False)
    p2, sums2, g2 = render_frame(vp, cam_b)
    second = vp.denoise(p2, temporal=True, variance=False, demodulate=False)
    history2, _, _, why = model_step(sums2, g2, history, p, demodulate=False)
    assert_same(second, history2["a"], "the second call, plain")
    assert (why == ref.BLENDED).sum() > 100 and not np.array_equal(words(second), words(sums2["color"] * np.float32(0.5)))
    # demodulated and unfiltered: outA * d
    vp.reset_history()
    third = vp.denoise(p2, temporal=True, variance=False, demodulate=True)
    started, _, _, _ = model_step(sums2, g2, None, None, demodulate=True)
    assert_same(third, ref.remodulate(started["a"], g2["base_color"]), "unfiltered, demodulated")


# ---- 5. the convention on the device -------------------------------------------------------------------------------------------------------------------
def test_a_frame_reprojected_through_its_own_camera_does_not_move(built):
    """camera A without lens effects, sampleOffset 0: the POSITION plane accumulated against itself with A's worldToScreen.  Float rounding through the matrix
    and the scale by the frame size is of the order 1e-4 pixel; a half-pixel or a row-flip mistake gives 0.5 or more"""
    scene, _ = scenes.sphere_area_light(W / H)
    cam_a, _ = cameras()
    cam_a.set_dof(False)
    cam_a.set_lens(0, 0.0, 0.0)
    vp = ra.Viewport(W, H, seed=4321, max_ray_depth=3)
    vp.set_renderer(scene)
    p = vp.next_pass_params(cam_a)
    p.sampleOffset[0] = p.sampleOffset[1] = 0.0
    g = vp.render_aovs(p, ("depth", "normal", "position", "object_id"))
    valid = np.isfinite(g["depth"])
    assert valid.sum() > 300 and (~valid).sum() > 300
    color = np.ones((H, W, 3), dtype=np.float32)
    kw = dict(depth=g["depth"], normal=g["normal"], position=g["position"], object_id=g["object_id"], demodulate=False)
    first = ra.temporal_accumulate(color, color * np.float32(0.5), **kw)
    second, motion = ra.temporal_accumulate(color, color * np.float32(0.5), history=first, prev_world_to_screen=list(p.camera.worldToScreen), prev_sample_offset=(0.0, 0.0),
                                            return_motion=True, **kw)
    assert (second["length"][valid] > 1.5).all() and (second["length"][~valid] == 1.0).all()   # every hit found its history (so its motion is a measured one)
    assert np.abs(motion[:, valid]).max() < 0.01, np.abs(motion[:, valid]).max()
    assert not motion[:, ~valid].any()


# ---- 6. the history's lifetime ----------------------------------------------------------------------------------------------------------------------------
def test_what_keeps_and_what_drops_the_history(built):
    """the context-level call does not return lengths; with variance=False and demodulate=False a pixel that starts returns sum * color_scale to the bit, which
    is what a length of 1 means, and one that blends does not"""
    scene, _ = scenes.sphere_area_light(W / H)
    cam_a, cam_b = cameras()
    vp = ra.Viewport(W, H, seed=4321, max_ray_depth=3)
    vp.set_renderer(scene)
    lib, ctx = ra.rtgpu_lib(), vp.device_context()

    def frame_starts(camera, before=None):
        """runs `before`, renders a frame (vp.reset() inside: rtgpu_reset) and says whether every pixel of the call started"""
        if before:
            before()
        p, sums, g = render_frame(vp, camera)
        out = vp.denoise(p, temporal=True, variance=False, demodulate=False, color_scale=0.5)
        started = np.array_equal(words(out), words(sums["color"] * np.float32(0.5)))
        return started, out, sums, np.isfinite(g["depth"])
    assert frame_starts(cam_a)[0]                      # no history yet
    started, out, sums, valid = frame_starts(cam_b)    # rtgpu_reset in between keeps it: the second frame's lengths exceed 1
    assert not started and (words(out) != words(sums["color"] * np.float32(0.5))).any(axis=-1)[valid].mean() > 0.5
    assert frame_starts(cam_a, before=vp.reset_history)[0]                                   # rtgpu_temporal_reset
    assert not frame_starts(cam_b)[0]

    def resize():
        assert lib.rtgpu_resize(ctx, C.c_uint32(W), C.c_uint32(H)) == OK   # (the same size: the film is rebuilt, empty)
    assert frame_starts(cam_a, before=resize)[0]                                             # rtgpu_resize
    assert not frame_starts(cam_b)[0]

    def upload():
        assert lib.rtgpu_upload_scene(ctx, scene.desc) == OK
    assert frame_starts(cam_a, before=upload)[0]                                             # a second rtgpu_upload_scene
    assert not frame_starts(cam_b)[0]


# ---- 7. statuses through the raw ABI ------------------------------------------------------------------------------------------------------------------------
NAMES = ("color", "half", "depth", "normal", "position", "albedo", "id", "prev_a", "prev_b", "prev_length", "prev_depth", "prev_normal", "prev_position", "prev_id",
         "out_a", "out_b", "out_length", "out_motion")
PREVIOUS = NAMES[7:13]


def raw_accumulate(ctx, p, w, h, null=(), entry="rtgpu_temporal_accumulate", pointers=None):
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
        eye = np.eye(4, dtype=np.float32)
        good, plain = ra.temporal_params(prev_world_to_screen=eye), ra.temporal_params(prev_world_to_screen=eye, demodulate=False)
        dev = torch.zeros(41 * 64 + 4, dtype=torch.float32, device="cuda")
        at = lambda k: C.c_void_p(dev.data_ptr() + 64 * 4 * k)   # noqa: E731
        sizes = (3, 3, 1, 3, 3, 3, 1, 3, 3, 1, 1, 3, 3, 1, 3, 3, 1, 2)
        starts = dict(zip(NAMES, np.cumsum((0,) + sizes[:-1])))
        device_pointers = {name: at(int(k)) for name, k in starts.items()}
        for entry, pointers in (("rtgpu_temporal_accumulate", None), ("rtgpu_temporal_accumulate_async", device_pointers)):
            call = lambda p, w=4, h=4, null=(), extra=None: raw_accumulate(ctx, p, w, h, null, entry, dict(pointers or {}, **(extra or {})))   # noqa: E731
            assert call(good) == OK                                   # a pure image operation: no scene, no rtgpu_resize
            assert call(None) == INVALID_ARGUMENT
            for name in ("color", "half", "depth", "normal", "position", "albedo", "out_a", "out_b", "out_length"):
                assert call(good, null=(name,)) == INVALID_ARGUMENT, name
            assert call(good, null=("out_motion",)) == OK             # outMotion is optional
            assert call(plain, null=("albedo",)) == OK                # albedo may be NULL without RT_DENOISE_DEMODULATE
            assert call(good, null=PREVIOUS + ("prev_id",)) == OK     # no history
            assert call(good, null=PREVIOUS + ("prev_id", "id")) == OK
            for name in PREVIOUS:                                     # previous pointers only partly given
                assert call(good, null=(name,)) == INVALID_ARGUMENT, name
                assert call(good, null=tuple(k for k in PREVIOUS if k != name) + ("prev_id",)) == INVALID_ARGUMENT, name
            assert call(good, null=PREVIOUS) == INVALID_ARGUMENT      # the previous ids alone
            assert call(good, null=("id",)) == INVALID_ARGUMENT and call(good, null=("prev_id",)) == INVALID_ARGUMENT   # exactly one id plane
            assert call(good, null=("id", "prev_id")) == OK
            for field, values in (("alpha_min", (0.0, -0.5, 1.5)), ("max_history", (0.5, 0.0, -1.0)), ("normal_threshold", (-1.5, 1.5)), ("plane_tolerance", (0.0, -1.0)),
                                  ("color_scale", (0.0, -1.0))):
                for value in values + (float("inf"), float("nan")):
                    assert call(ra.temporal_params(prev_world_to_screen=eye, **{field: value})) == INVALID_ARGUMENT, (field, value)
            assert call(ra.temporal_params(prev_world_to_screen=eye, alpha_min=1.0, max_history=1.0, normal_threshold=-1.0)) == OK
            for value in (float("inf"), float("nan")):
                bad = eye.copy()
                bad[2, 1] = value
                assert call(ra.temporal_params(prev_world_to_screen=bad)) == INVALID_ARGUMENT
                assert call(ra.temporal_params(prev_world_to_screen=eye, prev_sample_offset=(0.0, value))) == INVALID_ARGUMENT
            assert call(good, w=0) == INVALID_ARGUMENT and call(good, h=0) == INVALID_ARGUMENT
            assert call(good, w=4097, h=4096) == UNSUPPORTED          # > 16 Mi pixels: refused before a buffer is read
            assert call(good, w=65536, h=65536) == UNSUPPORTED
        # the async entry: 16-byte aligned device memory, and outputs that overlap no input and no other output
        async_call = lambda **extra: raw_accumulate(ctx, good, 4, 4, (), "rtgpu_temporal_accumulate_async", dict(device_pointers, **extra))   # noqa: E731
        base = dev.data_ptr()
        for name in ("out_a", "out_length", "out_motion", "half", "prev_length", "id"):
            assert async_call(**{name: C.c_void_p(base + 64 * 4 * int(starts[name]) + 4)}) == INVALID_ARGUMENT, name
        assert async_call(out_a=C.c_void_p(base + 4 * 32)) == INVALID_ARGUMENT and b"overlap" in lib.rtgpu_last_error()                  # over the colour
        assert async_call(out_b=device_pointers["prev_b"]) == INVALID_ARGUMENT and b"overlap" in lib.rtgpu_last_error()                  # the history itself
        assert async_call(out_length=device_pointers["depth"]) == INVALID_ARGUMENT and b"overlap" in lib.rtgpu_last_error()
        assert async_call(out_motion=C.c_void_p(base + 64 * 4 * int(starts["out_a"]) + 4 * 32)) == INVALID_ARGUMENT and b"overlap" in lib.rtgpu_last_error()   # inside outA
        assert async_call(out_b=device_pointers["out_a"]) == INVALID_ARGUMENT and b"overlap" in lib.rtgpu_last_error()
        assert lib.rtgpu_synchronize(ctx) == OK
        torch.cuda.synchronize()
        # rtgpu_denoise_temporal before rtgpu_upload_scene, then before rtgpu_resize
        scene, camera = scenes.sphere_area_light(1.5)
        probe = ra.Viewport(48, 32, seed=1, max_ray_depth=2)
        pp = probe.next_pass_params(camera)
        out, var = np.ones((32, 48, 3), dtype=np.float32), np.ones((32, 48), dtype=np.float32)
        optr, vptr = out.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p)
        big = torch.zeros(48 * 32 * 4 + 8, dtype=torch.float32, device="cuda")
        dout, dvar = C.c_void_p(big.data_ptr()), C.c_void_p(big.data_ptr() + 48 * 32 * 3 * 4)
        t, v = ra.temporal_params(), ra.denoise_var_params()
        tref, vref, pref = C.byref(t), C.byref(v), C.byref(pp)
        assert lib.rtgpu_temporal_reset(ctx) == OK
        assert lib.rtgpu_denoise_temporal(ctx, tref, vref, pref, optr, vptr) == NOT_READY
        assert lib.rtgpu_denoise_temporal_async(ctx, tref, vref, pref, dout, dvar, None) == NOT_READY
        assert lib.rtgpu_upload_scene(ctx, scene.desc) == OK
        assert lib.rtgpu_denoise_temporal(ctx, tref, vref, pref, optr, vptr) == NOT_READY
        assert lib.rtgpu_resize(ctx, 48, 32) == OK
        assert lib.rtgpu_denoise_temporal(ctx, tref, vref, pref, optr, vptr) == OK   # (an empty film: zeros in, zeros out)
        assert not out.any() and not var.any()
        assert lib.rtgpu_denoise_temporal(ctx, tref, vref, pref, optr, None) == OK
        assert lib.rtgpu_denoise_temporal(ctx, tref, None, pref, optr, None) == OK   # no spatial filter
        assert lib.rtgpu_denoise_temporal_async(ctx, tref, vref, pref, dout, dvar, None) == OK
        assert lib.rtgpu_denoise_temporal_async(ctx, tref, None, pref, dout, None, None) == OK
        assert lib.rtgpu_synchronize(ctx) == OK
        assert lib.rtgpu_denoise_temporal(ctx, None, vref, pref, optr, vptr) == INVALID_ARGUMENT and lib.rtgpu_denoise_temporal(ctx, tref, vref, None, optr, vptr) == INVALID_ARGUMENT
        assert lib.rtgpu_denoise_temporal(ctx, tref, vref, pref, None, vptr) == INVALID_ARGUMENT
        assert lib.rtgpu_denoise_temporal(ctx, C.byref(ra.temporal_params(alpha_min=0.0)), vref, pref, optr, vptr) == INVALID_ARGUMENT
        assert lib.rtgpu_denoise_temporal(ctx, C.byref(ra.temporal_params(max_history=float("nan"))), vref, pref, optr, vptr) == INVALID_ARGUMENT
        assert lib.rtgpu_denoise_temporal(ctx, tref, C.byref(ra.denoise_var_params(iterations=0)), pref, optr, vptr) == INVALID_ARGUMENT
        nan_camera = ra.temporal_params(prev_world_to_screen=np.full((4, 4), np.nan, dtype=np.float32))
        assert lib.rtgpu_denoise_temporal(ctx, C.byref(nan_camera), vref, pref, optr, vptr) == OK   # the context remembers its own
        assert lib.rtgpu_denoise_temporal_async(ctx, tref, vref, pref, C.c_void_p(big.data_ptr() + 4), dvar, None) == INVALID_ARGUMENT
        assert lib.rtgpu_denoise_temporal_async(ctx, tref, vref, pref, dout, C.c_void_p(big.data_ptr() + 64), None) == INVALID_ARGUMENT and b"overlap" in lib.rtgpu_last_error()
        # what rtgpu_render_aovs refuses in the guide params gets the status it gets there
        deep = ra.RtPassParams.from_buffer_copy(pp)
        deep.maxRayDepth = 255
        assert lib.rtgpu_denoise_temporal(ctx, tref, vref, C.byref(deep), optr, vptr) == INVALID_ARGUMENT
        assert lib.rtgpu_synchronize(ctx) == OK
    finally:
        lib.rtgpu_destroy(ctx)
