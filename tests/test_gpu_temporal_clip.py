"""History clipping on the device (rtgpu_temporal_accumulate_clip, rtgpu_denoise_temporal_clip and their _async twins; raytracer_amd.temporal_accumulate(clip=...),
Viewport.denoise(temporal=True, clip=...)) against its NumPy float32 model (tests/temporal_clip_ref.py).

Bar and helpers: those of tests/test_gpu_temporal.py -- BIT-EQUAL words in outA, outB, outLength, outMotion and outConfidence, no pixel left out.  The operation
is defined step by step (include/rtgpu.h), the model performs those steps in that order in IEEE float32, and the device library is compiled without contraction:
there is no tolerance to state.  The model's own properties: tests/test_temporal_clip_model.py.

The shapes are the tile's: a frame smaller than the window, exactly one 32 x 8 tile, one pixel over in both directions, the two degenerate strips, and several
tiles both ways.  Every shape, radius and variant runs under two settings:
  CLIP   gamma 1, min_count 9.  A pixel at radius 1 then clips only where its whole 3 x 3 window lies on its surface, which the random frames (a quarter of their
         pixels planted off the surface one way or another) grant 1 to 5 % of them, and on the one-row strip no window holds nine pixels at all; at radius 2 and 3,
         10 to 70 % clip.  Over the three radii of a frame of more than 500 pixels together a tenth clips and a tenth does not, and every radius clips some.
  DENSE  gamma 0.5, min_count 2: a count every shape but the single pixel reaches at every radius, so that the moment records reach the outputs everywhere -- the
         strips, the frame smaller than the window, the single tile.  Asserted per shape, radius and variant: a pixel clips; and wherever a tenth of the frame CAN
         clip (it blends, with min_count pixels of its surface in the window), a tenth does and a tenth does not.  (The strip under the motion table is the one
         case that cannot: its objects' motions carry all but two pixels of a one-row history off the frame.  Those two clip.)"""
import ctypes as C

import numpy as np
import pytest

import raytracer_amd as ra
import temporal_clip_ref as cref
import temporal_moving_ref as mref
import temporal_ref as ref
from test_gpu_temporal import OK, INVALID_ARGUMENT, PARAMS, OUTPUTS, NAMES, assert_history, assert_same, words
from test_gpu_temporal_moving import FRAMES, MOVED, W, H, camera_of, sphere_at, object_tables, render_frame

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 5), (32, 8), (33, 9), (70, 1), (3, 200), (67, 29)]
CLIP = dict(gamma=1.0, min_count=9)
DENSE = dict(gamma=0.5, min_count=2)
VARIANTS = [("table", True, True), ("static", False, True), ("static, no ids", False, False)]   # (label, the motion table, the id planes)

_frames = {}
_models = {}


def frame(w, h):
    if (w, h) not in _frames:
        _frames[w, h] = mref.random_moving_frame(w, h, seed=1000 * w + h, num_objects=3 + (w + h) % 3)
    return _frames[w, h]


def inputs(w, h, demodulate, table=True, ids=True):
    """the keyword arguments model and device take alike: the moving frame with its table, or the frame it was made from without one"""
    f = frame(w, h) if table else frame(w, h)["base"]
    cur, history = dict(f["current"]), dict(f["history"])
    if not demodulate:
        del cur["albedo"]
    if not ids:
        del cur["object_id"]
        history["object_id"] = None
    kw = dict(cur, demodulate=demodulate, history=history, prev_world_to_screen=f["prev_world_to_screen"], prev_sample_offset=f["prev_sample_offset"], **PARAMS)
    if table:
        kw["object_motion"] = f["object_motion"]
    return kw


def model(w, h, demodulate, table, ids, radius, gamma=CLIP["gamma"], min_count=CLIP["min_count"]):
    key = (w, h, demodulate, table, ids, radius, gamma, min_count)
    if key not in _models:
        out, motion, _, why, info = cref.accumulate_clip(clip=dict(radius=radius, gamma=gamma, min_count=min_count), **inputs(w, h, demodulate, table, ids))
        for a in [out[k] for k in OUTPUTS] + [motion, info["f"]]:
            a.setflags(write=False)
        _models[key] = (out, motion, why, info)
    return _models[key]


# ---- a. the pure entry on random inputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("demodulate", [True, False], ids=["demodulated", "plain"])
@pytest.mark.parametrize("w, h", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_the_pure_entry_equals_the_model(built, w, h, demodulate):
    for label, table, ids in VARIANTS:
        clipped = not_clipped = pixels = 0
        for radius in (1, 2, 3):
            kw = inputs(w, h, demodulate, table, ids)
            want, want_motion, why, info = model(w, h, demodulate, table, ids, radius)
            got, got_motion, got_confidence = ra.temporal_accumulate(return_motion=True, return_confidence=True, clip=dict(CLIP, radius=radius), **kw)
            what = "%d x %d, %s, radius %d" % (w, h, label, radius)
            assert_history(got, got_motion, want, want_motion, what)
            assert_same(got_confidence, info["f"], what + ", confidence")
            clipped, not_clipped, pixels = clipped + int(info["clipped"].sum()), not_clipped + int((~info["clipped"]).sum()), pixels + w * h
            if w * h > 500:
                assert info["clipped"].sum() >= 5 and (~info["clipped"]).sum() >= 5, what
            # DENSE: the moment records reach the outputs at every shape and radius
            want, want_motion, why, info = model(w, h, demodulate, table, ids, radius, **DENSE)
            got, got_motion, got_confidence = ra.temporal_accumulate(return_motion=True, return_confidence=True, clip=dict(DENSE, radius=radius), **kw)
            assert_history(got, got_motion, want, want_motion, what + ", dense")
            assert_same(got_confidence, info["f"], what + ", dense, confidence")
            can_clip = int(((why == ref.BLENDED) & (info["cnt"] >= DENSE["min_count"])).sum())
            does, does_not = int(info["clipped"].sum()), int((~info["clipped"]).sum())
            if w * h > 1:
                assert does > 0, what
            if can_clip * 10 >= w * h:
                assert does * 10 >= w * h and does_not * 10 >= w * h, (what, does, does_not)
            else:
                assert (w, h) == (1, 1) or ((w, h) == (70, 1) and table), what      # (the only frames that cannot)
        if w * h > 500:
            assert clipped * 10 >= pixels and not_clipped * 10 >= pixels, (label, clipped, not_clipped, pixels)
    # outMotion and outConfidence are optional: the same history without them
    kw = inputs(w, h, demodulate)
    alone = ra.temporal_accumulate(clip=dict(CLIP, radius=2), **kw)
    for k in OUTPUTS:
        assert_same(alone[k], model(w, h, demodulate, True, True, 2)[0][k], "no motion and no confidence asked for, " + k)
    # without a history every pixel starts with confidence 1
    started, confidence = ra.temporal_accumulate(clip=dict(CLIP, radius=3), return_confidence=True,
                                                 **{k: v for k, v in kw.items() if k not in ("history", "prev_world_to_screen", "prev_sample_offset")})
    assert (started["length"] == 1.0).all() and (confidence == 1.0).all()


# ---- b. where nothing clips it is the call without ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w, h", [(33, 9), (67, 29)], ids=["33x9", "67x29"])
def test_a_box_nothing_reaches_gives_the_words_of_the_call_without(built, w, h):
    for label, table, ids in VARIANTS:
        kw = inputs(w, h, True, table, ids)
        plain, plain_motion = ra.temporal_accumulate(return_motion=True, **kw)
        for radius in (1, 3):
            assert not model(w, h, True, table, ids, radius, gamma=1e4)[3]["clipped"].any()
            got, motion, confidence = ra.temporal_accumulate(return_motion=True, return_confidence=True, clip=dict(radius=radius, gamma=1e4, min_count=2), **kw)
            assert_history(got, motion, plain, plain_motion, "%s, radius %d" % (label, radius))
            assert (words(confidence) == words(np.float32(1.0))).all()
        assert (plain["length"] > 1.0).mean() > 0.3


# ---- c. a chain, on arrays and on tensors -----------------------------------------------------------------------------------------------------------
def on_device(torch, kw):
    t = {}
    for k, v in kw.items():
        if isinstance(v, np.ndarray) and k != "prev_world_to_screen":
            t[k] = torch.from_numpy(v.astype(np.int32) if v.dtype == np.uint32 else v).cuda()
        elif k == "history":
            t[k] = {name: None if a is None else torch.from_numpy(a.astype(np.int32) if a.dtype == np.uint32 else a).cuda() for name, a in v.items()}
        else:
            t[k] = v     # (the table stays NumPy: the wrapper takes it to the device)
    return t


def test_the_returned_history_goes_back_in_on_tensors_and_on_both_streams(built):
    """three frames over the same guides and the same motion, the returned history going back in: the model's chain once; the device's on a side stream and on
    torch's default stream (the wrapper's own side stream)"""
    import torch
    w, h = 67, 29
    kw = inputs(w, h, True)
    matrices, prev_ids, moved = kw["object_motion"]
    clip = dict(CLIP, radius=3)
    want, chain = kw["history"], []
    for step in range(3):
        table = (matrices, prev_ids if step == 0 else np.arange(len(prev_ids)), moved)
        want, motion, _, _, info = cref.accumulate_clip(**dict(kw, history=want, object_motion=table, clip=clip))
        chain.append((want, motion, info))
    assert all(info["clipped"].sum() >= 10 for _, _, info in chain) and chain[2][0]["length"].max() > 2.0
    tensors = on_device(torch, kw)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for label, stream in (("side stream", side), ("default stream", torch.cuda.default_stream())):
        with torch.cuda.stream(stream):
            got = tensors["history"]
            results = []
            for step in range(3):
                table = (matrices, prev_ids if step == 0 else np.arange(len(prev_ids)), moved)
                got, motion, confidence = ra.temporal_accumulate(**dict(tensors, history=got, object_motion=table, clip=clip, return_motion=True, return_confidence=True))
                results.append((got, motion, confidence))
        stream.synchronize()
        for step, ((got, motion, confidence), (want, want_motion, info)) in enumerate(zip(results, chain)):
            assert got["a"].is_cuda and tuple(confidence.shape) == (h, w)
            assert_history({k: got[k].cpu().numpy() for k in OUTPUTS}, motion.cpu().numpy(), want, want_motion, "%s, step %d" % (label, step))
            assert_same(confidence.cpu().numpy(), info["f"], "%s, step %d, confidence" % (label, step))


# ---- d. statuses through the raw ABI ----------------------------------------------------------------------------------------------------------------------
def raw_clip(ctx, p, w, h, table, count, clip, confidence, null=(), entry="rtgpu_temporal_accumulate_clip", pointers=None):
    n = max(1, min(w * h, 4096))
    keep = {name: np.zeros(3 * n, dtype=np.float32) for name in NAMES}
    ptr = {name: a.ctypes.data_as(C.c_void_p) for name, a in keep.items()}
    ptr.update(pointers or {})
    ptr.update({name: None for name in null})
    args = (ctx, C.byref(p) if p is not None else None, C.c_uint32(w), C.c_uint32(h)) + tuple(ptr[name] for name in NAMES) + (
        table, C.c_uint32(count), C.byref(clip) if clip is not None else None, confidence)
    if entry.endswith("_async"):
        args += (None,)
    return getattr(ra.rtgpu_lib(), entry)(*args)


def clip_of(radius=3, gamma=2.0, min_count=9):
    return ra.temporal_clip(dict(radius=radius, gamma=gamma, min_count=min_count))


def test_statuses(built):
    import torch
    from raytracer_amd import scenes
    lib = ra.rtgpu_lib()
    ctx = C.c_void_p()
    assert lib.rtgpu_create(0, C.byref(ctx)) == OK
    try:
        eye = np.eye(4, dtype=np.float32)
        good = ra.temporal_params(prev_world_to_screen=eye)
        host_table = ra.object_motion_table((np.stack([eye, eye]), [0, 1], [0, 1]))
        host_confidence = np.zeros(64, dtype=np.float32)
        dev = torch.zeros(43 * 64 + 4 + 64, dtype=torch.float32, device="cuda")
        at = lambda k: C.c_void_p(dev.data_ptr() + 64 * 4 * k)   # noqa: E731
        sizes = (3, 3, 1, 3, 3, 3, 1, 3, 3, 1, 1, 3, 3, 1, 3, 3, 1, 2)
        starts = dict(zip(NAMES, np.cumsum((0,) + sizes[:-1])))
        device_pointers = {name: at(int(k)) for name, k in starts.items()}
        device_table, device_confidence = at(41), at(42)
        for entry, pointers, table, confidence in (("rtgpu_temporal_accumulate_clip", None, host_table.ctypes.data_as(C.c_void_p), host_confidence.ctypes.data_as(C.c_void_p)),
                                                   ("rtgpu_temporal_accumulate_clip_async", device_pointers, device_table, device_confidence)):
            call = lambda clip, p=good, null=(), t=table, count=2, f=confidence: raw_clip(ctx, p, 4, 4, t, count, clip, f, null, entry, pointers)   # noqa: E731
            assert call(clip_of()) == OK
            assert call(clip_of(), f=None) == OK                                          # outConfidence is optional
            assert call(clip_of(), t=None, count=0) == OK                                 # no table: no object moved
            assert call(clip_of(), t=None, count=0, null=("id", "prev_id")) == OK         # ... and then the ids are optional, as for the static call
            assert call(clip_of(1, 0.0, 1)) == OK and call(clip_of(3, 1e6, 49)) == OK     # the ends of the ranges
            assert call(None) == INVALID_ARGUMENT and b"clip" in lib.rtgpu_last_error()   # clip NULL on the pure entry
            for bad in (clip_of(radius=0), clip_of(radius=4), clip_of(min_count=0), clip_of(min_count=50), clip_of(gamma=-1.0), clip_of(gamma=float("nan")),
                        clip_of(gamma=float("inf")), clip_of(gamma=2e6)):
                assert call(bad) == INVALID_ARGUMENT, (bad.radius, bad.gamma, bad.minCount)
            # as the _moving entry
            assert call(clip_of(), p=None) == INVALID_ARGUMENT
            assert call(clip_of(), t=None) == INVALID_ARGUMENT and call(clip_of(), count=0) == INVALID_ARGUMENT     # half a table
            assert call(clip_of(), null=("id",)) == INVALID_ARGUMENT and call(clip_of(), null=("prev_id",)) == INVALID_ARGUMENT
            assert call(clip_of(), null=("color",)) == INVALID_ARGUMENT and call(clip_of(), null=("out_a",)) == INVALID_ARGUMENT
            assert call(clip_of(), null=("prev_a",)) == INVALID_ARGUMENT
            assert call(clip_of(), p=ra.temporal_params(prev_world_to_screen=eye, alpha_min=0.0)) == INVALID_ARGUMENT
        # the async entry: the confidence plane aligned, and apart from every input and output
        async_call = lambda f: raw_clip(ctx, good, 4, 4, device_table, 2, clip_of(), f, (), "rtgpu_temporal_accumulate_clip_async", device_pointers)   # noqa: E731
        assert async_call(C.c_void_p(dev.data_ptr() + 64 * 4 * 42 + 4)) == INVALID_ARGUMENT and b"aligned" in lib.rtgpu_last_error()
        for name in ("color", "prev_length", "out_a", "out_motion"):
            assert async_call(device_pointers[name]) == INVALID_ARGUMENT and b"overlap" in lib.rtgpu_last_error(), name
        assert async_call(C.c_void_p(dev.data_ptr() + 64 * 4 * int(starts["out_b"]) + 4 * 32)) == INVALID_ARGUMENT and b"overlap" in lib.rtgpu_last_error()   # inside outB
        assert lib.rtgpu_synchronize(ctx) == OK
        torch.cuda.synchronize()
        # the context calls
        scene, camera = scenes.sphere_area_light(1.5)
        probe = ra.Viewport(48, 32, seed=1, max_ray_depth=2)
        pp = probe.next_pass_params(camera)
        out, var, conf = np.ones((32, 48, 3), dtype=np.float32), np.ones((32, 48), dtype=np.float32), np.zeros((32, 48), dtype=np.float32)
        optr, vptr, cptr = (a.ctypes.data_as(C.c_void_p) for a in (out, var, conf))
        big = torch.zeros(48 * 32 * 5 + 8, dtype=torch.float32, device="cuda")
        dout, dvar, dconf = C.c_void_p(big.data_ptr()), C.c_void_p(big.data_ptr() + 48 * 32 * 3 * 4), C.c_void_p(big.data_ptr() + 48 * 32 * 4 * 4)
        t, v, clip = ra.temporal_params(), ra.denoise_var_params(), clip_of()
        tref, vref, pref, cref_ = C.byref(t), C.byref(v), C.byref(pp), C.byref(clip)
        assert lib.rtgpu_upload_scene(ctx, scene.desc) == OK and lib.rtgpu_resize(ctx, 48, 32) == OK
        assert lib.rtgpu_denoise_temporal_clip(ctx, tref, vref, pref, optr, vptr, cref_, cptr) == OK      # an empty film: zeros in, zeros out; every pixel starts
        assert not out.any() and (conf == 1.0).all()
        conf[:] = 0.0
        assert lib.rtgpu_denoise_temporal_clip(ctx, tref, None, pref, optr, None, cref_, cptr) == OK and (conf == 1.0).all()   # (a history of zeros under zeros: nothing to pull)
        assert lib.rtgpu_denoise_temporal_clip(ctx, tref, vref, pref, optr, vptr, cref_, None) == OK
        conf[:] = 7.0
        assert lib.rtgpu_denoise_temporal_clip(ctx, tref, vref, pref, optr, vptr, None, cptr) == OK and (conf == 7.0).all()    # clip NULL: the call without; nothing written
        assert lib.rtgpu_denoise_temporal_clip_async(ctx, tref, vref, pref, dout, dvar, cref_, dconf, None) == OK
        assert lib.rtgpu_denoise_temporal_clip_async(ctx, tref, None, pref, dout, None, None, None, None) == OK
        assert lib.rtgpu_synchronize(ctx) == OK
        for bad in (clip_of(radius=0), clip_of(radius=4), clip_of(min_count=0), clip_of(min_count=50), clip_of(gamma=-1.0), clip_of(gamma=float("nan")), clip_of(gamma=float("inf"))):
            assert lib.rtgpu_denoise_temporal_clip(ctx, tref, vref, pref, optr, vptr, C.byref(bad), cptr) == INVALID_ARGUMENT
            assert lib.rtgpu_denoise_temporal_clip_async(ctx, tref, vref, pref, dout, dvar, C.byref(bad), dconf, None) == INVALID_ARGUMENT
        assert lib.rtgpu_denoise_temporal_clip(ctx, None, vref, pref, optr, vptr, cref_, cptr) == INVALID_ARGUMENT
        assert lib.rtgpu_denoise_temporal_clip(ctx, tref, vref, pref, None, vptr, cref_, cptr) == INVALID_ARGUMENT
        assert lib.rtgpu_denoise_temporal_clip_async(ctx, tref, vref, pref, dout, dvar, cref_, C.c_void_p(big.data_ptr() + 48 * 32 * 4 * 4 + 4), None) == INVALID_ARGUMENT
        assert lib.rtgpu_denoise_temporal_clip_async(ctx, tref, vref, pref, dout, dvar, cref_, C.c_void_p(big.data_ptr() + 64), None) == INVALID_ARGUMENT and b"overlap" in lib.rtgpu_last_error()
        assert lib.rtgpu_denoise_temporal_clip_async(ctx, tref, vref, pref, dout, dvar, cref_, dvar, None) == INVALID_ARGUMENT and b"overlap" in lib.rtgpu_last_error()
        assert lib.rtgpu_synchronize(ctx) == OK
        with pytest.raises(ValueError, match="clip"):
            ra.temporal_clip(dict(sigma=2.0))
        with pytest.raises(ValueError, match="return_confidence"):
            color = np.zeros((4, 4, 3), dtype=np.float32)
            ra.temporal_accumulate(color, color, np.zeros((4, 4), dtype=np.float32), np.zeros((3, 4, 4), dtype=np.float32), np.zeros((3, 4, 4), dtype=np.float32), demodulate=False,
                                   return_confidence=True)
    finally:
        lib.rtgpu_destroy(ctx)


# ---- e. through the context: rendered frames under a directional light, the sphere moved and the camera yawed between them -----------------------------------
SIGMAS = dict(sigma_lum=3.0, sigma_normal=0.5, sigma_plane=0.15)
CONTEXT_CLIP = dict(radius=3, gamma=1.0, min_count=9)


def stage():
    """the stage of the moving-objects test under a sun: the sphere's hard shadow slides over the floor with it"""
    s = ra.Scene()
    grey = s.add_material("diffuse", (0.7, 0.7, 0.7))
    red = s.add_material("diffuse", (0.8, 0.2, 0.1))
    blue = s.add_material("roughPlastic", (0.1, 0.3, 0.8), roughness=0.4)
    s.add_rect((6.0, 6.0), ra.transform_from_euler((0.0, -1.0, 0.0), (-90.0, 0.0, 0.0)), grey)
    s.add_sphere(0.9, ra.transform_from_euler((-1.2, -0.1, 0.0)), red)
    s.add_box((0.6, 0.8, 0.6), ra.transform_from_euler((1.4, -0.2, -0.5), (0.0, 25.0, 0.0)), blue)
    s.add_background_light((0.3, 0.4, 0.5))
    s.add_directional_light((3000.0, 2900.0, 2800.0), 0.02, ra.transform_from_euler((0.0, 0.0, 0.0), (70.0, 30.0, 0.0)))
    s.build()
    return s


def run_chain(clip, variance, check=None, return_confidence=False):
    """FRAMES frames of a fresh viewport; before each but the first the camera yaws and the sphere moves (Scene.update() / Viewport.update_scene()).  Returns
    what Viewport.denoise(temporal=True, clip=clip) returned per frame; check(k, ...): per frame"""
    scene = stage()
    vp = ra.Viewport(W, H, seed=2468, max_ray_depth=3)
    vp.set_renderer(scene)
    results = []
    for k in range(FRAMES):
        if k:
            scene.set_object_transform(MOVED, sphere_at(k))
            scene.update()
            vp.update_scene()
        p, sums, g = render_frame(vp, camera_of(k))
        before = (vp.sum_buffer(secondary=True), vp.counters(), vp.passes_finished)
        extra = dict(return_confidence=True) if return_confidence else {}
        results.append(vp.denoise(p, temporal=True, variance=variance, clip=clip, **(SIGMAS if variance else {}), **extra))
        after = (vp.sum_buffer(secondary=True), vp.counters(), vp.passes_finished)
        # film, both sum buffers, counters and the pass count are unchanged by the call, and no pass is left queued
        assert np.array_equal(words(before[0][0]), words(after[0][0])) and np.array_equal(words(before[0][1]), words(after[0][1])) and before[1:] == after[1:]
        assert after[2] == 2
        if check:
            check(k, scene, p, sums, g, results[-1])
    return results


@pytest.mark.parametrize("variance", [True, False], ids=["filtered", "filter=None"])
def test_the_context_call_is_the_composition_of_aovs_table_builder_and_model(built, variance):
    state = dict(history=None, prev=None, then=None, clipped=[])

    def check(k, scene, p, sums, g, result):
        image, confidence = result
        now, inverse = object_tables(scene)
        kw = dict(color=sums["color"], color_half=sums["color_half"], depth=g["depth"], normal=g["normal"], position=g["position"], albedo=g["base_color"],
                  object_id=g["object_id"], history=state["history"], color_scale=0.5, clip=CONTEXT_CLIP)
        if state["history"] is not None:
            # (no update reorders this scene's objects: every object keeps its index)
            table = mref.motion_table(now, inverse, state["then"], np.arange(len(now), dtype=np.uint32))
            assert table[2].sum() == 1
            kw.update(prev_world_to_screen=list(state["prev"].camera.worldToScreen), prev_sample_offset=tuple(state["prev"].sampleOffset), object_motion=table)
        history, _, _, _, info = cref.accumulate_clip(**kw)
        state["clipped"].append(int(info["clipped"].sum()))
        if variance:
            want, _ = ref.atrous_var_prepared(history["a"], history["b"], g["depth"], g["normal"], g["position"], g["base_color"], iterations=5, **SIGMAS)
        else:
            want = ref.remodulate(history["a"], g["base_color"])
        assert_same(image, want, "frame %d" % k)
        assert_same(confidence, info["f"], "frame %d, confidence" % k)
        state.update(history=history, prev=p, then=now)

    results = run_chain(CONTEXT_CLIP, variance, check, return_confidence=True)
    assert len(results) == FRAMES
    print("clipped pixels per frame, by the model: %r" % state["clipped"])
    assert state["clipped"][0] == 0 and min(state["clipped"][1:]) > 50, state["clipped"]


def test_clip_none_is_the_call_without_word_for_word(built):
    for variance in (True, False):
        twins = []
        for use_clip_entry in (False, True):
            scene = stage()
            vp = ra.Viewport(W, H, seed=2468, max_ray_depth=3)
            vp.set_renderer(scene)
            lib, ctx = ra.rtgpu_lib(), vp.device_context()
            images = []
            for k in range(FRAMES):
                if k:
                    scene.set_object_transform(MOVED, sphere_at(k))
                    scene.update()
                    vp.update_scene()
                p, _, _ = render_frame(vp, camera_of(k))
                if not use_clip_entry:
                    images.append(vp.denoise(p, temporal=True, variance=variance, **(SIGMAS if variance else {})))
                    continue
                # rtgpu_denoise_temporal_clip with clip == NULL, through the raw entry (the wrapper calls the entry without for clip=None)
                t = ra.temporal_params(color_scale=0.5)
                v = ra.denoise_var_params(5, SIGMAS["sigma_lum"], SIGMAS["sigma_normal"], SIGMAS["sigma_plane"], ra.DENOISE_VAR_DEFAULTS["variance_floor"], 1.0, True)
                out = np.zeros((H, W, 3), dtype=np.float32)
                assert lib.rtgpu_denoise_temporal_clip(ctx, C.byref(t), C.byref(v) if variance else None, C.byref(p), out.ctypes.data_as(C.c_void_p), None, None, None) == OK
                images.append(out)
            twins.append(images)
        for k, (a, b) in enumerate(zip(*twins)):
            assert_same(b, a, "variance %r, frame %d" % (variance, k))
        assert not np.array_equal(words(twins[0][1]), words(twins[0][2]))
        # ... and the wrapper's clip=None is that call
        for k, (a, b) in enumerate(zip(twins[0], run_chain(None, variance))):
            assert_same(b, a, "clip=None, variance %r, frame %d" % (variance, k))
