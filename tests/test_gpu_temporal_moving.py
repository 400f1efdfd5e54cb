"""Temporal accumulation that follows moving objects on the device (rtgpu_temporal_accumulate_moving and its _async twin; raytracer_amd.temporal_accumulate with
object_motion; Viewport.denoise(temporal=True) after Viewport.update_scene()) against its NumPy float32 model (tests/temporal_moving_ref.py).

Bar and helpers: those of tests/test_gpu_temporal.py -- BIT-EQUAL words in outA, outB, outLength and outMotion.  The operation is defined step by step
(include/rtgpu.h), the model performs those steps in that order in IEEE float32, the table builder's doubles have one result, and the device library is
compiled without contraction: there is no tolerance to state.  What the random frames cover is asserted by tests/test_temporal_moving_model.py."""
import ctypes as C

import numpy as np
import pytest

import raytracer_amd as ra
import temporal_moving_ref as mref
import temporal_ref as ref
import update_scenes as us
from test_gpu_temporal import OK, INVALID_ARGUMENT, UNSUPPORTED, SHAPES, PARAMS, OUTPUTS, NAMES, PREVIOUS, assert_history, assert_same, words

pytestmark = pytest.mark.gpu

_frames = {}
_models = {}


def frame(w, h):
    if (w, h) not in _frames:
        _frames[w, h] = mref.random_moving_frame(w, h, seed=1000 * w + h, num_objects=3 + (w + h) % 3)
    return _frames[w, h]


def inputs(w, h, demodulate):
    f = frame(w, h)
    cur = dict(f["current"])
    if not demodulate:
        del cur["albedo"]
    return dict(cur, demodulate=demodulate, history=f["history"], prev_world_to_screen=f["prev_world_to_screen"], prev_sample_offset=f["prev_sample_offset"],
                object_motion=f["object_motion"], **PARAMS)


def model(w, h, demodulate):
    key = (w, h, demodulate)
    if key not in _models:
        out, motion, _, why = mref.accumulate_moving(**inputs(w, h, demodulate))
        for a in [out[k] for k in OUTPUTS] + [motion]:
            a.setflags(write=False)
        _models[key] = (out, motion, why)
    return _models[key]


# ---- 1. the pure entry on random inputs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("demodulate", [True, False], ids=["demodulated", "plain"])
@pytest.mark.parametrize("w, h", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_the_pure_entry_equals_the_model(built, w, h, demodulate):
    kw = inputs(w, h, demodulate)
    want, want_motion, why = model(w, h, demodulate)
    got, got_motion = ra.temporal_accumulate(return_motion=True, **kw)
    what = "%d x %d" % (w, h)
    assert_history(got, got_motion, want, want_motion, what)
    # the returned history holds the CURRENT guides and ids
    for key in ("normal", "position", "object_id"):
        assert np.array_equal(words(got[key]), words(kw[key])), key
    if w * h > 500:
        moving = frame(w, h)["planted"]["moving"]
        assert (why == ref.BLENDED)[moving].mean() > 0.3 and (why != ref.BLENDED)[moving].mean() > 0.15 and want_motion.any()
        # and it is not the static call: that one finds the moved surfaces nowhere
        static = ra.temporal_accumulate(**{k: v for k, v in kw.items() if k != "object_motion"})
        assert (static["length"][moving] > 1.0).mean() < 0.5 * (want["length"][moving] > 1.0).mean()
    alone = ra.temporal_accumulate(**kw)      # outMotion == NULL: the same history
    for k in OUTPUTS:
        assert_same(alone[k], want[k], what + ", no motion asked for, " + k)
    # without a history every pixel starts, table or not
    started = ra.temporal_accumulate(**{k: v for k, v in kw.items() if k not in ("history", "prev_world_to_screen", "prev_sample_offset")})
    assert (started["length"] == 1.0).all()


def test_a_table_of_unmoved_objects_gives_the_static_call_s_words(built):
    w, h = 130, 70
    base = ref.random_temporal_frame(w, h, seed=1000 * w + h)
    kw = dict(base["current"], history=base["history"], prev_world_to_screen=base["prev_world_to_screen"], prev_sample_offset=base["prev_sample_offset"], **PARAMS)
    n = 10
    rubbish = np.random.default_rng(1).normal(size=(n, 4, 4)).astype(np.float32)
    rubbish[2, 1, 1] = np.nan
    static, static_motion = ra.temporal_accumulate(return_motion=True, **kw)
    moving, moving_motion = ra.temporal_accumulate(return_motion=True, object_motion=(rubbish, np.arange(n), np.zeros(n)), **kw)
    assert_history(moving, moving_motion, static, static_motion, "moved = 0")
    assert (static["length"] > 1.0).mean() > 0.3


def test_the_returned_history_goes_back_in(built):
    """three frames over the same guides and the same motion through the wrapper's own dict, against the model's chain: what comes back holds the current ids, so
    from the second step on the table's prev ids are the current ids"""
    w, h = 37, 23
    kw = inputs(w, h, True)
    matrices, prev_ids, moved = kw["object_motion"]
    got = want = kw["history"]
    for step in range(3):
        table = (matrices, prev_ids if step == 0 else np.arange(len(prev_ids)), moved)
        got = ra.temporal_accumulate(**dict(kw, history=got, object_motion=table))
        want, _, _, _ = mref.accumulate_moving(**dict(kw, history=want, object_motion=table))
        for k in OUTPUTS:
            assert_same(got[k], want[k], "step %d, %s" % (step, k))
    assert want["length"].max() > 1.0


# ---- 2. device tensors on a stream of the caller's --------------------------------------------------------------------------------------------------
def test_tensors_on_a_side_stream_and_on_the_default_stream(built):
    import torch
    w, h = 130, 70

    def on_device(kw):
        t = {}
        for k, v in kw.items():
            if isinstance(v, np.ndarray) and k != "prev_world_to_screen":
                t[k] = torch.from_numpy(v.astype(np.int32) if v.dtype == np.uint32 else v).cuda()
            elif k == "history":
                t[k] = {name: None if a is None else torch.from_numpy(a.astype(np.int32) if a.dtype == np.uint32 else a).cuda() for name, a in v.items()}
            else:
                t[k] = v     # (the table stays NumPy: the wrapper takes it to the device)
        return t
    cases = (True, False)
    tensors = [on_device(inputs(w, h, demodulate)) for demodulate in cases]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        on_side = [ra.temporal_accumulate(return_motion=True, **t) for t in tensors]
    on_default = ra.temporal_accumulate(return_motion=True, **tensors[0])
    stream.synchronize()
    for demodulate, (got, motion) in zip(cases, on_side):
        want, want_motion, _ = model(w, h, demodulate)
        assert got["a"].is_cuda and tuple(motion.shape) == (2, h, w)
        assert_history({k: got[k].cpu().numpy() for k in OUTPUTS}, motion.cpu().numpy(), want, want_motion, "side stream, demodulate %r" % demodulate)
    want, want_motion, _ = model(w, h, True)
    assert_history({k: on_default[0][k].cpu().numpy() for k in OUTPUTS}, on_default[1].cpu().numpy(), want, want_motion, "default stream")


# ---- 3. statuses through the raw ABI -----------------------------------------------------------------------------------------------------------------
def raw_moving(ctx, p, w, h, table, count, null=(), entry="rtgpu_temporal_accumulate_moving", pointers=None):
    n = max(1, min(w * h, 4096))
    keep = {name: np.zeros(3 * n, dtype=np.float32) for name in NAMES}
    ptr = {name: a.ctypes.data_as(C.c_void_p) for name, a in keep.items()}
    ptr.update(pointers or {})
    ptr.update({name: None for name in null})
    args = (ctx, C.byref(p) if p is not None else None, C.c_uint32(w), C.c_uint32(h)) + tuple(ptr[name] for name in NAMES) + (table, C.c_uint32(count))
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
        host_table = ra.object_motion_table((np.stack([eye, eye]), [0, 1], [0, 1]))
        dev = torch.zeros(41 * 64 + 4 + 64, dtype=torch.float32, device="cuda")
        at = lambda k: C.c_void_p(dev.data_ptr() + 64 * 4 * k)   # noqa: E731
        sizes = (3, 3, 1, 3, 3, 3, 1, 3, 3, 1, 1, 3, 3, 1, 3, 3, 1, 2)
        starts = dict(zip(NAMES, np.cumsum((0,) + sizes[:-1])))
        device_pointers = {name: at(int(k)) for name, k in starts.items()}
        device_table = at(41)
        for entry, pointers, table in (("rtgpu_temporal_accumulate_moving", None, host_table.ctypes.data_as(C.c_void_p)),
                                       ("rtgpu_temporal_accumulate_moving_async", device_pointers, device_table)):
            call = lambda p, w=4, h=4, null=(), t=table, count=2: raw_moving(ctx, p, w, h, t, count, null, entry, pointers)   # noqa: E731
            assert call(good) == OK                                   # a pure image operation: no scene, no rtgpu_resize
            assert call(None) == INVALID_ARGUMENT
            assert call(good, t=None) == INVALID_ARGUMENT and call(good, count=0) == INVALID_ARGUMENT      # the table
            for name in ("color", "half", "depth", "normal", "position", "albedo", "out_a", "out_b", "out_length"):
                assert call(good, null=(name,)) == INVALID_ARGUMENT, name
            assert call(good, null=("out_motion",)) == OK
            assert call(plain, null=("albedo",)) == OK
            assert call(good, null=PREVIOUS + ("prev_id",)) == OK     # no history: every pixel starts
            # both id planes are required
            assert call(good, null=("id",)) == INVALID_ARGUMENT and call(good, null=("prev_id",)) == INVALID_ARGUMENT
            assert call(good, null=("id", "prev_id")) == INVALID_ARGUMENT and b"id planes" in lib.rtgpu_last_error()
            assert call(good, null=PREVIOUS + ("prev_id", "id")) == INVALID_ARGUMENT
            for name in PREVIOUS:
                assert call(good, null=(name,)) == INVALID_ARGUMENT, name
            for field, value in (("alpha_min", 0.0), ("max_history", 0.5), ("normal_threshold", 1.5), ("plane_tolerance", 0.0), ("color_scale", float("nan"))):
                assert call(ra.temporal_params(prev_world_to_screen=eye, **{field: value})) == INVALID_ARGUMENT, field
            assert call(good, w=0) == INVALID_ARGUMENT and call(good, w=4097, h=4096) == UNSUPPORTED
        # the async entry: a 16-byte aligned table
        assert raw_moving(ctx, good, 4, 4, C.c_void_p(dev.data_ptr() + 64 * 4 * 41 + 4), 2, (), "rtgpu_temporal_accumulate_moving_async", device_pointers) == INVALID_ARGUMENT
        assert b"motion table" in lib.rtgpu_last_error()
        assert lib.rtgpu_synchronize(ctx) == OK
        torch.cuda.synchronize()
        with pytest.raises(ValueError, match="object_id"):
            color = np.zeros((4, 4, 3), dtype=np.float32)
            ra.temporal_accumulate(color, color, np.zeros((4, 4), dtype=np.float32), np.zeros((3, 4, 4), dtype=np.float32), np.zeros((3, 4, 4), dtype=np.float32), demodulate=False,
                                   object_motion=(eye[None], [0], [0]))
        with pytest.raises(ValueError, match="object_motion"):
            ra.object_motion_table((eye[None], [0, 1], [0]))
    finally:
        lib.rtgpu_destroy(ctx)


# ---- 4. through the context: rendered frames, an object moved and the camera yawed between them ----------------------------------------------------------
W, H = 64, 48
GUIDES = ("depth", "normal", "position", "base_color", "object_id")
FRAMES = 4
MOVED = 1        # the sphere


def stage(aspect):
    """a floor, a sphere that will move, a box that will not, a light"""
    s = ra.Scene()
    grey = s.add_material("diffuse", (0.7, 0.7, 0.7))
    red = s.add_material("diffuse", (0.8, 0.2, 0.1))
    blue = s.add_material("roughPlastic", (0.1, 0.3, 0.8), roughness=0.4)
    s.add_rect((6.0, 6.0), ra.transform_from_euler((0.0, -1.0, 0.0), (-90.0, 0.0, 0.0)), grey)
    s.add_sphere(0.9, ra.transform_from_euler((-1.2, -0.1, 0.0)), red)
    s.add_box((0.6, 0.8, 0.6), ra.transform_from_euler((1.4, -0.2, -0.5), (0.0, 25.0, 0.0)), blue)
    s.add_area_light("rect", [1.5, 1.5], (9.0, 9.0, 9.0), ra.transform_from_euler((0.0, 4.0, 0.0), (90.0, 0.0, 0.0)))
    s.build()
    return s


def camera_of(k):
    return ra.Camera((0.0, 1.0, 7.0), (6.0, 180.0 + 1.5 * k, 0.0), W / H, 45.0)


def sphere_at(k):
    """slides along x, rises a little and spins: far enough in three frames to change places with the box in the leaf order or not -- the test does not care"""
    return ra.transform_from_euler((-1.2 + 0.35 * k, -0.1 + 0.05 * k, 0.1 * k), (0.0, 20.0 * k, 5.0 * k))


def object_tables(scene):
    o = us.desc_arrays(scene)["objects"]
    return o[:, :16].copy().view(np.float32).reshape(-1, 4, 4), o[:, 16:32].copy().view(np.float32).reshape(-1, 4, 4)


def render_frame(vp, camera, passes=2):
    vp.reset()
    params = [vp.next_pass_params(camera) for _ in range(passes + 1)]
    for p in params[:passes]:
        vp.render_pass_with(p)
    s, s2 = vp.sum_buffer(secondary=True)
    return params[passes], dict(color=s, color_half=s2), vp.render_aovs(params[passes], GUIDES)


def run_chain(update, move, check=None):
    """FRAMES frames of a fresh viewport; before each but the first the camera yaws and -- with `update` -- Scene.update() / Viewport.update_scene() run, the
    sphere moved (`move`) or set to the transform it has.  Returns the images of Viewport.denoise(temporal=True, variance=False); check(k, vp, ...): per frame"""
    scene = stage(W / H)
    vp = ra.Viewport(W, H, seed=2468, max_ray_depth=3)
    vp.set_renderer(scene)
    images = []
    for k in range(FRAMES):
        previous_index = None
        if k and update:
            scene.set_object_transform(MOVED, sphere_at(k if move else 0))
            scene.update()
            vp.update_scene()
            u = scene.update_desc()
            previous_index = np.array([u.previousIndex[i] for i in range(u.numObjects)])
        p, sums, g = render_frame(vp, camera_of(k))
        before = (vp.sum_buffer(secondary=True), vp.counters(), vp.passes_finished)
        images.append(vp.denoise(p, temporal=True, variance=False))
        after = (vp.sum_buffer(secondary=True), vp.counters(), vp.passes_finished)
        # film, both sum buffers, counters and the pass count are unchanged by the call
        assert np.array_equal(words(before[0][0]), words(after[0][0])) and np.array_equal(words(before[0][1]), words(after[0][1])) and before[1:] == after[1:]
        assert after[2] == 2
        if check:
            check(k, scene, p, sums, g, previous_index, images[-1])
    return images


def test_the_context_call_is_the_composition_of_aovs_table_builder_and_model(built):
    state = dict(history=None, prev=None, then=None, then_id=None, blended_on_sphere=[], static_on_sphere=[])

    def check(k, scene, p, sums, g, previous_index, image):
        now, inverse = object_tables(scene)
        kw = dict(color=sums["color"], color_half=sums["color_half"], depth=g["depth"], normal=g["normal"], position=g["position"], albedo=g["base_color"],
                  object_id=g["object_id"], history=state["history"], color_scale=0.5)
        if state["history"] is not None:
            kw.update(prev_world_to_screen=list(state["prev"].camera.worldToScreen), prev_sample_offset=tuple(state["prev"].sampleOffset))
        if previous_index is None:
            history, _, _, why = ref.accumulate(**kw)
        else:
            then, then_id = state["then"][previous_index], state["then_id"][previous_index]      # rtgpu_update_objects' composition (one update per frame here)
            table = mref.motion_table(now, inverse, then, then_id)
            assert table[2].sum() == 1                                                              # the sphere moved, nothing else
            history, _, _, why = mref.accumulate_moving(object_motion=table, **kw)
            sphere = g["object_id"] == int(np.flatnonzero(table[2])[0])
            state["blended_on_sphere"].append(float((why == ref.BLENDED)[sphere].mean()))
            state["static_on_sphere"].append(float((ref.accumulate(**kw)[3] == ref.BLENDED)[sphere].mean()))
            assert sphere.sum() > 100
        assert_same(image, ref.remodulate(history["a"], g["base_color"]), "frame %d" % k)
        state.update(history=history, prev=p, then=now, then_id=np.arange(len(now), dtype=np.uint32))

    images = run_chain(update=True, move=True, check=check)
    assert len(images) == FRAMES and not np.array_equal(words(images[1]), words(images[2]))
    # the sphere's pixels keep their history as it slides and spins; reprojected as if the world stood still they would lose most of it
    print("share of the sphere's pixels that accumulate, per frame: following it %r, as if it stood still %r" % (state["blended_on_sphere"], state["static_on_sphere"]))
    # (a rigid body in full view in both frames: most of its pixels should find their history; reprojected in place they land beside it or on another part of it)
    assert min(state["blended_on_sphere"]) > 0.5, state["blended_on_sphere"]
    assert max(state["static_on_sphere"]) < 0.5 * min(state["blended_on_sphere"]), (state["static_on_sphere"], state["blended_on_sphere"])


def test_an_update_that_changes_nothing_changes_no_word(built):
    plain = run_chain(update=False, move=False)
    updated = run_chain(update=True, move=False)
    for k, (a, b) in enumerate(zip(plain, updated)):
        assert_same(b, a, "frame %d" % k)
    assert not np.array_equal(words(plain[0]), words(plain[1]))
