"""Temporal accumulation over chain guides on the device (rtgpu_temporal_accumulate_chain, rtgpu_denoise_temporal_chain and their _async twins;
raytracer_amd.temporal_accumulate(chain=...), Viewport.denoise(temporal=True, chain=N)) against its NumPy float32 model (tests/temporal_chain_ref.py).

Bar and helpers: those of tests/test_gpu_temporal.py -- BIT-EQUAL words in outA, outB, outLength, outMotion and outConfidence, no pixel left out.  The operation is
defined step by step (include/rtgpu.h), the model performs those steps in that order in IEEE float32, and the device library is compiled without contraction:
there is no tolerance to state.  The model's own properties: tests/test_temporal_chain_model.py.

The shapes straddle k_temporal's 64 x 4 block and k_temporal_moments' 32 x 8 tile: one pixel, a frame smaller than the window, one pixel over a tile both ways,
the two degenerate strips, several tiles and blocks both ways."""
import ctypes as C

import numpy as np
import pytest

import guide_chain_ref as gref
import raytracer_amd as ra
import temporal_chain_ref as chain_ref
import temporal_moving_ref as mref
import temporal_ref as ref
from test_gpu_temporal import OK, INVALID_ARGUMENT, PARAMS, OUTPUTS, NAMES, assert_history, assert_same, words
from test_gpu_temporal_clip import on_device
from test_gpu_temporal_moving import object_tables

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 5), (33, 9), (70, 1), (3, 200), (67, 29)]
DENSE = dict(gamma=0.5, min_count=2)
F = np.float32

_frames = {}


def frame(w, h):
    """mref.random_moving_frame (its table and the static frame it was made from) with chain planes: chain lengths 0 .. 3 in patches in both frames, a virtual
    position a fraction of a pixel off the position, a chain distance of one to four depths (+inf on the misses), and two colours that are not numbers"""
    if (w, h) not in _frames:
        f = mref.random_moving_frame(w, h, seed=1000 * w + h, num_objects=3 + (w + h) % 3)
        rng = np.random.default_rng(7000 * w + h)

        def lengths():
            k = np.kron(rng.integers(0, 4, size=((h + 3) // 4, (w + 5) // 6)), np.ones((4, 6), dtype=np.int64))[:h, :w]
            return np.where(rng.random((h, w)) < 0.05, rng.integers(0, 4, size=(h, w)), k).astype(np.uint32)
        chains = {}
        for label, cur in (("table", f["current"]), ("static", f["base"]["current"])):
            k = lengths()
            distance = (cur["depth"] * (F(1.0) + k.astype(F) * rng.random((h, w), dtype=F))).astype(F)
            virtual = (cur["position"] + rng.normal(scale=0.2, size=(3, h, w)).astype(F) * np.array([1.0, 1.0, 0.0], dtype=F).reshape(3, 1, 1)).astype(F)
            chains[label] = dict(virtual_position=virtual, chain_length=k, chain_distance=distance)
        f["chains"], f["prev_chain_length"] = chains, lengths()
        if w * h >= 16:
            for cur in (f["current"], f["base"]["current"]):
                cur["color"] = cur["color"].copy()
                cur["color"][h // 3, w // 3, 1] = np.nan
                cur["color"][h // 2, w // 4, :] = np.nan
        _frames[w, h] = f
    return _frames[w, h]


def inputs(w, h, demodulate=True, table=True, ids=True):
    """the keyword arguments model and device take alike, and the chain planes (the device: chain=dict(...); the model: keywords)"""
    top = frame(w, h)
    f = top if table else top["base"]
    cur, history = dict(f["current"]), dict(f["history"], chain_length=top["prev_chain_length"])
    if not demodulate:
        del cur["albedo"]
    if not ids:
        del cur["object_id"]
        history["object_id"] = None
    kw = dict(cur, demodulate=demodulate, history=history, prev_world_to_screen=f["prev_world_to_screen"], prev_sample_offset=f["prev_sample_offset"], **PARAMS)
    if table:
        kw["object_motion"] = top["object_motion"]
    return kw, top["chains"]["table" if table else "static"]


# ---- a. the pure entry on random inputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("demodulate", [True, False], ids=["demodulated", "plain"])
@pytest.mark.parametrize("w, h", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_the_pure_entry_equals_the_model(built, w, h, demodulate):
    blended = dropped_by_chain = 0
    for label, table, ids in (("table", True, True), ("static", False, True), ("static, no ids", False, False)):
        kw, chain = inputs(w, h, demodulate, table, ids)
        for clip in (None, dict(DENSE, radius=1), dict(DENSE, radius=2), dict(DENSE, radius=3), dict(radius=3, gamma=1.0, min_count=9)):
            what = "%d x %d, %s, clip %r" % (w, h, label, clip)
            want, want_motion, taken, why, info = chain_ref.accumulate_chain(clip=clip, **kw, **chain)
            if clip is None:
                got, got_motion = ra.temporal_accumulate(return_motion=True, chain=chain, **kw)
            else:
                got, got_motion, got_confidence = ra.temporal_accumulate(return_motion=True, return_confidence=True, clip=clip, chain=chain, **kw)
                assert_same(got_confidence, info["f"], what + ", confidence")
                if w * h > 500 and clip["min_count"] == 2:
                    assert info["clipped"].sum() >= 5, what
            assert_history(got, got_motion, want, want_motion, what)
            assert np.array_equal(got["chain_length"], chain["chain_length"]) and got["chain_length"].dtype == np.uint32
        blended += int((why == ref.BLENDED).sum())
        # the rules bite: the same planes with every history pixel at the pixel's own chain length take more taps
        _, _, all_taken, _, _ = chain_ref.accumulate_chain(**dict(kw, history=dict(kw["history"], chain_length=chain["chain_length"])), **chain)
        dropped_by_chain += int((why != ref.BLENDED).sum() - (all_taken == 0).sum())
        if table and w * h > 500:
            assert (why == chain_ref.START_CHAIN_MOVED).sum() > 100 and ((why == ref.BLENDED) & (chain["chain_length"] == 0)).sum() > 20, what
    if w * h > 500:
        assert blended > 100 and dropped_by_chain > 50, (blended, dropped_by_chain)
    # without a history every pixel starts
    kw, chain = inputs(w, h, demodulate)
    started = ra.temporal_accumulate(chain=chain, **{k: v for k, v in kw.items() if k not in ("history", "prev_world_to_screen", "prev_sample_offset")})
    assert (started["length"] == 1.0).all() and np.array_equal(started["chain_length"], chain["chain_length"])


# ---- b. the identity: chain planes of a first hit give the words of the calls without -------------------------------------------------------------------
@pytest.mark.parametrize("w, h", [(33, 9), (67, 29)], ids=["33x9", "67x29"])
def test_first_hit_chain_planes_give_the_words_of_the_calls_without(built, w, h):
    for label, table, ids in (("table", True, True), ("static", False, True), ("static, no ids", False, False)):
        kw, _ = inputs(w, h, True, table, ids)
        zero = np.zeros((h, w), dtype=np.uint32)
        kw["history"] = dict(kw["history"], chain_length=zero)
        chain = dict(virtual_position=kw["position"], chain_length=zero, chain_distance=kw["depth"])
        plain_history = {k: v for k, v in kw["history"].items() if k != "chain_length"}
        for clip in (None, dict(DENSE, radius=1), dict(DENSE, radius=3)):
            extra = dict(return_confidence=True) if clip else {}
            got = ra.temporal_accumulate(return_motion=True, clip=clip, chain=chain, **extra, **kw)
            want = ra.temporal_accumulate(return_motion=True, clip=clip, **extra, **dict(kw, history=plain_history))
            assert_history(got[0], got[1], want[0], want[1], "%s, clip %r" % (label, clip))
            if clip:
                assert_same(got[2], want[2], "%s, confidence" % label)
                assert (want[2] != 1.0).sum() >= 5
        assert (want[0]["length"] > 1.0).mean() > 0.3


# ---- c. a chain of calls, on arrays and on tensors ------------------------------------------------------------------------------------------------------
def test_the_returned_history_goes_back_in_on_tensors_and_on_both_streams(built):
    import torch
    w, h = 67, 29
    kw, chain = inputs(w, h, True, table=False)
    clip = dict(DENSE, radius=2)
    want, steps = kw["history"], []
    for step in range(3):
        want, motion, _, why, info = chain_ref.accumulate_chain(**dict(kw, history=want, clip=clip), **chain)
        steps.append((want, motion, info))
    assert steps[2][0]["length"].max() > 2.0 and (steps[2][0]["length"] > 1.0).sum() > 300
    tensors = on_device(torch, kw)
    tchain = {k: torch.from_numpy(v.astype(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in chain.items()}
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for label, stream in (("side stream", side), ("default stream", torch.cuda.default_stream())):
        with torch.cuda.stream(stream):
            got = tensors["history"]
            results = []
            for step in range(3):
                got, motion, confidence = ra.temporal_accumulate(**dict(tensors, history=got, clip=clip, chain=tchain, return_motion=True, return_confidence=True))
                results.append((got, motion, confidence))
        stream.synchronize()
        for step, ((got, motion, confidence), (want, want_motion, info)) in enumerate(zip(results, steps)):
            assert got["a"].is_cuda and got["chain_length"].is_cuda
            assert_history({k: got[k].cpu().numpy() for k in OUTPUTS}, motion.cpu().numpy(), want, want_motion, "%s, step %d" % (label, step))
            assert_same(confidence.cpu().numpy(), info["f"], "%s, step %d, confidence" % (label, step))


# ---- d. statuses through the raw ABI ----------------------------------------------------------------------------------------------------------------------
CHAIN_NAMES = ("virtual", "length", "distance", "prev_length_k")


def raw_chain(ctx, p, w, h, table, count, clip, confidence, entry, pointers, chain="given", null=()):
    ptr = dict(pointers)
    ptr.update({name: None for name in null})
    block = ra.RtTemporalChain(*[ptr[name].value if ptr[name] is not None else None for name in CHAIN_NAMES])
    args = (ctx, C.byref(p) if p is not None else None, C.c_uint32(w), C.c_uint32(h)) + tuple(ptr[name] for name in NAMES) + (
        table, C.c_uint32(count), C.byref(clip) if clip is not None else None, confidence, C.byref(block) if chain == "given" else None)
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
        good = ra.temporal_params(prev_world_to_screen=eye)
        clip = ra.temporal_clip(dict(radius=2, gamma=2.0, min_count=4))
        host_table = ra.object_motion_table((np.stack([eye, eye]), [0, 1], [0, 1]))
        sizes = dict(zip(NAMES + CHAIN_NAMES, (3, 3, 1, 3, 3, 3, 1, 3, 3, 1, 1, 3, 3, 1, 3, 3, 1, 2) + (3, 1, 1, 1)))
        host = {name: np.zeros(64 * n, dtype=np.float32) for name, n in sizes.items()}
        host_confidence = np.zeros(64, dtype=np.float32)
        dev = torch.zeros(64 * (sum(sizes.values()) + 8), dtype=torch.float32, device="cuda")
        at = lambda k: C.c_void_p(dev.data_ptr() + 64 * 4 * k)   # noqa: E731
        starts = dict(zip(sizes, np.cumsum([0] + list(sizes.values())[:-1])))
        total = sum(sizes.values())
        for entry, pointers, table, confidence in (
                ("rtgpu_temporal_accumulate_chain", {name: a.ctypes.data_as(C.c_void_p) for name, a in host.items()}, host_table.ctypes.data_as(C.c_void_p), host_confidence.ctypes.data_as(C.c_void_p)),
                ("rtgpu_temporal_accumulate_chain_async", {name: at(int(k)) for name, k in starts.items()}, at(total + 1), at(total))):
            if entry.endswith("_async"):
                dev[64 * (total + 1):64 * (total + 1) + 40] = torch.from_numpy(host_table.view(np.float32).reshape(-1)).cuda()
            call = lambda c=clip, p=good, null=(), t=table, count=2, f=confidence, chain="given": raw_chain(ctx, p, 4, 4, t, count, c, f, entry, pointers, chain, null)   # noqa: E731
            assert call() == OK
            assert call(c=None) == OK and call(c=None, f=None) == OK                       # clip NULL: no clipping
            assert call(t=None, count=0) == OK and call(t=None, count=0, null=("id", "prev_id")) == OK
            assert call(chain=None) == INVALID_ARGUMENT and b"chain" in lib.rtgpu_last_error()
            for name in ("virtual", "length", "distance"):
                assert call(null=(name,)) == INVALID_ARGUMENT and b"chain" in lib.rtgpu_last_error(), name
            assert call(null=("prev_length_k",)) == INVALID_ARGUMENT and b"prevChainLength" in lib.rtgpu_last_error()      # missing beside a history
            previous = NAMES[7:14]
            assert call(null=previous + ("prev_length_k",)) == OK                             # no history: every pixel starts
            assert call(null=previous) == INVALID_ARGUMENT and b"prevChainLength" in lib.rtgpu_last_error()   # given without a history
            # as the clip entry
            assert call(p=None) == INVALID_ARGUMENT and call(null=("color",)) == INVALID_ARGUMENT and call(null=("out_a",)) == INVALID_ARGUMENT
            assert call(t=None) == INVALID_ARGUMENT and call(count=0) == INVALID_ARGUMENT and call(null=("prev_a",)) == INVALID_ARGUMENT
            assert call(c=ra.temporal_clip(dict(radius=4))) == INVALID_ARGUMENT and call(c=ra.temporal_clip(dict(min_count=0))) == INVALID_ARGUMENT
        # the async entry: the chain planes aligned, and no output over them
        pointers = {name: at(int(k)) for name, k in starts.items()}
        async_call = lambda **moved: raw_chain(ctx, good, 4, 4, at(total + 1), 2, clip, at(total), "rtgpu_temporal_accumulate_chain_async", dict(pointers, **moved))   # noqa: E731
        for name in CHAIN_NAMES:
            assert async_call(**{name: C.c_void_p(pointers[name].value + 4)}) == INVALID_ARGUMENT and b"aligned" in lib.rtgpu_last_error(), name
            assert async_call(out_a=pointers[name]) == INVALID_ARGUMENT and b"overlap" in lib.rtgpu_last_error(), name
        assert async_call() == OK
        assert lib.rtgpu_synchronize(ctx) == OK
        torch.cuda.synchronize()
    finally:
        lib.rtgpu_destroy(ctx)
    # the context entry
    vp = gref.viewport("hall")
    p = gref.params()
    assert vp.render_aovs(p, ("depth",))["depth"].shape == (gref.H, gref.W)
    ctx = vp.device_context()
    out = np.zeros((gref.H, gref.W, 3), dtype=np.float32)
    t, chain = ra.temporal_params(), ra.RtAovChain(3, 0)
    call = lambda c, **kw: lib.rtgpu_denoise_temporal_chain(ctx, kw.get("t", C.byref(t)), None, C.byref(p), c, kw.get("out", out.ctypes.data_as(C.c_void_p)), None, None, None)   # noqa: E731
    assert call(C.byref(chain)) == OK
    assert call(None) == INVALID_ARGUMENT and b"chain" in lib.rtgpu_last_error()
    assert call(C.byref(ra.RtAovChain(17, 0))) == INVALID_ARGUMENT and call(C.byref(ra.RtAovChain(3, 1))) == INVALID_ARGUMENT
    assert call(C.byref(chain), t=None) == INVALID_ARGUMENT and call(C.byref(chain), out=None) == INVALID_ARGUMENT
    bad = ra.temporal_clip(dict(radius=4))
    assert lib.rtgpu_denoise_temporal_chain(ctx, C.byref(t), None, C.byref(p), C.byref(chain), out.ctypes.data_as(C.c_void_p), None, C.byref(bad), None) == INVALID_ARGUMENT
    assert lib.rtgpu_denoise_temporal_chain_async(ctx, C.byref(t), None, C.byref(p), C.byref(chain), C.c_void_p(out.ctypes.data + 4), None, None, None, None) == INVALID_ARGUMENT
    vp.reset_history()


# ---- e. through the context: the hall under a yawing camera ---------------------------------------------------------------------------------------------
W, H = gref.W, gref.H
FRAMES = 3
MAX_CHAIN = 3
SIGMAS = dict(sigma_lum=3.0, sigma_normal=0.5, sigma_plane=0.15)
CONTEXT_CLIP = dict(radius=2, gamma=1.0, min_count=6)
GUIDES = ("depth", "normal", "position", "base_color", "object_id")
CHAIN_GUIDES = GUIDES + ("chain_length", "chain_distance", "virtual_position")


def camera_of(k):
    return ra.Camera((-12.5, 2.5, 0.3), (-6.0, 88.0 + 0.5 * k, 0.0), W / H, 75.0)


def fresh_viewport(scene=None):
    vp = ra.Viewport(W, H, **gref.viewport_args())
    vp.set_renderer(scene if scene is not None else gref.scene("hall"))
    return vp


def render_frame(vp, camera, passes=2):
    vp.reset()
    params = [vp.next_pass_params(camera) for _ in range(passes + 1)]
    for p in params[:passes]:
        vp.render_pass_with(p)
    s, s2 = vp.sum_buffer(secondary=True)
    return params[passes], dict(color=s, color_half=s2)


def chain_of(g):
    return {name: g[name] for name in ra.CHAIN_KEYS}


@pytest.mark.parametrize("clip", [None, CONTEXT_CLIP], ids=["no_clip", "clip"])
@pytest.mark.parametrize("variance", [True, False], ids=["filtered", "filter=None"])
def test_the_context_call_is_the_composition_of_its_parts(built, variance, clip):
    """three frames, two passes each: Viewport.denoise(temporal=True, chain=N) equals render_aovs (the virtual entry), the pure wrapper and the prepared filter; the
    history length exceeds 1 on exactly the pixels the model says"""
    vp = fresh_viewport()
    history, prev, longer = None, None, []
    for k in range(FRAMES):
        p, sums = render_frame(vp, camera_of(k))
        g = vp.render_aovs(p, CHAIN_GUIDES, chain=MAX_CHAIN)
        kw = dict(color=sums["color"], color_half=sums["color_half"], depth=g["depth"], normal=g["normal"], position=g["position"], albedo=g["base_color"], object_id=g["object_id"],
                  history=history, color_scale=0.5, clip=clip)
        if history is not None:
            kw.update(prev_world_to_screen=list(prev.camera.worldToScreen), prev_sample_offset=tuple(prev.sampleOffset))
        history = ra.temporal_accumulate(chain=chain_of(g), **kw)
        model, _, _, why, _ = chain_ref.accumulate_chain(**kw, **chain_of(g)) if k == 0 else chain_ref.accumulate_chain(**dict(kw, history=model), **chain_of(g))
        assert_same(history["length"], model["length"], "frame %d, length" % k)
        assert np.array_equal(history["length"] > 1.0, model["length"] > 1.0)
        if clip is None:   # (clipped to a box of no width -- a black pixel's -- a blended pixel's length is cut to exactly 1)
            assert np.array_equal(history["length"] > 1.0, why == ref.BLENDED)
        inside = g["chain_length"] >= 1
        longer.append((int((history["length"][inside] > 1.0).sum()), int(inside.sum())))
        if variance:
            want = ra.atrous_filter(history["a"], g["depth"], g["normal"], g["position"], g["base_color"], color_half=history["b"], prepared=True, iterations=5, **SIGMAS)
        else:
            want = ref.remodulate(history["a"], g["base_color"])
        before = (vp.sum_buffer(secondary=True), vp.counters(), vp.passes_finished)
        got = vp.denoise(p, temporal=True, variance=variance, clip=clip, chain=MAX_CHAIN, **(SIGMAS if variance else {}))
        after = (vp.sum_buffer(secondary=True), vp.counters(), vp.passes_finished)
        assert np.array_equal(words(before[0][0]), words(after[0][0])) and np.array_equal(words(before[0][1]), words(after[0][1])) and before[1:] == after[1:]
        assert_same(got, want, "frame %d" % k)
        prev = p
    print("chain pixels with a history longer than 1, per frame: %r" % longer)
    assert longer[0][0] == 0 and min(n for n, _ in longer[1:]) > 100 and min(total for _, total in longer) > 300


def test_chain_zero_is_the_call_with_first_hit_guides(built):
    for clip in (None, CONTEXT_CLIP):
        a, b = fresh_viewport(), fresh_viewport()
        for k in range(FRAMES):
            pa, _ = render_frame(a, camera_of(k))
            pb, _ = render_frame(b, camera_of(k))
            extra = dict(return_confidence=True) if clip else {}
            got = a.denoise(pa, temporal=True, variance=True, clip=clip, chain=0, **SIGMAS, **extra)
            want = b.denoise(pb, temporal=True, variance=True, clip=clip, **SIGMAS, **extra)
            for x, y in zip(got if clip else (got,), want if clip else (want,)):
                assert_same(x, y, "clip %r, frame %d" % (clip, k))


def test_a_device_call_on_a_stream_equals_the_host_call(built):
    import torch
    a, b = fresh_viewport(), fresh_viewport()
    side = torch.cuda.Stream()
    for k in range(2):
        pa, _ = render_frame(a, camera_of(k))
        pb, _ = render_frame(b, camera_of(k))
        want = a.denoise(pa, temporal=True, variance=True, clip=CONTEXT_CLIP, chain=MAX_CHAIN, return_variance=True, return_confidence=True, **SIGMAS)
        with torch.cuda.stream(side):
            got = b.denoise(pb, temporal=True, variance=True, clip=CONTEXT_CLIP, chain=MAX_CHAIN, return_variance=True, return_confidence=True, device=True, **SIGMAS)
        side.synchronize()
        for x, y in zip(got, want):
            assert_same(x.cpu().numpy(), y, "frame %d" % k)


def test_after_an_update_chain_pixels_start_and_the_others_follow_the_moving_model(built):
    scene = gref._hall()   # a scene of this test's own: it moves an object
    bn = ra.load_blue_noise()
    scene.desc.contents.blueNoise = bn.ctypes.data
    vp = fresh_viewport(scene)
    moved = 5   # the plastic box (the mesh is object 0, the three mirrors 1 .. 3, the sphere 4)
    p0, sums0 = render_frame(vp, camera_of(0))
    g0 = vp.render_aovs(p0, CHAIN_GUIDES, chain=MAX_CHAIN)
    vp.denoise(p0, temporal=True, chain=MAX_CHAIN)
    then, _ = object_tables(scene)
    scene.set_object_transform(moved, ra.transform_from_euler((-5.0, 0.9, -0.2), (0.0, 35.0, 0.0)))
    scene.update()
    vp.update_scene()
    now, inverse = object_tables(scene)
    assert len(now) == len(then)
    p1, sums1 = render_frame(vp, camera_of(0))
    g1 = vp.render_aovs(p1, CHAIN_GUIDES, chain=MAX_CHAIN)
    got = vp.denoise(p1, temporal=True, chain=MAX_CHAIN)
    # (no update reorders this scene's objects: every object keeps its index)
    table = mref.motion_table(now, inverse, then, np.arange(len(now), dtype=np.uint32))
    assert table[2].sum() == 1
    first = dict(color=sums0["color"], color_half=sums0["color_half"], depth=g0["depth"], normal=g0["normal"], position=g0["position"], albedo=g0["base_color"], object_id=g0["object_id"],
                 color_scale=0.5)
    history, _, _, _, _ = chain_ref.accumulate_chain(**first, **chain_of(g0))
    second = dict(color=sums1["color"], color_half=sums1["color_half"], depth=g1["depth"], normal=g1["normal"], position=g1["position"], albedo=g1["base_color"], object_id=g1["object_id"],
                  color_scale=0.5, prev_world_to_screen=list(p0.camera.worldToScreen), prev_sample_offset=tuple(p0.sampleOffset), object_motion=table)
    want, _, _, why, _ = chain_ref.accumulate_chain(history=history, **second, **chain_of(g1))
    assert_same(got, ref.remodulate(want["a"], g1["base_color"]), "the frame after the update")
    inside = g1["chain_length"] >= 1
    assert inside.sum() > 300 and (want["length"][inside] == 1.0).all() and (why[inside] == chain_ref.START_CHAIN_MOVED).sum() > 250
    # the others: the moving call's words, on first-hit planes (which the chain planes are where k = 0).  A history pixel with a chain is no tap of theirs:
    # to the moving model it is given an id no object has
    apart = np.where(history["chain_length"] > 0, np.uint32(0xFFFFFFF0), history["object_id"]).astype(np.uint32)
    plain, _, _, plain_why = mref.accumulate_moving(history=dict({k: v for k, v in history.items() if k != "chain_length"}, object_id=apart), **second)
    for key in OUTPUTS:
        assert np.array_equal(words(want[key])[~inside], words(plain[key])[~inside]), key
    assert (plain_why[~inside] == ref.BLENDED).sum() > 1000


def test_a_plain_temporal_call_after_a_chained_one_starts_every_pixel(built):
    a, b = fresh_viewport(), fresh_viewport()
    images, kept = {}, None
    for label, vp in (("chained", a), ("reset", b)):
        out = []
        for k in range(4):
            p, sums = render_frame(vp, camera_of(k))
            if k == 2 and label == "chained":
                kept = (sums, vp.render_aovs(p, GUIDES))
            if k < 2:
                out.append(vp.denoise(p, temporal=True, chain=MAX_CHAIN))
                continue
            if k == 2 and label == "reset":
                vp.reset_history()
            out.append(vp.denoise(p, temporal=True))
        images[label] = out
    for k in range(4):
        assert_same(images["chained"][k], images["reset"][k], "frame %d" % k)
    # frame 2 started every pixel: it is the frame itself, remodulated
    sums, g = kept
    start, _, _, _ = ref.accumulate(sums["color"], sums["color_half"], g["depth"], g["normal"], g["position"], g["base_color"], color_scale=0.5)
    assert_same(images["chained"][2], ref.remodulate(start["a"], g["base_color"]), "the plain call after the chained one")
    assert not np.array_equal(words(images["chained"][3]), words(ref.remodulate(start["a"], g["base_color"])))
    # and a history the plain call wrote is valid input to the chained one: all its chain lengths are 0
    c = fresh_viewport()
    p0, sums0 = render_frame(c, camera_of(0))
    c.denoise(p0, temporal=True)
    g0 = c.render_aovs(p0, GUIDES)
    p1, sums1 = render_frame(c, camera_of(1))
    got = c.denoise(p1, temporal=True, chain=MAX_CHAIN)
    g1 = c.render_aovs(p1, CHAIN_GUIDES, chain=MAX_CHAIN)
    history, _, _, _ = ref.accumulate(sums0["color"], sums0["color_half"], g0["depth"], g0["normal"], g0["position"], g0["base_color"], object_id=g0["object_id"], color_scale=0.5)
    want, _, _, why, _ = chain_ref.accumulate_chain(sums1["color"], sums1["color_half"], g1["depth"], g1["normal"], g1["position"], albedo=g1["base_color"], object_id=g1["object_id"],
                                                    history=dict(history, chain_length=np.zeros((H, W), dtype=np.uint32)), color_scale=0.5,
                                                    prev_world_to_screen=list(p0.camera.worldToScreen), prev_sample_offset=tuple(p0.sampleOffset), **chain_of(g1))
    assert_same(got, ref.remodulate(want["a"], g1["base_color"]), "a chained call over a plain history")
    assert (why[g1["chain_length"] == 0] == ref.BLENDED).sum() > 1000 and not (why[g1["chain_length"] >= 1] == ref.BLENDED).any()


def test_the_calls_without_a_chain_still_refuse_under_set_guide_chain(built):
    vp = fresh_viewport()
    p, _ = render_frame(vp, camera_of(0))
    vp.set_guide_chain(3)
    with pytest.raises(RuntimeError, match=r"\(-6\)"):
        vp.denoise(p, temporal=True)
    with pytest.raises(RuntimeError, match=r"\(-6\)"):
        vp.denoise(p, temporal=True, clip=True)
    # the chained call takes its chain from its argument: the set chain does not affect it
    under = vp.denoise(p, temporal=True, chain=1)
    other = fresh_viewport()
    q, _ = render_frame(other, camera_of(0))
    assert_same(under, other.denoise(q, temporal=True, chain=1), "under a set guide chain")
    vp.set_guide_chain(None)
