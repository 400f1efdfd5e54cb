"""RT_AOV_VIRTUAL_POSITION on the device (rtgpu_render_aovs_virtual[_async]; Viewport.render_aovs(chain=N) with "virtual_position") against the rule of
include/rtgpu.h folded over the CPU oracle's path recordings (tests/temporal_chain_ref.py on tests/guide_chain_ref.py), on 70 x 37 frames, every pixel.

Bar: BIT-EQUAL words.  The plane is a rounded multiply and a rounded add of words the chain call is already held to (vertex 0's ray, the chain distance): there is
no tolerance to state.  tests/test_guide_chain_cpu.py asserts from the oracle alone that the frames hold chains of two and more, misses and lights behind mirrors;
the cases this plane branches on are asserted again here."""
import ctypes as C

import numpy as np
import pytest

import aov_ref
import guide_chain_ref as ref
import temporal_chain_ref as chain_ref
import raytracer_amd as ra

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT = 0, -1
W, H = ref.W, ref.H
CHAIN_PLANES = tuple(ra.AOV_CHAIN_PLANES)
NON_COST = tuple(n for n in ra.AOV_PLANES if n not in aov_ref.COST_PLANES)
VIRTUAL = "virtual_position"
VIRTUAL_ID = ra.AOV_VIRTUAL_PLANES[VIRTUAL][0]


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def pixel_words(plane):
    """a (3, H, W) plane as (P, 3) words"""
    return words(np.ascontiguousarray(plane).reshape(3, -1).T.copy())


# ---- 1. the oracle ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [False, True], ids=["plain", "lens"])
@pytest.mark.parametrize("name", ["hall", "textured"])
def test_the_plane_equals_the_fold_over_the_oracles_paths(built, name, lens):
    frame, p, desc = ref.oracle_frame(name, lens=lens), ref.params(lens=lens), ref.scene(name).desc.contents
    vp = ref.viewport(name)
    c = ref.census(frame, desc, 3)
    assert c["light_behind_mirror"] >= 8 and c["miss_behind_mirror"] >= 8   # the two guide vertices without a surface: one is a point, one is 0, 0, 0
    if name == "hall":
        assert c["k2"] >= 8 and c["diffuse_behind_mirror"] >= 8
    first = vp.render_aovs(p, ("position",))["position"]
    for max_chain in (0, 1, 3, 16):
        got = vp.render_aovs(p, aov_ref.GEOMETRY_PLANES + CHAIN_PLANES + (VIRTUAL,), chain=max_chain)
        assert got[VIRTUAL].shape == (3, H, W) and got[VIRTUAL].dtype == np.float32
        want = chain_ref.virtual_frame(frame, desc, max_chain)
        have = pixel_words(got[VIRTUAL])
        bad = np.argwhere(have != words(want))
        k = got["chain_length"].reshape(-1)
        assert len(bad) == 0, "%s, maxChain %d: pixel %d channel %d (chain length %d): %#x, the fold has %#x" % (
            name, max_chain, bad[0][0], bad[0][1], k[bad[0][0]], have[tuple(bad[0])], words(want)[tuple(bad[0])])
        # the three cases of the definition, on the planes of the same call
        miss = np.isinf(got["chain_distance"]).reshape(-1)
        assert not have[miss].any() and np.array_equal(have[k == 0], pixel_words(got["position"])[k == 0])
        moved = (k >= 1) & ~miss
        if max_chain:
            assert moved.sum() >= (100 if name == "hall" else 30) and (have[moved] != pixel_words(got["position"])[moved]).any(axis=1).mean() > 0.9
            assert (miss & (k >= 1)).sum() >= 8
        else:
            assert np.array_equal(words(got[VIRTUAL]), words(first))   # maxChain 0: the POSITION words of the first-hit call
        # every plane the chain call knows holds the chain call's bits
        chain = vp.render_aovs(p, aov_ref.GEOMETRY_PLANES + CHAIN_PLANES, chain=max_chain)
        for plane in chain:
            assert np.array_equal(words(got[plane]), words(chain[plane])), plane


def test_every_other_plane_of_the_call_is_the_chain_calls(built):
    """all 15 non-cost planes and the three chain planes beside the virtual one, on the textured scene (the generic kernels)"""
    vp, p = ref.viewport("textured"), ref.params()
    got = vp.render_aovs(p, NON_COST + CHAIN_PLANES + (VIRTUAL,), chain=3)
    chain = vp.render_aovs(p, NON_COST + CHAIN_PLANES, chain=3)
    for plane in chain:
        assert np.array_equal(words(got[plane]), words(chain[plane])), plane
    # the plane alone: the position is evaluated for it
    alone = vp.render_aovs(p, (VIRTUAL,), chain=3)
    assert np.array_equal(words(alone[VIRTUAL]), words(got[VIRTUAL]))


def test_the_async_entry_writes_torch_tensors(built, monkeypatch):
    import torch
    vp, p = ref.viewport("hall"), ref.params()
    host = vp.render_aovs(p, ("depth", "chain_length", VIRTUAL), chain=3)
    got = vp.render_aovs(p, ("depth", "chain_length", VIRTUAL), chain=3, device=True)
    assert got[VIRTUAL].is_cuda and got[VIRTUAL].dtype == torch.float32 and tuple(got[VIRTUAL].shape) == (3, H, W)
    assert np.array_equal(words(got[VIRTUAL].cpu().numpy()), words(host[VIRTUAL])) and np.array_equal(got["chain_length"].cpu().numpy(), host["chain_length"])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        again = vp.render_aovs(p, (VIRTUAL,), chain=3, device=True)
    side.synchronize()
    assert np.array_equal(words(again[VIRTUAL].cpu().numpy()), words(host[VIRTUAL]))
    monkeypatch.setenv("RTGPU_AOV_CHUNK", "1000")   # three chunks, the last one short
    chunked = ref.viewport("hall")
    assert np.array_equal(words(chunked.render_aovs(p, (VIRTUAL,), chain=3)[VIRTUAL]), words(host[VIRTUAL]))
    assert np.array_equal(words(chunked.render_aovs(p, (VIRTUAL,), chain=3, device=True)[VIRTUAL].cpu().numpy()), words(host[VIRTUAL]))


# ---- 2. statuses through the raw ABI -----------------------------------------------------------------------------------------------------------
def raw_call(ctx, p, planes, entry, chain=(2, 0), outputs="own"):
    ids = (C.c_uint32 * max(len(planes), 1))(*planes)
    keep = [np.zeros(3 * W * H, dtype=np.uint32) for _ in planes]
    ptrs = (C.c_void_p * max(len(planes), 1))(*[a.ctypes.data for a in keep]) if outputs == "own" else outputs
    desc = ra.RtAovChain(*chain) if chain is not None else None
    args = (ctx, C.byref(p), C.byref(desc) if desc is not None else None, ids, C.c_uint32(len(planes)), ptrs)
    if entry.endswith("_async"):
        args += (None,)
    return getattr(ra.rtgpu_lib(), entry)(*args)


def test_statuses(built):
    import torch
    lib = ra.rtgpu_lib()
    vp, p = ref.viewport("hall"), ref.params()
    ctx = vp.device_context()
    assert vp.render_aovs(p, ("depth",), chain=1)["depth"].shape == (H, W)   # (the renderer uploads its scene on first use)
    t = torch.zeros(3 * W * H + 4, dtype=torch.float32, device="cuda")
    for entry in ("rtgpu_render_aovs_virtual", "rtgpu_render_aovs_virtual_async"):
        device = (C.c_void_p * 1)(t.data_ptr()) if entry.endswith("_async") else "own"
        assert raw_call(ctx, p, [], entry) == OK
        assert raw_call(ctx, p, [VIRTUAL_ID], entry, outputs=device) == OK
        assert raw_call(ctx, p, [VIRTUAL_ID], entry, chain=None) == INVALID_ARGUMENT and b"chain" in lib.rtgpu_last_error()
        assert raw_call(ctx, p, [VIRTUAL_ID], entry, chain=(17, 0)) == INVALID_ARGUMENT and raw_call(ctx, p, [VIRTUAL_ID], entry, chain=(2, 1)) == INVALID_ARGUMENT
        for cost in aov_ref.COST_PLANES:
            assert raw_call(ctx, p, [VIRTUAL_ID, ra.AOV_PLANES[cost][0]], entry) == INVALID_ARGUMENT and b"cost" in lib.rtgpu_last_error()
        assert raw_call(ctx, p, [VIRTUAL_ID + 1], entry) == INVALID_ARGUMENT and b"unknown" in lib.rtgpu_last_error()
        assert raw_call(ctx, p, [0, 0xFFFFFFFF], entry) == INVALID_ARGUMENT
        assert raw_call(ctx, p, [VIRTUAL_ID, 0, VIRTUAL_ID], entry) == INVALID_ARGUMENT and b"twice" in lib.rtgpu_last_error()
    assert raw_call(ctx, p, [VIRTUAL_ID], "rtgpu_render_aovs_virtual_async", outputs=(C.c_void_p * 1)(t.data_ptr() + 4)) == INVALID_ARGUMENT
    assert lib.rtgpu_synchronize(ctx) == OK
    # the plane belongs to the virtual entries alone
    for entry in ("rtgpu_render_aovs_chain", "rtgpu_render_aovs_chain_async"):
        assert raw_call(ctx, p, [VIRTUAL_ID], entry) == INVALID_ARGUMENT and b"unknown" in lib.rtgpu_last_error()
    with pytest.raises(ValueError, match="chain=N"):
        vp.render_aovs(p, (VIRTUAL,))


# ---- 3. the call leaves the render state alone -----------------------------------------------------------------------------------------------
def test_a_call_leaves_film_counters_and_history_alone(built):
    lib = ra.rtgpu_lib()

    def run(interrupt):
        vp = ra.Viewport(W, H, seed=ref.SEED, max_ray_depth=3)
        vp.set_renderer(ref.scene("hall"))
        ctx, cam = vp.device_context(), ref.camera()
        params = [vp.next_pass_params(cam) for _ in range(4)]
        vp.render_pass_with(params[0])
        if interrupt:   # while a pass is still queued
            before = vp.passes_finished
            vp.render_aovs(ref.params(), (VIRTUAL, "chain_length"), chain=3)
            assert vp.passes_finished == before
        vp.render_pass_with(params[1])
        first = vp.denoise(params[2], temporal=True, variance=True)
        if interrupt:
            vp.render_aovs(ref.params(skip=1), (VIRTUAL,), chain=16, device=True)
        second = vp.denoise(params[3], temporal=True, variance=True)
        s, s2 = vp.sum_buffer(secondary=True)
        raw = ra.RtCounters()
        assert lib.rtgpu_get_counters(ctx, C.byref(raw)) == 0
        return dict(s=s, s2=s2, counters=vp.counters(), raw=bytes(raw), passes=vp.passes_finished, first=first, second=second)
    plain, cut = run(False), run(True)
    for name in ("s", "s2", "first", "second"):
        assert np.array_equal(words(plain[name]), words(cut[name])), name
    assert plain["counters"] == cut["counters"] and plain["raw"] == cut["raw"] and plain["passes"] == cut["passes"] == 2 and plain["s"].any()
    assert not np.array_equal(words(plain["first"]), words(plain["second"]))   # the second temporal frame does depend on the history
