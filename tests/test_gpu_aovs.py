"""AOVs on the device (rtgpu_render_aovs, Viewport.render_aovs) against the CPU oracle: the geometry planes against the first vertex of the oracle's path
records, the material planes and the bitangent against its Debug renderer, the cost planes against its per-pixel counters -- on a 70 x 37 frame
(tests/aov_ref.py), every pixel.

Bar: BIT-EQUAL words.  Both sides evaluate the reference's arithmetic in its order with IEEE operations, so there is no tolerance to state.  One set of
words is not compared: a first vertex's fields that the reference never writes -- on a miss words 7 and 9..21, off mesh triangles u and v, the list
include/rtgpu.h gives for path records (path_records_ref.stale_mask).  The oracle's record holds whatever its stack held there; the planes must hold
zero, and that is asserted instead."""
import ctypes as C

import numpy as np
import pytest

import aov_ref as ref
import raytracer_amd as ra

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, NOT_READY, UNSUPPORTED = 0, -1, -5, -6
W, H = ref.W, ref.H
NON_COST = tuple(n for n in ref.ALL_PLANES if n not in ref.COST_PLANES)


def same_words(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_same_planes(a, b, names=None, what=""):
    for name in (names if names is not None else a):
        bad = np.argwhere(np.ascontiguousarray(a[name]).view(np.uint32) != np.ascontiguousarray(b[name]).view(np.uint32))
        assert a[name].shape == b[name].shape and len(bad) == 0, "%s: plane %s differs in %d words, first at %r" % (what, name, len(bad), tuple(bad[0]))


def to_numpy(planes):
    """render_aovs(device=True) -> what the host call returns: ids and costs are int64 tensors of the unsigned values"""
    return {name: (t.cpu().numpy() if ra.AOV_PLANES[name][2] is np.float32 else t.cpu().numpy().astype(np.uint32)) for name, t in planes.items()}


@pytest.fixture(scope="module")
def default_planes(built):
    """every plane of the mixed scene from a default context, computed once: what the invariance tests compare with"""
    return ref.viewport("mixed").render_aovs(ref.params(), ref.ALL_PLANES)


# ---- 1. geometry planes against the oracle's path records ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, lens", [("mixed", False), ("mixed", True), ("textured", False)], ids=["pinhole", "dof_hexagon_barrel", "textured_pinhole"])
def test_geometry_planes_equal_the_oracles_first_vertices(built, name, lens):
    """"mixed" has no textures (k_aov_resolve<3>); "textured" takes the generic kernel, normal maps applied (k_aov_resolve<0>)"""
    expected = ref.oracle_first_vertices(name, lens)
    p = ref.params(lens)
    if lens:
        assert p.camera.dofEnable == 1 and p.camera.bokehShape == 1 and p.camera.barrelDistortionVariableFactor != 0.0
    got = ref.viewport(name).render_aovs(p, ref.GEOMETRY_PLANES + ("material",))
    assert got["depth"].shape == (H, W) and got["position"].shape == (3, H, W) and got["texcoord"].shape == (2, H, W) and got["object_id"].dtype == np.uint32
    miss, light, mesh, analytic = ref.hit_classes(name, expected)
    print("misses %d, light hits %d, mesh hits %d, analytic hits %d" % (miss.sum(), light.sum(), mesh.sum(), analytic.sum()))
    assert miss.any() and light.any() and mesh.any() and analytic.any()
    words = ref.planes_as_vertex_words(got)                       # (pixels, 16): words 6..21 of RtPathVertex
    want = expected[:, 6:22].view(np.uint32)
    stale = ref.stale_words(name, expected)[:, 6:22]
    differs = (words != want) & ~stale
    assert not differs.any(), "pixel %d word %d differs: %#x, the oracle has %#x" % (
        tuple(int(k) for k in np.argwhere(differs)[0] + (0, 6)) + (int(words[differs][0]), int(want[differs][0])))
    assert not words[stale].any(), "a field the reference leaves unwritten is not zero"
    # the value rules on a miss and on a light
    depth = got["depth"].reshape(-1)
    assert np.isposinf(depth[miss]).all() and (got["object_id"].reshape(-1)[miss] == ref.INVALID_OBJECT).all()
    assert (words[miss][:, [1] + list(range(3, 16))] == 0).all()
    material = got["material"].reshape(-1)
    assert (material[miss | light] == ref.NO_MATERIAL).all() and (material[mesh | analytic] != ref.NO_MATERIAL).all()
    assert (got["sub_object_id"].reshape(-1)[light] == ref.LIGHT_OBJECT).all() and np.isfinite(got["position"].reshape(3, -1)[:, light]).all()


# ---- 2. material planes and the bitangent against the oracle's Debug renderer -------------------------------------------------------------------
def test_material_planes_rebuild_the_debug_renderers_colours(built):
    colours = ref.oracle_debug_colors("textured")
    got = ref.viewport("textured").render_aovs(ref.params(), tuple(ref.DEBUG_MODES) + ("object_id", "sub_object_id", "material"))
    miss = got["object_id"] == ref.INVALID_OBJECT
    light = ~miss & (got["sub_object_id"] == ref.LIGHT_OBJECT)
    desc = ref.scene("textured").desc.contents
    used = set(int(m) for m in np.unique(got["material"][~miss & ~light]))
    textured = [m for m in used if desc.materials[m].baseColorTexture != ra.RT_NO_TEXTURE or desc.materials[m].normalMapTexture != ra.RT_NO_TEXTURE or
                desc.materials[m].roughnessTexture != ra.RT_NO_TEXTURE or desc.materials[m].metalnessTexture != ra.RT_NO_TEXTURE]
    assert any(desc.materials[m].baseColorTexture != ra.RT_NO_TEXTURE for m in used) and any(desc.materials[m].normalMapTexture != ra.RT_NO_TEXTURE for m in used)
    assert any(desc.materials[m].roughnessTexture != ra.RT_NO_TEXTURE or desc.materials[m].metalnessTexture != ra.RT_NO_TEXTURE for m in used), textured
    half, zero, one = np.float32(0.5), np.float32(0.0), np.float32(1.0)
    for plane in ref.DEBUG_MODES:
        raw = got[plane]
        if plane in ("roughness", "metalness", "ior"):
            colour = np.repeat(raw[None], 3, axis=0)                  # Vector4(value)
        elif plane in ("normal", "tangent", "bitangent"):
            colour = np.minimum(one, np.maximum(zero, raw * half + half))   # x * 0.5 is exact, one rounding follows either way
        elif plane == "position":
            colour = np.maximum(zero, raw)
        else:
            colour = raw.copy()
        colour = np.moveaxis(colour, 0, -1).astype(np.float32)           # (H, W, 3), as the film
        colour[light] = (1.0, 1.0, 0.0)
        colour[miss] = 0.0
        colour = np.zeros_like(colour) + colour                          # the film adds the colour to its zeros (-0 becomes +0)
        bad = np.argwhere(colour.view(np.uint32) != colours[plane].view(np.uint32))
        assert len(bad) == 0, "%s: %d channel words differ from the Debug renderer's, first at %r" % (plane, len(bad), tuple(bad[0]))
        # the material planes of a light are 0 (its geometry planes are not)
        if plane in ref.MATERIAL_PLANES:
            assert not raw.reshape(raw.shape[0] if raw.ndim == 3 else 1, H, W)[:, light].any()
    assert got["bitangent"][:, light].any()


# ---- 3. cost planes against the oracle's per-pixel counters --------------------------------------------------------------------------------------
def test_cost_planes_equal_the_oracles_pixel_counters(built):
    counters = ref.oracle_pixel_counters("mixed")
    assert (counters[..., 0] == 1).all()   # numRays: counters 4..7 are the primary ray's and nothing else's
    p = ref.params()
    got = ref.viewport("mixed").render_aovs(p, ref.COST_PLANES)
    for k, plane in enumerate(ref.COST_PLANES):
        assert got[plane].dtype == np.uint32 and got[plane].shape == (H, W)
        bad = np.argwhere(got[plane].astype(np.uint64) != counters[..., 4 + k])
        assert len(bad) == 0, "%s: %d pixels differ, first at %r: %d, the oracle has %d" % (
            plane, len(bad), tuple(bad[0]), got[plane][tuple(bad[0])], counters[tuple(bad[0]) + (4 + k,)])
    assert got["box_tests"].any() and got["triangle_tests_passed"].any()
    # summed over the frame: what one Debug pass with the same params counts on a context with the intersection counters on
    vp = ra.Viewport(W, H, seed=ref.SEED, max_ray_depth=0)
    vp.set_renderer(ref.scene("mixed"), name="Debug", intersection_counters=True)
    vp.render_pass_with(p)
    rendered = vp.counters()
    for plane, name in zip(ref.COST_PLANES, ("numRayBoxTests", "numPassedRayBoxTests", "numRayTriangleTests", "numPassedRayTriangleTests")):
        assert int(got[plane].sum(dtype=np.uint64)) == rendered[name], (plane, name)


# ---- 4. invariance -----------------------------------------------------------------------------------------------------------------------------
def test_cost_planes_do_not_change_the_others(built, default_planes):
    """default walks without the cost planes (the 4-wide walks and their re-trace hand-over) against default walks with them (the counting binary walk)"""
    got = ref.viewport("mixed").render_aovs(ref.params(), NON_COST)
    assert list(got) == list(NON_COST)
    assert_same_planes(got, default_planes, NON_COST, "without the cost planes")
    few = ref.viewport("mixed").render_aovs(ref.params(), ("depth", "object_id"))   # no frame and no material evaluation
    assert_same_planes(few, default_planes, None, "depth and ids alone")


def test_a_counting_context_answers_alike(built, default_planes):
    vp = ref.viewport("mixed", intersection_counters=True)
    assert_same_planes(vp.render_aovs(ref.params(), ref.ALL_PLANES), default_planes, None, "intersection counters on")
    assert_same_planes(vp.render_aovs(ref.params(), NON_COST), default_planes, NON_COST, "intersection counters on, no cost planes")


def test_every_integrator_answers_alike(built, default_planes):
    vp = ref.viewport("mixed")
    ctx = vp.device_context()
    for integrator in (1, 2, 3, 4, 0):   # VCM, Path Tracer, Debug, Light Tracer, Path Tracer MIS
        assert ra.rtgpu_lib().rtgpu_set_integrator(ctx, C.c_uint32(integrator), None) == OK
        assert_same_planes(vp.render_aovs(ref.params(), ref.ALL_PLANES), default_planes, None, "integrator %d" % integrator)


def test_chunks_do_not_show(built, default_planes, monkeypatch):
    monkeypatch.setenv("RTGPU_AOV_CHUNK", "1000")   # 2590 pixels: three chunks, the last one short, none a multiple of the block
    vp = ref.viewport("mixed")
    assert_same_planes(vp.render_aovs(ref.params(), ref.ALL_PLANES), default_planes, None, "three chunks")
    assert_same_planes(to_numpy(vp.render_aovs(ref.params(), ref.ALL_PLANES, device=True)), default_planes, None, "three chunks, device tensors")


def test_shards_and_active_blocks_do_not_restrict_the_call(built, default_planes):
    multi = ref.viewport("mixed", devices=[0, 0])   # one device index, repeated: two shards
    assert_same_planes(multi.render_aovs(ref.params(), ref.ALL_PLANES), default_planes, None, "two shards")
    vp = ref.viewport("mixed")
    block = ra.RtBlock(8, 24, 4, 12)
    assert ra.rtgpu_lib().rtgpu_set_active_blocks(vp.device_context(), C.c_uint32(1), C.byref(block)) == OK
    assert_same_planes(vp.render_aovs(ref.params(), ref.ALL_PLANES), default_planes, None, "one active block")


# ---- 5. it is not a pass -----------------------------------------------------------------------------------------------------------------------
def test_a_call_leaves_the_render_state_alone(built):
    """three passes with kernel timing on: uninterrupted; with a render_aovs call between the second and the third; and with a plain rtgpu_synchronize at that
    point, which submits the two queued passes as the call does (the launch sequence of a batch depends on how many passes ride in it, so the launch counts are
    compared with that run)"""
    lib = ra.rtgpu_lib()

    def three_passes(between):
        vp = ra.Viewport(W, H, seed=ref.SEED, max_ray_depth=3)
        vp.set_renderer(ref.scene("mixed"))
        ctx = vp.device_context()
        assert lib.rtgpu_enable_timing(ctx, 1) == OK
        cam = ref.camera()
        got = None
        for k in range(3):
            p = vp.next_pass_params(cam)
            if k == 2 and between == "aovs":   # between the second and the third pass, while they are still queued
                before = vp.passes_finished
                got = vp.render_aovs(p, ref.ALL_PLANES)
                assert vp.passes_finished == before
            elif k == 2 and between == "synchronize":
                assert lib.rtgpu_synchronize(ctx) == OK
            vp.render_pass_with(p)
        s, s2 = vp.sum_buffer(secondary=True)
        raw = ra.RtCounters()
        assert lib.rtgpu_get_counters(ctx, C.byref(raw)) == 0
        ms, launches, names = (C.c_double * 8)(), (C.c_uint64 * 8)(), (C.c_char_p * 8)()
        assert lib.rtgpu_get_kernel_times(ctx, ms, launches, names) == OK
        launches = {names[i].decode(): int(launches[i]) for i in range(8) if names[i]}
        return s, s2, vp.counters(), bytes(raw), vp.passes_finished, got, launches
    plain, interrupted, synchronized = three_passes(None), three_passes("aovs"), three_passes("synchronize")
    assert same_words(plain[0], interrupted[0]) and same_words(plain[1], interrupted[1])
    assert plain[2] == interrupted[2] and plain[3] == interrupted[3]
    assert plain[4] == interrupted[4] == 3
    assert np.isfinite(interrupted[5]["depth"]).any() and plain[0].any()
    # the kernel times: the queued passes the call submits are timed as passes, its own launches are in no class
    print("launches: uninterrupted %r, with the call %r" % (plain[6], interrupted[6]))
    assert interrupted[6] == synchronized[6]
    assert interrupted[6]["generate"] == 2 and interrupted[6]["accumulate"] == 2 and interrupted[6]["shade"] > 0


# ---- 6. device tensors -------------------------------------------------------------------------------------------------------------------------
def test_device_tensors_equal_the_host_arrays(built, default_planes):
    import torch
    vp = ref.viewport("mixed")
    got = vp.render_aovs(ref.params(), ref.ALL_PLANES, device=True)
    for name, t in got.items():
        assert t.is_cuda and t.dtype == (torch.float32 if ra.AOV_PLANES[name][2] is np.float32 else torch.int64)
        assert tuple(t.shape) == default_planes[name].shape
    assert_same_planes(to_numpy(got), default_planes, None, "device tensors")


def test_two_streams_do_not_disturb_each_other(built, default_planes):
    import torch
    vp = ref.viewport("mixed")
    p0, p1 = ref.params(), ref.params(skip=1)
    assert (p0.sampleOffset[0], p0.sampleOffset[1]) != (p1.sampleOffset[0], p1.sampleOffset[1])
    host1 = vp.render_aovs(p1, ref.ALL_PLANES)
    assert not same_words(host1["position"], default_planes["position"])   # another pass: other rays
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s0):
        a = vp.render_aovs(p0, ref.ALL_PLANES, device=True)
    with torch.cuda.stream(s1):
        b = vp.render_aovs(p1, ref.ALL_PLANES, device=True)
    with torch.cuda.stream(s0):
        c = vp.render_aovs(p1, NON_COST, device=True)
    s0.synchronize()
    s1.synchronize()
    assert_same_planes(to_numpy(a), default_planes, None, "stream 0")
    assert_same_planes(to_numpy(b), host1, None, "stream 1")
    assert_same_planes(to_numpy(c), host1, NON_COST, "stream 0, second call")


# ---- 7. statuses through the raw ABI -----------------------------------------------------------------------------------------------------------
def raw_call(ctx, p, planes, outputs="own", count=None, entry="rtgpu_render_aovs", planes_ptr=True):
    ids = (C.c_uint32 * max(len(planes), 1))(*planes)
    keep = [np.zeros(3 * W * H, dtype=np.uint32) for _ in planes]
    ptrs = (C.c_void_p * max(len(planes), 1))(*[a.ctypes.data for a in keep]) if outputs == "own" else outputs
    n = len(planes) if count is None else count
    args = (ctx, C.byref(p) if p is not None else None, ids if planes_ptr else None, C.c_uint32(n), ptrs)
    if entry == "rtgpu_render_aovs_async":
        args += (None,)
    return getattr(ra.rtgpu_lib(), entry)(*args)


def changed(p, **fields):
    q = ra.RtPassParams.from_buffer_copy(p)
    q._seed_keepalive = p._seed_keepalive
    for k, v in fields.items():
        setattr(q, k, v)
    return q


def test_statuses(built):
    lib = ra.rtgpu_lib()
    scene, p = ref.scene("mixed"), ref.params()
    # before rtgpu_upload_scene, then before rtgpu_resize
    ctx = C.c_void_p()
    assert lib.rtgpu_create(0, C.byref(ctx)) == OK
    try:
        assert raw_call(ctx, p, [0]) == NOT_READY and raw_call(ctx, p, [0], entry="rtgpu_render_aovs_async") == NOT_READY
        assert lib.rtgpu_upload_scene(ctx, scene.desc) == OK
        assert raw_call(ctx, p, [0]) == NOT_READY
        assert raw_call(ctx, p, [], count=0) == OK and raw_call(ctx, None, [], outputs=None, count=0, planes_ptr=False) == OK   # nothing to do
    finally:
        lib.rtgpu_destroy(ctx)

    vp = ref.viewport("mixed")
    ctx = vp.device_context()
    assert vp.render_aovs(p, ("depth",))["depth"].shape == (H, W)   # (the renderer uploads its scene on first use: the wrapper sees to it)
    last = ra.AOV_PLANES["triangle_tests_passed"][0]
    for entry in ("rtgpu_render_aovs", "rtgpu_render_aovs_async"):
        assert raw_call(ctx, p, [], count=0, entry=entry) == OK
        assert raw_call(ctx, None, [0], entry=entry) == INVALID_ARGUMENT
        assert raw_call(ctx, p, [0], outputs=None, entry=entry) == INVALID_ARGUMENT
        assert raw_call(ctx, p, [0], planes_ptr=False, entry=entry) == INVALID_ARGUMENT
        assert raw_call(ctx, p, [0], outputs=(C.c_void_p * 1)(None), entry=entry) == INVALID_ARGUMENT
        assert raw_call(ctx, p, [last + 1], entry=entry) == INVALID_ARGUMENT and b"unknown" in lib.rtgpu_last_error()
        assert raw_call(ctx, p, [0, 0xFFFFFFFF], entry=entry) == INVALID_ARGUMENT
        assert raw_call(ctx, p, [2, 0, 2], entry=entry) == INVALID_ARGUMENT and b"twice" in lib.rtgpu_last_error()
        # what rtgpu_render_pass refuses in the params
        assert raw_call(ctx, changed(p, numDimensions=4097), [0], entry=entry) == INVALID_ARGUMENT
        assert raw_call(ctx, changed(p, seed=C.POINTER(C.c_uint32)()), [0], entry=entry) == INVALID_ARGUMENT
        assert raw_call(ctx, changed(p, maxRayDepth=255), [0], entry=entry) == INVALID_ARGUMENT
        bokeh = changed(p)
        bokeh.camera.dofEnable, bokeh.camera.bokehShape = 1, 3
        assert raw_call(ctx, bokeh, [0], entry=entry) == lib.rtgpu_render_pass(ctx, C.byref(bokeh)) == UNSUPPORTED
    assert raw_call(ctx, p, [0, last]) == OK
    # the async entry point takes device pointers, 16-byte aligned
    import torch
    t = torch.zeros(W * H + 4, dtype=torch.float32, device="cuda")
    assert raw_call(ctx, p, [0], outputs=(C.c_void_p * 1)(t.data_ptr() + 4), entry="rtgpu_render_aovs_async") == INVALID_ARGUMENT
    assert raw_call(ctx, p, [0], outputs=(C.c_void_p * 1)(t.data_ptr()), entry="rtgpu_render_aovs_async") == OK
    assert lib.rtgpu_synchronize(ctx) == OK
    with pytest.raises(ValueError):
        vp.render_aovs(changed(p, maxRayDepth=255), ("depth",))
