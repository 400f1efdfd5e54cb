"""Guide chains on the device (rtgpu_render_aovs_chain, rtgpu_set_guide_chain; Viewport.render_aovs(chain=N), Viewport.set_guide_chain) against the rule of
include/rtgpu.h folded over the CPU oracle's path recordings (tests/guide_chain_ref.py), on 70 x 37 frames, every pixel.

Bar: BIT-EQUAL words, as for the first-hit planes (tests/test_gpu_aovs.py): both sides run the reference's arithmetic in its order.  The words the reference
leaves unwritten in a vertex (path_records_ref.stale_mask) must be zero in the planes.  tests/test_guide_chain_cpu.py asserts, from the oracle alone, that the
frames hold every case: chains of one, two and three vertices, stops on diffuse surfaces, on plastic, by maxChain, on the sky, on the light, by the depth limit and
by roulette."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aov_ref
import guide_chain_ref as ref
import scene_zoo
import raytracer_amd as ra

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARGUMENT, NOT_READY, UNSUPPORTED = 0, -1, -5, -6
W, H = ref.W, ref.H
NON_COST = tuple(n for n in ra.AOV_PLANES if n not in aov_ref.COST_PLANES)
CHAIN_PLANES = tuple(ra.AOV_CHAIN_PLANES)
ALL_CHAIN = NON_COST + CHAIN_PLANES
MATERIAL_PLANES = aov_ref.MATERIAL_PLANES


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_planes(a, b, names, what=""):
    for name in names:
        bad = np.argwhere(words(a[name]) != words(b[name]))
        assert a[name].shape == b[name].shape and len(bad) == 0, "%s: plane %s differs in %d words, first at %r" % (what, name, len(bad), tuple(bad[0]))


def to_numpy(planes):
    table = dict(ra.AOV_PLANES, **ra.AOV_CHAIN_PLANES)
    return {name: (t.cpu().numpy() if table[name][2] is np.float32 else t.cpu().numpy().astype(np.uint32)) for name, t in planes.items()}


def assert_equals_the_fold(got, frame, desc, max_chain, what):
    """geometry planes against the fold's guide vertex (words 6..21) outside the stale words and zero inside them; the three chain planes against the fold"""
    k, distance, throughput, guides, stale = ref.folded_frame(frame, desc, max_chain)
    have = aov_ref.planes_as_vertex_words(got)
    want, masked = guides[:, 6:22].view(np.uint32), stale[:, 6:22]
    differs = (have != want) & ~masked
    assert not differs.any(), "%s: pixel %d word %d differs: %#x, the fold's vertex has %#x (chain length %d)" % (
        (what,) + tuple(int(i) for i in np.argwhere(differs)[0] + (0, 6)) + (int(have[differs][0]), int(want[differs][0]), int(k[np.argwhere(differs)[0][0]])))
    assert not have[masked].any(), "%s: a field the reference leaves unwritten is not zero" % what
    length, dist_words, tp_words = ref.chain_planes_as_words(got)
    assert np.array_equal(length, k), "%s: chain_length differs at pixel %d" % (what, int(np.argwhere(length != k)[0][0]))
    assert np.array_equal(dist_words, distance.view(np.uint32)), "%s: chain_distance differs at pixel %d" % (what, int(np.argwhere(dist_words != distance.view(np.uint32))[0][0]))
    assert np.array_equal(tp_words, np.ascontiguousarray(throughput).view(np.uint32)), "%s: chain_throughput differs" % what
    return k, guides


# ---- 1. the oracle ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling_all, lens, roulette", [(False, False, False), (True, False, False), (False, True, False), (True, True, False), (False, False, True),
                                                          (True, False, True)],
                         ids=["single", "all", "single_lens", "all_lens", "single_roulette", "all_roulette"])
def test_hall_equals_the_fold_over_the_oracles_paths(built, walk, sampling_all, lens, roulette):
    frame = ref.oracle_frame("hall", sampling_all, lens, roulette)
    p = ref.params(sampling_all, lens, roulette)
    assert p.minRussianRouletteDepth == (0 if roulette else ref.NO_ROULETTE) and p.maxRayDepth == ref.MAX_RAY_DEPTH
    vp = ref.viewport("hall", sampling_all, roulette, intersection_counters=walk == "counting")
    desc = ref.scene("hall").desc.contents
    for max_chain in (1, 2, 3, 16):
        got = vp.render_aovs(p, aov_ref.GEOMETRY_PLANES + CHAIN_PLANES, chain=max_chain)
        k, _ = assert_equals_the_fold(got, frame, desc, max_chain, "maxChain %d" % max_chain)
        print("maxChain %d: chain lengths %r" % (max_chain, np.bincount(k).tolist()))
        assert k.max() == min(max_chain, ref.MAX_RAY_DEPTH) or max_chain == 16
        assert got["chain_length"].dtype == np.uint32 and got["chain_length"].shape == (H, W) and got["chain_throughput"].shape == (3, H, W)
    assert k.max() >= 4   # (maxChain 16: the facing mirrors and the sphere's inside)


# ---- 2. material planes -------------------------------------------------------------------------------------------------------------------------
def test_hall_material_planes_are_the_guide_vertexs_material(built):
    frame, p, desc = ref.oracle_frame("hall"), ref.params(), ref.scene("hall").desc.contents
    got = ref.viewport("hall").render_aovs(p, MATERIAL_PLANES + ("material", "chain_length"), chain=3)
    k, _, _, guides, _ = ref.folded_frame(frame, desc, 3)
    surface = np.array([ref.is_surface(g) for g in guides])
    index = np.array([ref.material_of(g, desc) if s else ref.NO_MATERIAL for g, s in zip(guides, surface)], dtype=np.uint32)
    assert np.array_equal(got["material"].reshape(-1), index)
    want = {name: np.zeros((3 if name in ("base_color", "emission") else 1, H * W), dtype=np.float32) for name in MATERIAL_PLANES}
    for i in np.nonzero(surface)[0]:
        m = desc.materials[int(index[i])]
        want["base_color"][:, i], want["emission"][:, i] = m.baseColor[:3], m.emission[:3]
        want["roughness"][0, i], want["metalness"][0, i], want["ior"][0, i] = m.roughness, m.metalness, m.IoR
    for name in MATERIAL_PLANES:
        assert np.array_equal(words(got[name]).reshape(want[name].shape[0], -1), words(want[name])), name
    kinds = set(desc.materials[int(m)].bsdf for m in index[surface & (k >= 1)])
    assert len(kinds) >= 3 and (~surface & (k >= 1)).sum() >= 16   # several kinds of surface seen in the mirrors; lights and sky there are 0


@pytest.fixture(scope="module")
def textured(built):
    """the textured frame at maxChain 3: every plane from the device, the oracle's paths, the device's own recording of every pixel"""
    p = ref.params()
    vp = ref.viewport("textured")
    got = vp.render_aovs(p, ALL_CHAIN, chain=3)
    recorded = [v for v, _, _ in vp.record_paths(p, [(x, y) for y in range(H) for x in range(W)])]
    return dict(p=p, vp=vp, got=got, recorded=recorded, frame=ref.oracle_frame("textured"), desc=ref.scene("textured").desc.contents)


def test_textured_geometry_equals_the_fold_over_the_oracles_paths(textured):
    """the generic kernels (kLean = 0): normal maps on the mesh, on the sphere and on the mirror itself"""
    t = textured
    k, guides = assert_equals_the_fold(t["got"], t["frame"], t["desc"], 3, "textured")
    surface = np.array([ref.is_surface(g) for g in guides])
    index = np.array([ref.material_of(g, t["desc"]) if s else ref.NO_MATERIAL for g, s in zip(guides, surface)], dtype=np.uint32)
    assert np.array_equal(t["got"]["material"].reshape(-1), index)
    # the stale-material rule: the light seen in the normal-mapped mirror, evaluated with the mirror's material still in place
    lit = (k >= 1) & (guides[:, 7].view(np.uint32) == ref.LIGHT_OBJECT)
    mapped = [i for i in np.nonzero(lit)[0] if t["desc"].materials[ref.material_of(t["frame"][i][k[i] - 1], t["desc"])].normalMapTexture != ra.RT_NO_TEXTURE]
    assert len(mapped) >= 8
    assert (t["got"]["material"].reshape(-1)[lit] == ref.NO_MATERIAL).all() and not t["got"]["base_color"].reshape(3, -1)[:, lit].any()


def test_textured_equals_the_fold_over_the_devices_own_recording(textured):
    """the same fold over Viewport.record_paths of every pixel: whatever the recorder's vertices hold, the chain call holds for the guide vertex"""
    t = textured
    assert_equals_the_fold(t["got"], t["recorded"], t["desc"], 3, "textured, device recording")


def test_textured_base_colour_is_the_constant_times_the_texel(textured):
    """Material::EvaluateShadingData for a base-colour texture is one rounded multiply of the constant and the texel (materialEvaluateShadingData): checked against
    rtgpu_evaluate_textures at the texcoord plane, at the guide vertices behind the mirror and everywhere else"""
    t = textured
    got, desc = t["got"], t["desc"]
    material = got["material"].reshape(-1)
    pixels = [i for i in range(H * W) if material[i] != ref.NO_MATERIAL and desc.materials[int(material[i])].baseColorTexture != ra.RT_NO_TEXTURE]
    behind = [i for i in pixels if got["chain_length"].reshape(-1)[i] >= 1]
    assert len(pixels) > 200 and len(behind) >= 1
    idx = np.array([desc.materials[int(material[i])].baseColorTexture for i in pixels], dtype=np.uint32)
    uv = np.ascontiguousarray(got["texcoord"].reshape(2, -1).T[pixels], dtype=np.float32)
    texel = np.zeros((len(pixels), 4), dtype=np.float32)
    assert ra.rtgpu_lib().rtgpu_evaluate_textures(t["vp"].device_context(), C.c_uint32(len(pixels)), idx.ctypes.data_as(C.c_void_p), uv.ctypes.data_as(C.c_void_p),
                                                  texel.ctypes.data_as(C.c_void_p)) == OK
    constant = np.array([desc.materials[int(material[i])].baseColor[:3] for i in pixels], dtype=np.float32)
    assert np.array_equal(words(got["base_color"].reshape(3, -1).T[pixels]), words(constant * texel[:, :3]))


# ---- 3. identities ------------------------------------------------------------------------------------------------------------------------------
def test_chain_zero_is_the_first_hit_call(built):
    for name in ("hall", "textured"):
        vp, p = ref.viewport(name), ref.params()
        first = vp.render_aovs(p, NON_COST)
        got = vp.render_aovs(p, ALL_CHAIN, chain=0)
        assert_same_planes(got, first, NON_COST, "%s, chain=0" % name)
        assert not got["chain_length"].any() and np.array_equal(words(got["chain_distance"]), words(first["depth"])) and (got["chain_throughput"] == 1.0).all()


def test_nothing_passes_in_a_diffuse_scene(built):
    scene, _ = scene_zoo.mesh_scene(W / H, triangles=2000, with_analytic=False)
    bn = ra.load_blue_noise()
    scene.desc.contents.blueNoise = bn.ctypes.data
    vp = ra.Viewport(W, H, **ref.viewport_args())
    vp.set_renderer(scene)
    p = vp.next_pass_params(aov_ref.camera())
    first = vp.render_aovs(p, NON_COST)
    assert np.isfinite(first["depth"]).any() and np.isinf(first["depth"]).any()
    for max_chain in (1, 3, 16):
        got = vp.render_aovs(p, ALL_CHAIN, chain=max_chain)
        assert_same_planes(got, first, NON_COST, "maxChain %d" % max_chain)
        assert not got["chain_length"].any() and (got["chain_throughput"] == 1.0).all() and np.array_equal(words(got["chain_distance"]), words(first["depth"]))


def test_plastic_is_never_passed(built):
    vp, p, desc = ref.viewport("hall"), ref.params(), ref.scene("hall").desc.contents
    first = vp.render_aovs(p, ("material",))["material"]
    plastic = np.isin(first, [m for m in range(desc.numMaterials) if desc.materials[m].bsdf in ref.PLASTIC_BSDFS])
    assert plastic.sum() >= 30
    for max_chain in (1, 3, 16):
        got = vp.render_aovs(p, ("chain_length", "material"), chain=max_chain)
        assert not got["chain_length"][plastic].any() and np.array_equal(got["material"][plastic], first[plastic])


# ---- 4. plumbing --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def default_planes(built):
    return ref.viewport("hall").render_aovs(ref.params(), ALL_CHAIN, chain=3)


def test_chunks_do_not_show(built, default_planes, monkeypatch):
    monkeypatch.setenv("RTGPU_AOV_CHUNK", "1000")   # 2590 pixels: three chunks, the last one short, none a multiple of the block
    vp = ref.viewport("hall")
    assert_same_planes(vp.render_aovs(ref.params(), ALL_CHAIN, chain=3), default_planes, ALL_CHAIN, "three chunks")
    assert_same_planes(to_numpy(vp.render_aovs(ref.params(), ALL_CHAIN, device=True, chain=3)), default_planes, ALL_CHAIN, "three chunks, device tensors")


def test_device_tensors_and_two_streams(built, default_planes):
    import torch
    vp = ref.viewport("hall")
    p0, p1 = ref.params(), ref.params(skip=1)
    got = vp.render_aovs(p0, ALL_CHAIN, device=True, chain=3)   # on the current (default) stream
    for name, t in got.items():
        assert t.is_cuda and t.dtype == (torch.int64 if name in ("object_id", "sub_object_id", "material", "chain_length") else torch.float32)
        assert tuple(t.shape) == default_planes[name].shape
    assert_same_planes(to_numpy(got), default_planes, ALL_CHAIN, "device tensors")
    host1 = vp.render_aovs(p1, ALL_CHAIN, chain=2)
    assert not np.array_equal(words(host1["position"]), words(default_planes["position"]))   # another pass, another maxChain
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s0):
        a = vp.render_aovs(p0, ALL_CHAIN, device=True, chain=3)
    with torch.cuda.stream(s1):
        b = vp.render_aovs(p1, ALL_CHAIN, device=True, chain=2)
    with torch.cuda.stream(s0):
        c = vp.render_aovs(p1, CHAIN_PLANES, device=True, chain=2)
    s0.synchronize()
    s1.synchronize()
    assert_same_planes(to_numpy(a), default_planes, ALL_CHAIN, "stream 0")
    assert_same_planes(to_numpy(b), host1, ALL_CHAIN, "stream 1")
    assert_same_planes(to_numpy(c), host1, CHAIN_PLANES, "stream 0, second call")


def test_a_multi_device_context_answers_alike(built, default_planes):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    vp = ref.viewport("hall", devices=[0, 1])
    assert_same_planes(vp.render_aovs(ref.params(), ALL_CHAIN, chain=3), default_planes, ALL_CHAIN, "two devices")


def test_shards_active_blocks_and_integrators_do_not_restrict_the_call(built, default_planes):
    multi = ref.viewport("hall", devices=[0, 0])   # one device index, repeated: two shards
    assert_same_planes(multi.render_aovs(ref.params(), ALL_CHAIN, chain=3), default_planes, ALL_CHAIN, "two shards")
    vp = ref.viewport("hall")
    block = ra.RtBlock(8, 24, 4, 12)
    assert ra.rtgpu_lib().rtgpu_set_active_blocks(vp.device_context(), C.c_uint32(1), C.byref(block)) == OK
    assert_same_planes(vp.render_aovs(ref.params(), ALL_CHAIN, chain=3), default_planes, ALL_CHAIN, "one active block")
    for integrator in (1, 2, 3, 4, 0):   # VCM, Path Tracer, Debug, Light Tracer, Path Tracer MIS: the chain is the MIS path tracer's path whichever is selected
        assert ra.rtgpu_lib().rtgpu_set_integrator(vp.device_context(), C.c_uint32(integrator), None) == OK
        assert_same_planes(vp.render_aovs(ref.params(), ALL_CHAIN, chain=3), default_planes, ALL_CHAIN, "integrator %d" % integrator)


def test_a_call_leaves_the_render_state_alone(built, default_planes):
    """three passes, a recording and two temporal frames: uninterrupted, and with chain calls in between -- film, both sum buffers, counters, the queued passes, the
    recorder's answer and the temporal history come out the same"""
    lib = ra.rtgpu_lib()

    def run(interrupt):
        vp = ra.Viewport(W, H, seed=ref.SEED, max_ray_depth=3)
        vp.set_renderer(ref.scene("hall"))
        ctx, cam = vp.device_context(), ref.camera()
        got = None
        params = [vp.next_pass_params(cam) for _ in range(5)]
        pixels = [(x, 20) for x in range(0, W, 3)]
        for k in range(3):
            if k == 2 and interrupt:   # between the second and the third pass, while they are still queued
                before = vp.passes_finished
                got = vp.render_aovs(ref.params(), ALL_CHAIN, chain=3)
                assert vp.passes_finished == before
            vp.render_pass_with(params[k])
        recorded = vp.record_paths(params[3], pixels)
        first = vp.denoise(params[3], temporal=True, variance=True)
        if interrupt:
            vp.render_aovs(ref.params(skip=1), CHAIN_PLANES, chain=16)
            vp.render_aovs(ref.params(), ("depth",), device=True, chain=2)
        again = vp.record_paths(params[3], pixels)
        vp.render_pass_with(params[3])
        second = vp.denoise(params[4], temporal=True, variance=True)
        s, s2 = vp.sum_buffer(secondary=True)
        raw = ra.RtCounters()
        assert lib.rtgpu_get_counters(ctx, C.byref(raw)) == 0
        return dict(s=s, s2=s2, counters=vp.counters(), raw=bytes(raw), passes=vp.passes_finished, got=got, recorded=recorded, again=again, first=first, second=second)
    plain, cut = run(False), run(True)
    assert_same_planes(cut["got"], default_planes, ALL_CHAIN, "between two queued passes")
    for name in ("s", "s2", "first", "second"):
        assert np.array_equal(words(plain[name]), words(cut[name])), name
    assert plain["counters"] == cut["counters"] and plain["raw"] == cut["raw"] and plain["passes"] == cut["passes"] == 4 and plain["s"].any()
    assert not np.array_equal(words(plain["first"]), words(plain["second"]))   # the second temporal frame does depend on the history
    for a, b in zip(plain["recorded"] + plain["again"], cut["recorded"] + cut["again"]):
        assert np.array_equal(words(a[0]), words(b[0])) and a[1] == b[1] and np.array_equal(words(a[2]), words(b[2]))


# ---- 5. statuses through the raw ABI ------------------------------------------------------------------------------------------------------------
def raw_call(ctx, p, planes, chain=(2, 0), outputs="own", count=None, entry="rtgpu_render_aovs_chain", planes_ptr=True):
    ids = (C.c_uint32 * max(len(planes), 1))(*planes)
    keep = [np.zeros(3 * W * H, dtype=np.uint32) for _ in planes]
    ptrs = (C.c_void_p * max(len(planes), 1))(*[a.ctypes.data for a in keep]) if outputs == "own" else outputs
    n = len(planes) if count is None else count
    desc = ra.RtAovChain(*chain) if chain is not None else None
    args = (ctx, C.byref(p) if p is not None else None)
    if "chain" in entry:
        args += (C.byref(desc) if desc is not None else None,)
    args += (ids if planes_ptr else None, C.c_uint32(n), ptrs)
    if entry.endswith("_async"):
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
    scene, p = ref.scene("hall"), ref.params()
    ctx = C.c_void_p()
    assert lib.rtgpu_create(0, C.byref(ctx)) == OK
    try:
        assert raw_call(ctx, p, [0]) == NOT_READY and raw_call(ctx, p, [0], entry="rtgpu_render_aovs_chain_async") == NOT_READY
        assert lib.rtgpu_upload_scene(ctx, scene.desc) == OK
        assert raw_call(ctx, p, [0]) == NOT_READY
        assert raw_call(ctx, p, [], count=0) == OK   # nothing to do
        assert lib.rtgpu_set_guide_chain(ctx, C.byref(ra.RtAovChain(17, 0))) == INVALID_ARGUMENT and lib.rtgpu_set_guide_chain(ctx, C.byref(ra.RtAovChain(1, 1))) == INVALID_ARGUMENT
        assert lib.rtgpu_set_guide_chain(ctx, C.byref(ra.RtAovChain(16, 0))) == OK and lib.rtgpu_set_guide_chain(ctx, None) == OK
    finally:
        lib.rtgpu_destroy(ctx)

    vp = ref.viewport("hall")
    ctx = vp.device_context()
    assert vp.render_aovs(p, ("depth",), chain=1)["depth"].shape == (H, W)   # (the renderer uploads its scene on first use: the wrapper sees to it)
    length, throughput = ra.AOV_CHAIN_PLANES["chain_length"][0], ra.AOV_CHAIN_PLANES["chain_throughput"][0]
    for entry in ("rtgpu_render_aovs_chain", "rtgpu_render_aovs_chain_async"):
        assert raw_call(ctx, p, [], count=0, entry=entry) == OK
        assert raw_call(ctx, p, [0], chain=None, entry=entry) == INVALID_ARGUMENT and b"chain" in lib.rtgpu_last_error()
        assert raw_call(ctx, p, [0], chain=(17, 0), entry=entry) == INVALID_ARGUMENT and b"maxChain" in lib.rtgpu_last_error()
        assert raw_call(ctx, p, [0], chain=(2, 1), entry=entry) == INVALID_ARGUMENT and b"flags" in lib.rtgpu_last_error()
        assert raw_call(ctx, None, [0], entry=entry) == INVALID_ARGUMENT
        assert raw_call(ctx, p, [0], outputs=None, entry=entry) == INVALID_ARGUMENT
        assert raw_call(ctx, p, [0], planes_ptr=False, entry=entry) == INVALID_ARGUMENT
        assert raw_call(ctx, p, [0], outputs=(C.c_void_p * 1)(None), entry=entry) == INVALID_ARGUMENT
        for cost in aov_ref.COST_PLANES:
            assert raw_call(ctx, p, [0, ra.AOV_PLANES[cost][0]], entry=entry) == INVALID_ARGUMENT and b"cost" in lib.rtgpu_last_error()
        assert raw_call(ctx, p, [throughput + 1], entry=entry) == INVALID_ARGUMENT and b"unknown" in lib.rtgpu_last_error()
        assert raw_call(ctx, p, [0, 0xFFFFFFFF], entry=entry) == INVALID_ARGUMENT
        assert raw_call(ctx, p, [length, 0, length], entry=entry) == INVALID_ARGUMENT and b"twice" in lib.rtgpu_last_error()
        # what rtgpu_render_pass refuses in the params
        assert raw_call(ctx, changed(p, numDimensions=4097), [0], entry=entry) == INVALID_ARGUMENT
        assert raw_call(ctx, changed(p, maxRayDepth=255), [0], entry=entry) == INVALID_ARGUMENT
        bokeh = changed(p)
        bokeh.camera.dofEnable, bokeh.camera.bokehShape = 1, 3
        assert raw_call(ctx, bokeh, [0], entry=entry) == UNSUPPORTED
    # the chain planes belong to the chain entries alone
    for plane in (length, throughput):
        assert raw_call(ctx, p, [plane], entry="rtgpu_render_aovs") == INVALID_ARGUMENT and raw_call(ctx, p, [plane], entry="rtgpu_render_aovs_async") == INVALID_ARGUMENT
    assert raw_call(ctx, p, [0, length, throughput], chain=(16, 0)) == OK and raw_call(ctx, p, [0], chain=(0, 0)) == OK
    import torch
    t = torch.zeros(W * H + 4, dtype=torch.float32, device="cuda")
    assert raw_call(ctx, p, [length], outputs=(C.c_void_p * 1)(t.data_ptr() + 4), entry="rtgpu_render_aovs_chain_async") == INVALID_ARGUMENT
    assert raw_call(ctx, p, [length], outputs=(C.c_void_p * 1)(t.data_ptr()), entry="rtgpu_render_aovs_chain_async") == OK
    assert lib.rtgpu_synchronize(ctx) == OK
    with pytest.raises(ValueError):
        vp.render_aovs(p, ("depth",), chain=17)
    with pytest.raises(ValueError, match="chain=N"):
        vp.render_aovs(p, ("chain_length",))


# ---- 6. denoise ---------------------------------------------------------------------------------------------------------------------------------
def test_denoise_under_a_guide_chain_is_the_filter_over_the_chain_planes(built):
    vp = ra.Viewport(W, H, **ref.viewport_args())
    vp.set_renderer(ref.scene("hall"))
    cam = ref.camera()
    params = [vp.next_pass_params(cam) for _ in range(6)]
    for p in params[:4]:
        vp.render_pass_with(p)
    guide = params[4]
    sigmas = dict(sigma_normal=0.3, sigma_plane=0.2)
    calls = dict(plain=lambda **kw: vp.denoise(guide, iterations=3, sigma_color=1.5, **sigmas, **kw),
                 variance=lambda **kw: vp.denoise(guide, iterations=3, variance=True, return_variance=True, sigma_lum=3.0, **sigmas, **kw))
    before = {name: call() for name, call in calls.items()}
    history = vp.denoise(guide, temporal=True)
    vp.set_guide_chain(3)
    s, s2 = vp.sum_buffer(secondary=True)
    g = vp.render_aovs(guide, ("depth", "normal", "position", "base_color", "chain_length"), chain=3)
    assert (g["chain_length"] >= 1).sum() > 300
    want = ra.atrous_filter(s, g["depth"], g["normal"], g["position"], g["base_color"], iterations=3, sigma_color=1.5, color_scale=0.25, **sigmas)
    want_v = ra.atrous_filter(s, g["depth"], g["normal"], g["position"], g["base_color"], iterations=3, color_half=s2, sigma_lum=3.0, color_scale=0.25, return_variance=True, **sigmas)
    got, got_v = calls["plain"](), calls["variance"]()
    assert np.array_equal(words(got), words(want)) and not np.array_equal(words(got), words(before["plain"]))
    assert np.array_equal(words(got_v[0]), words(want_v[0])) and np.array_equal(words(got_v[1]), words(want_v[1]))
    assert np.array_equal(words(calls["plain"](device=True).cpu().numpy()), words(want))
    # the guides changed inside the mirrors and the glass
    changed_pixels = np.any(words(got) != words(before["plain"]), axis=-1)
    assert changed_pixels[g["chain_length"] >= 1].any()
    # temporal accumulation does not reproject through a chain, and a refused call leaves the history alone
    for kw in (dict(temporal=True), dict(temporal=True, clip=True), dict(temporal=True, device=True)):
        with pytest.raises(RuntimeError, match=r"\(-6\)"):
            vp.denoise(guide, **kw)
    vp.set_guide_chain(None)
    after = {name: call() for name, call in calls.items()}
    assert np.array_equal(words(after["plain"]), words(before["plain"]))
    assert np.array_equal(words(after["variance"][0]), words(before["variance"][0])) and np.array_equal(words(after["variance"][1]), words(before["variance"][1]))
    vp.render_pass_with(guide)
    continued = vp.denoise(params[5], temporal=True)

    # the same two temporal frames on a context that never had a chain
    vp2 = ra.Viewport(W, H, **ref.viewport_args())
    vp2.set_renderer(ref.scene("hall"))
    params2 = [vp2.next_pass_params(cam) for _ in range(6)]
    for p in params2[:4]:
        vp2.render_pass_with(p)
    assert np.array_equal(words(vp2.denoise(params2[4], temporal=True)), words(history))
    vp2.render_pass_with(params2[4])
    assert np.array_equal(words(vp2.denoise(params2[5], temporal=True)), words(continued))
    assert not np.array_equal(words(history), words(continued))


# ---- 7. the headless demo -----------------------------------------------------------------------------------------------------------------------
DEMO_SCENE = """{
    "materials": [
        { "name": "floor", "bsdf": "diffuse", "baseColor": [0.7, 0.6, 0.5] },
        { "name": "ball", "bsdf": "diffuse", "baseColor": [0.2, 0.6, 0.9] },
        { "name": "mirror", "bsdf": "metal", "baseColor": [0.95, 0.95, 0.95] }
    ],
    "objects": [
        { "type": "plane", "size": [12.0, 12.0], "material": "floor", "transform": { "translation": [0.0, -2.5, 0.0], "orientation": [-90.0, 0.0, 0.0] } },
        { "type": "sphere", "radius": 1.1, "material": "ball", "transform": { "translation": [3.0, -1.4, 3.5] } },
        { "type": "plane", "size": [2.5, 2.0], "material": "mirror", "transform": { "translation": [-1.0, 0.0, -2.0], "orientation": [0.0, 20.0, 0.0] } }
    ],
    "lights": [
        { "type": "background", "color": [0.6, 0.7, 0.9] },
        { "type": "area", "color": [18.0, 17.0, 15.0], "shape": { "type": "rect", "size": [1.5, 1.5] },
          "transform": { "translation": [0.0, 7.0, 1.0], "orientation": [90.0, 0.0, 0.0] } }
    ],
    "camera": { "transform": { "translation": [1.0, 2.5, 13.0], "orientation": [10.0, 180.0, 0.0] }, "fieldOfView": 48.0 }
}
"""


def test_rt_demo_guide_chain_changes_the_frame_around_the_mirror_only(built, tmp_path):
    """rt_demo --guide-chain 2 --denoise 2: the frame differs from the one filtered with first-hit guides, and only where the filter can see the mirror.  Two levels
    of the 5 x 5 a-trous kernel reach 2 * (1 + 2) = 6 pixels: a pixel further than that from every pixel with chain_length >= 1 takes no tap whose guides
    changed, so its filtered colour -- and the byte the tone mapper makes of it -- is the same in both frames."""
    w, h, levels = 64, 48, 2
    path = tmp_path / "scene.json"
    path.write_text(DEMO_SCENE)
    demo = os.path.join(ROOT, "raytracer_amd", "lib", "rt_demo")
    images = {}
    for label, extra in (("first_hit", []), ("chain", ["--guide-chain", "2"])):
        out = str(tmp_path / (label + ".bmp"))
        r = subprocess.run([demo, "-s", str(path), "--width", str(w), "--height", str(h), "--passes", "2", "--depth", "3", "--seed", "11", "--denoise", str(levels)] + extra +
                           ["--output", out], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("guides: chains of at most 2" in r.stdout) == (label == "chain"), r.stdout
        data = open(out, "rb").read()
        assert len(data) == 54 + w * h * 3
        images[label] = np.frombuffer(data[54:], dtype=np.uint8).reshape(h, w, 3)[::-1]   # rows bottom-up in the file
    r = subprocess.run([demo, "-s", str(path), "--guide-chain", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--denoise" in r.stderr
    r = subprocess.run([demo, "-s", str(path), "--denoise", "--guide-chain", "17"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "0..16" in r.stderr
    # chain_length of the demo's guide pass: the third pass of the same seed's sequence, through the same loader
    scene, cam = ra.Scene(), ra.Camera()
    scene.load_json(str(path), camera=cam)
    scene.build()
    cam.set_perspective(w / h, np.float32(48.0) / np.float32(180.0) * np.float32(3.14159265359))   # the file's fieldOfView, as rt_demo passes it back
    vp = ra.Viewport(w, h, seed=11, max_ray_depth=3)
    vp.set_renderer(scene)
    for _ in range(2):
        vp.next_pass_params(cam)
    length = vp.render_aovs(vp.next_pass_params(cam), ("chain_length",), chain=2)["chain_length"]
    mirror = length >= 1
    assert 50 < mirror.sum() < w * h // 2
    reach = 2 * ((1 << levels) - 1)
    near = np.zeros_like(mirror)
    for y, x in np.argwhere(mirror):
        near[max(0, y - reach):y + reach + 1, max(0, x - reach):x + reach + 1] = True
    differs = np.any(images["first_hit"] != images["chain"], axis=-1)
    print("%d pixels in the mirror, %d within reach of it, %d differ" % (mirror.sum(), near.sum(), differs.sum()))
    assert differs[mirror].any() and not differs[~near].any()

