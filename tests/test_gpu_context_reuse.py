"""One context, many states: what an application does with an RtgpuContext -- rtgpu_resize, rtgpu_upload_scene, rtgpu_set_integrator, rtgpu_set_shard and pass
parameters of varying depth on the same context, again and again -- held to the bar of the parity tests in every state, not only in the first.

Every other GPU test builds a fresh context per case, so the comparisons by which the runtime decides that device memory sized for an earlier state may stay
(ensurePaths, ensureVcm, the recorder's, the AOV calls', the filters' and the history's capacities; DESIGN.md section 5, "Context lifetime") were never taken with
a kept buffer behind them.  Here they are: each test walks one context through a group of transitions and probes it after each (tests/context_reuse.py: three
passes without a read-back, both sum buffers equal to the CPU oracle's as uint32 words, the counters' difference equal to the oracle's counters).  The reference in
groups 1 to 7 and 9 is the oracle and nothing else.  A probe cannot pass on two black frames: the oracle's frame of every state has lit pixels and differs from
the frame of the state before wherever the transition changes what is seen (asserted on the oracle's images alone: context_reuse.check_state_list).

Every comparison is equality of bits or of integers; the one exception is the Light Tracer leg, whose film splats are float atomics and which takes the bound
tests/test_gpu_vcm.py states for them."""
import ctypes as C

import numpy as np
import pytest

import context_reuse as cr
import guide_chain_ref
import ray_query_shim
import ref_scenes
import scene_zoo
import raytracer_amd as ra
from raytracer_amd import scenes
from context_reuse import Context, State, probe, words
from test_vcm_oracle import _two_estimator_scene

pytestmark = pytest.mark.gpu

_lists = {}
STATE_LISTS = []   # every state list of this file, for check_all_state_lists


def state_list(make):
    """registers a state list under its function's name and builds it once: [(State, its frame differs from the one before)]"""
    def cached():
        if make.__name__ not in _lists:
            _lists[make.__name__] = make()
        return _lists[make.__name__]
    cached.__name__ = make.__name__
    STATE_LISTS.append(cached)
    return cached


def check_all_state_lists():
    """the CPU half of every probe of this file: no device is touched"""
    for make in STATE_LISTS:
        cr.check_state_list(make())


def assert_zero_film(ctx, w, h, what):
    s, s2 = ctx.read(w, h)
    assert not words(s).any() and not words(s2).any(), what


# ---- 1. frame size --------------------------------------------------------------------------------------------------------------------------------
SIZES = [(96, 64), (200, 136), (67, 41), (1, 1), (96, 64)]   # grow; shrink to a size that is no multiple of 8 or 64; one pixel; a size seen before


def cornell_at(w, h, scene=None, tag="", **kw):
    s, camera = scenes.cornell_box(w / h)
    return State("cornell %dx%d%s" % (w, h, tag), scene if scene is not None else s, camera, w, h, max_ray_depth=4, **kw)


@state_list
def sizes():
    first = cornell_at(*SIZES[0])
    out, seen = [(first, False)], {SIZES[0]: first}
    for w, h in SIZES[1:]:
        if (w, h) not in seen:
            seen[w, h] = cornell_at(w, h, first.scene)
        out.append((seen[w, h], True))
    out.append((cornell_at(130, 70, first.scene), True))   # the size the context is moved to with two passes still queued
    return out


def test_frame_sizes_on_one_context(built, walk):
    """rtgpu_resize on a live context: the arenas of the lanes are sized by the slot count (ensurePaths: kept while capacity >= arenaCapacityFor(slots x batch)),
    the slot table, the film and the pass batch are rebuilt (rebuildFilm).  After every resize the film reads as zeros before any pass; then the probe.  Last,
    two passes are queued and the context is resized without a synchronising call in between: they render the old film, which is gone, and the probe of the
    new size is the oracle's three passes alone."""
    states = sizes()
    ctx = Context(walk)
    try:
        ctx.upload(states[0][0].scene)
        previous = None
        for state, _ in states[:-1]:
            ctx.resize(state.w, state.h)
            assert_zero_film(ctx, state.w, state.h, state.name)
            probe(ctx, state, previous, reset=False)
            previous = state
        last = states[-1][0]
        before = ctx.counters()
        for p in previous.params(2):
            ctx.render(p)
        ctx.resize(last.w, last.h)
        assert_zero_film(ctx, last.w, last.h, "behind two queued passes")
        # the queued passes were rendered (the counters are the context's, not the film's) before the film was replaced
        queued = cr.oracle_of(previous, 2)
        cr.assert_counters(before, ctx.counters(), queued, walk, "the two queued passes")
        probe(ctx, last, previous, reset=False)
    finally:
        ctx.close()


# ---- 2. scene class ---------------------------------------------------------------------------------------------------------------------------------
W2, H2 = 96, 64


def sky_only(aspect):
    s = ra.Scene()
    s.add_background_light((1.0, 2.0, 3.0))
    s.build()
    return s, ra.Camera((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), aspect, 90.0)


@state_list
def scene_classes():
    a = W2 / H2
    makes = [("cornell", scenes.cornell_box, {}),                                              # analytic shapes, a top-level tree
             ("mesh_single", ref_scenes.mesh_single, {}),                                      # one object: the bypass and the one-level 4-wide walk
             ("mesh_scene", lambda a: scene_zoo.mesh_scene(a, triangles=6000), {}),            # two-level 4-wide
             ("textured", lambda a: scene_zoo.textured_scene(a, triangles=2000), {}),          # the textured classes
             ("sky only", sky_only, {}),                                                       # no objects at all
             ("many lights, All", scene_zoo.many_lights_scene, dict(light_sampling_all=True, dimensions=128)),   # 16 lights: fat slots, no dense state
             ("cornell, two lights", ref_scenes.cornell_two_lights, {})]                       # Single: dense state again
    out = []
    for name, make, args in makes:
        scene, camera = make(a)
        out.append((State("class: " + name, scene, camera, W2, H2, max_ray_depth=5, **args), True))
    out.append((out[0][0], True))
    return out


def test_scene_classes_on_one_context(built, walk):
    """rtgpu_upload_scene on a live context, in an order that crosses every boundary of ensurePaths and of the kernel choice: the walk (binary, one-level 4-wide,
    two-level 4-wide and back: `wide`, `wide2`), the shading class (leanScene), no objects, 16 lights under `All` (maxLights 16: the dense pair is freed, the
    slots are fat) and back to one request per vertex (the dense pair is needed again; a kept arena would carry maxLights 16 as its record stride).  After every
    upload rtgpu_get_walk_info is that of a fresh context given only that scene, and film and counters are what the probe before left."""
    states = scene_classes()
    assert states[5][0].scene.desc.contents.numLights == 16
    ctx = Context(walk)
    try:
        ctx.resize(W2, H2)
        previous, kept = None, None
        for state, _ in states:
            ctx.upload(state.scene)
            if kept is not None:   # the film and the counters are the caller's to reset: an upload leaves them as they stand
                got, got2 = ctx.read(W2, H2)
                assert np.array_equal(words(got), words(kept[0])) and np.array_equal(words(got2), words(kept[1])) and ctx.counters() == kept[2], state.name
            fresh = Context(walk)
            try:
                fresh.upload(state.scene)
                assert ctx.walk_info() == fresh.walk_info(), state.name
            finally:
                fresh.close()
            kept = probe(ctx, state, previous) + (ctx.counters(),)
            previous = state
    finally:
        ctx.close()


# ---- 3. depth ---------------------------------------------------------------------------------------------------------------------------------------
@state_list
def depths():
    scene, camera = scene_zoo.mesh_scene(W2 / H2, triangles=6000)
    return [(State("depth %d, roulette from %d" % (d, rr), scene, camera, W2, H2, max_ray_depth=d, min_russian_roulette_depth=rr), True)
            for d, rr in ((2, 1), (12, 0), (0, 1), (5, 1))]


def test_depths_on_one_context(built):
    """maxRayDepth 2 -> 12 -> 0 -> 5 on one context: queueCounts and denseCounts hold maxDepth + 2 words per plane and only ever grow, so from the second state on
    the planes are wider than the pass needs and LaneCounts must place them by the capacity, not by the depth."""
    ctx = Context()
    try:
        states = depths()
        ctx.upload(states[0][0].scene)
        ctx.resize(W2, H2)
        previous = None
        for state, _ in states:
            probe(ctx, state, previous)
            previous = state
    finally:
        ctx.close()


# ---- 4. integrators ---------------------------------------------------------------------------------------------------------------------------------
W4, H4 = 96, 72
BIG = (200, 136)


@state_list
def integrators():
    small = _two_estimator_scene(W4 / H4)
    big_camera = _two_estimator_scene(BIG[0] / BIG[1])[1]
    scene = small[0]
    vcm4 = dict(max_path_length=4, initial_merging_radius=0.4, min_merging_radius=0.4, camera_connecting_weight=0.0)
    vcm10 = dict(vcm4, max_path_length=10)
    at = lambda name, big=False, **kw: State("integrators: " + name, scene, big_camera if big else small[1], *(BIG if big else (W4, H4)), max_ray_depth=5, **kw)   # noqa: E731
    return [(at("MIS"), False),
            (at("VCM 4", integrator=cr.VCM, vcm=vcm4), True),
            (at("VCM 4, resized", big=True, integrator=cr.VCM, vcm=vcm4), True),
            (at("VCM 10, resized", big=True, integrator=cr.VCM, vcm=vcm10), True),
            (at("VCM 10", integrator=cr.VCM, vcm=vcm10), True),
            (at("Light Tracer", integrator=cr.LIGHT_TRACER), True),
            (at("Debug normals", integrator=cr.DEBUG, debug_mode=4), True),
            (at("Debug base colour", integrator=cr.DEBUG, debug_mode=8), True),
            (at("Path Tracer", integrator=cr.PATH_TRACER), True)]


def vcm_probe(ctx, state, previous, reset):
    """three synchronised passes from pass 0: camera paths bit for bit, the counters' difference, the photon count behind every pass"""
    want = cr.check_oracle(state, previous)
    if reset:
        ctx.reset()
    assert ctx.photons() == 0, state.name   # nothing to merge with in the first pass: rtgpu_set_integrator, rtgpu_resize and rtgpu_upload_scene drop the photons
    before = ctx.counters()
    for p, photons in zip(state.params(), want["photons"]):
        ctx.render(p)
        assert ctx.photons() == photons, (state.name, p.passIndex)
    got, got2 = ctx.read(state.w, state.h)
    cr.assert_film(got, got2, want, state.name)
    cr.assert_counters(before, ctx.counters(), want, ctx.walk, state.name)
    assert want["photons"][-1] > 0


def test_integrators_on_one_context(built, walk):
    """rtgpu_set_integrator and rtgpu_resize on one context.  ensureVcm keeps every arena of the bidirectional integrator while four capacities suffice, with the
    allocation's own capacity and maxLV as the strides of what is kept: the walk goes 96 x 72 at path length 4 -> 200 x 136 (the slots grow: freed, photon grids
    included) -> path length 10 (maxLV grows) -> back to 96 x 72 (everything kept, all strides larger than the state needs).  A resize drops the photons: the
    first pass behind it merges nothing, which the oracle restarted from pass 0 says (at radius 0.4 every camera vertex would merge).  Two passes queued
    in front of the resize render the old film -- the bidirectional integrator holds its own queue (up to eight passes ride one launch sequence), and before
    this test rtgpu_resize, rtgpu_set_shard, rtgpu_reset, rtgpu_upload_scene and rtgpu_update_objects submitted only the PathTracerMIS queue: the two passes
    came out in the NEW film, at the new size.  Then the Light Tracer on the same arenas (comparison and bound of test_light_tracer_matches_the_oracle:
    1e-5 relative + 1e-6 absolute for the float-atomic splats), two debug modes, the plain path tracer, and PathTracerMIS again, which must be the first probe's
    bits."""
    states = [s for s, _ in integrators()]
    mis, vcm4, vcm4_big, vcm10_big, vcm10, lt, dbg_a, dbg_b, pt = states
    ctx = Context(walk)
    try:
        ctx.upload(mis.scene)
        ctx.resize(W4, H4)
        first = probe(ctx, mis, reset=False)
        ctx.set_integrator(vcm4)
        kept = ctx.read(W4, H4)   # the film stays until the caller resets it
        assert np.array_equal(words(kept[0]), words(first[0])) and np.array_equal(words(kept[1]), words(first[1]))
        vcm_probe(ctx, vcm4, mis, reset=True)
        # two more passes, queued: no synchronising call before the resize
        for p in vcm4.params(5)[3:]:
            ctx.render(p)
        ctx.resize(*BIG)
        assert_zero_film(ctx, *BIG, "behind two queued VCM passes")
        vcm_probe(ctx, vcm4_big, vcm4, reset=False)
        # ... and the same in front of rtgpu_reset: the film is empty behind it
        for p in vcm4_big.params(5)[3:]:
            ctx.render(p)
        ctx.reset()
        assert_zero_film(ctx, *BIG, "rtgpu_reset behind two queued VCM passes")
        ctx.set_integrator(vcm10_big)
        vcm_probe(ctx, vcm10_big, vcm4_big, reset=True)
        ctx.resize(W4, H4)
        vcm_probe(ctx, vcm10, vcm10_big, reset=False)
        # Light Tracer
        want = cr.check_oracle(lt, vcm10)
        ctx.set_integrator(lt)
        ctx.reset()
        before = ctx.counters()
        for p in lt.params():
            ctx.render(p)
        img, img2 = ctx.read(W4, H4)
        assert np.all(np.abs(img - want["sum"]) <= 1e-5 * np.abs(want["sum"]) + 1e-6), float(np.abs(img - want["sum"]).max())
        assert np.all(np.abs(img2 - want["secondary"]) <= 1e-5 * np.abs(want["secondary"]) + 1e-6)
        cr.assert_counters(before, ctx.counters(), want, walk, lt.name)
        previous = lt
        for state in (dbg_a, dbg_b, pt, mis):
            ctx.set_integrator(state)
            again = probe(ctx, state, previous)
            previous = state
        assert np.array_equal(words(again[0]), words(first[0])) and np.array_equal(words(again[1]), words(first[1]))
    finally:
        ctx.close()


# ---- 5. shards ------------------------------------------------------------------------------------------------------------------------------------------
SHARDS = [(0, 1), (1, 3), (2, 3), (0, 1)]


@state_list
def shards():
    whole = cornell_at(*BIG, tag=", shard 0 of 1")
    seen = {(0, 1): whole}
    for shard in SHARDS:
        if shard not in seen:
            seen[shard] = cornell_at(*BIG, scene=whole.scene, tag=", shard %d of %d" % shard, shard=shard)
    return [(seen[s], True) for s in SHARDS]


def test_shards_on_one_context(built):
    """rtgpu_set_shard on a live context, 200 x 136 = 12 tiles: the slot table shrinks to a third and grows back (rebuildFilm; the lanes' arenas stay).  Owned pixels
    are the oracle's rendered with shard=, every other pixel of both buffers is zero."""
    w, h = BIG
    tiles_x = (w + 63) // 64
    tile = (np.arange(h)[:, None] // 64) * tiles_x + np.arange(w)[None, :] // 64
    ctx = Context()
    try:
        states = [s for s, _ in shards()]
        ctx.upload(states[0].scene)
        ctx.resize(w, h)
        previous = None
        for state in states:
            ctx.set_shard(*state.shard)
            assert_zero_film(ctx, w, h, state.name)
            got, got2 = probe(ctx, state, previous, reset=False)
            owned = tile % state.shard[1] == state.shard[0]
            assert not words(got)[~owned].any() and not words(got2)[~owned].any() and got[owned].any(), state.name
            previous = state
    finally:
        ctx.close()


# ---- 6. active blocks ---------------------------------------------------------------------------------------------------------------------------------
@state_list
def active_blocks():
    before = cornell_at(96, 64, tag=", two blocks active")
    return [(before, False), (cornell_at(67, 41, before.scene, tag=", after active blocks"), True)]


def test_a_resize_restores_the_whole_image(built):
    """rtgpu_set_active_blocks with two blocks, two passes (the pixels of the blocks are the oracle's, every other pixel is zero), then rtgpu_resize: rebuildFilm
    clears the mask, so the probe covers the whole image."""
    (before, _), (after, _) = active_blocks()
    blocks = (ra.RtBlock * 2)(ra.RtBlock(8, 40, 8, 24), ra.RtBlock(48, 96, 32, 64))
    ctx = Context()
    try:
        ctx.upload(before.scene)
        ctx.resize(before.w, before.h)
        assert ctx.lib.rtgpu_set_active_blocks(ctx.ctx, C.c_uint32(2), blocks) == cr.OK, ctx.error()
        for p in before.params(2):
            ctx.render(p)
        got, got2 = ctx.read(before.w, before.h)
        want = cr.check_oracle(before, n=2)
        inside = np.zeros((before.h, before.w), dtype=bool)
        for b in blocks:
            inside[b.minY:b.maxY, b.minX:b.maxX] = True
        assert np.array_equal(words(got)[inside], words(want["sum"])[inside]) and np.array_equal(words(got2)[inside], words(want["secondary"])[inside])
        assert want["sum"][inside].any() and want["sum"][~inside].any() and not words(got)[~inside].any() and not words(got2)[~inside].any()
        ctx.resize(after.w, after.h)
        probe(ctx, after, before, reset=False)
    finally:
        ctx.close()


# ---- 7. refused calls -----------------------------------------------------------------------------------------------------------------------------------
@state_list
def refused():
    return [(cornell_at(96, 64, tag=", refused calls"), False)]


def bad_descriptors(scene):
    """the descriptors of test_c_abi_error_paths, made from a good one: another abiVersion; a material index out of range (the objects copied, the first shape's changed)"""
    good = scene.desc.contents
    version = ra.RtSceneDesc.from_buffer_copy(good)
    version.abiVersion = 999
    material = ra.RtSceneDesc.from_buffer_copy(good)
    objects = (ra.RtObject * good.numObjects)()
    C.memmove(objects, good.objects, C.sizeof(objects))
    shape = next(i for i in range(good.numObjects) if objects[i].objectKind != 1)   # (RT_OBJECT_LIGHT = 1)
    objects[shape].materialIndex = good.numMaterials
    material.objects = C.cast(objects, C.POINTER(ra.RtObject))
    return (version, None), (material, objects)


def test_refused_calls_change_nothing(built):
    """rtgpu_upload_scene validates before it frees and rtgpu_resize before it touches the film: after a good upload and two passes, two refused scenes and a
    refused size, a third pass completes the oracle's three -- film and counters."""
    state = refused()[0][0]
    want = cr.check_oracle(state)
    ctx = Context()
    try:
        ctx.upload(state.scene)
        ctx.resize(state.w, state.h)
        before = ctx.counters()
        p = state.params()
        ctx.render(p[0])
        ctx.render(p[1])
        for desc, _keep in bad_descriptors(state.scene):
            assert ctx.lib.rtgpu_upload_scene(ctx.ctx, C.byref(desc)) == cr.INVALID_ARGUMENT
        assert b"material" in ctx.lib.rtgpu_last_error()
        assert ctx.lib.rtgpu_resize(ctx.ctx, C.c_uint32(0), C.c_uint32(10)) == cr.INVALID_ARGUMENT
        ctx.render(p[2])
        got, got2 = ctx.read(state.w, state.h)
        cr.assert_film(got, got2, want, state.name)
        cr.assert_counters(before, ctx.counters(), want, ctx.walk, state.name)
    finally:
        ctx.close()


# ---- 8. the side entries ----------------------------------------------------------------------------------------------------------------------------------
HALL_DEPTH = guide_chain_ref.MAX_RAY_DEPTH
COST_PLANES = ("box_tests", "box_tests_passed", "triangle_tests", "triangle_tests_passed")


def hall_at(w, h):
    camera = ra.Camera((-12.5, 2.5, 0.3), (-6.0, 88.0, 0.0), w / h, 75.0)   # guide_chain_ref.camera() at the frame's aspect
    return State("hall %dx%d" % (w, h), guide_chain_ref.scene("hall"), camera, w, h, seed=guide_chain_ref.SEED, max_ray_depth=HALL_DEPTH, min_russian_roulette_depth=0)


def query_rays(scene, n=300, seed=4):
    rng = np.random.RandomState(seed)
    lo, hi = ray_query_shim.scene_bounds(scene)
    origins = (lo + rng.rand(n, 3) * (hi - lo)).astype(np.float32)
    directions = rng.normal(size=(n, 3)).astype(np.float32)
    directions[::7, 1] = 0.0   # (the 0 * inf slab case)
    distance = np.where(rng.rand(n) < 0.5, np.inf, 0.5 + 10.0 * rng.rand(n)).astype(np.float32)
    return ray_query_shim.pack(origins, directions, distance)


def side_entries(ctx, state, counting):
    """One call of each side entry on the context as it stands, behind two passes of `state` on a fresh film: every plane and record, by name"""
    lib, c, w, h = ctx.lib, ctx.ctx, state.w, state.h
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
    out = {}
    ctx.reset()
    p = state.params(5)
    ctx.render(p[0])
    ctx.render(p[1])
    # ray queries: closest hit with surfaces, any-hit
    rays = query_rays(state.scene)
    hits, surfaces, occluded = np.zeros((len(rays), 8), np.uint32), np.zeros((len(rays), 12), np.uint32), np.zeros(len(rays), np.uint32)
    assert lib.rtgpu_trace_rays(c, C.c_uint32(ra.TRACE_CLOSEST), ptr(rays), C.c_uint32(len(rays)), ptr(hits), ptr(surfaces), None, None) == cr.OK, ctx.error()
    assert lib.rtgpu_trace_rays(c, C.c_uint32(ra.TRACE_ANY), ptr(rays), C.c_uint32(len(rays)), None, None, ptr(occluded), None) == cr.OK, ctx.error()
    out.update(hits=hits, surfaces=surfaces, occluded=occluded)
    assert 20 < np.count_nonzero(hits[:, 1] != ra.RT_INVALID_OBJECT) and 0 < np.count_nonzero(occluded) < len(rays)
    # path records of 8 pixels
    pixels = np.array([(0, 0), (w - 1, h - 1), (w // 2, h // 2), (w // 3, h // 4), (w - 1, 0), (0, h - 1), (w // 5, (2 * h) // 3), (w // 2, h // 2)], dtype=np.uint32)
    vertices, infos = np.zeros((len(pixels), HALL_DEPTH + 1, 28), np.float32), np.zeros((len(pixels), 8), np.uint32)
    assert lib.rtgpu_record_paths(c, C.byref(p[2]), ptr(pixels), C.c_uint32(len(pixels)), C.c_uint32(HALL_DEPTH + 1), ptr(vertices), ptr(infos)) == cr.OK, ctx.error()
    out.update(vertices=vertices, infos=infos)
    assert infos[:, 0].max() >= 3
    # AOVs: every first-hit plane, the cost planes too under `counting`; then the chain call's
    names = [n for n in ra.AOV_PLANES if n not in COST_PLANES] + (list(COST_PLANES) if counting else [])
    known = dict(ra.AOV_PLANES)

    def planes(names, known, call):
        arrays = {n: np.zeros((known[n][1], h, w), dtype=known[n][2]) for n in names}
        ids = (C.c_uint32 * len(names))(*[known[n][0] for n in names])
        ptrs = (C.c_void_p * len(names))(*[arrays[n].ctypes.data for n in names])
        assert call(ids, C.c_uint32(len(names)), ptrs) == cr.OK, ctx.error()
        return arrays
    first_hit = planes(names, known, lambda ids, n, ptrs: lib.rtgpu_render_aovs(c, C.byref(p[2]), ids, n, ptrs))
    out.update({"aov " + n: a for n, a in first_hit.items()})
    assert np.isfinite(first_hit["depth"]).sum() > w * h // 2
    known.update(ra.AOV_CHAIN_PLANES)
    chain = ra.RtAovChain(3, 0)
    names = [n for n in known if n not in COST_PLANES]
    chained = planes(names, known, lambda ids, n, ptrs: lib.rtgpu_render_aovs_chain(c, C.byref(p[2]), C.byref(chain), ids, n, ptrs))
    out.update({"chain " + n: a for n, a in chained.items()})
    assert chained["chain_length"].max() >= 1
    # the filters over the film of the two passes
    image = lambda: np.zeros((h, w, 3), np.float32)   # noqa: E731
    plane = lambda: np.zeros((h, w), np.float32)      # noqa: E731
    d, dv, t = ra.denoise_params(color_scale=0.5), ra.denoise_var_params(color_scale=0.5), ra.temporal_params(color_scale=0.5)
    tv = ra.denoise_var_params()
    out["denoise"] = image()
    assert lib.rtgpu_denoise(c, C.byref(d), C.byref(p[2]), ptr(out["denoise"])) == cr.OK, ctx.error()
    out["denoise_var"], out["denoise_var variance"] = image(), plane()
    assert lib.rtgpu_denoise_var(c, C.byref(dv), C.byref(p[2]), ptr(out["denoise_var"]), ptr(out["denoise_var variance"])) == cr.OK, ctx.error()
    for k in range(2):
        out["temporal %d" % k], out["temporal %d variance" % k] = image(), plane()
        assert lib.rtgpu_denoise_temporal(c, C.byref(t), C.byref(tv), C.byref(p[2 + k]), ptr(out["temporal %d" % k]), ptr(out["temporal %d variance" % k])) == cr.OK, ctx.error()
    clip = ra.temporal_clip(True)
    for k in range(2):
        out["clip %d" % k], out["clip %d variance" % k], out["clip %d confidence" % k] = image(), plane(), plane()
        assert lib.rtgpu_denoise_temporal_clip(c, C.byref(t), C.byref(tv), C.byref(p[3 + k]), ptr(out["clip %d" % k]), ptr(out["clip %d variance" % k]), C.byref(clip),
                                               ptr(out["clip %d confidence" % k])) == cr.OK, ctx.error()
    assert out["denoise"].any() and out["temporal 1"].any() and out["clip 1"].any() and not np.array_equal(words(out["temporal 0"]), words(out["temporal 1"]))
    return out


def assert_same_entries(got, want, what):
    assert got.keys() == want.keys()
    for name in want:
        assert got[name].shape == want[name].shape and got[name].dtype == want[name].dtype, (what, name)
        bad = np.argwhere(words(got[name]) != words(want[name]))
        assert len(bad) == 0, "%s, %s: %d of %d words differ from the fresh context's, first at %r" % (what, name, len(bad), want[name].size, tuple(bad[0]))


def test_the_side_entries_after_a_transition(built, walk):
    """rtgpu_trace_rays, rtgpu_record_paths, rtgpu_render_aovs, rtgpu_render_aovs_chain, rtgpu_denoise, rtgpu_denoise_var and two frames each of
    rtgpu_denoise_temporal and rtgpu_denoise_temporal_clip, on a context that served every one of them at 200 x 136 on the mesh scene and was then moved to 67 x 41 on
    the hall of the guide-chain tests, and again after growing back to 200 x 136: the arenas, staging buffers, filter scratch and history records of the
    earlier state are all still there, larger than the state needs.

    The reference here is a FRESH context given the same calls in the same final state, bit for bit, every plane and record.  That is a reference and not a second
    run of the code under test because each of these entries is already pinned on fresh contexts, in its own file, to the oracle or to its NumPy model
    (test_gpu_ray_queries, test_gpu_path_records, test_gpu_aovs, test_gpu_guide_chain, test_gpu_denoise, test_gpu_denoise_var, test_gpu_temporal,
    test_gpu_temporal_clip): what a fresh context returns is what those references return, and what is left to check is that a reused context returns the same."""
    counting = walk == "counting"
    mesh, mesh_camera = scene_zoo.mesh_scene(BIG[0] / BIG[1], triangles=6000)
    earlier = State("side entries: mesh scene", mesh, mesh_camera, *BIG, max_ray_depth=HALL_DEPTH)
    ctx = Context(walk)
    try:
        ctx.upload(earlier.scene)
        ctx.resize(*BIG)
        side_entries(ctx, earlier, counting)
        ctx.upload(guide_chain_ref.scene("hall"))
        for size in ((67, 41), BIG):
            state = hall_at(*size)
            ctx.resize(*size)
            got = side_entries(ctx, state, counting)
            fresh = Context(walk)
            try:
                fresh.upload(state.scene)
                fresh.resize(*size)
                want = side_entries(fresh, state, counting)
            finally:
                fresh.close()
            assert_same_entries(got, want, state.name)
    finally:
        ctx.close()


def test_what_drops_the_history_on_a_reused_context(built):
    """The history-lifetime check of tests/test_gpu_temporal.py, on what it leaves out: a resize to a SMALLER frame and back to the original size (the record
    capacity still suffices, so temporal.have alone keeps the frame behind it from blending with records of the frame two sizes ago), and a DIFFERENT scene.  After
    each the next temporal frame starts every pixel: unfiltered and not demodulated it is sum * color_scale to the bit.  A REFUSED scene drops nothing: the frame
    behind it blends."""
    w, h = 64, 48
    sphere, _ = scenes.sphere_area_light(w / h)
    other, _ = scenes.cornell_box(w / h)
    cam_a = ra.Camera((0.0, 0.0, 6.0), (0.0, 180.0, 0.0), w / h, 40.0)
    cam_b = ra.Camera((0.0, 0.0, 6.0), (0.0, 182.0, 0.0), w / h, 40.0)
    states = {(name, k): State("history: %s, camera %d" % (name, k), scene, cam, w, h, seed=4321, max_ray_depth=3)
              for name, scene in (("sphere", sphere), ("cornell", other)) for k, cam in enumerate((cam_a, cam_b))}
    t = ra.temporal_params(color_scale=0.5, demodulate=False, normal_threshold=0.99)
    ctx = Context()
    try:
        def frame_starts(state):
            """two passes of a fresh film (rtgpu_reset keeps the history), one temporal frame; whether every pixel of it started"""
            ctx.reset()
            p = state.params()
            ctx.render(p[0])
            ctx.render(p[1])
            s, _ = ctx.read(w, h)
            out = np.zeros((h, w, 3), np.float32)
            assert ctx.lib.rtgpu_denoise_temporal(ctx.ctx, C.byref(t), None, C.byref(p[2]), out.ctypes.data_as(C.c_void_p), None) == cr.OK, ctx.error()
            assert s.any()
            return np.array_equal(words(out), words(s * np.float32(0.5)))
        ctx.upload(sphere)
        ctx.resize(w, h)
        assert frame_starts(states["sphere", 0])            # no history yet
        assert not frame_starts(states["sphere", 1])        # it blends
        ctx.resize(w // 2, h // 2)
        ctx.resize(w, h)
        assert frame_starts(states["sphere", 0])            # a smaller frame and back: the records of before are still allocated, and not a history
        assert not frame_starts(states["sphere", 1])
        for desc, _keep in bad_descriptors(sphere):
            assert ctx.lib.rtgpu_upload_scene(ctx.ctx, C.byref(desc)) == cr.INVALID_ARGUMENT
        assert not frame_starts(states["sphere", 0])        # a refused scene leaves the old one and its history
        ctx.upload(other)
        assert frame_starts(states["cornell", 1])           # a different scene
        assert not frame_starts(states["cornell", 0])
    finally:
        ctx.close()


# ---- 9. two live contexts -----------------------------------------------------------------------------------------------------------------------------------
@state_list
def two_contexts():
    scene, camera = scene_zoo.mesh_scene(67 / 41, triangles=6000)
    return [(cornell_at(96, 64, tag=", context A"), False), (State("mesh scene 67x41, context B", scene, camera, 67, 41, max_ray_depth=5), True)]


def test_two_live_contexts_interleaved(built):
    """Two contexts on one device alternate single passes and read-backs: the staging buffer and the stream pool are process-wide, rtgpu_last_error is
    thread-local, everything else must be the context's own.  Each film equals the oracle's after every pass."""
    (a, _), (b, _) = two_contexts()
    ca, cb = Context(), Context()
    try:
        for ctx, state in ((ca, a), (cb, b)):
            ctx.upload(state.scene)
            ctx.resize(state.w, state.h)
        for k in range(cr.PASSES):
            for ctx, state in ((ca, a), (cb, b)):
                ctx.render(state.params()[k])
                got, got2 = ctx.read(state.w, state.h)
                cr.assert_film(got, got2, cr.check_oracle(state, n=k + 1), "%s, pass %d" % (state.name, k))
        for ctx, state in ((ca, a), (cb, b)):
            cr.assert_counters(dict.fromkeys(ra.COUNTER_NAMES, 0), ctx.counters(), cr.oracle_of(state), ctx.walk, state.name)
    finally:
        ca.close()
        cb.close()
