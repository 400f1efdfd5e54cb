"""The ray source on the device (include/rtgpu.h: rtgpu_set_ray_source, rtgpu_read_camera_rays; Viewport.set_ray_source / camera_rays): passes, AOVs, path
records and the denoisers along caller-supplied primary rays.

Bar: BIT-EQUAL words everywhere.  A table exported from a camera holds the words the camera's generate kernel stores, the table kernels store those words,
and everything behind the primary ray is the code the camera's passes run: both sides perform the same IEEE operations, so there is no tolerance to state.
The CPU side: tests/test_ray_source_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import scene_zoo
import raytracer_amd as ra
from raytracer_amd import scenes

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, NOT_READY, UNSUPPORTED = -1, -5, -6
FIXTURES = {
    "single_mesh": (lambda a: scenes.sponza_class(a, 6000), 96, 54, 6),
    "two_level": (scenes.cornell_box, 64, 48, 4),
    "textured": (lambda a: scene_zoo.textured_scene(a, triangles=6000), 96, 54, 5),
}


BLUE_NOISE = ra.load_blue_noise()   # kept alive: the scene descriptions point into it


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b, what=""):
    bad = np.argwhere(words(a) != words(b))
    assert len(bad) == 0, "%s: %d of %d words differ, first at %r: %r against %r" % (what, len(bad), a.size, tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])])


def viewport(scene, w, h, walk="default", name="Path Tracer MIS", seed=31, spread=0.0, **kw):
    """a viewport on `scene`; spread 0: every pass has sample offset 0, so one exported table serves them all"""
    scene.desc.contents.blueNoise = BLUE_NOISE.ctypes.data   # (for the oracle and the direct uploads: the mirror brings its own)
    vp = ra.Viewport(w, h, seed=seed, anti_aliasing_spread=spread, **kw)
    vp.set_renderer(scene, name=name, intersection_counters=(walk == "counting"))
    return vp


def without_camera(p):
    """the pass constants with a camera no kernel could use and checkPass would refuse: under a source neither it nor the sample offset is read"""
    q = ra.RtPassParams.from_buffer_copy(p)
    q._seed_keepalive = p._seed_keepalive
    for k in range(16):
        q.camera.localToWorld[k] = float("nan")
        q.camera.worldToScreen[k] = float("nan")
    q.camera.aspectRatio = q.camera.tanHalfFoV = float("nan")
    q.camera.dofEnable, q.camera.bokehShape = 1, 7
    q.sampleOffset[0] = q.sampleOffset[1] = float("inf")
    return q


def frame_of(vp):
    return vp.sum_buffer(secondary=True) + (vp.counters(),)


def same_frame(got, want, what=""):
    same(got[0], want[0], what + " sum")
    same(got[1], want[1], what + " secondary")
    assert got[2] == want[2], (what, got[2], want[2])


def twins(make, w, h, depth, walk, passes, name="Path Tracer MIS", configure=None, sync_between=True, **kw):
    """`passes` passes through the camera on one viewport and through the camera's exported table on its twin: the two frames, and the pass constants"""
    scene, camera = make(w / h)
    a, b = (viewport(scene, w, h, walk, name, max_ray_depth=depth, **kw) for _ in range(2))
    for vp in (a, b):
        if configure:
            configure(vp)
    params = [a.next_pass_params(camera) for _ in range(passes)]
    for i, p in enumerate(params):
        p.passIndex = i   # (drawn before any pass has finished: the viewport numbered them all 0)
    b.set_ray_source(b.camera_rays(params[0]))
    assert b.ray_source() and not a.ray_source()
    for p in params:
        a.render_pass_with(p)
        b.render_pass_with(without_camera(p))
        if sync_between:
            a.sum_buffer(), b.sum_buffer()
    return frame_of(a), frame_of(b), scene, params


# ---- 1. the camera's frame from the camera's table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture", sorted(FIXTURES))
def test_the_cameras_table_renders_the_cameras_frame(built, walk, fixture):
    """three passes (both parities of passIndex): sum, secondary sum and every counter are those of the same passes through the camera"""
    make, w, h, depth = FIXTURES[fixture]
    want, got, scene, params = twins(make, w, h, depth, walk, 3)
    same_frame(got, want, fixture)
    assert want[2]["numPrimaryRays"] == 3 * w * h and want[0].any()
    if fixture == "two_level":   # ... and the oracle's
        ref, ref2 = np.zeros((h, w, 3), dtype=np.float32), np.zeros((h, w, 3), dtype=np.float32)
        for p in params:
            oracle_lib.render_pass(scene.desc, p, w, h, ref, ref2, threads=8)
        same(got[0], ref, "oracle sum")
        same(got[1], ref2, "oracle secondary")


@pytest.mark.parametrize("knob,value,fixture,passes", [("RTGPU_NO_DENSE", "1", "single_mesh", 3), ("RTGPU_PACKET", "0", "single_mesh", 3), ("RTGPU_WIDE", "0", "single_mesh", 3),
                                                       ("RTGPU_NO_LEAN", "1", "single_mesh", 3), ("RTGPU_WIDE2", "0", "two_level", 3), ("RTGPU_NO_DENSE", "1", "two_level", 3),
                                                       ("RTGPU_PASS_BATCH", "2", "single_mesh", 5)])
def test_under_each_path_state_layout_and_walk(built, monkeypatch, knob, value, fixture, passes):
    """the settings the parity tests exercise with the counters off: the slot-per-pixel layout (k_generate_rays), dense state without the packet walk, the
    binary walk, the generic shading kernels, a two-level scene on the binary walk, and five queued passes in batches of two over the lanes"""
    monkeypatch.setenv(knob, value)
    make, w, h, depth = FIXTURES[fixture]
    want, got, _, _ = twins(make, w, h, depth, "default", passes, sync_between=(knob != "RTGPU_PASS_BATCH"))
    same_frame(got, want, "%s=%s" % (knob, value))


@pytest.mark.parametrize("tail_bounce,local_retrace", [(0, 0), (1, 1), (3, -1)])
def test_under_each_schedule(built, tail_bounce, local_retrace):
    """rtgpu_set_schedule: the fused tail taking over at bounce 1, 3 or never, the block-local re-trace on and off"""
    lib = ra.rtgpu_lib()
    def configure(vp):
        assert lib.rtgpu_set_schedule(vp.device_context(), C.c_uint32(0), C.c_int32(tail_bounce)) == 0
        assert lib.rtgpu_set_schedule(vp.device_context(), C.c_uint32(1), C.c_int32(local_retrace)) == 0
    make, w, h, depth = FIXTURES["single_mesh"]
    want, got, _, _ = twins(make, w, h, depth, "default", 3, configure=configure)
    same_frame(got, want, "schedule %d %d" % (tail_bounce, local_retrace))


def test_eight_queued_passes_form_a_batch(built, walk):
    make, w, h, depth = FIXTURES["single_mesh"]
    want, got, _, _ = twins(make, w, h, depth, walk, 8, sync_between=False)
    same_frame(got, want, "batch")
    assert got[2]["numPrimaryRays"] == 8 * w * h


def test_all_lights_strategy(built):
    """LightSamplingStrategy::All: the dense layout with a request per light"""
    make, w, h, depth = FIXTURES["two_level"]
    want, got, _, _ = twins(make, w, h, depth, "default", 3, light_sampling_all=True)
    same_frame(got, want, "all lights")


def test_plain_path_tracer_and_debug_renderer(built, walk):
    make, w, h, depth = FIXTURES["two_level"]
    want, got, _, _ = twins(make, w, h, depth, walk, 3, name="Path Tracer")
    same_frame(got, want, "Path Tracer")
    assert got[2]["numShadowRays"] == 0
    want, got, _, _ = twins(make, w, h, depth, walk, 2, name="Debug", configure=lambda vp: vp.set_debug_mode(4))
    same_frame(got, want, "Debug")


def test_a_table_per_pass_follows_the_anti_aliasing_offsets(built):
    """the viewport's own normal-distributed sample offsets: a table exported and set before every pass"""
    make, w, h, depth = FIXTURES["two_level"]
    scene, camera = make(w / h)
    a, b = (viewport(scene, w, h, spread=0.5, max_ray_depth=depth) for _ in range(2))
    for _ in range(3):
        p = a.next_pass_params(camera)
        assert p.sampleOffset[0] != 0.0
        a.render_pass_with(p)
        b.set_ray_source(b.camera_rays(p))   # (ends the batch: the pass queued before it renders the table it was queued under)
        b.render_pass_with(without_camera(p))
    same_frame(frame_of(b), frame_of(a), "a table per pass")


# ---- 2. the export ---------------------------------------------------------------------------------------------------------------------------------
def test_the_export(built):
    make, w, h, depth = scenes.cornell_box, 37, 23, 4   # (the oracle is asked for every pixel's path)
    scene, camera = make(w / h)
    vp = viewport(scene, w, h, spread=0.5, max_ray_depth=depth)
    params = [vp.next_pass_params(camera) for _ in range(2)]
    vp.render_pass_with(params[0])
    before = frame_of(vp)
    table = vp.camera_rays(params[1])
    assert table.shape == (h, w, 8) and table.dtype == np.float32 and np.isfinite(table).all()
    assert not table[:, :, 3].any() and not table[:, :, 7].any()
    # vertex 0 of the oracle's path recording carries the ray as generated: origin words 0..2, the NORMALISED direction words 3..5
    for y in range(h):
        for x in range(w):
            v0 = oracle_lib.render_pixel_paths(scene.desc, params[1], w, h, x, y)[0]
            same(table[y, x, 0:3], v0[0:3], "origin of pixel %d %d" % (x, y))
            d = table[y, x, 4:7].astype(np.float64)
            assert np.allclose(d / np.sqrt(d @ d), v0[3:6], atol=1e-6), (x, y)
    same(vp.camera_rays(params[1], device=True).cpu().numpy(), table, "device export")
    assert not np.array_equal(words(vp.camera_rays(params[0])), words(table))   # (another sample offset: other rays)
    same_frame(frame_of(vp), before, "the export is not a pass")
    # the export writes the camera's rays whether or not a source is set
    vp.set_ray_source(table[:, ::-1].copy())
    same(vp.camera_rays(params[1]), table, "export under a source")
    # a camera that draws has no table
    p = vp.next_pass_params(camera)
    camera.set_dof(True, 11.0, 0.3)
    lens = vp.next_pass_params(camera)
    camera.set_dof(False)
    camera.set_lens(barrel_const=0.02, barrel_variable=0.03)
    barrel = vp.next_pass_params(camera)
    lib, out = ra.rtgpu_lib(), np.zeros((h, w, 8), dtype=np.float32)
    for q in (lens, barrel):
        assert lib.rtgpu_read_camera_rays(vp.device_context(), C.byref(q), out.ctypes.data_as(C.c_void_p)) == UNSUPPORTED
        with pytest.raises(RuntimeError, match="draws"):
            vp.camera_rays(q, device=True)
    assert not out.any()
    assert lib.rtgpu_read_camera_rays(vp.device_context(), C.byref(p), out.ctypes.data_as(C.c_void_p)) == 0 and out.any()


# ---- 3. arbitrary rays -------------------------------------------------------------------------------------------------------------------------------
def random_table(w, h, lo, hi, seed):
    rng = np.random.default_rng(seed)
    origins = rng.uniform(lo, hi, (h, w, 3)).astype(np.float32)
    directions = rng.normal(size=(h, w, 3))
    directions /= np.linalg.norm(directions, axis=-1, keepdims=True)
    directions = (directions * rng.uniform(0.1, 10.0, (h, w, 1))).astype(np.float32)
    return origins, directions


@pytest.mark.parametrize("fixture", ["single_mesh", "two_level"])
def test_arbitrary_rays(built, walk, fixture):
    """a seeded random table inside the scene's box: the AOV planes are the ray queries' answers for the same rays, vertex 0 of a path record carries the
    table's origin, and its radiance is what the pass adds to the pixel"""
    make, w, h, depth = FIXTURES[fixture]
    scene, camera = make(w / h)
    vp = viewport(scene, w, h, walk, max_ray_depth=depth)
    seen = vp.render_aovs(vp.next_pass_params(camera), ("depth", "position"))   # the scene's box: what the camera sees of it
    visible = np.isfinite(seen["depth"])
    lo, hi = seen["position"][:, visible].min(axis=1), seen["position"][:, visible].max(axis=1)
    origins, directions = random_table(w, h, lo, hi, seed=17)
    vp.set_ray_source(origins, directions)
    p = without_camera(vp.next_pass_params(camera))
    planes = vp.render_aovs(p, ("depth", "position", "normal", "object_id", "sub_object_id", "material"))
    hits = vp.trace_rays(origins.reshape(-1, 3), directions.reshape(-1, 3), surfaces=True)
    hit = hits.object_id != ra.RT_INVALID_OBJECT
    assert 0.05 < hit.mean() <= 1.0
    same(planes["depth"].reshape(-1), hits.distance, "depth")
    same(planes["object_id"].reshape(-1), hits.object_id, "object id")
    same(planes["sub_object_id"].reshape(-1), hits.sub_object_id, "sub-object id")
    same(planes["material"].reshape(-1), hits.material, "material")
    same(planes["position"].reshape(3, -1).T, hits.position, "position")
    same(planes["normal"].reshape(3, -1).T, hits.normal, "normal")
    pixels = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h // 3), (5, 7), (w - 3, h - 2)]
    records = vp.record_paths(p, pixels)
    vp.render_pass_with(p)
    film = vp.sum_buffer()
    for (x, y), (vertices, _, radiance) in zip(pixels, records):
        same(vertices[0, 0:3], origins[y, x], "vertex 0 of pixel %d %d" % (x, y))
        d = directions[y, x].astype(np.float64)
        assert np.allclose(vertices[0, 3:6], d / np.sqrt(d @ d), atol=1e-6)
        same(np.float32(0.0) + radiance, film[y, x], "radiance of pixel %d %d" % (x, y))
    assert film.any() and np.isfinite(film).all()
    # device tensors go in without a host copy and render the same frame
    import torch
    twin = viewport(scene, w, h, walk, max_ray_depth=depth)
    twin.set_ray_source(torch.from_numpy(origins).cuda(), torch.from_numpy(directions).cuda())
    twin.next_pass_params(camera)
    twin.render_pass_with(p)
    same(twin.sum_buffer(), film, "tensors")
    packed = np.zeros((h, w, 8), dtype=np.float32)
    packed[:, :, 0:3], packed[:, :, 3], packed[:, :, 4:7], packed[:, :, 7] = origins, np.float32("nan"), directions, np.float32("inf")   # (words 3 and 7 are never read)
    twin.reset()
    twin.set_ray_source(torch.from_numpy(packed).cuda())
    twin.render_pass_with(p)
    same(twin.sum_buffer(), film, "a packed tensor")


# ---- 4. indexing -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(37, 23), (70, 1), (1, 1)])
def test_every_pixel_is_rendered_once_per_pass(built, size):
    w, h = size
    scene = ra.Scene()
    scene.add_background_light((1.0, 1.0, 1.0))
    scene.build()
    camera = ra.Camera((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), w / h, 60.0)
    vp = viewport(scene, w, h)
    origins, directions = random_table(w, h, -1.0, 1.0, seed=w)
    vp.set_ray_source(origins, directions)
    for _ in range(3):
        vp.render_pass_with(vp.next_pass_params(camera))
    film, half, counters = frame_of(vp)
    assert (film == 3.0).all() and (half == 2.0).all() and counters["numPrimaryRays"] == 3 * w * h


@pytest.mark.parametrize("size", [(37, 23), (70, 1), (1, 1)])
def test_entry_y_times_width_plus_x_is_pixel_x_y(built, size):
    """a table that looks away from an emitter everywhere except in ONE entry: exactly that pixel of the sum buffer is lit -- a corner, the last row, the
    interior.  Pins the row order and the film flip."""
    w, h = size
    scene = ra.Scene()
    light = scene.add_material(bsdf="null", base_color=(0.0, 0.0, 0.0), emission=(2.0, 3.0, 4.0))
    scene.add_sphere(1.0, ra.transform_from_euler((0.0, 0.0, 10.0)), light)
    scene.build()
    camera = ra.Camera((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), w / h, 60.0)
    vp = viewport(scene, w, h)
    for x, y in sorted({(0, 0), (w - 1, h - 1), (0, h - 1), (w // 2, h // 2), (w - 1, 0)}):
        table = np.zeros((h, w, 8), dtype=np.float32)
        table[:, :, 6] = -1.0           # away from the sphere
        table[y, x, 6] = 5.0            # at it (not unit length)
        vp.reset()
        vp.set_ray_source(table)
        vp.render_pass_with(vp.next_pass_params(camera))
        film = vp.sum_buffer()
        lit = np.argwhere(film.any(axis=2))
        assert [tuple(v) for v in lit] == [(y, x)], (x, y, lit)


# ---- 5. shards, blocks, several devices --------------------------------------------------------------------------------------------------------------
def test_shards_and_active_blocks(built):
    w, h = 200, 136   # 4 x 3 tiles
    scene, camera = scenes.cornell_box(w / h)
    whole = viewport(scene, w, h, max_ray_depth=3)
    params = [whole.next_pass_params(camera) for _ in range(2)]
    table = whole.camera_rays(params[0])[::-1, ::-1].copy()   # (the frame upside down and mirrored: not the camera's)
    whole.set_ray_source(table)
    for p in params:
        whole.render_pass_with(p)
    want = whole.sum_buffer()
    assert want.any()
    part = viewport(scene, w, h, max_ray_depth=3)
    part.set_ray_source(table)
    part.set_shard(1, 2)
    assert part.ray_source()
    for p in params:
        part.render_pass_with(p)
    got = part.sum_buffer()
    tile = (np.arange(h)[:, None] // 64) * 4 + np.arange(w)[None, :] // 64
    owned = tile % 2 == 1
    same(got[owned], want[owned], "owned tiles")
    assert not got[~owned].any() and part.counters()["numPrimaryRays"] == 2 * int(owned.sum())
    blocks = viewport(scene, w, h, max_ray_depth=3)
    blocks.set_ray_source(table)
    rect = (ra.RtBlock * 2)(ra.RtBlock(3, 77, 5, 70), ra.RtBlock(100, 200, 64, 136))
    assert ra.rtgpu_lib().rtgpu_set_active_blocks(blocks.device_context(), C.c_uint32(2), rect) == 0
    assert blocks.ray_source()
    for p in params:
        blocks.render_pass_with(p)
    got = blocks.sum_buffer()
    active = np.zeros((h, w), dtype=bool)
    active[5:70, 3:77] = True
    active[64:136, 100:200] = True
    same(got[active], want[active], "active blocks")
    assert not got[~active].any()


def test_a_multi_device_context(built):
    import torch
    w, h = 200, 136
    scene, camera = scenes.cornell_box(w / h)
    one = viewport(scene, w, h, max_ray_depth=3)
    params = [one.next_pass_params(camera) for _ in range(2)]
    table = one.camera_rays(params[0])[::-1].copy()
    one.set_ray_source(table)
    many = ra.Viewport(w, h, seed=31, anti_aliasing_spread=0.0, max_ray_depth=3)
    many.set_renderer(scene, devices=[0, 0])
    many.set_ray_source(table)   # the host entry replicates the table
    for p in params:
        one.render_pass_with(p)
        many.render_pass_with(p)
    same_frame(frame_of(many), frame_of(one), "two shards on one device")
    with pytest.raises(RuntimeError, match="multi-device"):
        many.set_ray_source(torch.from_numpy(table).cuda())
    assert many.ray_source()


# ---- 6. state ------------------------------------------------------------------------------------------------------------------------------------------
def test_what_keeps_and_what_drops_the_source(built):
    lib = ra.rtgpu_lib()
    make, w, h, depth = FIXTURES["two_level"]
    scene, camera = make(w / h)
    a, b, fresh = (viewport(scene, w, h, max_ray_depth=depth) for _ in range(3))
    params = [a.next_pass_params(camera) for _ in range(4)]
    table = a.camera_rays(params[0])[:, ::-1].copy()
    for vp in (a, b):
        vp.set_ray_source(table)
    ctx = b.device_context()
    b.render_pass_with(params[0])
    b.reset()
    assert b.ray_source()
    b.set_shard(0, 1)
    assert b.ray_source()
    assert lib.rtgpu_set_integrator(ctx, C.c_uint32(2), None) == 0 and lib.rtgpu_set_integrator(ctx, C.c_uint32(0), None) == 0
    assert b.ray_source()
    assert lib.rtgpu_upload_scene(ctx, scene.desc) == 0
    assert b.ray_source()
    scene.update()
    b.update_scene()   # rtgpu_update_objects
    assert b.ray_source()
    for p in params[:2]:
        a.render_pass_with(p)
        b.render_pass_with(p)
    same(b.sum_buffer(), a.sum_buffer(), "after the calls that keep the source")
    assert not np.array_equal(words(a.sum_buffer()[:, ::-1]), words(a.sum_buffer()))
    # clearing: the camera renders again, as on a fresh viewport
    a.set_ray_source(None)
    assert not a.ray_source()
    a.reset()
    for p in params[2:]:
        a.render_pass_with(p)
        fresh.render_pass_with(p)
    same(a.sum_buffer(), fresh.sum_buffer(), "cleared")
    # a resize drops it, also to the size the context has
    assert lib.rtgpu_resize(ctx, C.c_uint32(w), C.c_uint32(h)) == 0
    assert not b.ray_source()
    for p in params[2:]:
        b.render_pass_with(p)
    same(b.sum_buffer(), fresh.sum_buffer(), "resized")


def test_refusals(built):
    import torch
    lib = ra.rtgpu_lib()
    make, w, h, depth = FIXTURES["two_level"]
    scene, camera = make(w / h)
    vp, twin = (viewport(scene, w, h, max_ray_depth=depth) for _ in range(2))
    params = [vp.next_pass_params(camera) for _ in range(3)]
    good = vp.camera_rays(params[0])[::-1].copy()
    for v in (vp, twin):
        v.set_ray_source(good)
    ctx = vp.device_context()
    # one degenerate entry, through either entry: refused, and the next pass renders the previous source's frame
    for word, value in ((1, np.nan), (2, np.inf), (5, -np.inf), (4, 0.0)):
        bad = good.copy()
        if word == 4:
            bad[h - 1, w - 1, 4:7] = 0.0
        else:
            bad[h // 2, 3, word] = value
        with pytest.raises(ValueError, match="degenerate"):
            vp.set_ray_source(bad)
        with pytest.raises(ValueError, match="degenerate"):
            vp.set_ray_source(torch.from_numpy(bad).cuda())
        assert vp.ray_source()
    tiny = good.copy()
    tiny[0, 0, 4:7] = 1e-30   # (its squared length underflows to 0)
    with pytest.raises(ValueError, match="degenerate"):
        vp.set_ray_source(tiny)
    for p in params[:2]:
        vp.render_pass_with(p)
        twin.render_pass_with(p)
    same(vp.sum_buffer(), twin.sum_buffer(), "after refused tables")
    # a refused FIRST table leaves the camera
    fresh, camera_twin = (viewport(scene, w, h, max_ray_depth=depth) for _ in range(2))
    with pytest.raises(ValueError, match="degenerate"):
        fresh.set_ray_source(tiny)
    assert not fresh.ray_source()
    fresh.render_pass_with(params[2])
    camera_twin.render_pass_with(params[2])
    same(fresh.sum_buffer(), camera_twin.sum_buffer(), "the camera after a refused table")
    # counts, pointers, order of calls
    ptr = good.ctypes.data_as(C.c_void_p)
    assert lib.rtgpu_set_ray_source(ctx, ptr, C.c_uint64(w * h - 1)) == INVALID_ARGUMENT
    assert lib.rtgpu_set_ray_source(ctx, ptr, C.c_uint64(0)) == INVALID_ARGUMENT
    assert lib.rtgpu_set_ray_source(ctx, None, C.c_uint64(w * h)) == INVALID_ARGUMENT
    assert lib.rtgpu_set_ray_source_device(ctx, ptr, C.c_uint64(w * h), None) == INVALID_ARGUMENT and b"device" in lib.rtgpu_last_error()
    on_device = torch.from_numpy(good).cuda()
    assert lib.rtgpu_set_ray_source_device(ctx, C.c_void_p(on_device.data_ptr() + 2), C.c_uint64(w * h), None) == INVALID_ARGUMENT and b"aligned" in lib.rtgpu_last_error()
    out_of_line = torch.zeros(w * h * 8 + 8, dtype=torch.float32, device="cuda")
    assert lib.rtgpu_read_camera_rays_async(ctx, C.byref(params[0]), C.c_void_p(out_of_line.data_ptr() + 4), None) == INVALID_ARGUMENT and not out_of_line.any()
    with pytest.raises(ValueError):
        vp.set_ray_source(good[:-1])
    assert vp.ray_source()
    raw = C.c_void_p()
    assert lib.rtgpu_create(0, C.byref(raw)) == 0
    n = C.c_uint64(7)
    assert lib.rtgpu_set_ray_source(raw, ptr, C.c_uint64(w * h)) == NOT_READY and lib.rtgpu_get_ray_source(raw, C.byref(n)) == 0 and n.value == 0
    assert lib.rtgpu_read_camera_rays(raw, C.byref(params[0]), ptr) == NOT_READY
    assert lib.rtgpu_set_ray_source(raw, None, C.c_uint64(0)) == 0
    lib.rtgpu_destroy(raw)
    # the integrators that splat through the camera, and the reprojection
    vp.sum_buffer()
    for integrator in (1, 4):
        assert lib.rtgpu_set_integrator(ctx, C.c_uint32(integrator), None) == 0
        assert lib.rtgpu_render_pass(ctx, C.byref(params[2])) == UNSUPPORTED and b"ray source" in lib.rtgpu_last_error()
    assert lib.rtgpu_set_integrator(ctx, C.c_uint32(0), None) == 0
    with pytest.raises(RuntimeError, match="ray source"):
        vp.denoise(params[2], temporal=True)
    with pytest.raises(RuntimeError, match="ray source"):
        vp.denoise(params[2], temporal=True, chain=2)
    same(vp.sum_buffer(), twin.sum_buffer(), "after the refusals")


def test_the_denoisers_follow_the_source(built):
    """denoise() and denoise(variance=True) run under a source and are the pure filter over the planes the AOV call returns under it"""
    make, w, h, depth = FIXTURES["single_mesh"]
    scene, camera = make(w / h)
    vp = viewport(scene, w, h, max_ray_depth=depth)
    params = [vp.next_pass_params(camera) for _ in range(5)]
    vp.set_ray_source(vp.camera_rays(params[0])[:, ::-1].copy())
    for p in params[:4]:
        vp.render_pass_with(p)
    g = vp.render_aovs(params[4], ("depth", "normal", "position", "base_color"))
    film, half = vp.sum_buffer(secondary=True)
    mirrored = viewport(scene, w, h, max_ray_depth=depth).render_aovs(params[4], ("depth",))["depth"]
    same(g["depth"], mirrored[:, ::-1], "the guides are the source's")
    assert not np.array_equal(words(g["depth"]), words(mirrored))
    got = vp.denoise(params[4])
    want = ra.atrous_filter(film, g["depth"], g["normal"], g["position"], g["base_color"], color_scale=1.0 / 4.0)
    same(got, want, "denoise")
    got, variance = vp.denoise(params[4], variance=True, return_variance=True)
    want, want_variance = ra.atrous_filter(film, g["depth"], g["normal"], g["position"], g["base_color"], color_scale=1.0 / 4.0, color_half=half, return_variance=True)
    same(got, want, "denoise(variance=True)")
    same(variance, want_variance, "its variance")
    same_frame(frame_of(vp), (film, half, vp.counters()), "not a pass")


# ---- 7. the headless demo --------------------------------------------------------------------------------------------------------------------------
def test_rt_demo_renders_through_a_projection(built, tmp_path):
    """rt_demo --projection: the table is built from the scene file's camera transform, the frame is rendered as usual, and the denoisers follow it"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    scene = os.path.join(root, "tests", "golden", "obj", "scene.json")
    exe = os.path.join(root, "raytracer_amd", "lib", "rt_demo")
    images = {}
    for label, extra in (("camera", []), ("orthographic", ["--projection", "orthographic", "--projection-size", "3"]),
                         ("panorama", ["--projection", "panorama", "--denoise", "3"]), ("fisheye", ["--projection", "fisheye", "--projection-fov", "150", "--denoise-variance", "2"])):
        path = str(tmp_path / (label + ".bmp"))
        r = subprocess.run([exe, "-s", scene, "--data", os.path.dirname(scene) + "/", "--width", "64", "--height", "48", "--passes", "2", "--depth", "3", "--seed", "11"] +
                           extra + ["--output", path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("projection: %s, 3072 primary rays" % label in r.stdout) == (label != "camera"), r.stdout
        assert ("denoised:" in r.stdout) == (label in ("panorama", "fisheye")) and "2 passes of 64x48" in r.stdout
        images[label] = open(path, "rb").read()
    assert len({len(v) for v in images.values()}) == 1 and len(set(images.values())) == 4
    r = subprocess.run([exe, "-s", scene, "--projection", "cylinder"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "orthographic, panorama or fisheye" in r.stderr
