"""Temporal accumulation that follows deforming meshes on the device (rtgpu_temporal_accumulate_deform and its _async twin; raytracer_amd.temporal_accumulate
with deform; Viewport.track_deformation() and Viewport.denoise(temporal=True) after Scene.set_mesh_vertices / Viewport.update_scene()) against its NumPy float32
model (tests/temporal_deform_ref.py).

Bar and helpers: those of tests/test_gpu_temporal.py -- BIT-EQUAL words.  The operation is defined step by step (include/rtgpu.h), the model performs those steps
in that order in IEEE float32, and the device library is compiled without contraction: there is no tolerance to state.  What the random frames cover, and that
the deformation of the context tests lets most of the mesh blend, is asserted by tests/test_temporal_deform_model.py on the CPU."""
import ctypes as C

import numpy as np
import pytest

import deform_scenes as ds
import mesh_refit_scenes as ms
import raytracer_amd as ra
import temporal_clip_ref as cref
import temporal_deform_ref as dref
import temporal_ref as ref
from test_gpu_temporal import OK, INVALID_ARGUMENT, PARAMS, OUTPUTS, NAMES, assert_history, assert_same, words
from test_gpu_update import BLUE_NOISE

pytestmark = pytest.mark.gpu

SHAPES = [(37, 23), (70, 41)]     # neither a multiple of the block
CLIP = dict(radius=2, gamma=1.0, min_count=5)
_frames = {}
_models = {}


def frame(w, h):
    if (w, h) not in _frames:
        _frames[w, h] = dref.random_deform_frame(w, h, seed=1000 * w + h)
    return _frames[w, h]


def inputs(w, h, history=True, deform=None):
    f = frame(w, h)
    kw = dict(f["current"], object_motion=f["object_motion"], deform=deform or f["deform"], **PARAMS)
    if history:
        kw.update(history=f["history"], prev_world_to_screen=f["prev_world_to_screen"], prev_sample_offset=f["prev_sample_offset"])
    return kw


def model(w, h, clip, history=True, short=False):
    key = (w, h, clip is not None, history, short)
    if key not in _models:
        out, motion, _, why, extra = dref.accumulate_deform(clip=clip, **inputs(w, h, history, shortened(w, h) if short else None))
        for a in [out[k] for k in OUTPUTS] + [motion, extra["f"]]:
            a.setflags(write=False)
        _models[key] = (out, motion, why, extra["f"])
    return _models[key]


def shortened(w, h):
    """the frame's deform with a triangle table that ends halfway through the deformed mesh's range"""
    d = frame(w, h)["deform"]
    return dict(d, prev_triangles=d["prev_triangles"][:dref.LEADING + int(d["num_triangles"].max()) // 2].copy())


# ---- 1. the pure entry on random inputs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("history", [True, False], ids=["history", "none"])
@pytest.mark.parametrize("clip", [None, CLIP], ids=["plain", "clip"])
@pytest.mark.parametrize("w, h", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_the_pure_entry_equals_the_model(built, w, h, clip, history):
    f = frame(w, h)
    assert sorted(set(f["object_motion"][2].tolist())) == [0, 1, 2] and f["planted"]["bad_triangle"].sum() >= 3      # a mixed table, triangle ids out of range
    want, want_motion, why, want_f = model(w, h, clip, history)
    got = ra.temporal_accumulate(return_motion=True, clip=clip, return_confidence=clip is not None, **inputs(w, h, history))
    what = "%d x %d" % (w, h)
    assert_history(got[0], got[1], want, want_motion, what)
    if clip is not None:
        assert_same(got[2], want_f, what + ", confidence")
    mine, bad = f["planted"]["deformed"], f["planted"]["bad_triangle"]
    if history:
        assert (why == ref.BLENDED)[mine & ~bad].mean() > 0.5 and (want["length"][bad] == 1).all()
    else:
        assert (want["length"] == 1).all()


def test_without_a_deformed_record_the_words_are_the_clip_entrys(built):
    """the identity of the header, on the device: the moving frame through both entries, with planes and triangles nobody may read a value from"""
    import temporal_moving_ref as mref
    w, h = 70, 41
    f = mref.random_moving_frame(w, h, seed=77)
    n = len(f["object_motion"][2])
    rng = np.random.default_rng(5)
    rubbish = dict(sub_object_id=rng.integers(0, 1 << 32, size=(h, w)).astype(np.uint32), barycentrics=np.full((2, h, w), np.nan, dtype=np.float32),
                   prev_triangles=np.full((4, 9), np.nan, dtype=np.float32), first_triangle=np.zeros(n), num_triangles=np.full(n, 4))
    kw = dict(f["current"], object_motion=f["object_motion"], history=f["history"], prev_world_to_screen=f["prev_world_to_screen"], prev_sample_offset=f["prev_sample_offset"], **PARAMS)
    for clip in (None, CLIP):
        want = ra.temporal_accumulate(return_motion=True, clip=clip, **kw)
        got = ra.temporal_accumulate(return_motion=True, clip=clip, deform=rubbish, **kw)
        assert_history(got[0], got[1], want[0], want[1], "clip %r" % (clip,))
        assert (want[0]["length"] > 1).mean() > 0.3


# ---- 2. device tensors on a stream of the caller's --------------------------------------------------------------------------------------------------
def test_tensors_on_a_side_stream_and_on_the_default_stream(built):
    """... where the table lives on the device and no host check sees it: also with a triangle array that ends inside the mesh's range (the kernel's own guard)"""
    import torch
    w, h = 70, 41

    def on_device(kw):
        t = {}
        for k, v in kw.items():
            if isinstance(v, np.ndarray) and k != "prev_world_to_screen":
                t[k] = torch.from_numpy(v.astype(np.int32) if v.dtype == np.uint32 else v).cuda()
            elif k == "history":
                t[k] = {name: None if a is None else torch.from_numpy(a.astype(np.int32) if a.dtype == np.uint32 else a).cuda() for name, a in v.items()}
            elif k == "deform":
                t[k] = dict(v, sub_object_id=torch.from_numpy(v["sub_object_id"].astype(np.int32)).cuda(), barycentrics=torch.from_numpy(v["barycentrics"]).cuda())
            else:
                t[k] = v     # (the table and the triangles stay NumPy: the wrapper takes them to the device)
        return t
    cases = ((None, False), (CLIP, False), (None, True))
    tensors = [on_device(inputs(w, h, True, shortened(w, h) if short else None)) for _, short in cases]
    tensors[1]["deform"]["prev_triangles"] = torch.from_numpy(tensors[1]["deform"]["prev_triangles"]).cuda()      # ... or a tensor of the caller's
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        on_side = [ra.temporal_accumulate(return_motion=True, clip=clip, **t) for (clip, _), t in zip(cases, tensors)]
    on_default = ra.temporal_accumulate(return_motion=True, **tensors[0])
    stream.synchronize()
    for (clip, short), (got, motion) in zip(cases, on_side):
        want, want_motion, why, _ = model(w, h, clip, True, short)
        assert got["a"].is_cuda and tuple(motion.shape) == (2, h, w)
        assert_history({k: got[k].cpu().numpy() for k in OUTPUTS}, motion.cpu().numpy(), want, want_motion, "side stream, clip %r, short %r" % (clip, short))
        if short:
            cut = frame(w, h)["planted"]["deformed"] & (frame(w, h)["deform"]["sub_object_id"] >= int(frame(w, h)["deform"]["num_triangles"].max()) // 2)
            kept = frame(w, h)["planted"]["deformed"] & ~cut
            assert cut.sum() > 50 and (why[cut] == ref.START_INVALID).all() and (why[kept] == ref.BLENDED).mean() > 0.5
    want, want_motion, _, _ = model(w, h, None)
    assert_history({k: on_default[0][k].cpu().numpy() for k in OUTPUTS}, on_default[1].cpu().numpy(), want, want_motion, "default stream")


# ---- 3. statuses through the raw ABI -----------------------------------------------------------------------------------------------------------------
def test_statuses(built):
    import torch
    lib = ra.rtgpu_lib()
    ctx = C.c_void_p()
    assert lib.rtgpu_create(0, C.byref(ctx)) == OK
    try:
        eye = np.eye(4, dtype=np.float32)
        good = ra.temporal_params(prev_world_to_screen=eye)
        w = h = 4
        sizes = (3, 3, 1, 3, 3, 3, 1, 3, 3, 1, 1, 3, 3, 1, 3, 3, 1, 2)
        names = NAMES + ("sub", "bary", "confidence")
        sizes += (1, 2, 1)
        starts = dict(zip(names, np.cumsum((0,) + sizes[:-1])))
        host = np.zeros(64 * (sum(sizes) + 8), dtype=np.float32)
        dev = torch.zeros(64 * (sum(sizes) + 8), dtype=torch.float32, device="cuda")
        tables = {}

        def table_of(moved=(0, 2), first=(0, 1), count=(0, 2)):
            key = (moved, first, count)
            if key not in tables:
                t = ra.object_motion_table((np.stack([eye, eye]), [0, 1], list(moved)), dict(first_triangle=list(first), num_triangles=list(count)))
                t[:, 17] = moved
                tables[key] = (t, torch.from_numpy(t.view(np.int32)).cuda())
            return tables[key]

        for asynchronous in (False, True):
            base = dev.data_ptr() if asynchronous else host.ctypes.data
            at = lambda name, off=0: C.c_void_p(base + 64 * 4 * int(starts[name]) + off)   # noqa: E731
            triangles = base + 64 * 4 * sum(sizes)

            def call(null=(), shift=None, table=None, deform=True, tri=triangles, num=3, pad=0, clip=None, entry=None, alias=None):
                host_table, dev_table = table_of() if table is None else table
                ptr = {name: at(name) for name in names}
                if shift:
                    ptr[shift[0]] = at(shift[0], shift[1])
                if alias:
                    ptr[alias[0]] = at(alias[1])
                ptr.update({name: None for name in null})
                block = ra.RtTemporalDeform(ptr["sub"], ptr["bary"], tri, num, pad)
                objects = None if "table" in null else C.c_void_p(dev_table.data_ptr() if asynchronous else host_table.ctypes.data)
                args = [ctx, C.byref(good), C.c_uint32(w), C.c_uint32(h)] + [ptr[name] for name in NAMES] + [objects, C.c_uint32(2), C.byref(clip) if clip else None, ptr["confidence"],
                                                                                                               C.byref(block) if deform else None]
                return getattr(lib, "rtgpu_temporal_accumulate_deform" + ("_async" if asynchronous else ""))(*(args + ([None] if asynchronous else [])))

            assert call() == OK and call(clip=ra.temporal_clip(True)) == OK            # clip == NULL is allowed, and so is one
            assert call(deform=False) == INVALID_ARGUMENT and b"deform" in lib.rtgpu_last_error()
            assert call(null=("table",)) == INVALID_ARGUMENT
            assert call(null=("sub",)) == INVALID_ARGUMENT and call(null=("bary",)) == INVALID_ARGUMENT and b"planes" in lib.rtgpu_last_error()
            assert call(tri=None) == INVALID_ARGUMENT and b"prevTriangles" in lib.rtgpu_last_error()
            assert call(tri=None, num=0, table=table_of(first=(0, 0), count=(0, 0))) == OK            # an empty array: every deformed pixel starts
            assert call(pad=1) == INVALID_ARGUMENT and b"_pad" in lib.rtgpu_last_error()
            assert call(null=("id",)) == INVALID_ARGUMENT                               # the errors of the moving entries stay
            if not asynchronous:
                assert call(table=table_of(moved=(0, 3))) == INVALID_ARGUMENT and b"moved" in lib.rtgpu_last_error()
                assert call(table=table_of(first=(0, 2))) == INVALID_ARGUMENT and b"range" in lib.rtgpu_last_error()        # 2 + 2 > 3
                assert call(table=table_of(first=(0, 0xFFFFFFFF))) == INVALID_ARGUMENT                                     # (no wrap-around)
                assert call(table=table_of(moved=(0, 1), first=(0, 9))) == OK                                               # (the words of a record that is not deformed mean nothing)
            else:
                assert call(shift=("sub", 4)) == INVALID_ARGUMENT and call(shift=("bary", 8)) == INVALID_ARGUMENT and b"aligned" in lib.rtgpu_last_error()
                assert call(tri=triangles + 2) == INVALID_ARGUMENT and b"4-byte" in lib.rtgpu_last_error()
                assert call(tri=triangles + 4) == OK
                assert call(alias=("out_length", "sub")) == INVALID_ARGUMENT and b"overlaps" in lib.rtgpu_last_error()
                assert call(table=table_of(first=(0, 2))) == OK                          # a device table is not read on the host: the kernel's own range test stands
        assert lib.rtgpu_set_deform_tracking(ctx, 1) == OK and lib.rtgpu_set_deform_tracking(ctx, 0) == OK     # no scene needed
        assert lib.rtgpu_synchronize(ctx) == OK
        torch.cuda.synchronize()
    finally:
        lib.rtgpu_destroy(ctx)


# ---- 4. through the context: rendered frames, the mesh deformed between them ---------------------------------------------------------------------------
GUIDES = ("depth", "normal", "position", "base_color", "object_id", "sub_object_id", "barycentrics")


def viewport(scene, track=True, before_renderer=False):
    scene.desc.contents.blueNoise = BLUE_NOISE.ctypes.data
    vp = ra.Viewport(ds.W, ds.H, seed=ds.SEED, max_ray_depth=4)
    if track and before_renderer:
        vp.track_deformation()        # remembered until the device context exists
    vp.set_renderer(scene)
    if track and not before_renderer:
        vp.track_deformation()
    return vp


def render_frame(vp, camera):
    vp.reset()
    params = [vp.next_pass_params(camera) for _ in range(3)]
    for p in params[:2]:
        vp.render_pass_with(p)
    s, s2 = vp.sum_buffer(secondary=True)
    return params[2], dict(color=s, color_half=s2, color_scale=0.5), vp.render_aovs(params[2], GUIDES)


def model_inputs(sums, g):
    return dict(sums, depth=g["depth"], normal=g["normal"], position=g["position"], albedo=g["base_color"], object_id=g["object_id"])


def first_frame(vp, camera, clip):
    """renders frame 0, holds the call without a history to the model, and returns what frame 1's model needs of it"""
    p, sums, g = render_frame(vp, camera)
    image = vp.denoise(p, temporal=True, variance=False, clip=clip)
    history = cref.accumulate_clip(clip=model_clip(clip), **model_inputs(sums, g))[0]
    assert_same(image, ref.remodulate(history["a"], g["base_color"]), "frame 0")
    return dict(history=history, prev_world_to_screen=list(p.camera.worldToScreen), prev_sample_offset=tuple(p.sampleOffset))


def model_clip(clip):
    return dict(ra.TEMPORAL_CLIP_DEFAULTS) if clip is True else clip


def second_frame(vp, camera, scene, clip, previous, then, triangles, prev_index=None, tracked=True):
    """renders frame 1 and holds the call to the model under the table and the triangles of the header; returns (start reasons, pixels on the mesh in both frames)"""
    p, sums, g = render_frame(vp, camera)
    image = vp.denoise(p, temporal=True, variance=False, clip=clip)
    table, deform = ds.context_inputs(scene, then, triangles, g, prev_index, tracked)
    want = dref.accumulate_deform(object_motion=table, deform=deform, clip=model_clip(clip), **dict(model_inputs(sums, g), **previous))
    assert_same(image, ref.remodulate(want[0]["a"], g["base_color"]), "frame 1")
    on_mesh = np.isin(g["object_id"], ds.mesh_objects(scene)) & np.isfinite(g["depth"]) & np.isin(previous["history"]["object_id"], ds.mesh_objects(scene))
    return want[3], want[0], on_mesh, table


@pytest.mark.parametrize("clip", [None, True], ids=["plain", "clip"])
@pytest.mark.parametrize("kind", list(ms.SCENES))
def test_the_context_call_follows_the_deformed_mesh(built, kind, clip):
    """tracking on; frame 0 stores a history; the triangles are read; the mesh sways; frame 1's call equals the model on render_aovs' planes, those triangles and
    the table of the header.  The two-level scene's instance: two objects over one snapshot"""
    scene, camera, pos, idx, nrm = ms.SCENES[kind]("grid17", ds.W / ds.H)
    vp = viewport(scene, before_renderer=(kind == "single"))
    previous = first_frame(vp, camera, clip)
    then, triangles = ds.object_tables(scene), ds.scene_triangles(scene, vp.device_context())
    ds.deform(scene, vp, pos, idx, 1)
    why, history, on_mesh, table = second_frame(vp, camera, scene, clip, previous, then, triangles)
    assert int((table[2] == dref.RT_MOTION_DEFORMED).sum()) == (2 if kind == "two_level" else 1)
    # not vacuously: more than half of the mesh's pixels blend (tests/test_temporal_deform_model.py holds the deformation to that on the CPU)
    assert on_mesh.sum() > 300 and (why == ref.BLENDED)[on_mesh].mean() > 0.5 and (history["length"][on_mesh] > 1).mean() > 0.5


def test_two_updates_between_two_frames_keep_the_first_snapshot(built):
    scene, camera, pos, idx, nrm = ms.two_level_scene("grid17", ds.W / ds.H)
    vp = viewport(scene)
    previous = first_frame(vp, camera, None)
    then, triangles = ds.object_tables(scene), ds.scene_triangles(scene, vp.device_context())
    ds.deform(scene, vp, pos, idx, 0.5)
    first = ds.previous_index(scene)
    ds.deform(scene, vp, pos, idx, 1)
    assert not np.array_equal(words(ds.scene_triangles(scene, vp.device_context())), words(triangles))
    why, history, on_mesh, _ = second_frame(vp, camera, scene, None, previous, then, triangles, first[ds.previous_index(scene)])
    assert (why == ref.BLENDED)[on_mesh].mean() > 0.5


def test_a_deformation_beside_a_rigid_move_and_a_reordered_top_level(built):
    """set_mesh_vertices and set_object_transform of the same object, and the sphere carried across the scene so that the top level reorders: prevId follows
    previousIndex, and m is the transform the object had"""
    E = ra.transform_from_euler
    scene, camera, pos, idx, nrm = ms.two_level_scene("grid17", ds.W / ds.H)
    vp = viewport(scene)
    previous = first_frame(vp, camera, None)
    then, triangles = ds.object_tables(scene), ds.scene_triangles(scene, vp.device_context())
    ds.deform(scene, None, pos, idx, 1, update=False)
    scene.set_object_transform(ms.MESH_OBJECT, E((-0.8, 0.1, 0.1), (0.0, 23.0, 2.0)))
    scene.set_object_transform(2, E((-3.4, -0.7, -1.5)))
    scene.update()
    vp.update_scene()
    order = ds.previous_index(scene)
    assert not np.array_equal(order, np.arange(len(order)))
    why, history, on_mesh, table = second_frame(vp, camera, scene, None, previous, then, triangles)
    matrices, prev_ids, moved = table
    assert np.array_equal(prev_ids, order.astype(np.uint32)) and (moved == dref.RT_MOTION_DEFORMED).sum() == 2 and (moved == 1).sum() == 1
    for o in np.flatnonzero(moved == dref.RT_MOTION_DEFORMED):
        assert np.array_equal(words(matrices[o]), words(then["transform"][order[o]]))
    assert (why == ref.BLENDED)[on_mesh].mean() > 0.3


def test_tracking_switched_off_again_is_todays_behaviour(built):
    scene, camera, pos, idx, nrm = ms.two_level_scene("grid17", ds.W / ds.H)
    vp = viewport(scene)
    previous = first_frame(vp, camera, None)
    then, triangles = ds.object_tables(scene), ds.scene_triangles(scene, vp.device_context())
    vp.track_deformation(False)
    ds.deform(scene, vp, pos, idx, 1)
    why, history, on_mesh, table = second_frame(vp, camera, scene, None, previous, then, triangles, tracked=False)
    assert not (table[2] == dref.RT_MOTION_DEFORMED).any() and (table[1][ds.mesh_objects(scene)] == 0xFFFFFFFF).all()
    mesh_now = np.isin(history["object_id"], ds.mesh_objects(scene))
    assert mesh_now.sum() > 300 and (history["length"][mesh_now] == 1).all()
    others = ~mesh_now & np.isfinite(history["depth"])
    assert (why[others] == ref.BLENDED).mean() > 0.5


def test_without_a_temporal_call_before_the_update_every_pixel_starts(built):
    """tracking on, but no history when the mesh is updated: no snapshot is taken, and the first temporal call starts every pixel"""
    scene, camera, pos, idx, nrm = ms.single_mesh_scene("grid17", ds.W / ds.H)
    vp = viewport(scene)
    p, sums, g = render_frame(vp, camera)       # (rendered, never accumulated)
    ds.deform(scene, vp, pos, idx, 1)
    previous = first_frame(vp, camera, None)     # holds the call to the model without a history
    assert (previous["history"]["length"] == 1).all()
    # ... and from here on the mesh is followed as ever
    then, triangles = ds.object_tables(scene), ds.scene_triangles(scene, vp.device_context())
    ds.deform(scene, vp, pos, idx, 0.5)
    why, history, on_mesh, _ = second_frame(vp, camera, scene, None, previous, then, triangles)
    assert (why == ref.BLENDED)[on_mesh].mean() > 0.5
