"""rtgpu_update_objects on the device (through Scene.update() / Viewport.update_scene() of the host mirror): a scene whose objects moved must render,
answer ray queries and feed the bidirectional integrator exactly as the same scene uploaded whole -- bit-exact sum buffers, secondary buffers and
counters against the CPU oracle on the updated descriptor (the bar of tests/test_gpu_parity.py), and against a fresh Viewport over a freshly built
scene.  96 x 64, 2 passes, depth 4, both walks (tests/conftest.py)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import raytracer_amd as ra
import scene_zoo
import update_scenes as us
from test_gpu_parity import COMPARED, NOT_INTERSECTION, assert_identical

pytestmark = pytest.mark.gpu

W, H = 96, 64
GPU_CASES = ["cornell", "mesh", "sphere_light", "single_mesh"]
INVALID_ARGUMENT, NOT_READY, UNSUPPORTED = -1, -5, -6


def viewport(scene, walk, seed=77, name="Path Tracer MIS", devices=None, **args):
    scene.desc.contents.blueNoise = BLUE_NOISE.ctypes.data
    vp = ra.Viewport(W, H, seed=seed, max_ray_depth=4, **args)
    vp.set_renderer(scene, name=name, devices=devices, intersection_counters=(walk == "counting"))
    return vp


BLUE_NOISE = ra.load_blue_noise()


class Oracle:
    """sum, secondary and counters of the passes fed to it"""

    def __init__(self):
        self.sum = np.zeros((H, W, 3), dtype=np.float32); self.secondary = np.zeros((H, W, 3), dtype=np.float32); self.counters = np.zeros(16, dtype=np.uint64)

    def render(self, scene, params):
        scene.desc.contents.blueNoise = BLUE_NOISE.ctypes.data
        oracle_lib.render_pass(scene.desc, params, W, H, self.sum, self.secondary, self.counters, threads=8)

    def named(self):
        return {n: int(self.counters[i]) for i, n in enumerate(ra.COUNTER_NAMES)}


def passes(vp, camera, count, oracle=None, scene=None):
    """renders `count` passes; returns their constants"""
    out = []
    for _ in range(count):
        p = vp.next_pass_params(camera)
        vp.render_pass_with(p)
        if oracle is not None:
            oracle.render(scene, p)
        out.append(p)
    return out


def move(scene, name):
    for index, transform in us.CASES[name][1]:
        scene.set_object_transform(index, transform)
    scene.update()


def assert_same_frames(a, b, walk):
    (img, img2, cnt), (ref, ref2, ref_cnt) = a, b
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32)), int(np.count_nonzero(img.view(np.uint32) != ref.view(np.uint32)))
    assert np.array_equal(img2.view(np.uint32), ref2.view(np.uint32))
    for n in (COMPARED if walk == "counting" else NOT_INTERSECTION):
        assert cnt[n] == ref_cnt[n], n


def frame(vp):
    img, img2 = vp.sum_buffer(secondary=True)
    return img, img2, vp.counters()


@pytest.mark.parametrize("name", GPU_CASES)
def test_render_update_reset_render(built, walk, name):
    """the oracle on the updated descriptor, and a fresh Viewport over a freshly built scene fed the same per-pass constants"""
    scene, camera = us.CASES[name][0](W / H)
    vp = viewport(scene, walk)
    passes(vp, camera, 2)
    before = vp.sum_buffer()
    kernel_before = ra.update_info(vp.device_context())
    assert kernel_before["numUpdates"] == 0 and kernel_before["bytesUploaded"] == 0
    move(scene, name)
    vp.update_scene()
    vp.reset()
    oracle = Oracle()
    params = passes(vp, camera, 2, oracle, scene)
    got = frame(vp)
    assert_identical(got[0], got[1], got[2], oracle.sum, oracle.secondary, oracle.named(), walk)
    assert not np.array_equal(got[0], before)      # the move shows
    info = ra.update_info(vp.device_context())
    assert info["numUpdates"] == 1 and info["walk"] == kernel_before["walk"] and info["topDepth"] == us.top_depth(us.desc_arrays(scene)["topNodes"])
    if walk == "default":
        assert info["walk"] == {"cornell": "wide2", "mesh": "wide2", "sphere_light": "binary", "single_mesh": "wide"}[name]
    else:
        assert info["walk"] == "binary"
    new, _ = us.fresh(name, W / H)
    other = viewport(new, walk)
    for p in params:
        other.render_pass_with(p)
    assert_same_frames(got, frame(other), walk)


def test_an_update_with_passes_queued_equals_the_synchronised_sequence(built, walk):
    """passes queued before the call render the scene as it was, passes after it the new one: no read-back in between, one in between, and the oracle"""
    frames = []
    for synchronise in (False, True):
        scene, camera = us.CASES["mesh"][0](W / H)
        vp = viewport(scene, walk)
        oracle = Oracle()
        passes(vp, camera, 2, oracle, scene)
        if synchronise:
            vp.sum_buffer()
        move(scene, "mesh")
        vp.update_scene()
        passes(vp, camera, 2, oracle, scene)
        frames.append(frame(vp))
        assert_identical(frames[-1][0], frames[-1][1], frames[-1][2], oracle.sum, oracle.secondary, oracle.named(), walk)
    assert_same_frames(frames[0], frames[1], walk)


def test_two_updates_in_a_row_equal_one(built, walk):
    """the second update's previousIndex relates to the first one's order: half of the moves, then the rest, against all at once"""
    name = "cornell"
    moves = us.CASES[name][1]
    scene, camera = us.CASES[name][0](W / H)
    vp = viewport(scene, walk)
    passes(vp, camera, 1)
    scene.set_object_transform(*moves[0]); scene.update(); vp.update_scene()
    scene.set_object_transform(*moves[1]); scene.update(); vp.update_scene()
    assert ra.update_info(vp.device_context())["numUpdates"] == 2
    vp.reset()
    params = passes(vp, camera, 2)
    once, _ = us.CASES[name][0](W / H)
    other = viewport(once, walk)
    move(once, name)
    other.update_scene()       # (never uploaded before: goes up whole -- the updated flat scene)
    for p in params:
        other.render_pass_with(p)
    assert_same_frames(frame(vp), frame(other), walk)
    assert np.array_equal(us.desc_arrays(scene)["objects"], us.desc_arrays(once)["objects"])


def _bad_updates(scene):
    """(expected status, RtSceneUpdate, keep-alive) for an update that is valid for the scene as first built, broken in one way each"""
    u = scene.update_desc()
    n = u.numObjects
    out = []
    wrong_count = ra.RtSceneUpdate.from_buffer_copy(u); wrong_count.numObjects = n - 1
    out.append((INVALID_ARGUMENT, wrong_count, None))
    objects = (ra.RtObject * n)(*[u.objects[i] for i in range(n)])
    objects[n - 1].shapeKind = (objects[n - 1].shapeKind + 1) % 3
    changed = ra.RtSceneUpdate.from_buffer_copy(u); changed.objects = C.cast(objects, C.POINTER(ra.RtObject))
    out.append((INVALID_ARGUMENT, changed, objects))
    previous = (C.c_uint32 * n)(*[u.previousIndex[i] for i in range(n)])
    previous[0] = previous[1]
    twice = ra.RtSceneUpdate.from_buffer_copy(u); twice.previousIndex = C.cast(previous, C.POINTER(C.c_uint32))
    out.append((INVALID_ARGUMENT, twice, previous))
    nodes = (ra.RtNode * u.numTopNodes)(*[u.topNodes[i] for i in range(u.numTopNodes)])
    for i in range(u.numTopNodes):
        if nodes[i].leaves & 0x3FFFFFFF:
            nodes[i].childIndex = n     # a leaf past the object table
            break
    stray = ra.RtSceneUpdate.from_buffer_copy(u); stray.topNodes = C.cast(nodes, C.POINTER(ra.RtNode))
    out.append((INVALID_ARGUMENT, stray, nodes))
    wide_leaf = (ra.RtNode * u.numTopNodes)(*[u.topNodes[i] for i in range(u.numTopNodes)])
    for i in range(u.numTopNodes):
        if wide_leaf[i].leaves & 0x3FFFFFFF:
            wide_leaf[i].leaves = (wide_leaf[i].leaves & 0xC0000000) | 4
            break
    four = ra.RtSceneUpdate.from_buffer_copy(u); four.topNodes = C.cast(wide_leaf, C.POINTER(ra.RtNode))
    out.append((UNSUPPORTED, four, wide_leaf))
    version = ra.RtSceneUpdate.from_buffer_copy(u); version.abiVersion = 2
    out.append((INVALID_ARGUMENT, version, None))
    return out


def test_a_refused_update_leaves_the_scene_as_it_was(built, walk):
    lib = ra.rtgpu_lib()
    scene, camera = us.CASES["cornell"][0](W / H)
    vp = viewport(scene, walk)
    ctx = vp.device_context()
    moved, _ = us.updated("cornell", W / H)       # the same scene, moved: its update fits the device's state
    assert lib.rtgpu_update_objects(ctx, C.byref(moved.update_desc())) == NOT_READY      # nothing uploaded yet
    passes(vp, camera, 1)
    vp.sum_buffer()
    for status, update, _keep in _bad_updates(moved):
        assert lib.rtgpu_update_objects(ctx, C.byref(update)) == status, lib.rtgpu_last_error()
    assert ra.update_info(ctx)["numUpdates"] == 0
    vp.reset()
    oracle = Oracle()
    passes(vp, camera, 2, oracle, scene)
    got = frame(vp)
    assert_identical(got[0], got[1], got[2], oracle.sum, oracle.secondary, oracle.named(), walk)
    # and the update itself, unbroken, is taken
    assert lib.rtgpu_update_objects(ctx, C.byref(moved.update_desc())) == 0, lib.rtgpu_last_error()
    vp.reset()
    oracle = Oracle()
    passes(vp, camera, 2, oracle, moved)
    got = frame(vp)
    assert_identical(got[0], got[1], got[2], oracle.sum, oracle.secondary, oracle.named(), walk)


def test_the_update_reaches_both_peers(built):
    frames = []
    params = None
    for devices in (None, [0, 0]):
        scene, camera = us.CASES["mesh"][0](W / H)
        vp = viewport(scene, "default", devices=devices)
        passes(vp, camera, 1)
        move(scene, "mesh")
        vp.update_scene()
        vp.reset()
        if params is None:
            params = passes(vp, camera, 2)
        else:
            for p in params:
                vp.render_pass_with(p)
        frames.append(frame(vp))
    assert ra.multi_info(vp.device_context())["numDevices"] == 2
    assert_same_frames(frames[1], frames[0], "default")


def test_ray_queries_answer_the_new_scene(built, walk):
    scene, camera = us.CASES["mesh"][0](W / H)
    vp = viewport(scene, walk)
    passes(vp, camera, 1)
    rng = np.random.RandomState(3)
    origins = np.tile(np.array([[-12.5, 2.2, 0.6]], dtype=np.float32), (4096, 1))
    directions = rng.standard_normal((4096, 3)).astype(np.float32)
    old = vp.trace_rays(origins, directions, surfaces=True)
    move(scene, "mesh")
    vp.update_scene()
    got = vp.trace_rays(origins, directions, surfaces=True)
    new, _ = us.fresh("mesh", W / H)
    other = viewport(new, walk)
    other.update_scene()
    want = other.trace_rays(origins, directions, surfaces=True)
    for field in ("distance", "object_id", "sub_object_id", "uv", "position", "normal", "tangent", "tex_coord"):
        a, b = np.ascontiguousarray(getattr(got, field)), np.ascontiguousarray(getattr(want, field))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), field
    assert not np.array_equal(got.distance.view(np.uint32), old.distance.view(np.uint32))     # some rays met a moved object
    shadow, want_shadow = vp.occluded(origins, directions, 20.0), other.occluded(origins, directions, 20.0)
    assert np.array_equal(shadow, want_shadow) and 0 < np.count_nonzero(shadow) < len(shadow)
    # (material indices are left out: the fresh build numbers the materials in its own leaf order, tests/test_host_update.py)


VCM_ARGS = dict(camera_connecting_weight=0.0, initial_merging_radius=0.3, min_merging_radius=0.3)


def _vcm_viewport(scene, walk):
    scene.desc.contents.blueNoise = BLUE_NOISE.ctypes.data
    vp = ra.Viewport(W, H, seed=99)
    vp.set_renderer(scene, name="VCM", intersection_counters=(walk == "counting"))
    vp.set_vcm(**VCM_ARGS)
    return vp


def test_vcm_passes_after_an_update_against_the_oracle(built, walk):
    """update, reset, two VCM passes (the second merges with the first one's photons), compared as tests/test_gpu_vcm.py compares device and oracle: camera
    paths bit for bit, counters, photon counts"""
    scene, camera = us.CASES["cornell"][0](W / H)
    vp = _vcm_viewport(scene, walk)
    for _ in range(2):
        vp.render_pass_with(vp.next_pass_params(camera))
    assert vp.vcm_num_photons() > 0
    move(scene, "cornell")
    vp.update_scene()
    vp.reset()
    cam = np.zeros((H, W, 3), dtype=np.float32); cam2 = np.zeros((H, W, 3), dtype=np.float32); light = np.zeros((H, W, 3), dtype=np.float32)
    cnt = np.zeros(16, dtype=np.uint64)
    vcm = oracle_lib.Vcm(**VCM_ARGS)
    for i in range(2):
        p = vp.next_pass_params(camera)
        vp.render_pass_with(p)
        vcm.render_pass(scene.desc, p, W, H, cam, cam2 if i % 2 == 0 else None, light, cnt)
        assert vp.vcm_num_photons() == vcm.num_photons() > 0, i
    img, img2 = vp.sum_buffer(secondary=True)
    counters = vp.counters()
    assert np.isfinite(cam).all() and not light.any()
    assert np.array_equal(img.view(np.uint32), cam.view(np.uint32)), int(np.count_nonzero(img.view(np.uint32) != cam.view(np.uint32)))
    assert np.array_equal(img2.view(np.uint32), cam2.view(np.uint32))
    for n in (COMPARED if walk == "counting" else NOT_INTERSECTION):
        assert counters[n] == int(cnt[ra.COUNTER_NAMES.index(n)]), n


def test_a_vcm_pass_after_an_update_merges_no_stale_photons(built):
    """Two VCM passes over the scene as it was, the objects move, two more passes WITHOUT a reset: the first of them has no merge set (the photons the pass
    before it recorded show the old scene), exactly as after rtgpu_upload_scene.  Once through update_scene(), once through a whole upload of the
    rebuilt scene: the same frames, the same counters, the same photons.  (A restart -- pass index 0 -- drops the photons anyway: this is the sequence
    that tells.)"""
    frames, params = [], []
    for whole in (False, True):
        scene, camera = us.CASES["cornell"][0](W / H)
        vp = _vcm_viewport(scene, "default")
        photons = []
        for i in range(4):
            if i == 2:
                if whole:
                    for index, transform in us.CASES["cornell"][1]:
                        scene.set_object_transform(index, transform)
                    scene.build()          # a new build: the next pass uploads everything
                    scene.desc.contents.blueNoise = BLUE_NOISE.ctypes.data
                else:
                    move(scene, "cornell")
                    vp.update_scene()
            if not whole:
                params.append(vp.next_pass_params(camera))
            vp.render_pass_with(params[i])
            photons.append(vp.vcm_num_photons())
        assert ra.update_info(vp.device_context())["numUpdates"] == (0 if whole else 1)
        frames.append(frame(vp) + (photons,))
    assert np.isfinite(frames[0][0]).all() and min(frames[0][3]) > 0
    assert frames[0][3] == frames[1][3]
    assert_same_frames(frames[0][:3], frames[1][:3], "default")


def test_update_info_counts_no_triangle(built):
    """Two scenes that differ only in their mesh's triangle count upload the same bytes with an update, and that count is what the tables hold: n objects
    (192 bytes each), t top nodes (32), l lights (208), the n + 1 level records (64) and the 4-wide top level -- at most t nodes of 64 bytes and two
    16-byte gate records per object."""
    infos = []
    for triangles in (200, 20000):
        scene, camera = scene_zoo.mesh_scene(W / H, triangles=triangles)
        vp = viewport(scene, "default")
        passes(vp, camera, 1)
        move(scene, "mesh")
        vp.update_scene()
        passes(vp, camera, 1)
        assert np.isfinite(vp.sum_buffer()).all()
        d = scene.desc.contents
        infos.append((ra.update_info(vp.device_context()), d.numObjects, d.numTopNodes, d.numLights, d.numTriangles))
    (small, n, t, l, small_triangles), (large, n2, t2, l2, large_triangles) = infos
    assert (n, t, l) == (n2, t2, l2) and large_triangles > 50 * small_triangles
    assert small["walk"] == large["walk"] == "wide2"
    assert small["bytesUploaded"] == large["bytesUploaded"]
    tables = 192 * n + 32 * t + 208 * l
    assert tables < small["bytesUploaded"] <= tables + 64 * (n + 1) + 64 * t + 2 * 16 * n
    assert small["bytesUploaded"] < 36 * small_triangles       # less than the small mesh's triangles alone
