"""rtgpu_update_mesh_device (Viewport.update_mesh_device): a mesh deformed from tensors that are on the device already, held to everything
tests/test_gpu_mesh_refit.py holds the host entry to -- the same NumPy model of the refit rules (tests/mesh_refit_ref.py), the same pure host function's
4-wide tables (tests/cpp/mesh_refit_check.cpp's emit mode), the same oracle -- and to the host entry itself on a twin scene.

  tables     rtgpu_read_mesh, rtgpu_read_wide_level and the returned box, bit for bit, BEFORE anything is rendered.  The 4 096-triangle soup gives the
             check kernel 144 blocks (16 of them with triangles): its atomics meet across blocks.
  frames     twins built alike, A by Scene.set_mesh_vertices and B by update_mesh_device: the same sum buffer, secondary buffer and counters, and the
             oracle's on A's descriptor, under both walks (tests/conftest.py); with normals and tangents, and with normals alone.
  refusals   leave rtgpu_read_mesh, rtgpu_read_wide_level and a frame as they were, as a mesh's first update and after an accepted one.
  96 x 64, 2 passes, depth 4."""
import ctypes as C

import numpy as np
import pytest

import raytracer_amd as ra
import mesh_refit_ref as ref
import mesh_refit_scenes as ms
from test_gpu_parity import assert_identical
from test_gpu_update import H, W, Oracle, assert_same_frames, frame, passes, viewport
from test_mesh_refit_cpu import bits, expected_tables, flattened

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, NOT_READY, UNSUPPORTED = 0, -1, -5, -6
ASPECT = W / H
RENDER_MESH = "grid17"


@pytest.fixture(scope="module")
def expected(built, tmp_path_factory):
    """the pure host function's tables for every mesh at steps 0 (as uploaded), 1 and 2: computed once, on the CPU"""
    return expected_tables(tmp_path_factory.mktemp("refit_device"), (0, 1, 2))


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def mesh_objects(scene):
    """the flat objects that are the deforming mesh (leaf order)"""
    o, mi = scene.desc.contents, ms.mesh_index(scene)
    return [i for i in range(o.numObjects) if o.objects[i].objectKind == 0 and o.objects[i].shapeKind == 3 and o.objects[i].meshIndex == mi]


def shading_of(new, idx, normals, tangents):
    n = ms.vertex_normals(new, idx) if normals or tangents else None
    return (n if normals else None), (ms.vertex_tangents(n) if tangents else None)


def deform_host(scene, vp, new, normals=None, tangents=None):
    scene.set_mesh_vertices(ms.MESH_OBJECT, new, normals, tangents)
    scene.update()
    vp.update_scene()


def deform_device(scene, vp, new, normals=None, tangents=None):
    """the device route; where there is a top level the objects follow, exactly as after any move -- a one-object scene needs nothing more"""
    lo, hi = vp.update_mesh_device(ms.MESH_OBJECT, dev(new), dev(normals), dev(tangents))
    assert scene.mesh_on_device(ms.MESH_OBJECT)
    if scene.desc.contents.numObjects > 1:
        scene.update()
        assert scene.mesh_update_descs() == []
        vp.update_scene()
    return lo, hi


def read_tables(ctx, scene, num_nodes, num_triangles, wide=True):
    """everything a refit writes, as it stands on the device: the mesh's nodes and triangles, and the 4-wide level of every object over it"""
    nodes, tris = ra.read_mesh(ctx, ms.mesh_index(scene), num_nodes, num_triangles)
    return nodes, tris, [ra.read_wide_level(ctx, o) for o in mesh_objects(scene)] if wide else []


def assert_same_tables(got, want, what):
    assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])), what
    assert len(got[2]) == len(want[2])
    for (info, records, gates), (winfo, wrecords, wgates) in zip(got[2], want[2]):
        for key in ("base", "step", "bound"):
            assert np.array_equal(bits(info[key]), bits(winfo[key])), (what, key)
        assert np.array_equal(records, wrecords) and np.array_equal(bits(gates), bits(wgates)), what


def assert_tables_equal_the_model(ctx, scene, nodes0, indices, positions, e, what, wide=True):
    """the device's tables against the NumPy model and, where the mesh has a 4-wide level, against the pure host function's tables `e`"""
    want_nodes, want_tris, _ = ref.refit(nodes0, indices, positions)
    nodes, tris, levels = read_tables(ctx, scene, len(nodes0), len(indices), wide)
    assert np.array_equal(nodes, want_nodes), (what, int(np.count_nonzero(nodes != want_nodes)))
    assert np.array_equal(bits(tris), bits(want_tris)), what
    for info, records, gates in levels:
        assert info["valid"] == 1
        for key in ("base", "step", "bound"):
            assert np.array_equal(bits(info[key]), bits(e[key])), (what, key, info[key], e[key])
        assert np.array_equal(records, e["records"]), (what, int(np.count_nonzero(records != e["records"])))
        assert np.array_equal(bits(gates), bits(e["gates"])), what
    return want_nodes.view(np.float32)[0, 0:3], want_nodes.view(np.float32)[0, 4:7]


# ---- 1. tables -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(ms.SCENES))
@pytest.mark.parametrize("name", ms.MESHES)
def test_the_device_route_s_tables_equal_the_model_before_anything_is_rendered(built, expected, kind, name):
    scene, camera, pos, idx, nrm = ms.SCENES[kind](name, ASPECT)
    nodes0, indices, tris0 = ms.mesh_tables(scene)
    vp = viewport(scene, "default")
    vp.update_scene()            # never uploaded: goes up whole
    ctx = vp.device_context()
    wide = not (kind == "single" and name in ("tri1", "tri2"))     # a single mesh whose root is a leaf has no 4-wide tree: the binary walk serves it
    before = ra.update_info(ctx)
    assert before["numMeshUpdates"] == 0
    for step, with_normals in ((1, False), (2, True)):
        new = ms.deformed(pos, step)
        normals, tangents = shading_of(new, idx, with_normals, with_normals)
        lo, hi = deform_device(scene, vp, new, normals, tangents)
        want_lo, want_hi = assert_tables_equal_the_model(ctx, scene, nodes0, indices, new, expected[(name, step)], (name, step), wide)
        assert np.array_equal(bits(lo), bits(want_lo)) and np.array_equal(bits(hi), bits(want_hi)), (step, lo, hi, want_lo, want_hi)      # the refitted root's floats
        info = ra.update_info(ctx)
        assert info["numMeshUpdates"] == step and info["walk"] == before["walk"]
        if kind == "single":     # (two-level: the objects update that follows is the last one, and bytesUploaded is the last update's)
            # never the arrays: the first update brings the vertex indices (16 bytes a triangle) and the depth offsets; the root node comes back
            assert info["bytesUploaded"] <= (step == 1) * (16 * len(indices) + 4 * 66) + 32 and info["numUpdates"] == 0
            assert (info["bytesUploaded"] > 0) == (step == 1 or wide)
    # the original positions again: the uploaded tables return -- the device's tables are a function of the positions alone
    deform_device(scene, vp, pos)
    assert_tables_equal_the_model(ctx, scene, nodes0, indices, pos, expected[(name, 0)], (name, 0), wide)
    nodes, tris, _ = read_tables(ctx, scene, len(nodes0), len(indices), False)
    assert np.array_equal(nodes, nodes0) and np.array_equal(bits(tris), bits(tris0))


# ---- 2. frames -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(ms.SCENES))
def test_twin_scenes_render_the_same_frames_by_either_route(built, walk, kind):
    a, camera, pos, idx, nrm = ms.SCENES[kind](RENDER_MESH, ASPECT)
    b = ms.SCENES[kind](RENDER_MESH, ASPECT)[0]
    vpa, vpb = viewport(a, walk), viewport(b, walk)
    vpa.update_scene()
    vpb.update_scene()
    last = None
    # positions alone; normals and tangents; normals alone (the tangents keep what the records hold: those of step 2)
    for step, with_normals, with_tangents in ((1, False, False), (2, True, True), (1, True, False)):
        new = ms.deformed(pos, step)
        normals, tangents = shading_of(new, idx, with_normals, with_tangents)
        deform_host(a, vpa, new, normals, tangents)
        deform_device(b, vpb, new, normals, tangents)
        vpa.reset()
        vpb.reset()
        oracle = Oracle()
        params = passes(vpa, camera, 2, oracle, a)
        for p in params:
            vpb.render_pass_with(p)
        fa, fb = frame(vpa), frame(vpb)
        assert_same_frames(fb, fa, walk)
        assert_identical(fb[0], fb[1], fb[2], oracle.sum, oracle.secondary, oracle.named(), walk)
        assert last is None or not np.array_equal(fb[0], last)          # the deformation shows
        last = fb[0]
        assert ra.update_info(vpb.device_context())["walk"] == ra.update_info(vpa.device_context())["walk"]


# ---- 3. vertices no triangle uses ------------------------------------------------------------------------------------------------------------------------
def test_a_vertex_no_triangle_uses_counts_for_the_finite_check_alone(built, expected):
    import torch
    pos, idx, nrm = ms.mesh(RENDER_MESH)
    far = np.array([[4.0e5, -3.0e5, 2.5e5]], dtype=np.float32)
    scene = ra.Scene()
    scene.add_mesh(np.concatenate([pos, far]), idx, np.concatenate([nrm, nrm[:1]]), ms.vertex_tangents(np.concatenate([nrm, nrm[:1]])),
                   default_material=scene.add_material("diffuse", (0.7, 0.6, 0.5)))
    scene.add_background_light((1.0, 1.5, 2.0))
    scene.build()
    nodes0, indices, tris0 = ms.mesh_tables(scene)
    plain0 = ms.mesh_tables(ms.single_mesh_scene(RENDER_MESH, ASPECT)[0])
    assert np.array_equal(nodes0, plain0[0]) and np.array_equal(indices[:, :3], plain0[1][:, :3])      # the same tree as the mesh without the vertex: `expected` serves
    vp = viewport(scene, "default")
    vp.update_scene()
    ctx = vp.device_context()
    new = ms.deformed(pos, 1)
    boxes = []
    for extra in (far, -7.0 * far):
        lo, hi = vp.update_mesh_device(0, dev(np.concatenate([new, extra])))
        want_lo, want_hi = assert_tables_equal_the_model(ctx, scene, nodes0, indices, np.concatenate([new, extra]), expected[(RENDER_MESH, 1)], "unused vertex")
        assert np.array_equal(bits(lo), bits(want_lo)) and np.array_equal(bits(hi), bits(want_hi)) and np.abs(hi).max() < 10.0
        boxes.append((lo, hi))
    assert np.array_equal(boxes[0], boxes[1])
    held = read_tables(ctx, scene, len(nodes0), len(indices))
    # ... but every float is held to being finite, used or not
    for row, value in ((len(new), np.nan), (len(new), -np.inf), (5, np.inf), (len(new) // 2, np.nan)):
        bad = np.concatenate([ms.deformed(pos, 2), far])
        bad[row, 1] = value
        t = dev(bad)
        status, _ = ra.update_mesh_device(ctx, 0, len(bad), t.data_ptr())
        torch.cuda.synchronize()
        assert status == INVALID_ARGUMENT and b"not finite" in ra.rtgpu_lib().rtgpu_last_error(), (row, value)
        with pytest.raises(ValueError, match="not finite"):
            vp.update_mesh_device(0, t)
    assert_same_tables(read_tables(ctx, scene, len(nodes0), len(indices)), held, "after the refusals")
    assert ra.update_info(ctx)["numMeshUpdates"] == 2


def test_the_check_alone_is_the_box_over_the_referenced_positions(built):
    """rtgpu_refit_check_async's record against NumPy: a minimum and a maximum are exact, so the record is a function of the positions alone -- on the soup
    across 144 blocks.  Where a bound is a zero the keys' rule holds: -0 below +0, whichever the positions hold first"""
    import torch
    scene, camera, pos, idx, nrm = ms.single_mesh_scene("soup4096", ASPECT)
    vp = viewport(scene, "default")
    vp.update_scene()
    ctx = vp.device_context()
    for step in (0, 1, 2):
        new = pos if step == 0 else ms.deformed(pos, step)
        got = ra.refit_check(ctx, 0, dev(new))
        used = new[idx.reshape(-1)]
        assert not got["non_finite"] and np.array_equal(bits(got["lo"]), bits(used.min(axis=0))) and np.array_equal(bits(got["hi"]), bits(used.max(axis=0))), step
    zeros = np.abs(ms.deformed(pos, 1))
    zeros[:, 2] = np.where(np.arange(len(zeros)) % 3 == 0, -0.0, 0.0)      # z: flat at zero, of both signs; x and y: positive
    zeros[7, 0], zeros[11, 0], zeros[4000, 1] = 0.0, -0.0, 0.0             # x: both zeros below everything else; y: +0 alone
    got = ra.refit_check(ctx, 0, dev(zeros))
    assert bits(got["lo"]).tolist() == [0x80000000, 0x00000000, 0x80000000] and bits(got["hi"][2:]).tolist() == [0x00000000]
    assert np.array_equal(got["hi"][:2], zeros[:, :2].max(axis=0))
    bad = ms.deformed(pos, 1)
    bad[-1, 2] = np.nan
    assert ra.refit_check(ctx, 0, dev(bad))["non_finite"]
    with pytest.raises(ValueError):
        ra.refit_check(ctx, 0, dev(pos[:-1]))
    torch.cuda.synchronize()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("after_an_accepted_one", [False, True], ids=["first_update", "after_an_accepted_one"])
def test_a_refused_device_update_leaves_the_device_as_it_was(built, after_an_accepted_one):
    import torch
    lib = ra.rtgpu_lib()
    for devices in (None, [0, 0]):       # [0, 0]: one device used as two, the emulated multi-device context
        scene, camera, pos, idx, nrm = ms.two_level_scene(RENDER_MESH, ASPECT)
        nodes0, indices, _ = ms.mesh_tables(scene)
        vp = viewport(scene, "default", devices=devices)
        ctx, mi = vp.device_context(), ms.mesh_index(scene)
        good = dev(ms.deformed(pos, 2))
        if devices is None:
            assert ra.update_mesh_device(ctx, mi, len(pos), good.data_ptr())[0] == NOT_READY      # nothing uploaded yet
            with pytest.raises(RuntimeError, match="in step"):
                vp.update_mesh_device(ms.MESH_OBJECT, good)
        vp.update_scene()
        if after_an_accepted_one and devices is None:
            deform_device(scene, vp, ms.deformed(pos, 1))
        elif after_an_accepted_one:
            deform_host(scene, vp, ms.deformed(pos, 1))
        updates = ra.update_info(ctx)["numMeshUpdates"]
        assert updates == int(after_an_accepted_one)
        params = passes(vp, camera, 2)
        before, tables = frame(vp), read_tables(ctx, scene, len(nodes0), len(indices))
        if devices is not None:
            assert ra.multi_info(ctx)["numDevices"] == 2
            assert ra.update_mesh_device(ctx, mi, len(pos), good.data_ptr())[0] == UNSUPPORTED and b"multi-device" in lib.rtgpu_last_error()
            with pytest.raises(RuntimeError, match="multi-device"):
                vp.update_mesh_device(ms.MESH_OBJECT, good)
        else:
            # the sheet settled flat at z = 0.25, and the mesh far from its origin: the 16-bit grid cannot hold the box with its margin
            for positions in (flattened(ms.deformed(pos, 2)), ms.deformed(pos, 2) + np.float32(1.0e4)):
                t = dev(positions)
                assert ra.update_mesh_device(ctx, mi, len(pos), t.data_ptr())[0] == UNSUPPORTED and b"grid" in lib.rtgpu_last_error(), lib.rtgpu_last_error()
            host = np.ascontiguousarray(ms.deformed(pos, 2))
            normals = dev(ms.vertex_normals(host, idx))
            for args, word in (((mi, len(pos) - 1, good.data_ptr()), b"vertex count"),                          # a wrong vertex count
                               ((mi, len(pos), host.ctypes.data), b"positions"),                                # a host pointer
                               ((mi, len(pos), good.data_ptr(), host.ctypes.data), b"normals"),
                               ((mi, len(pos), good.data_ptr(), normals.data_ptr(), host.ctypes.data), b"tangents"),
                               ((mi, len(pos), good.data_ptr() + 2), b"aligned"),
                               ((mi, len(pos), None), b"NULL"),
                               ((2, len(pos), good.data_ptr()), b"range"),
                               ((1 - mi, len(pos), good.data_ptr()), b"vertex count")):                        # the prop's mesh, which has another vertex count
                assert ra.update_mesh_device(ctx, *args)[0] == INVALID_ARGUMENT and word in lib.rtgpu_last_error(), (args, lib.rtgpu_last_error())
            # an array a float short of 12 bytes per vertex before its ALLOCATION ends (torch carves tensors out of larger segments: the library can hold a
            # pointer to the segment alone, whose end torch's snapshot tells)
            at = good.data_ptr()
            segment = next(s for s in torch.cuda.memory_snapshot() if s["address"] <= at < s["address"] + s["total_size"])
            near_the_end = segment["address"] + segment["total_size"] - (12 * len(pos) - 4)
            assert ra.update_mesh_device(ctx, mi, len(pos), near_the_end)[0] == INVALID_ARGUMENT and b"allocation" in lib.rtgpu_last_error(), lib.rtgpu_last_error()
            assert ra.update_mesh_device(ctx, mi, len(pos), good.data_ptr(), near_the_end)[0] == INVALID_ARGUMENT and b"normals" in lib.rtgpu_last_error()
            u = ra.RtMeshUpdateDevice(2, mi, len(pos), 0, good.data_ptr(), None, None)
            assert lib.rtgpu_update_mesh_device(ctx, C.byref(u), None, None) == INVALID_ARGUMENT and b"abiVersion" in lib.rtgpu_last_error()
            u = ra.RtMeshUpdateDevice(3, mi, len(pos), 1, good.data_ptr(), None, None)
            assert lib.rtgpu_update_mesh_device(ctx, C.byref(u), None, None) == INVALID_ARGUMENT and b"flags" in lib.rtgpu_last_error()
            assert lib.rtgpu_update_mesh_device(ctx, None, None, None) == INVALID_ARGUMENT
            # Python-level: before the library is called
            for bad in (good.cpu(), good.double(), dev(np.zeros((len(pos), 6), dtype=np.float32))[:, :3], good[:-1], good.reshape(-1)):
                with pytest.raises(ValueError, match="must"):
                    vp.update_mesh_device(ms.MESH_OBJECT, bad)
            with pytest.raises(ValueError, match="normals"):
                vp.update_mesh_device(ms.MESH_OBJECT, good, normals=good.cpu())
            with pytest.raises(ValueError):
                vp.update_mesh_device(2, good)            # the sphere
            assert not scene.mesh_on_device(ms.MESH_OBJECT) or after_an_accepted_one
        torch.cuda.synchronize()
        assert ra.update_info(ctx)["numMeshUpdates"] == updates
        assert_same_tables(read_tables(ctx, scene, len(nodes0), len(indices)), tables, devices)
        vp.reset()
        for p in params:
            vp.render_pass_with(p)
        assert_same_frames(frame(vp), before, "default")
        if devices is None:
            # ... and the update itself, unbroken, is taken
            assert ra.update_mesh_device(ctx, mi, len(pos), good.data_ptr())[0] == OK, lib.rtgpu_last_error()
            assert ra.update_info(ctx)["numMeshUpdates"] == updates + 1


def test_a_whole_upload_refuses_while_a_mesh_is_device_owned(built, capfd):
    scene, camera, pos, idx, nrm = ms.two_level_scene("tri3", ASPECT)
    vp = viewport(scene, "default")
    vp.update_scene()
    deform_device(scene, vp, ms.deformed(pos, 1))
    other = ra.Viewport(W, H, seed=77, max_ray_depth=4)
    other.set_renderer(scene)
    with pytest.raises(RuntimeError):
        other.update_scene()                         # would put the scene's stale copy of the mesh on a device
    assert "deformed on the device" in capfd.readouterr().err
    scene.set_mesh_vertices(ms.MESH_OBJECT, ms.deformed(pos, 1))
    assert not scene.mesh_on_device(ms.MESH_OBJECT)
    other.update_scene()


# ---- 5. streams ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [True, False], ids=["side_stream", "default_stream"])
def test_the_call_waits_for_the_stream_that_made_the_positions_and_is_done_on_return(built, expected, side):
    """the positions are the result of a torch op queued (behind a matrix product that keeps the stream busy) immediately before the call, and are zeroed
    immediately after it returns: tables of zeros, or of what the tensor held before, would show a call that did not wait or had not finished"""
    import torch
    name = "soup4096"
    scene, camera, pos, idx, nrm = ms.single_mesh_scene(name, ASPECT)
    nodes0, indices, _ = ms.mesh_tables(scene)
    vp = viewport(scene, "default")
    vp.update_scene()
    ctx = vp.device_context()
    stream = torch.cuda.Stream() if side else torch.cuda.default_stream()
    busy = torch.rand((2048, 2048), device="cuda")
    for step in (1, 2):
        new = ms.deformed(pos, step)
        source, normals_source = dev(new), dev(ms.vertex_normals(new, idx))
        positions, normals = torch.full_like(source, 3.0), torch.zeros_like(source)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for _ in range(4):
                busy = busy @ busy * 1.0e-3
            positions.copy_(source)
            normals.copy_(normals_source)
            lo, hi = vp.update_mesh_device(0, positions, normals)
            positions.zero_()
            normals.zero_()
        want_lo, want_hi = assert_tables_equal_the_model(ctx, scene, nodes0, indices, new, expected[(name, step)], (side, step))
        assert np.array_equal(bits(lo), bits(want_lo)) and np.array_equal(bits(hi), bits(want_hi))
    # the normals arrived too: a frame against the oracle on a twin that took the same arrays on the host
    twin = ms.single_mesh_scene(name, ASPECT)[0]
    twin.set_mesh_vertices(0, new, ms.vertex_normals(new, idx))
    twin.update()
    oracle = Oracle()
    passes(vp, camera, 2, oracle, twin)
    got = frame(vp)
    assert_identical(got[0], got[1], got[2], oracle.sum, oracle.secondary, oracle.named(), "default")


# ---- 6. the temporal history -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("track", [True, False], ids=["tracking", "no_tracking"])
def test_the_history_takes_a_device_update_as_it_takes_a_host_update(built, track):
    """twin contexts, frame by frame: denoise(temporal=True) after a device-route update equals the call after a host-route update bit for bit.  The
    history's lengths are not read back: frame 2's output is blended with weights that are the lengths frame 1 stored, so frame 2 holds them"""
    a, camera, pos, idx, nrm = ms.two_level_scene(RENDER_MESH, ASPECT)
    b = ms.two_level_scene(RENDER_MESH, ASPECT)[0]
    vpa, vpb = viewport(a, "default"), viewport(b, "default")
    for vp in (vpa, vpb):
        vp.track_deformation(track)
    images = []
    for k in range(3):
        if k:
            new = ms.deformed(pos, k)
            normals, tangents = shading_of(new, idx, True, True)
            deform_host(a, vpa, new, normals, tangents)
            deform_device(b, vpb, new, normals, tangents)
        vpa.reset()
        vpb.reset()
        params = [vpa.next_pass_params(camera) for _ in range(3)]
        for vp in (vpa, vpb):
            for p in params[:2]:
                vp.render_pass_with(p)
        ia = vpa.denoise(params[2], temporal=True, variance=False, color_scale=0.5)
        ib = vpb.denoise(params[2], temporal=True, variance=False, color_scale=0.5)
        assert np.array_equal(bits(ib), bits(ia)), (k, int(np.count_nonzero(bits(ib) != bits(ia))))
        images.append(ia)
    # the history matters: frame 2 is not what a context without one makes of the same passes
    vpa.reset_history()
    fresh = vpa.denoise(params[2], temporal=True, variance=False, color_scale=0.5)
    assert not np.array_equal(bits(fresh), bits(images[2]))
