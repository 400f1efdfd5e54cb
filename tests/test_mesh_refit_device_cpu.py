"""The host's half of deforming a mesh from device memory (rtgpu_update_mesh_device), on the CPU: the mirror that learns a new bounding box alone
(Scene.set_mesh_bounds), the float keys the device's check reduces a box through (raytracer_amd/csrc/rt_refit_keys.h, tests/cpp/refit_keys_check.cpp) and
the ABI.  The device side: tests/test_gpu_mesh_refit_device.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import raytracer_amd as ra
import mesh_refit_ref as ref
import mesh_refit_scenes as ms
import update_scenes as us

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "refit_keys_check.cpp")
HEADER = os.path.join(ROOT, "raytracer_amd", "csrc", "rt_refit_keys.h")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
ASPECT = 96 / 64


def root_box(nodes0, indices, positions):
    """(lo, hi) of the model's refitted root node: what rtgpu_update_mesh_device returns"""
    nodes, _, _ = ref.refit(nodes0, indices, positions)
    f = nodes.view(np.float32)
    return f[0, 0:3].copy(), f[0, 4:7].copy()


# ---- the mirror ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(ms.SCENES))
def test_the_mirror_follows_a_box_alone_as_it_follows_the_vertices(built, kind):
    """twins: A takes the new positions (set_mesh_vertices), B only the root box the model gives for them (set_mesh_bounds).  The top level, the objects and
    previousIndex of update() are the same to the bit; B lists no mesh for the device and says the objects moved."""
    a, _, pos, idx, _ = ms.SCENES[kind]("grid17", ASPECT)
    b = ms.SCENES[kind]("grid17", ASPECT)[0]
    nodes0, indices, tris0 = ms.mesh_tables(b)
    assert not b.mesh_on_device(ms.MESH_OBJECT)
    for step in (1, 2):
        new = ms.deformed(pos, step)
        a.set_mesh_vertices(ms.MESH_OBJECT, new)
        lo, hi = root_box(nodes0, indices, new)
        b.set_mesh_bounds(ms.MESH_OBJECT, lo, hi)
        assert b.mesh_on_device(ms.MESH_OBJECT) and not a.mesh_on_device(ms.MESH_OBJECT)
        if kind == "two_level":
            assert b.mesh_on_device(1) and not b.mesh_on_device(3) and not b.mesh_on_device(2)     # the instance shares the mesh; the prop and the sphere do not
        a.update()
        b.update()
        ta, tb = us.desc_arrays(a), us.desc_arrays(b)
        for key in ("topNodes", "objects", "lights"):
            assert np.array_equal(ta[key], tb[key]), (step, key)
        n = a.desc.contents.numObjects
        ua, ub = a.update_desc(), b.update_desc()
        assert [ua.previousIndex[i] for i in range(n)] == [ub.previousIndex[i] for i in range(n)]
        assert [u.meshIndex for u in a.mesh_update_descs()] == [ms.mesh_index(a)] and b.mesh_update_descs() == []
        # B's share of the mesh is stale, as documented: still the tables of the upload
        nodes, _, tris = ms.mesh_tables(b)
        assert np.array_equal(nodes, nodes0) and np.array_equal(tris.view(np.uint32), tris0.view(np.uint32))
    if kind == "two_level":
        assert not np.array_equal(us.desc_arrays(b)["topNodes"], us.desc_arrays(ms.SCENES[kind]("grid17", ASPECT)[0])["topNodes"])       # the box did move the top level


def test_a_device_owned_mesh_refuses_a_rebuild_and_vertices_take_it_back(built, capfd):
    scene, _, pos, idx, _ = ms.two_level_scene("tri3", ASPECT)
    nodes0, indices, _ = ms.mesh_tables(scene)
    new = ms.deformed(pos, 1)
    with pytest.raises(ValueError):
        scene.set_mesh_bounds(2, *root_box(nodes0, indices, new))           # the sphere
    with pytest.raises(ValueError):
        scene.set_mesh_bounds(99, *root_box(nodes0, indices, new))
    assert not scene.mesh_on_device(2) and not scene.mesh_on_device(99)
    scene.set_mesh_bounds(1, *root_box(nodes0, indices, new))               # through the instance: the same mesh
    assert scene.mesh_on_device(ms.MESH_OBJECT)
    with pytest.raises(RuntimeError, match="deformed on the device"):
        scene.build()                                                       # would flatten the stale mesh
    assert "deformed on the device" in capfd.readouterr().err
    scene.update()                                                          # the objects alone: fine
    assert scene.mesh_update_descs() == []
    # the scene's own vertices take the mesh back: listed for the device again, normals and tangents with it (the device's may be newer)
    scene.set_mesh_vertices(ms.MESH_OBJECT, new)
    assert not scene.mesh_on_device(ms.MESH_OBJECT) and not scene.mesh_on_device(1)
    scene.update()
    u = scene.mesh_update_descs()
    assert len(u) == 1 and u[0].meshIndex == ms.mesh_index(scene) and u[0].shading
    want_nodes, want_tris, _ = ref.refit(nodes0, indices, new)
    nodes, _, tris = ms.mesh_tables(scene)
    assert np.array_equal(nodes, want_nodes) and np.array_equal(tris.view(np.uint32), want_tris.view(np.uint32))
    scene.build()                                                           # and a rebuild is allowed again
    assert scene.object_mesh(ms.MESH_OBJECT)[1] == len(pos) and scene.object_mesh(1) == scene.object_mesh(ms.MESH_OBJECT)
    with pytest.raises(ValueError):
        scene.object_mesh(2)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_abi_of_device_mesh_updates(built):
    header = open(os.path.join(ROOT, "include", "rtgpu.h")).read()
    lib = ra.rtgpu_lib()
    assert hasattr(lib, "rtgpu_update_mesh_device") and re.search(r"\bint rtgpu_update_mesh_device\(", header)
    assert lib.rtgpu_abi_version() == 3
    assert C.sizeof(ra.RtMeshUpdateDevice) == 40
    assert [n for n, _ in ra.RtMeshUpdateDevice._fields_] == ["abiVersion", "meshIndex", "numVertices", "flags", "positions", "normals", "tangents"]
    assert C.sizeof(ra.RtMeshUpdate) == 32                                                  # nothing existing changed its layout
    status, box = ra.update_mesh_device(None, 0, 3, None)
    assert status == -1 and b"NULL" in lib.rtgpu_last_error() and not box.any()
    for name in ("rth_scene_set_mesh_bounds", "rth_scene_mesh_on_device", "rth_scene_object_mesh", "rth_viewport_scene_in_step"):
        assert hasattr(ra.host_lib(), name), name


# ---- the keys --------------------------------------------------------------------------------------------------------------------------------------------
def build_keys_check(flags=(), suffix=""):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "refit_keys_check" + suffix)
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in (SRC, HEADER)):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + list(flags) + [SRC, "-o", exe])   # plain g++: nothing of ROCm on the include path
    return exe


@pytest.mark.parametrize("flags, suffix", [((), ""), (("-fsanitize=address,undefined", "-fno-sanitize-recover=all"), "_asan")], ids=["plain", "sanitizers"])
def test_the_float_keys_keep_their_contract(flags, suffix):
    """host code only, a program of its own: no preload"""
    r = subprocess.run([build_keys_check(flags, suffix)], capture_output=True, text=True)
    assert r.returncode == 0 and "refit keys: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
