"""Deforming meshes on the CPU: the host mirror's MeshShape::UpdateVertices (Scene.set_mesh_vertices + update()) against the NumPy model of the refit rules
(tests/mesh_refit_ref.py), bit for bit, and the pure refit function of raytracer_amd/csrc/rt_scene_prepare.h -- the model of the device kernels -- against
the contract the 4-wide walks rest on (tests/cpp/mesh_refit_check.cpp), once more under AddressSanitizer and UBSan.  The device side:
tests/test_gpu_mesh_refit.py, which takes its expected 4-wide tables from the checker's emit mode here."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import raytracer_amd as ra

import mesh_refit_ref as ref
import mesh_refit_scenes as ms
import temporal_moving_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mesh_refit_check.cpp")
HEADERS = [os.path.join(ROOT, "raytracer_amd", "csrc", h) for h in ("rt_scene_prepare.h", "rt_wide_format.h")] + [os.path.join(ROOT, "include", "rtgpu.h")]
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
ASPECT = 96 / 64


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the host mirror against the NumPy model -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(ms.SCENES))
@pytest.mark.parametrize("name", ms.MESHES)
def test_the_host_mirror_refits_as_the_model_does(built, kind, name):
    scene, _, pos, idx, nrm = ms.SCENES[kind](name, ASPECT)
    nodes0, indices, tris0 = ms.mesh_tables(scene)
    mi = ms.mesh_index(scene)
    assert len(indices) == len(idx) and scene.desc.contents.numMeshes == (2 if kind == "two_level" else 1)     # (the instance shares the mesh; the prop is the other)
    if kind == "two_level" and name == "grid17":
        import update_scenes as us
        assert mi == 1 and (us.desc_arrays(scene)["meshes"][mi][[0, 2, 4]] > 0).all()      # its ranges do not start at 0: the offsets count
    # the same positions: nothing moves, to the bit (== would pass over a zero's sign; there is none, and the words say so)
    scene.set_mesh_vertices(ms.MESH_OBJECT, pos)
    scene.update()
    nodes1, indices1, tris1 = ms.mesh_tables(scene)
    assert np.array_equal(nodes1.view(np.float32)[:, [0, 1, 2, 4, 5, 6]], nodes0.view(np.float32)[:, [0, 1, 2, 4, 5, 6]]) and np.array_equal(tris1, tris0)
    assert np.array_equal(nodes1, nodes0) and np.array_equal(bits(tris1), bits(tris0)) and np.array_equal(indices1, indices)
    assert [u.meshIndex for u in scene.mesh_update_descs()] == [mi] and not scene.mesh_update_descs()[0].shading
    # two deformations in a row, the second with normals: the model from the nodes AS UPLOADED (a refit never reads the old boxes)
    for step, with_normals in ((1, False), (2, True)):
        new = ms.deformed(pos, step)
        normals = ms.vertex_normals(new, idx) if with_normals else None
        scene.set_mesh_vertices(ms.MESH_OBJECT, new, normals, ms.vertex_tangents(normals) if with_normals else None)
        scene.update()
        nodes, _, tris = ms.mesh_tables(scene)
        want_nodes, want_tris, _ = ref.refit(nodes0, indices, new)
        assert np.array_equal(nodes, want_nodes), int(np.count_nonzero(nodes != want_nodes))
        assert np.array_equal(bits(tris), bits(want_tris))
        assert not np.array_equal(nodes, nodes0) and np.array_equal(nodes[:, [3, 7]], nodes0[:, [3, 7]])       # boxes moved, topology did not
        if len(nodes0) > 1:
            assert np.array_equal(nodes[1], nodes0[1])                                                          # node 1 is never written
        u = scene.mesh_update_descs()
        assert len(u) == 1 and u[0].numVertices == len(pos) and bool(u[0].shading) == with_normals
        assert np.array_equal(np.ctypeslib.as_array(u[0].positions, shape=(len(pos), 3)), new)
        if with_normals:
            import update_scenes as us
            a = us.desc_arrays(scene)
            shading = a["vertexShading"].view(np.float32)[a["meshes"][mi][4]:a["meshes"][mi][4] + a["meshes"][mi][5]]
            assert np.array_equal(shading[:, :3], normals) and np.array_equal(shading[:, 3:6], ms.vertex_tangents(normals)) and np.array_equal(shading[:, 6:8], pos[:, :2] * 0.5 + 0.5)
    # an update without a deformation lists no mesh
    scene.update()
    assert scene.mesh_update_descs() == []


def test_set_mesh_vertices_refuses_what_is_no_such_mesh(built):
    scene, _, pos, idx, nrm = ms.two_level_scene("tri3", ASPECT)
    with pytest.raises(ValueError):
        scene.set_mesh_vertices(ms.MESH_OBJECT, pos[:-1])          # another vertex count
    with pytest.raises(ValueError):
        scene.set_mesh_vertices(2, pos)                           # the sphere
    with pytest.raises(ValueError):
        scene.set_mesh_vertices(99, pos)
    with pytest.raises(ValueError):
        scene.set_mesh_vertices(ms.MESH_OBJECT, pos, normals=nrm[:-1])
    scene.set_mesh_vertices(1, pos)                               # through the instance: the same mesh
    with pytest.raises(ValueError):
        scene.set_mesh_vertices(3, pos)                           # the prop: another mesh, another vertex count


def test_the_abi_of_mesh_updates(built):
    import re
    header = open(os.path.join(ROOT, "include", "rtgpu.h")).read()
    lib = ra.rtgpu_lib()
    for name in ("rtgpu_update_mesh", "rtgpu_read_mesh", "rtgpu_read_wide_level"):
        assert hasattr(lib, name) and re.search(r"\bint %s\(" % name, header), name
    assert lib.rtgpu_abi_version() == 3
    assert C.sizeof(ra.RtMeshUpdate) == 32 and [n for n, _ in ra.RtMeshUpdate._fields_] == ["abiVersion", "meshIndex", "numVertices", "flags", "positions", "shading"]
    assert C.sizeof(ra.RtWideLevelInfo) == 64
    u = ra.RtMeshUpdate()
    assert lib.rtgpu_update_mesh(None, C.byref(u)) == -1 and b"NULL" in lib.rtgpu_last_error()
    assert lib.rtgpu_read_mesh(None, 0, None, None) == -1 and lib.rtgpu_read_wide_level(None, 0, None, None, C.c_uint64(0), None, C.c_uint64(0)) == -1


# ---- the pure refit function against the contract -----------------------------------------------------------------------------------------------------
def checker_input(path, steps=(1,)):
    """the meshes as uploaded with their positions of every step, one block each: (name, step) in order"""
    blocks, names = [], []
    for name in ms.MESHES:
        scene, _, pos, idx, nrm = ms.single_mesh_scene(name, ASPECT)
        nodes, indices, _ = ms.mesh_tables(scene)
        for step in steps:
            new = pos if step == 0 else ms.deformed(pos, step)
            label = "%s.%d" % (name, step)
            blocks.append(label.encode().ljust(32, b"\0") + struct.pack("<3I", len(nodes), len(indices), len(new)) + nodes.tobytes() + indices.tobytes() + new.tobytes())
            names.append((name, step))
    with open(path, "wb") as f:
        f.write(b"RTREFIT1" + struct.pack("<I", len(blocks)) + b"".join(blocks))
    return names


def build_checker(flags=(), suffix=""):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "mesh_refit_check" + suffix)
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in [SRC] + HEADERS):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + list(flags) + [SRC, "-o", exe])   # plain g++: nothing of ROCm on the include path
    return exe


def read_expected(path, names):
    """{(mesh, step): dict(grid, nodes words, triangles, records words, gates)} of the checker's emit mode"""
    out, data, at = {}, open(path, "rb").read(), 0
    for key in names:
        n_nodes, n_tris, n_rec, n_gates = struct.unpack_from("<4I", data, at); at += 16
        grid = np.frombuffer(data, np.float32, 9, at).reshape(3, 3); at += 36
        nodes = np.frombuffer(data, np.uint32, 8 * n_nodes, at).reshape(-1, 8); at += 32 * n_nodes
        tris = np.frombuffer(data, np.float32, 9 * n_tris, at).reshape(-1, 9); at += 36 * n_tris
        records = np.frombuffer(data, np.uint32, 4 * n_rec, at).reshape(-1, 4); at += 16 * n_rec
        gates = np.frombuffer(data, np.float32, 4 * n_gates, at).reshape(-1, 4); at += 16 * n_gates
        out[key] = dict(base=grid[0], step=grid[1], bound=grid[2], nodes=nodes, triangles=tris, records=records, gates=gates)
    assert at == len(data)
    return out


def expected_tables(tmp_dir, steps):
    """what the GPU tests compare the device's tables with: the pure function, run here on the CPU"""
    path = os.path.join(str(tmp_dir), "meshes.bin")
    names = checker_input(path, steps)
    out = os.path.join(str(tmp_dir), "expected.bin")
    r = subprocess.run([build_checker(), "emit", path, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return read_expected(out, names)


def test_the_pure_refit_keeps_the_contract_and_equals_the_model(built, tmp_path):
    expected = expected_tables(tmp_path, (0, 1, 2))
    assert len(expected) == 3 * len(ms.MESHES)
    for (name, step), e in expected.items():
        scene, _, pos, idx, nrm = ms.single_mesh_scene(name, ASPECT)
        nodes0, indices, _ = ms.mesh_tables(scene)
        new = pos if step == 0 else ms.deformed(pos, step)
        want_nodes, want_tris, want_gates = ref.refit(nodes0, indices, new)
        assert np.array_equal(e["nodes"], want_nodes) and np.array_equal(bits(e["triangles"]), bits(want_tris)) and np.array_equal(bits(e["gates"]), bits(want_gates)), (name, step)
        if step == 0:
            assert np.array_equal(e["nodes"], nodes0)      # the same positions: the upload's nodes


def flattened(pos):
    """the mesh settled flat at z = 0.25: the grid's base, min - 4 steps of a millionth of the extent, rounds back onto 0.25 and no record can keep its margin"""
    flat = pos.copy()
    flat[:, 2] = 0.25
    return flat


def test_the_pure_refit_says_when_the_grid_cannot_hold_the_new_box(built, tmp_path):
    """what an upload answers by leaving the mesh to the binary walk (scene_prepare_check's variants 2 and 3), rtgpu_update_mesh answers by refusing: the pure
    function's gridOk is that answer, and the checker holds it to the records themselves (a name that starts with "refuse:")"""
    scene, _, pos, idx, nrm = ms.single_mesh_scene("grid17", ASPECT)
    nodes, indices, _ = ms.mesh_tables(scene)
    blocks = []
    for label, new in (("refuse:flat", flattened(pos)), ("refuse:far", pos + np.float32(1.0e4))):
        blocks.append(label.encode().ljust(32, b"\0") + struct.pack("<3I", len(nodes), len(indices), len(new)) + nodes.tobytes() + indices.tobytes() + np.ascontiguousarray(new, dtype=np.float32).tobytes())
    path = str(tmp_path / "refused.bin")
    with open(path, "wb") as f:
        f.write(b"RTREFIT1" + struct.pack("<I", len(blocks)) + b"".join(blocks))
    r = subprocess.run([build_checker(), "check", path], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count("refused, as an upload") == 2, r.stdout[-2000:] + r.stderr[-2000:]


def test_the_pure_refit_under_the_sanitizers(built, tmp_path):
    """host code only, a program of its own: no preload"""
    exe = build_checker(("-fsanitize=address,undefined", "-fno-sanitize-recover=all"), "_asan")
    path = str(tmp_path / "meshes.bin")
    checker_input(path, (1, 2))
    r = subprocess.run([exe, "check", path], capture_output=True, text=True)
    assert r.returncode == 0 and "mesh refit: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the temporal history across a mesh update ---------------------------------------------------------------------------------------------------------
def test_a_table_with_prev_id_none_starts_that_object_s_pixels():
    """rtgpu_update_mesh gives every object of the mesh prevId = 0xFFFFFFFF in the table rtgpu_denoise_temporal builds: no tap matches, exactly those pixels
    start (history length 1), every other pixel is, word for word, what the table without that entry gives"""
    import temporal_ref
    base = temporal_ref.random_temporal_frame(37, 23, 5)
    cur = base["current"]
    n = int(max(cur["object_id"].max(), base["history"]["object_id"].max())) + 1
    counts = np.bincount(cur["object_id"].reshape(-1)[np.isfinite(cur["depth"]).reshape(-1)], minlength=n)
    updated = int(np.argmax(counts))                         # the object with the most pixels
    matrices = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    results = []
    for mark in (False, True):
        prev = np.arange(n, dtype=np.uint32)
        if mark:
            prev[updated] = 0xFFFFFFFF
        results.append(temporal_moving_ref.accumulate_moving(cur["color"], cur["color_half"], cur["depth"], cur["normal"], cur["position"], cur["albedo"], cur["object_id"],
                                                             base["history"], base["prev_world_to_screen"], base["prev_sample_offset"],
                                                             object_motion=(matrices, prev, np.zeros(n, dtype=np.uint32))))
    (plain, _, _, plain_reason), (marked, _, _, reason) = results
    mine = (cur["object_id"] == updated) & np.isfinite(cur["depth"])
    assert mine.sum() > 20 and (~mine).sum() > 20
    assert (plain_reason[mine] == temporal_ref.BLENDED).mean() > 0.3          # they would have accumulated
    assert np.array_equal(marked["length"][mine], np.ones(int(mine.sum()), dtype=np.float32)) and not (reason[mine] == temporal_ref.BLENDED).any()
    for key in ("a", "b", "length"):
        assert np.array_equal(bits(marked[key][~mine]), bits(plain[key][~mine])), key
    assert np.array_equal(reason[~mine], plain_reason[~mine])
