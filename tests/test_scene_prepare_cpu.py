"""The host half of the 4-wide trees (raytracer_amd/csrc/rt_scene_prepare.h) on the CPU: tests/cpp/scene_prepare_check.cpp restates the contract the kernels'
exactness rests on -- every stored 16-bit box contains the exact box with a grid step to spare, every leaf's exact box is the reference's -- and checks it on
synthetic trees, on live scenes built here, on the update cases (an update's rebuild == the assembly of the moved scene built afresh) and on the committed
tables of tests/golden/prepare_inputs.bin, whose prepared arrays must hash to what the PARENT commit's builders made of them
(tests/golden/prepared_scenes.json).  No GPU, no HIP: the checker includes two headers and include/rtgpu.h."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import raytracer_amd as ra
from raytracer_amd import scenes

import scene_zoo
import update_scenes as us

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "scene_prepare_check.cpp")
HEADERS = [os.path.join(ROOT, "raytracer_amd", "csrc", h) for h in ("rt_scene_prepare.h", "rt_wide_format.h")] + [os.path.join(ROOT, "include", "rtgpu.h")]
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "scene_prepare_check")
GOLDEN = os.path.join(ROOT, "tests", "golden")
ASPECT = 96 / 64

# the tables the prepare step reads, in the file's order (scene_prepare_check.cpp, readScenes)
TABLES = ("topNodes", "objects", "lights", "materials", "meshes", "meshNodes", "vertexIndices", "vertexShading", "textures")
SIZED = (ra.RtObject, ra.RtLight, ra.RtMaterial, ra.RtMesh, ra.RtTexture)


def scene_block(name, arrays, previous_index=()):
    """One scene of a checker input file from update_scenes.desc_arrays(scene)."""
    counts = [len(arrays[t]) for t in TABLES] + [len(previous_index)]   # (vertexIndices: one per triangle; vertexShading: one per vertex)
    out = [name.encode().ljust(32, b"\0")[:32], struct.pack("<10I", *counts), struct.pack("<5I", *[C.sizeof(t) for t in SIZED])]
    out += [np.ascontiguousarray(arrays[t], dtype=np.uint32).tobytes() for t in TABLES]
    out.append(np.asarray(previous_index, dtype=np.uint32).tobytes())
    return b"".join(out)


def write_scenes(path, blocks):
    with open(path, "wb") as f:
        f.write(b"RTPREP1\0" + struct.pack("<I", len(blocks)) + b"".join(blocks))


@pytest.fixture(scope="module")
def checker(built):
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    if not os.path.exists(EXE) or any(os.path.getmtime(s) > os.path.getmtime(EXE) for s in [SRC] + HEADERS):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", SRC, "-o", EXE])   # plain g++: nothing of ROCm on the include path

    def run(*args):
        r = subprocess.run([EXE] + list(args), capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout
    return run


def test_synthetic_trees_keep_the_contract_and_malformed_ones_are_refused(checker):
    assert "synthetic trees: ok" in checker("synthetic")


LIVE = {"cornell": lambda: scenes.cornell_box(ASPECT)[0],
        "mesh_1500": lambda: scene_zoo.mesh_scene(ASPECT, triangles=1500)[0],
        "all_lights": lambda: scene_zoo.all_lights_scene(ASPECT)[0],
        "single_mesh_1500": lambda: us.single_mesh_scene(ASPECT, 1500)[0]}


def test_live_scenes_keep_the_contract(checker, tmp_path):
    path = str(tmp_path / "live.bin")
    write_scenes(path, [scene_block(name, us.desc_arrays(make())) for name, make in LIVE.items()])
    out = checker("scenes", path)
    lines = {tuple(line.split()[:2]): line.split()[2:] for line in out.splitlines()}   # (scene, array) -> [hash, bytes]
    # the walk each scene was chosen for: two-level trees for the first three, the single-mesh tree for the last
    for name in ("cornell", "mesh_1500", "all_lights"):
        assert int(lines[(name, "wide2.nodes")][1]) > 0 and int(lines[(name, "wide.nodes")][1]) == 0, name
    assert int(lines[("single_mesh_1500", "wide.nodes")][1]) > 0 and int(lines[("single_mesh_1500", "wide2.nodes")][1]) == 0


@pytest.mark.parametrize("name", ["cornell", "mesh", "all_lights"])
def test_an_update_rebuilds_what_a_fresh_upload_would_assemble(checker, tmp_path, name):
    builder, _ = us.CASES[name]
    before, _ = builder(ASPECT)
    scene, _ = us.updated(name, ASPECT)
    fresh, _ = us.fresh(name, ASPECT)
    u = scene.update_desc()
    previous = [u.previousIndex[i] for i in range(u.numObjects)]
    path = str(tmp_path / (name + ".bin"))
    write_scenes(path, [scene_block("before", us.desc_arrays(before)), scene_block(name, us.desc_arrays(scene), previous), scene_block("fresh", us.desc_arrays(fresh))])
    assert "update == fresh" in checker("update", path)


def test_committed_inputs_prepare_to_the_parent_commit_s_bytes(checker):
    """Behaviour is pinned to the builders as they were BEFORE they moved into rt_scene_prepare.h: the hashes were made by the parent commit's code (the three
    device files compiled stand-alone) from the same committed tables, so they do not depend on the NumPy that generates live scenes."""
    golden = json.load(open(os.path.join(GOLDEN, "prepared_scenes.json")))
    out = checker("scenes", os.path.join(GOLDEN, "prepare_inputs.bin"))
    got = {}
    for line in out.splitlines():
        words = line.split()
        if len(words) == 4:
            got.setdefault(words[0], {})[words[1]] = {"fnv1a64": words[2], "bytes": int(words[3])}
    assert set(got) == set(golden["scenes"]) and len(got) >= 3
    for scene, arrays in golden["scenes"].items():
        assert got[scene] == arrays, scene
    # the inputs cover both walks
    assert any(a["wide2.nodes"]["bytes"] for a in got.values()) and any(a["wide.nodes"]["bytes"] for a in got.values())
