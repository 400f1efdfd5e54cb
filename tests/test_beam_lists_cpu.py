"""The host builder of the beam lists (raytracer_amd/csrc/rt_beam_lists.h) on the CPU: tests/cpp/beam_lists_check.cpp builds the lists of a frame's tiles
from a scene's one mesh and holds them to brute force -- for every pixel and the sample offsets at the corners and the centre of [-m, m]^2, every leaf whose
exact box the reference's camera ray passes (the oracle's slab test and ray arithmetic) is in its tile's list and is entered no earlier than its dmin; lists
ascend in dmin; a capacity of 2 leaves most tiles without a list.  No GPU, no HIP."""
import os
import subprocess

import pytest

import raytracer_amd as ra

import beam_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "beam_lists_check.cpp")
HEADERS = [os.path.join(ROOT, "raytracer_amd", "csrc", h) for h in ("rt_beam_lists.h", "rt_scene_prepare.h", "rt_wide_format.h")] + \
          [os.path.join(ROOT, "include", "rtgpu.h"), os.path.join(ROOT, "oracle", "rto_math.h")]
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "beam_lists_check")
SPREAD = 0.5
MARGIN = 3.0 * SPREAD

SCENES = {"box_room": beam_scenes.box_room,
          "mesh_2000": lambda aspect: beam_scenes.mesh_scene(aspect, 2000),
          "mesh_2000_rigid": lambda aspect: beam_scenes.mesh_scene(aspect, 2000, beam_scenes.RIGID)}
# the eye half a thousandth of a unit from a wall (a leaf box of no thickness), looking four ways, one of them at it: dmin's absolute margin (rt_beam_lists.h) --
# the entry parameter is then of the order of the coordinates' rounding, which a margin relative to the distance alone would not cover
for _yaw in (0.0, 90.0, 180.0, 270.0):
    SCENES["box_room_nose_to_the_wall_%d" % _yaw] = lambda aspect, yaw=_yaw: beam_scenes.box_room(aspect, eye=(2.9995, -0.5, 0.3), look=(3.0, yaw, 0.0))


@pytest.fixture(scope="module")
def checker(built):
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    if not os.path.exists(EXE) or any(os.path.getmtime(s) > os.path.getmtime(EXE) for s in [SRC] + HEADERS):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", SRC, "-o", EXE])   # plain g++: nothing of ROCm on the include path

    def run(scene_name, width, height, capacity, tmp_path, margin=MARGIN):
        scene, camera = SCENES[scene_name](width / height)
        params = ra.Viewport(width, height, seed=11, anti_aliasing_spread=SPREAD).next_pass_params(camera)
        path = str(tmp_path / ("%s_%dx%d_%d.bin" % (scene_name, width, height, capacity)))
        with open(path, "wb") as f:
            f.write(beam_scenes.checker_input(scene, params.camera, width, height, margin, capacity))
        r = subprocess.run([EXE, path], capture_output=True, text=True)
        return r.returncode, r.stdout + r.stderr
    return run


def fields(out):
    words = out.split()
    assert words[0] == "ok", out
    return {words[i]: float(words[i + 1]) for i in range(1, len(words) - 1, 2)}


@pytest.mark.parametrize("size", [(64, 48), (60, 44)])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_leaf_a_ray_passes_is_in_its_tile_s_list_behind_its_dmin(checker, tmp_path, name, size):
    code, out = checker(name, size[0], size[1], 64, tmp_path)
    assert code == 0, out[-3000:]
    f = fields(out)
    assert f["tiles"] == -(-size[0] * size[1] // 64) and f["pairs"] > size[0] * size[1]   # every pixel's rays pass some leaf: the check had something to check
    if name == "box_room":
        assert f["noList"] == 0 and f["longest"] <= 12


@pytest.mark.parametrize("name", ["box_room", "mesh_2000"])
def test_a_list_that_outgrows_its_capacity_is_no_list(checker, tmp_path, name):
    code, out = checker(name, 64, 48, 2, tmp_path)
    assert code == 0, out[-3000:]
    f = fields(out)
    # (a wall of the room is one leaf of two triangles: the tiles that see one or two walls keep their lists; of the building's tiles hardly any does)
    assert f["noList"] > (0 if name == "box_room" else 0.5 * f["tiles"]) and f["longest"] <= 2


def test_a_scaled_object_gets_no_lists(checker, tmp_path):
    scene, camera = beam_scenes.mesh_scene(64 / 48, 2000)
    params = ra.Viewport(64, 48, seed=11).next_pass_params(camera)
    blob = bytearray(beam_scenes.checker_input(scene, params.camera, 64, 48, MARGIN, 64))
    import struct
    at = 24 + len(bytes(params.camera))   # invTransform: scale its first row
    row = struct.unpack_from("<3f", blob, at)
    struct.pack_into("<3f", blob, at, *[2.0 * v for v in row])
    path = str(tmp_path / "scaled.bin")
    with open(path, "wb") as f:
        f.write(bytes(blob))
    r = subprocess.run([EXE, path], capture_output=True, text=True)
    assert r.returncode == 3 and "no lists" in r.stdout
