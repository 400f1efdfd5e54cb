"""Single-mesh scenes for the beam-list tests (tests/test_beam_lists_cpu.py, tests/test_gpu_beam_lists.py): one mesh object under global lights, so that
k_trace_wide / k_trace_packet serve them, and what the CPU checker (tests/cpp/beam_lists_check.cpp) reads of such a scene."""
import ctypes as C
import struct

import numpy as np

import raytracer_amd as ra
from raytracer_amd import scenes

E = ra.transform_from_euler
RIGID = E((0.5, -0.3, 0.4), (0.0, 12.0, 5.0))   # a rotation plus a translation of the mesh object


def _lights(s):
    s.add_background_light((1.0, 1.5, 2.0))
    s.add_directional_light((8.0, 7.5, 7.0), np.float32(0.02), E((0.0, 0.0, 0.0), (80.0, 20.0, 0.0)))


def box_room(aspect, transform=None, eye=(0.4, -0.5, 0.3), look=(10.0, 35.0, 0.0)):
    """The 12-triangle box mesh seen from inside: a room whose six walls fill the frame."""
    pos, idx, nrm, tan, uv, mat = scenes.box_mesh(3.0)
    s = ra.Scene()
    mats = [s.add_material("diffuse", (0.8, 0.3, 0.2)), s.add_material("diffuse", (0.7, 0.7, 0.7))]
    if transform is None:
        s.add_mesh(pos, idx, nrm, tan, uv, mat, mats)
    else:
        s.add_mesh(pos, idx, nrm, tan, uv, mat, mats, transform=transform)
    _lights(s)
    s.build()
    return s, ra.Camera(eye, look, aspect, 70.0)


def mesh_scene(aspect, triangles=2000, transform=None):
    """The Sponza-class building at about `triangles` triangles, the benchmark's camera."""
    pos, idx, nrm, tan, uv, mat = scenes.sponza_class_mesh(triangles, seed=5)
    s = ra.Scene()
    mats = [s.add_material("diffuse", c) for _, c in scenes.SPONZA_MATERIALS]
    if transform is None:
        s.add_mesh(pos, idx, nrm, tan, uv, mat, mats)
    else:
        s.add_mesh(pos, idx, nrm, tan, uv, mat, mats, transform=transform)
    _lights(s)
    s.build()
    return s, ra.Camera((-12.5, 2.2, 0.6), (4.0, 82.0, 0.0), aspect, 65.0)


def checker_input(scene, camera_desc, width, height, margin, capacity):
    """tests/cpp/beam_lists_check.cpp's input for the scene's one mesh object seen through `camera_desc` (an RtCamera)."""
    d = scene.desc.contents
    assert d.numObjects == 1 and d.numMeshes == 1
    mesh = d.meshes[0]
    nodes = np.ctypeslib.as_array(C.cast(d.meshNodes, C.POINTER(C.c_uint32)), shape=(d.numMeshNodes, 8))[mesh.firstNode:mesh.firstNode + mesh.numNodes]
    inv = np.array(d.objects[0].invTransform[:], dtype=np.float32)
    return (struct.pack("<5If", width, height, mesh.numNodes, mesh.numTriangles, capacity, margin) + bytes(camera_desc) + inv.tobytes() +
            np.ascontiguousarray(nodes, dtype=np.uint32).tobytes())
