"""Scenes with moved objects, shared by the CPU and GPU tests of Scene.update() / rtgpu_update_objects.

A case is a scene builder and a list of moves (index among the add_* calls, new transform).  `updated(case)` builds the scene, applies the
moves with set_object_transform and update(); `fresh(case)` replays what the first scene recorded in `.calls` into a NEW Scene, the moved
transforms in place of the old ones, and builds it: the scene a caller without update() would have to build and upload whole."""
import ctypes as C

import numpy as np

import raytracer_amd as ra
from raytracer_amd import scenes

import scene_zoo

OBJECT_CALLS = ra.Scene._OBJECT_CALLS


def _m16(values):
    return (C.c_float * 16)(*[float(v) for v in values])


def replay(calls, moves=()):
    """A new, unbuilt Scene from the `.calls` of another one; moves: {object index: transform}."""
    moves = dict(moves)
    s = ra.Scene()
    index = 0
    for kind, a in calls:
        t = None
        if kind in OBJECT_CALLS:
            if "transform" in a:
                t = _m16(moves.get(index, a["transform"]))
            index += 1
        if kind == "material":
            s.add_material(a["bsdf"], a["base_color"], a["emission"], a["roughness"], a["metalness"], a["ior"], a["k"])
        elif kind == "sphere":
            s.add_sphere(a["radius"], t, a["material"])
        elif kind == "box":
            s.add_box(a["size"], t, a["material"])
        elif kind == "rect":
            s.add_rect(a["size"], t, a["material"], a["tex_scale"])
        elif kind == "mesh":
            s.add_mesh(a["positions"], a["indices"], a["normals"], a["tangents"], a["tex_coords"], a["material_indices"], a["materials"], t, a["material"])
        elif kind == "area_light":
            s.add_area_light(["sphere", "box", "rect"][a["shape"]], list(a["params"]), a["color"], t)
        elif kind == "background_light":
            s.add_background_light(a["color"], a["texture"])
        elif kind == "directional_light":
            s.add_directional_light(a["color"], np.float32(a["angle"]), t)
        elif kind == "point_light":
            s.add_point_light(a["color"], t)
        elif kind == "spot_light":
            s.add_spot_light(a["color"], np.float32(a["angle"]), t)
        else:
            raise NotImplementedError(kind)
    return s


def _small_mesh_scene(aspect, triangles):
    return scene_zoo.mesh_scene(aspect, triangles=triangles)


def single_mesh_scene(aspect, triangles=1500):
    """ONE mesh object under global lights: Scene::Traverse's one-object bypass, the 4-wide walk of a single mesh."""
    pos, idx, nrm, tan, uv, mat = scenes.sponza_class_mesh(triangles, seed=5)
    s = ra.Scene()
    mats = [s.add_material("diffuse", c) for _, c in scenes.SPONZA_MATERIALS]
    s.add_mesh(pos, idx, nrm, tan, uv, mat, mats)
    s.add_background_light((1.0, 1.5, 2.0))
    s.add_directional_light((8.0, 7.5, 7.0), np.float32(0.02), ra.transform_from_euler((0.0, 0.0, 0.0), (80.0, 20.0, 0.0)))
    s.build()
    return s, ra.Camera((-12.5, 2.2, 0.6), (4.0, 82.0, 0.0), aspect, 65.0)


E = ra.transform_from_euler

# name -> (builder(aspect), moves).  Indices count add_* calls of objects, lights included (Scene.set_object_transform).
CASES = {
    # ten analytic instances: the glass sphere goes to the other side of the room and up, the tall box turns and crosses over
    "cornell": (scenes.cornell_box, [(7, E((2.6, 2.4, -2.0))), (5, E((1.0, -3.5, -2.5), (0.0, 40.0, 0.0)))]),
    # mesh + sphere + box + rect light: the sphere leaves the building's far end for the other one, the box follows half way
    "mesh": (lambda aspect: _small_mesh_scene(aspect, 20000), [(1, E((9.0, 3.0, -2.0))), (2, E((-6.0, 1.5, 1.0), (0.0, 75.0, 0.0)))]),
    # every light type: the rect area light (object 11) swings aside and tilts, the box light (13) crosses the scene
    "all_lights": (scene_zoo.all_lights_scene, [(11, E((2.5, 3.0, -2.0), (70.0, 20.0, 0.0))), (13, E((3.0, 0.5, 3.5), (0.0, 60.0, 10.0)))]),
    # sphere + area light: the binary kernel's scene, the light moved
    "sphere_light": (scenes.sphere_area_light, [(1, E((1.5, 3.0, 1.0), (75.0, 0.0, 20.0)))]),
    # a single mesh: its transform only (the 4-wide tree of the single-mesh walk is in the mesh's local space)
    "single_mesh": (single_mesh_scene, [(0, E((0.5, -0.3, 0.4), (0.0, 12.0, 0.0)))]),
}


def updated(name, aspect, moves=None):
    """(scene, camera) after set_object_transform + update(); also returns the scene's RtSceneUpdate."""
    builder, case_moves = CASES[name]
    scene, camera = builder(aspect)
    for index, transform in (case_moves if moves is None else moves):
        scene.set_object_transform(index, transform)
    scene.update()
    return scene, camera


def fresh(name, aspect, moves=None):
    builder, case_moves = CASES[name]
    scene, camera = builder(aspect)
    new = replay(scene.calls, {i: list(t) for i, t in (case_moves if moves is None else moves)})
    new.build()
    return new, camera


def desc_arrays(scene):
    """The flat tables of a built scene as numpy copies (words): what the CPU tests compare."""
    d = scene.desc.contents

    def words(ptr, count, size):
        if not count:
            return np.zeros((0, size // 4), dtype=np.uint32)
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint32)), shape=(count, size // 4)).copy()

    return {"topNodes": words(d.topNodes, d.numTopNodes, 32), "objects": words(d.objects, d.numObjects, C.sizeof(ra.RtObject)),
            "lights": words(d.lights, d.numLights, C.sizeof(ra.RtLight)), "materials": words(d.materials, d.numMaterials, C.sizeof(ra.RtMaterial)),
            "meshes": words(d.meshes, d.numMeshes, C.sizeof(ra.RtMesh)), "meshNodes": words(d.meshNodes, d.numMeshNodes, 32),
            "triangles": words(d.triangles, d.numTriangles, 36), "vertexIndices": words(d.vertexIndices, d.numTriangles, 16),
            "vertexShading": words(d.vertexShading, d.numVertices, 32), "textures": words(d.textures, d.numTextures, C.sizeof(ra.RtTexture)),
            "globalLights": words(d.globalLights, d.numGlobalLights, 4)}


def top_depth(nodes):
    """Depth of the flat top-level tree in stack entries (rows of 8 words: min, childIndex, max, leaves)."""
    if len(nodes) == 0:
        return 0
    best, stack = 0, [(0, 0)]
    while stack:
        i, d = stack.pop()
        if nodes[i][7] & 0x3FFFFFFF:
            best = max(best, d)
        else:
            c = int(nodes[i][3])
            stack += [(c, d + 1), (c + 1, d + 1)]
    return best
