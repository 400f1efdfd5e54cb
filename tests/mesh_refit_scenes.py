"""Meshes and scenes shared by the CPU and GPU tests of deforming meshes (Scene.set_mesh_vertices / rtgpu_update_mesh).

The meshes are the smallest at which a refit can go wrong in its own way: one triangle (the root is a leaf), two (a leaf of two), three (the smallest tree
with the unused node 1), a 17 x 17 vertex grid of 512 triangles, and a 4 096-triangle random soup -- deep and unbalanced, the smallest shape here whose
tree has depths wider than one block of the single-block refit kernel (1 024 nodes), so it takes the per-depth launches and the single-block path both.
Every coordinate is jittered away from zero: the sign of a zero is the only place the fold order of the Box operations could show."""
import numpy as np

import raytracer_amd as ra

MESHES = ("tri1", "tri2", "tri3", "grid17", "soup4096")


def _jitter(p, seed):
    """no coordinate exactly zero (nor one of the round values a generator likes)"""
    rng = np.random.RandomState(seed)
    p = (np.asarray(p, dtype=np.float64) + rng.uniform(0.001, 0.003, np.shape(p)) * rng.choice([-1.0, 1.0], np.shape(p))).astype(np.float32)
    assert not (p == 0).any()
    return p


def mesh(name):
    """(positions (V, 3) float32, indices (T, 3) uint32, normals (V, 3) float32) in mesh-local space, about two units across"""
    if name in ("tri1", "tri2", "tri3"):
        p = [[-1.0, -0.8, 0.1], [1.0, -0.9, -0.1], [0.1, 1.0, 0.2], [1.2, 0.9, 0.3], [-1.1, 0.8, -0.4]]
        idx = [[0, 1, 2], [1, 3, 2], [0, 2, 4]][:int(name[3])]
        pos = _jitter(p[:2 + len(idx)], 11)
    elif name == "grid17":
        g = np.linspace(-1.0, 1.0, 17)
        x, y = np.meshgrid(g, g, indexing="xy")
        pos = _jitter(np.stack([x, y, 0.15 * np.sin(3.0 * x) * np.cos(2.0 * y)], axis=-1).reshape(-1, 3), 12)
        quad = np.array([[r * 17 + c for c in range(16)] for r in range(16)]).reshape(-1)
        idx = np.concatenate([np.stack([quad, quad + 1, quad + 18], axis=1), np.stack([quad, quad + 18, quad + 17], axis=1)])
    elif name == "soup4096":
        rng = np.random.RandomState(13)
        # clustered: a few dense clumps and a thin far tail, so the SAH tree is deep and unbalanced
        centres = np.concatenate([rng.uniform(-1.0, 1.0, (3000, 3)) * [1.0, 0.2, 1.0], rng.uniform(-0.05, 0.05, (1000, 3)) + [0.5, 0.5, 0.5],
                                  np.cumsum(rng.uniform(0.0, 0.004, (96, 3)), axis=0) + [-1.0, 0.6, -1.0]])
        pos = _jitter((centres[:, None, :] + rng.uniform(-0.03, 0.03, (4096, 3, 3))).reshape(-1, 3), 14)
        idx = np.arange(3 * 4096).reshape(-1, 3)
    else:
        raise KeyError(name)
    idx = np.asarray(idx, dtype=np.uint32)
    return pos, idx, vertex_normals(pos, idx)


def vertex_normals(pos, idx):
    a, b, c = pos[idx[:, 0]].astype(np.float64), pos[idx[:, 1]].astype(np.float64), pos[idx[:, 2]].astype(np.float64)
    face = np.cross(b - a, c - a)
    n = np.zeros(pos.shape, dtype=np.float64)
    for k in range(3):
        np.add.at(n, idx[:, k], face)
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(length > 0, n / np.maximum(length, 1e-30), [0.0, 0.0, 1.0]).astype(np.float32)


def vertex_tangents(normals):
    """unit tangents orthogonal to the normals (a mesh without tangents shades with NaN tangent frames, whose payload bits are nobody's contract)"""
    n = normals.astype(np.float64)
    axis = np.where(np.abs(n[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    t = axis - n * np.sum(axis * n, axis=1, keepdims=True)
    return (t / np.linalg.norm(t, axis=1, keepdims=True)).astype(np.float32)


def deformed(pos, step):
    """the mesh under a travelling sine: every vertex moves, the bounds change"""
    p = pos.astype(np.float64)
    out = p + np.stack([0.05 * np.sin(4.0 * p[:, 1] + 0.9 * step), 0.12 * np.sin(3.0 * p[:, 0] + 2.0 * p[:, 2] + 1.3 * step), 0.04 * np.cos(5.0 * p[:, 0] - step)], axis=1)
    return _jitter(out * (1.0 + 0.03 * step), 20 + step)


E = ra.transform_from_euler
MESH_OBJECT = 0     # the add_* index of the deforming mesh in both scenes


def prop_mesh():
    """a second, different mesh (a five-triangle fan) that stands still: with it in the scene the deforming mesh's node, triangle, 4-wide node and gate ranges
    do not all start at 0"""
    pos = _jitter([[0.0, 0.5, 0.0], [0.5, -0.4, 0.3], [0.2, -0.4, -0.5], [-0.5, -0.4, -0.2], [-0.3, -0.4, 0.5], [0.35, -0.45, 0.45], [0.6, 0.1, 0.1]], 15)
    idx = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 5], [1, 6, 2]], dtype=np.uint32)
    return pos, idx, vertex_normals(pos, idx)


def mesh_index(scene):
    """the flat index of the deforming mesh: the one two objects share; a single-mesh scene's only one"""
    d = scene.desc.contents
    used = [d.objects[i].meshIndex for i in range(d.numObjects) if d.objects[i].objectKind == 0 and d.objects[i].shapeKind == 3]
    return 0 if d.numMeshes == 1 else next(m for m in used if used.count(m) == 2)


def two_level_scene(name, aspect):
    """the mesh twice (an instance: one tree, two objects) and a second mesh among a sphere, a box and a rect light: the two-level 4-wide walk"""
    pos, idx, nrm = mesh(name)
    s = ra.Scene()
    grey, red, glass = s.add_material("diffuse", (0.7, 0.7, 0.65)), s.add_material("diffuse", (0.8, 0.25, 0.2)), s.add_material("roughMetal", (0.9, 0.8, 0.5), roughness=0.3)
    s.add_mesh(pos, idx, nrm, vertex_tangents(nrm), pos[:, :2] * 0.5 + 0.5, transform=E((-0.9, 0.0, 0.0), (0.0, 20.0, 0.0)), default_material=grey)
    s.add_instance(MESH_OBJECT, E((1.2, 0.2, -0.4), (10.0, -35.0, 5.0)), red)
    s.add_sphere(0.45, E((0.1, -0.7, 0.9)), glass)
    ppos, pidx, pnrm = prop_mesh()
    s.add_mesh(ppos, pidx, pnrm, vertex_tangents(pnrm), ppos[:, :2] + 0.5, transform=E((-2.4, -0.6, 0.8), (0.0, 30.0, 0.0)), default_material=red)
    s.add_box((3.0, 0.05, 3.0), E((0.0, -1.3, 0.0)), grey)
    s.add_area_light("rect", (0.8, 0.8), (14.0, 13.0, 12.0), E((0.0, 2.6, 0.5), (90.0, 0.0, 0.0)))
    s.add_background_light((0.3, 0.4, 0.6))
    s.build()
    return s, ra.Camera((0.0, 0.4, 5.2), (2.0, 180.0, 0.0), aspect, 42.0), pos, idx, nrm


def single_mesh_scene(name, aspect):
    """ONE mesh object under global lights: Scene::Traverse's one-object bypass (the 4-wide walk of a single mesh, or the binary walk where the root is a leaf)"""
    pos, idx, nrm = mesh(name)
    s = ra.Scene()
    s.add_mesh(pos, idx, nrm, vertex_tangents(nrm), pos[:, :2] * 0.5 + 0.5, default_material=s.add_material("diffuse", (0.7, 0.6, 0.5)))
    s.add_background_light((1.0, 1.5, 2.0))
    s.add_directional_light((8.0, 7.5, 7.0), np.float32(0.02), E((0.0, 0.0, 0.0), (80.0, 20.0, 0.0)))
    s.build()
    return s, ra.Camera((0.3, 0.5, 4.0), (5.0, 184.0, 0.0), aspect, 40.0), pos, idx, nrm


SCENES = {"two_level": two_level_scene, "single": single_mesh_scene}


def mesh_tables(scene):
    """(nodes (N, 8) words, vertex indices (T, 4) words, triangles (T, 9) float32) of the deforming mesh in the scene's flat descriptor, as copies"""
    import update_scenes as us
    a = us.desc_arrays(scene)
    m = a["meshes"][mesh_index(scene)]     # firstNode, numNodes, firstTriangle, numTriangles, firstVertex, numVertices
    return (a["meshNodes"][m[0]:m[0] + m[1]].copy(), a["vertexIndices"][m[2]:m[2] + m[3]].copy(),
            a["triangles"][m[2]:m[2] + m[3]].copy().view(np.float32))
