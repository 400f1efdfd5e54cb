"""What the CPU and GPU tests of temporal accumulation over deforming meshes share (tests/test_temporal_deform_model.py, tests/test_gpu_temporal_deform.py): the
frame size, a deformation gentle enough to stay on screen and inside the surface tests, the first-hit planes of a frame from the CPU oracle, and the inputs of the
model for a frame of the context call -- the table of include/rtgpu.h's "Temporal accumulation that follows deforming meshes" and the old triangle records."""
import ctypes as C

import numpy as np

import mesh_refit_scenes as ms
import oracle_lib
import raytracer_amd as ra
import temporal_deform_ref as dref
import update_scenes as us

W, H = 96, 64
SEED = 2468
INVALID_OBJECT = 0xFFFFFFFF


def swayed(pos, step):
    """the mesh under a slow sway: every vertex moves by a few hundredths of the mesh's size -- a pixel or so on screen --, and normals turn by a few degrees"""
    p = pos.astype(np.float64)
    out = p + np.stack([0.06 * np.sin(2.5 * p[:, 1] + 0.7 * step), 0.05 * np.cos(2.0 * p[:, 0] + step), 0.04 * np.sin(3.0 * p[:, 0] + 2.0 * p[:, 1] + step)], axis=1) * step
    return out.astype(np.float32)


def deform(scene, vp, pos, idx, step, update=True):
    """set_mesh_vertices(swayed) with new normals; update() and -- with a viewport -- update_scene()"""
    new = swayed(pos, step)
    normals = ms.vertex_normals(new, idx)
    scene.set_mesh_vertices(ms.MESH_OBJECT, new, normals, ms.vertex_tangents(normals))
    if update:
        scene.update()
        if vp is not None:
            vp.update_scene()
    return new


def guide_params(camera, depth=0):
    """the constants of the third pass of two frames that each begin with a reset() (a viewport without a renderer: the sequence depends on the seed alone)"""
    vp = ra.Viewport(W, H, seed=SEED, max_ray_depth=depth)
    out = []
    for _ in range(2):
        vp.reset()
        out.append([vp.next_pass_params(camera) for _ in range(3)][2])
    return out


def oracle_planes(scene, params):
    """object_id, sub_object_id (H, W) uint32, depth (H, W), barycentrics (2, H, W), position, normal (3, H, W) of the primary rays' first hits, from the CPU
    oracle's path records (words 6 .. 16 of a vertex, as tests/aov_ref.py reads them); params of ray depth 0"""
    assert params.maxRayDepth == 0
    rows = np.zeros((H * W, 28), dtype=np.float32)
    for y in range(H):
        for x in range(W):
            rows[y * W + x] = oracle_lib.render_pixel_paths(scene.desc, params, W, H, x, y, capacity=2)[0]
    ids = rows[:, 6].view(np.uint32).reshape(H, W).copy()
    depth = np.where(ids == INVALID_OBJECT, np.float32(np.inf), rows[:, 8].reshape(H, W)).astype(np.float32)
    return dict(object_id=ids, sub_object_id=rows[:, 7].view(np.uint32).reshape(H, W).copy(), depth=depth, barycentrics=rows[:, 9:11].T.reshape(2, H, W).copy(),
                position=rows[:, 11:14].T.reshape(3, H, W).copy(), normal=rows[:, 14:17].T.reshape(3, H, W).copy())


def mesh_objects(scene):
    """the flat objects that are the deforming mesh"""
    o, mi = scene.desc.contents, ms.mesh_index(scene)
    return [i for i in range(o.numObjects) if o.objects[i].objectKind == 0 and o.objects[i].shapeKind == 3 and o.objects[i].meshIndex == mi]


def object_tables(scene):
    """dict(transform, inverse (n, 4, 4) float32) of the flat objects as they stand"""
    words = us.desc_arrays(scene)["objects"]
    return dict(transform=words[:, :16].copy().view(np.float32).reshape(-1, 4, 4), inverse=words[:, 16:32].copy().view(np.float32).reshape(-1, 4, 4))


def scene_triangles(scene, ctx=None):
    """the (numTriangles, 9) float32 records of the whole scene with the deforming mesh's range as it stands -- on the device (ra.read_mesh) with a context, in the
    flat descriptor without: the layout of the context's snapshot"""
    a = us.desc_arrays(scene)
    out = a["triangles"].copy().view(np.float32)
    if ctx is not None:
        mi = ms.mesh_index(scene)
        first, count = int(a["meshes"][mi][2]), int(a["meshes"][mi][3])
        out[first:first + count] = ra.read_mesh(ctx, mi, int(a["meshes"][mi][1]), count)[1]
    return out


def previous_index(scene):
    u = scene.update_desc()
    return np.array([u.previousIndex[i] for i in range(scene.desc.contents.numObjects)], dtype=np.int64)


def context_inputs(scene, then, triangles, planes, prev_index=None, tracked=True):
    """(object_motion, deform) of the model for the frame the context call accumulates: `then` = object_tables when the history was stored, `triangles` =
    scene_triangles of that time, `planes` this frame's; prev_index[i]: which object of then current object i was (default: the last update()'s previousIndex).
    tracked=False: the table without tracking -- the mesh's objects get prevId 0xFFFFFFFF"""
    now = object_tables(scene)
    prev_index = previous_index(scene) if prev_index is None else np.asarray(prev_index, dtype=np.int64)
    n = len(prev_index)
    meshes = us.desc_arrays(scene)["meshes"]
    mi = ms.mesh_index(scene)
    on_mesh = np.isin(np.arange(n), mesh_objects(scene))
    ids = prev_index.astype(np.uint32)
    if not tracked:
        ids[on_mesh] = INVALID_OBJECT
    table, first, count = dref.context_table(now["transform"], now["inverse"], then["transform"][prev_index], ids, on_mesh & tracked, np.full(n, meshes[mi][2]), np.full(n, meshes[mi][3]))
    return table, dict(sub_object_id=planes["sub_object_id"].reshape(H, W), barycentrics=planes["barycentrics"], prev_triangles=triangles, first_triangle=first, num_triangles=count)
