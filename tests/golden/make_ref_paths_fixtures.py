"""Writes tests/golden/ref_paths/<name>.bin: every vertex of every path of ONE pass of the reference's own PathTracerMIS::RenderPixel, as its
own path-debugging hook records them (PathDebugData, Core/Rendering/PathDebugging.h:27-53, filled at PathTracerMIS.cpp:377-410 -- the
hook the reference's Demo uses for its path inspector).  oracle/_ref/ref_paths is oracle/ref_harness/ref_render.cpp over a build of the
reference's translation units WITHOUT RT_CONFIGURATION_FINAL (the hook and RenderingContext::pathDebugData exist only there), one
thread.  Build container only.  Regenerate: python tests/golden/make_ref_paths_fixtures.py

File: uint32 magic 'RPV1', width, height, maxRayDepth, samplingAll, dimensions, numVertices, 0; float32 vertices[numVertices][28]:
ray origin xyz, ray direction xyz, hit objectId, subObjectId (bit-cast), distance, u, v, frame position xyz, normal xyz, tangent xyz,
texCoord xy, throughput xyzw, bsdfEvent (bit-cast; unset in a path's last record), 0.  Paths follow each other in the order the pixels
were rendered; a path starts where the ray origin is the camera position.

The fields the reference leaves unset hold whatever its stack held, which changes from run to run; they are written as zeros
(clear_unset_fields), so that a regeneration reproduces the committed files byte for byte.  tests/test_reference_paths.py ignores them."""
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("RT_FIXTURE_OUT", HERE)   # tests/test_golden_regeneration.py regenerates into a scratch directory and compares
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_render   # noqa: E402
import ref_scenes   # noqa: E402

EXE = ref_render.EXE.replace("ref_render", "ref_paths")
SIZE = (40, 30)
SCENES = ("box_mesh", "cornell", "mesh_2k_all", "mesh_single")


def run_paths(scene_path, w, h):
    tree = tempfile.mkdtemp(prefix="rtref_cwd_")
    os.symlink(os.path.join(ref_render.DATA_PARENT, "data"), os.path.join(tree, "Data"))
    cwd = os.path.join(tree, "run")
    os.mkdir(cwd)
    out = scene_path + ".out"
    try:
        r = subprocess.run([EXE, scene_path, out, "1", "1"], cwd=cwd, capture_output=True, text=True)
    finally:
        shutil.rmtree(tree, ignore_errors=True)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(out, dtype=np.uint8)
    os.remove(out)
    head = raw[:32].view(np.uint32)
    off = 32 + 32 + 8 + 8 + 4 * int(head[4]) + 12 * w * h
    n = int(raw[off:off + 4].view(np.uint32)[0])
    return raw[off + 4:off + 4 + n * 112].view(np.float32).reshape(n, 28).copy()


def clear_unset_fields(v, desc):
    """Zeroes, in place, what the reference does not write (the same fields tests/test_reference_paths.py leaves out of its comparison):
    bsdfEvent of a path's last record; sub-object, (u, v) and the shading data of a record whose ray hit nothing; (u, v) of any hit but a
    triangle's."""
    bits = v.view(np.uint32)
    starts = (bits[:, :3] == bits[0, :3]).all(axis=1)        # a path starts where the ray leaves the camera
    bits[np.append(starts[1:], True), 26] = 0
    miss = bits[:, 6] == 0xFFFFFFFF
    bits[miss, 7] = 0
    bits[miss, 9:22] = 0
    mesh = np.array([(not m) and desc.objects[int(o)].objectKind == 0 and desc.objects[int(o)].shapeKind == 3 for m, o in zip(miss, bits[:, 6])], dtype=bool)
    bits[~mesh, 9:11] = 0
    return v


if __name__ == "__main__":
    w, h = SIZE
    os.makedirs(os.path.join(OUT, "ref_paths"), exist_ok=True)
    scratch = tempfile.mkdtemp(prefix="ref_paths_")   # private to this run: two runs at once must not read each other's scene or output files
    for name in SCENES:
        make, _, _, _, depth, sampling_all, dims = ref_scenes.FIXTURES[name]
        scene, camera = make(w / h)
        path = os.path.join(scratch, name + ".bin")
        ref_render.export_scene(path, scene, camera, w, h, 1, 1, depth, dimensions=dims, light_sampling_all=sampling_all, seed=ref_scenes.SEED)
        v = clear_unset_fields(run_paths(path, w, h), scene.desc.contents)
        os.remove(path)
        with open(os.path.join(OUT, "ref_paths", name + ".bin"), "wb") as f:
            f.write(struct.pack("<8I", 0x31565052, w, h, depth, int(sampling_all), dims, len(v), 0))
            f.write(v.astype("<f4").tobytes())
        print(name, len(v), "vertices")
    shutil.rmtree(scratch, ignore_errors=True)
