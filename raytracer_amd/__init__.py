"""raytracer_amd -- MI355X-native PathTracerMIS core behind the reference's Scene/Viewport API.

Python is plumbing only: ctypes bindings over
  * lib/librtgpu.so               the C-ABI of include/rtgpu.h (hand-written HIP wavefront path tracer)
  * lib/libraytracer_amd_host.so  the C++ mirror of the reference's host API (rt::Scene, rt::Viewport ...)
                                  through its flat ``rth_*`` facade (host/src/c_api.cpp)

There is NO CPU fallback: creating a renderer without the HIP library / a GPU raises.
"""
import collections
import ctypes as C
import os

import numpy as np

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
_LIB_DIR = os.path.join(_PKG_DIR, "lib")
DATA_DIR = os.path.join(_PKG_DIR, "data")
os.environ.setdefault("RT_DATA_DIR", DATA_DIR)

RTGPU_LIB_PATH = os.path.join(_LIB_DIR, "librtgpu.so")
HOST_LIB_PATH = os.path.join(_LIB_DIR, "libraytracer_amd_host.so")


class BuildError(RuntimeError):
    pass


def _load(path):
    if not os.path.exists(path):
        raise BuildError(
            "%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
            "raytracer_amd has no CPU fallback." % path)
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


_rtgpu = None
_host = None


def rtgpu_lib():
    """The device C-ABI library (include/rtgpu.h)."""
    global _rtgpu
    if _rtgpu is None:
        _rtgpu = _load(RTGPU_LIB_PATH)
        _rtgpu.rtgpu_last_error.restype = C.c_char_p
        _rtgpu.rtgpu_abi_version.restype = C.c_uint32
        # guide chains: (ctx, params, chain, planes, numPlanes, outputs[, stream])
        chain_args = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        _rtgpu.rtgpu_render_aovs_chain.argtypes, _rtgpu.rtgpu_render_aovs_chain.restype = chain_args, C.c_int
        _rtgpu.rtgpu_render_aovs_chain_async.argtypes, _rtgpu.rtgpu_render_aovs_chain_async.restype = chain_args + [C.c_void_p], C.c_int
        _rtgpu.rtgpu_set_guide_chain.argtypes, _rtgpu.rtgpu_set_guide_chain.restype = [C.c_void_p, C.c_void_p], C.c_int
        _rtgpu.rtgpu_render_aovs_virtual.argtypes, _rtgpu.rtgpu_render_aovs_virtual.restype = chain_args, C.c_int
        _rtgpu.rtgpu_render_aovs_virtual_async.argtypes, _rtgpu.rtgpu_render_aovs_virtual_async.restype = chain_args + [C.c_void_p], C.c_int
        # the ray source: (ctx, rays, count[, stream]), (ctx, outCount), (ctx, params, out[, stream])
        _rtgpu.rtgpu_set_ray_source.argtypes, _rtgpu.rtgpu_set_ray_source.restype = [C.c_void_p, C.c_void_p, C.c_uint64], C.c_int
        _rtgpu.rtgpu_set_ray_source_device.argtypes, _rtgpu.rtgpu_set_ray_source_device.restype = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p], C.c_int
        _rtgpu.rtgpu_get_ray_source.argtypes, _rtgpu.rtgpu_get_ray_source.restype = [C.c_void_p, C.POINTER(C.c_uint64)], C.c_int
        _rtgpu.rtgpu_read_camera_rays.argtypes, _rtgpu.rtgpu_read_camera_rays.restype = [C.c_void_p, C.c_void_p, C.c_void_p], C.c_int
        _rtgpu.rtgpu_read_camera_rays_async.argtypes, _rtgpu.rtgpu_read_camera_rays_async.restype = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int
        # the lens source: (ctx, rays, count, params[, stream]), (ctx, outKind), (ctx, params, out[, stream])
        _rtgpu.rtgpu_set_lens_source.argtypes, _rtgpu.rtgpu_set_lens_source.restype = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p], C.c_int
        _rtgpu.rtgpu_set_lens_source_device.argtypes, _rtgpu.rtgpu_set_lens_source_device.restype = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p], C.c_int
        _rtgpu.rtgpu_get_ray_source_kind.argtypes, _rtgpu.rtgpu_get_ray_source_kind.restype = [C.c_void_p, C.POINTER(C.c_uint32)], C.c_int
        for name in ("rtgpu_read_lens_source_rays", "rtgpu_read_camera_footprints"):
            getattr(_rtgpu, name).argtypes, getattr(_rtgpu, name).restype = [C.c_void_p, C.c_void_p, C.c_void_p], C.c_int
            getattr(_rtgpu, name + "_async").argtypes, getattr(_rtgpu, name + "_async").restype = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int
        # known-answer hooks of post-processing: (ctx, params[n], rgb[n * 3], n, outBGR[n], outToneMapped[n * 3] or NULL), (ctx, rgb in place, width, height, sigma)
        _rtgpu.rtgpu_kat_postprocess.argtypes, _rtgpu.rtgpu_kat_postprocess.restype = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p], C.c_int
        _rtgpu.rtgpu_kat_blur.argtypes, _rtgpu.rtgpu_kat_blur.restype = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float], C.c_int
        # beam lists: (ctx, pixels), (ctx, outInfo), (ctx, fromHost, counts, entries)
        _rtgpu.rtgpu_set_beam_margin.argtypes, _rtgpu.rtgpu_set_beam_margin.restype = [C.c_void_p, C.c_float], C.c_int
        _rtgpu.rtgpu_get_beam_list_info.argtypes, _rtgpu.rtgpu_get_beam_list_info.restype = [C.c_void_p, C.c_void_p], C.c_int
        _rtgpu.rtgpu_read_beam_lists.argtypes, _rtgpu.rtgpu_read_beam_lists.restype = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p], C.c_int
    return _rtgpu


def host_lib():
    """The C++ host mirror (rt::Scene / rt::Viewport ...) through its rth_* facade."""
    global _host
    if _host is None:
        rtgpu_lib()
        _host = _load(HOST_LIB_PATH)
        h = _host
        for name in ("rth_scene_create", "rth_camera_create", "rth_viewport_create", "rth_viewport_device_ctx"):
            getattr(h, name).restype = C.c_void_p
        h.rth_scene_desc.restype = C.POINTER(RtSceneDesc)
        h.rth_viewport_passes_finished.restype = C.c_uint32
    return _host


# --------------------------------------------------------------------------------------------------
# ctypes mirrors of the PODs in include/rtgpu.h
# --------------------------------------------------------------------------------------------------
class RtNode(C.Structure):
    _fields_ = [("min", C.c_float * 3), ("childIndex", C.c_uint32), ("max", C.c_float * 3), ("leaves", C.c_uint32)]


class RtMesh(C.Structure):
    _fields_ = [("firstNode", C.c_uint32), ("numNodes", C.c_uint32), ("firstTriangle", C.c_uint32), ("numTriangles", C.c_uint32),
                ("firstVertex", C.c_uint32), ("numVertices", C.c_uint32), ("_pad", C.c_uint32 * 2)]


class RtObject(C.Structure):
    _fields_ = [("transform", C.c_float * 16), ("invTransform", C.c_float * 16), ("objectKind", C.c_uint32), ("shapeKind", C.c_uint32),
                ("materialIndex", C.c_uint32), ("meshIndex", C.c_uint32), ("lightIndex", C.c_uint32), ("_pad", C.c_uint32 * 3),
                ("shapeParam", C.c_float * 4), ("shapeParam2", C.c_float * 4)]


class RtLight(C.Structure):
    _fields_ = [("transform", C.c_float * 16), ("invTransform", C.c_float * 16), ("color", C.c_float * 4), ("type", C.c_uint32),
                ("flags", C.c_uint32), ("shapeKind", C.c_uint32), ("isDelta", C.c_uint32), ("cosAngle", C.c_float), ("texture", C.c_uint32), ("_pad", C.c_float * 2),
                ("shapeParam", C.c_float * 4), ("shapeParam2", C.c_float * 4)]


RT_NO_TEXTURE = 0xFFFFFFFF


class RtTexture(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("format", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("stride", C.c_uint32),
                ("linearSpace", C.c_uint32), ("filter", C.c_uint32), ("numOctaves", C.c_uint32), ("dataOffset", C.c_uint64),
                ("paletteOffset", C.c_uint64), ("colorA", C.c_float * 4), ("colorB", C.c_float * 4), ("mixA", C.c_uint32),
                ("mixB", C.c_uint32), ("mixWeight", C.c_uint32), ("_pad", C.c_uint32)]


class RtMaterial(C.Structure):
    _fields_ = [("emission", C.c_float * 4), ("baseColor", C.c_float * 4), ("roughness", C.c_float), ("metalness", C.c_float),
                ("IoR", C.c_float), ("K", C.c_float), ("bsdf", C.c_uint32), ("baseColorTexture", C.c_uint32),
                ("emissionTexture", C.c_uint32), ("roughnessTexture", C.c_uint32), ("metalnessTexture", C.c_uint32),
                ("normalMapTexture", C.c_uint32), ("normalMapStrength", C.c_float), ("_pad", C.c_uint32)]


class RtSceneDesc(C.Structure):
    _fields_ = [("abiVersion", C.c_uint32), ("numObjects", C.c_uint32), ("numTopNodes", C.c_uint32), ("numLights", C.c_uint32),
                ("numGlobalLights", C.c_uint32), ("numMaterials", C.c_uint32), ("numMeshes", C.c_uint32), ("numMeshNodes", C.c_uint32),
                ("numTriangles", C.c_uint32), ("numVertices", C.c_uint32), ("numTextures", C.c_uint32), ("_pad", C.c_uint32),
                ("topNodes", C.POINTER(RtNode)), ("objects", C.POINTER(RtObject)), ("lights", C.POINTER(RtLight)),
                ("globalLights", C.POINTER(C.c_uint32)), ("materials", C.POINTER(RtMaterial)), ("meshes", C.POINTER(RtMesh)),
                ("meshNodes", C.POINTER(RtNode)), ("triangles", C.c_void_p), ("vertexIndices", C.c_void_p),
                ("vertexShading", C.c_void_p), ("blueNoise", C.c_void_p), ("textures", C.POINTER(RtTexture)), ("texelData", C.c_void_p),
                ("texelBytes", C.c_uint64)]


class RtSceneUpdate(C.Structure):
    _fields_ = [("abiVersion", C.c_uint32), ("numObjects", C.c_uint32), ("numTopNodes", C.c_uint32), ("numLights", C.c_uint32),
                ("topNodes", C.POINTER(RtNode)), ("objects", C.POINTER(RtObject)), ("previousIndex", C.POINTER(C.c_uint32)),
                ("lights", C.POINTER(RtLight))]


class RtUpdateInfo(C.Structure):
    _fields_ = [("bytesUploaded", C.c_uint64), ("numUpdates", C.c_uint32), ("topDepth", C.c_uint32), ("walk", C.c_uint32), ("_pad", C.c_uint32 * 3)]


class RtMeshUpdate(C.Structure):
    _fields_ = [("abiVersion", C.c_uint32), ("meshIndex", C.c_uint32), ("numVertices", C.c_uint32), ("flags", C.c_uint32),
                ("positions", C.POINTER(C.c_float)), ("shading", C.c_void_p)]


class RtMeshUpdateDevice(C.Structure):
    _fields_ = [("abiVersion", C.c_uint32), ("meshIndex", C.c_uint32), ("numVertices", C.c_uint32), ("flags", C.c_uint32),
                ("positions", C.c_void_p), ("normals", C.c_void_p), ("tangents", C.c_void_p)]


def update_mesh_device(ctx, mesh_index, num_vertices, positions, normals=None, tangents=None, stream=None):
    """rtgpu_update_mesh_device, the thin call: the arrays are DEVICE addresses (ints, or None), `stream` a HIP stream handle (None: the context's own).
    Returns (status, box): the library's status as it is and the refitted root box as a (2, 3) float32 array (min, max) -- zeros where the call refused."""
    u = RtMeshUpdateDevice(3, int(mesh_index), int(num_vertices), 0, positions, normals, tangents)
    box = np.zeros((2, 3), dtype=np.float32)
    lib = rtgpu_lib()
    lib.rtgpu_update_mesh_device.argtypes, lib.rtgpu_update_mesh_device.restype = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int
    status = lib.rtgpu_update_mesh_device(ctx, C.byref(u), stream, box.ctypes.data_as(C.c_void_p))
    return int(status), box


def refit_check(ctx, mesh_index, positions, stream=None, record=None):
    """rtgpu_refit_check_async, the check of rtgpu_update_mesh_device alone: `positions` a contiguous float32 (V, 3) tensor on the context's device.  With
    `record` (an int32 tensor of 8 words on that device) the call is left asynchronous on `stream` and returns the status; without, it is waited for and
    returns dict(lo, hi: the box over the positions the mesh's triangles refer to, float32, from the record's keys; non_finite: bool)."""
    import torch
    lib = rtgpu_lib()
    lib.rtgpu_refit_check_async.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rtgpu_refit_check_async.restype = C.c_int
    out = record if record is not None else torch.empty(8, dtype=torch.int32, device=positions.device)
    if stream is None and record is None:
        stream = C.c_void_p(torch.cuda.current_stream(positions.device).cuda_stream)
    r = lib.rtgpu_refit_check_async(ctx, int(mesh_index), int(positions.shape[0]), positions.data_ptr(), out.data_ptr(), stream)
    if record is not None:
        return int(r)
    if r != 0:
        raise (ValueError if r == -1 else RuntimeError)("rtgpu_refit_check_async failed (%d): %s" % (r, (lib.rtgpu_last_error() or b"").decode()))
    torch.cuda.current_stream(positions.device).synchronize()
    keys = out.cpu().numpy().view(np.uint32)
    unkey = np.where(keys[:6] & 0x80000000, keys[:6] & 0x7FFFFFFF, ~keys[:6]).astype(np.uint32).view(np.float32)
    return dict(lo=unkey[0:3].copy(), hi=unkey[3:6].copy(), non_finite=bool(keys[6]))


class RtWideLevelInfo(C.Structure):
    _fields_ = [("nodeBase", C.c_uint32), ("gateBase", C.c_uint32), ("triBase", C.c_uint32), ("valid", C.c_uint32), ("base", C.c_float * 3),
                ("step", C.c_float * 3), ("bound", C.c_float * 3), ("pad", C.c_uint32 * 3)]


def read_mesh(ctx, mesh_index, num_nodes, num_triangles):
    """rtgpu_read_mesh: the mesh's nodes (caller's order, (num_nodes, 8) uint32 words) and triangles ((num_triangles, 9) float32) as they stand on the device."""
    nodes = np.zeros((num_nodes, 8), dtype=np.uint32)
    triangles = np.zeros((num_triangles, 9), dtype=np.float32)
    if rtgpu_lib().rtgpu_read_mesh(ctx, C.c_uint32(mesh_index), nodes.ctypes.data_as(C.c_void_p), triangles.ctypes.data_as(C.c_void_p)) != 0:
        raise RuntimeError("rtgpu_read_mesh failed: %s" % (rtgpu_lib().rtgpu_last_error() or b"").decode())
    return nodes, triangles


def read_wide_level(ctx, object_index):
    """rtgpu_read_wide_level: (info dict with the grid, node records (n, 4) uint32, gate records (m, 4) float32) of the 4-wide level that serves the object."""
    lib, info = rtgpu_lib(), RtWideLevelInfo()
    if lib.rtgpu_read_wide_level(ctx, C.c_uint32(object_index), C.byref(info), None, C.c_uint64(0), None, C.c_uint64(0)) != 0:
        raise RuntimeError("rtgpu_read_wide_level failed: %s" % (lib.rtgpu_last_error() or b"").decode())
    nodes = np.zeros((info.pad[0], 4), dtype=np.uint32)
    gates = np.zeros((info.pad[1], 4), dtype=np.float32)
    if lib.rtgpu_read_wide_level(ctx, C.c_uint32(object_index), C.byref(info), nodes.ctypes.data_as(C.c_void_p), C.c_uint64(nodes.nbytes),
                                 gates.ctypes.data_as(C.c_void_p), C.c_uint64(gates.nbytes)) != 0:
        raise RuntimeError("rtgpu_read_wide_level failed: %s" % (lib.rtgpu_last_error() or b"").decode())
    grid = dict(base=np.array(info.base[:], dtype=np.float32), step=np.array(info.step[:], dtype=np.float32), bound=np.array(info.bound[:], dtype=np.float32))
    return dict(grid, nodeBase=int(info.nodeBase), gateBase=int(info.gateBase), triBase=int(info.triBase), valid=int(info.valid)), nodes, gates


def update_info(ctx):
    """rtgpu_get_update_info as a dict: what the last rtgpu_update_objects / rtgpu_update_mesh copied to the device, how many of each there were, and the walk
    that serves the scene."""
    info = RtUpdateInfo()
    if rtgpu_lib().rtgpu_get_update_info(ctx, C.byref(info)) != 0:
        raise RuntimeError("rtgpu_get_update_info failed")
    return {"bytesUploaded": int(info.bytesUploaded), "numUpdates": int(info.numUpdates), "numMeshUpdates": int(info._pad[0]), "topDepth": int(info.topDepth),
            "walk": ["binary", "wide", "wide2"][info.walk]}


class RtPostprocessParams(C.Structure):
    _fields_ = [("colorFilter", C.c_float * 4), ("exposure", C.c_float), ("contrast", C.c_float), ("saturation", C.c_float),
                ("ditheringStrength", C.c_float), ("bloomFactor", C.c_float), ("tonemapper", C.c_uint32), ("numPasses", C.c_uint32),
                ("ditherSeed", C.c_uint32)]


class RtBlock(C.Structure):
    _fields_ = [("minX", C.c_uint32), ("maxX", C.c_uint32), ("minY", C.c_uint32), ("maxY", C.c_uint32)]


class RtCamera(C.Structure):
    _fields_ = [("localToWorld", C.c_float * 16), ("aspectRatio", C.c_float), ("tanHalfFoV", C.c_float), ("dofEnable", C.c_uint32),
                ("bokehShape", C.c_uint32), ("focalPlaneDistance", C.c_float), ("aperture", C.c_float), ("barrelDistortionConstFactor", C.c_float),
                ("barrelDistortionVariableFactor", C.c_float),
                ("worldToScreen", C.c_float * 16)]


class RtMultiInfo(C.Structure):
    _fields_ = [("numDevices", C.c_uint32), ("gatherMode", C.c_uint32), ("gatherReason", C.c_uint32), ("reasonDevice", C.c_int32), ("reasonError", C.c_int32),
                ("devices", C.c_int32 * 16), ("peerAccess", C.c_uint32 * 16), ("reserved", C.c_uint32), ("gathers", C.c_uint64),
                ("lastGatherMs", C.c_double), ("totalGatherMs", C.c_double)]


class RtBeamListInfo(C.Structure):
    _fields_ = [("builds", C.c_uint64), ("packetsScanned", C.c_uint64), ("packetsWalkedOffset", C.c_uint64), ("packetsWalkedNoList", C.c_uint64),
                ("valid", C.c_uint32), ("capacity", C.c_uint32), ("numTiles", C.c_uint32), ("margin", C.c_float),
                ("allocations", C.c_uint64), ("retiredArrays", C.c_uint32), ("reserved", C.c_uint32)]


def multi_info(ctx):
    """rtgpu_get_multi_info as a dict: how a (multi-device) context gathers the peers' tiles at read-back, and why."""
    m = RtMultiInfo()
    if rtgpu_lib().rtgpu_get_multi_info(ctx, C.byref(m)) != 0:
        raise RuntimeError("rtgpu_get_multi_info failed")
    n = int(m.numDevices)
    return {"numDevices": n, "gatherMode": ["none", "peer-kernel", "staged-copy"][m.gatherMode], "gatherReason": ["", "RTGPU_MULTI_STAGED=1", "hipDeviceCanAccessPeer: no", "hipDeviceEnablePeerAccess failed"][m.gatherReason],
            "reasonDevice": int(m.reasonDevice), "reasonError": int(m.reasonError), "devices": [int(m.devices[i]) for i in range(n)], "peerAccess": [bool(m.peerAccess[i]) for i in range(n)],
            "gathers": int(m.gathers), "lastGatherMs": float(m.lastGatherMs), "totalGatherMs": float(m.totalGatherMs)}


class RtPassParams(C.Structure):
    _fields_ = [("camera", RtCamera), ("seed", C.POINTER(C.c_uint32)), ("numDimensions", C.c_uint32), ("useBlueNoise", C.c_uint32),
                ("sampleOffset", C.c_float * 2), ("passIndex", C.c_uint32), ("maxRayDepth", C.c_uint32),
                ("minRussianRouletteDepth", C.c_uint32), ("lightSamplingStrategy", C.c_uint32),
                ("lightSamplingWeight", C.c_float * 4), ("bsdfSamplingWeight", C.c_float * 4), ("rngKey", C.c_uint64 * 2)]


class RtCounters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("numRays", "numShadowRays", "numShadowRaysHit", "numPrimaryRays", "numRayBoxTests",
                                          "numPassedRayBoxTests", "numRayTriangleTests", "numPassedRayTriangleTests",
                                          "numMeshHits", "numAnalyticHits", "numShadowRayBoxTests",
                                          "numShadowRayTriangleTests", "numRetracedRays")] + [("_reserved", C.c_uint64 * 3)]


class RtPathVertex(C.Structure):
    _fields_ = [("w", C.c_float * 28)]


class RtPathInfo(C.Structure):
    _fields_ = [("numVertices", C.c_uint32), ("terminationReason", C.c_uint32), ("radiance", C.c_float * 3), ("_pad", C.c_uint32 * 3)]


# PathTerminationReason (Core/Rendering/PathDebugging.h:9-18)
PATH_TERMINATION_REASONS = ("None", "HitBackground", "HitLight", "Depth", "Throughput", "NoSampledEvent", "RussianRoulette")


class RtQueryRay(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("maxDistance", C.c_float), ("direction", C.c_float * 3), ("_pad", C.c_float)]


class RtPrimaryRay(C.Structure):
    """an entry of a ray source (Viewport.set_ray_source): RtQueryRay's layout, words 3 and 7 never read"""
    _fields_ = [("origin", C.c_float * 3), ("_pad0", C.c_float), ("direction", C.c_float * 3), ("_pad1", C.c_float)]


class RtLensRay(C.Structure):
    """an entry of a lens source (Viewport.set_lens_source): 128 bytes, eight quads; the pads of quads 2..7 are never read"""
    _fields_ = [("origin", C.c_float * 3), ("aperture", C.c_float), ("direction", C.c_float * 3), ("focalDistance", C.c_float),
                ("dOriginDsx", C.c_float * 3), ("_pad2", C.c_float), ("dOriginDsy", C.c_float * 3), ("_pad3", C.c_float),
                ("dDirectionDsx", C.c_float * 3), ("_pad4", C.c_float), ("dDirectionDsy", C.c_float * 3), ("_pad5", C.c_float),
                ("lensU", C.c_float * 3), ("_pad6", C.c_float), ("lensV", C.c_float * 3), ("_pad7", C.c_float)]


class RtLensSourceParams(C.Structure):
    _fields_ = [("lens", C.c_uint32), ("bokehShape", C.c_uint32)]


class RtQueryHit(C.Structure):
    _fields_ = [("distance", C.c_float), ("objectId", C.c_uint32), ("subObjectId", C.c_uint32), ("u", C.c_float), ("v", C.c_float), ("_pad", C.c_uint32 * 3)]


class RtQuerySurface(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("normal", C.c_float * 3), ("tangent", C.c_float * 3), ("texCoord", C.c_float * 2), ("material", C.c_uint32)]


TRACE_CLOSEST, TRACE_ANY = 0, 1
RT_INVALID_OBJECT, RT_LIGHT_OBJECT, RT_NO_MATERIAL = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF

# Viewport.trace_rays: Scene::Traverse (+ Scene::EvaluateIntersection with surfaces=True) per ray; the surface fields are None without surfaces
RayHits = collections.namedtuple("RayHits", ["distance", "object_id", "sub_object_id", "uv", "position", "normal", "tangent", "tex_coord", "material"],
                                 defaults=(None,) * 5)


COUNTER_NAMES = ("numRays", "numShadowRays", "numShadowRaysHit", "numPrimaryRays", "numRayBoxTests", "numPassedRayBoxTests",
                 "numRayTriangleTests", "numPassedRayTriangleTests", "numMeshHits", "numAnalyticHits", "numShadowRayBoxTests",
                 "numShadowRayTriangleTests", "numRetracedRays")

# RtAovPlane (include/rtgpu.h): name -> (id, channels, dtype), in the enum's order
AOV_PLANES = collections.OrderedDict(
    (name, (i, channels, dtype)) for i, (name, channels, dtype) in enumerate((
        ("depth", 1, np.float32), ("position", 3, np.float32), ("normal", 3, np.float32), ("tangent", 3, np.float32), ("bitangent", 3, np.float32),
        ("texcoord", 2, np.float32), ("barycentrics", 2, np.float32), ("base_color", 3, np.float32), ("emission", 3, np.float32),
        ("roughness", 1, np.float32), ("metalness", 1, np.float32), ("ior", 1, np.float32), ("object_id", 1, np.uint32),
        ("sub_object_id", 1, np.uint32), ("material", 1, np.uint32), ("box_tests", 1, np.uint32), ("box_tests_passed", 1, np.uint32),
        ("triangle_tests", 1, np.uint32), ("triangle_tests_passed", 1, np.uint32))))

# RtAovChainPlane (include/rtgpu.h): the planes of render_aovs(chain=N) alone, behind AOV_PLANES' ids
AOV_CHAIN_PLANES = collections.OrderedDict(
    (name, (len(AOV_PLANES) + i, channels, dtype)) for i, (name, channels, dtype) in enumerate((
        ("chain_length", 1, np.uint32), ("chain_distance", 1, np.float32), ("chain_throughput", 3, np.float32))))
AOV_CHAIN_MAX = 16
# RtAovVirtualPlane (include/rtgpu.h): the plane of rtgpu_render_aovs_virtual alone, behind AOV_CHAIN_PLANES' ids
AOV_VIRTUAL_PLANES = {"virtual_position": (22, 3, np.float32)}


class RtAovChain(C.Structure):
    _fields_ = [("maxChain", C.c_uint32), ("flags", C.c_uint32), ("_pad", C.c_uint32 * 2)]


# ---- denoise (include/rtgpu.h: rtgpu_filter_atrous / rtgpu_denoise) --------------------------------------------------------------------------
class RtDenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("flags", C.c_uint32), ("colorScale", C.c_float), ("sigmaColor", C.c_float), ("sigmaNormal", C.c_float),
                ("sigmaPlane", C.c_float), ("_pad", C.c_uint32 * 2)]


RT_DENOISE_DEMODULATE = 1
RT_DENOISE_INPUT_PREPARED = 2   # (the variance-guided filter: the inputs are the accumulated pair of temporal_accumulate)
# the wrappers' defaults: a wide colour sigma at the first level (it halves per level), normals within about 15 degrees, planes within a tenth of a scene unit
DENOISE_DEFAULTS = dict(sigma_color=2.0, sigma_normal=0.25, sigma_plane=0.1)


def denoise_params(iterations=5, sigma_color=DENOISE_DEFAULTS["sigma_color"], sigma_normal=DENOISE_DEFAULTS["sigma_normal"],
                   sigma_plane=DENOISE_DEFAULTS["sigma_plane"], color_scale=1.0, demodulate=True):
    p = RtDenoiseParams()
    p.iterations, p.flags = int(iterations), RT_DENOISE_DEMODULATE if demodulate else 0
    p.colorScale, p.sigmaColor, p.sigmaNormal, p.sigmaPlane = float(color_scale), float(sigma_color), float(sigma_normal), float(sigma_plane)
    return p


class RtDenoiseVarParams(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("flags", C.c_uint32), ("colorScale", C.c_float), ("sigmaLum", C.c_float), ("sigmaNormal", C.c_float),
                ("sigmaPlane", C.c_float), ("varianceFloor", C.c_float), ("_pad", C.c_uint32)]


# the variance-guided filter's own defaults: luminance within four standard deviations; a floor far below any variance a render produces
DENOISE_VAR_DEFAULTS = dict(sigma_lum=4.0, variance_floor=1e-10)


def denoise_var_params(iterations=5, sigma_lum=DENOISE_VAR_DEFAULTS["sigma_lum"], sigma_normal=DENOISE_DEFAULTS["sigma_normal"],
                       sigma_plane=DENOISE_DEFAULTS["sigma_plane"], variance_floor=DENOISE_VAR_DEFAULTS["variance_floor"], color_scale=1.0, demodulate=True):
    p = RtDenoiseVarParams()
    p.iterations, p.flags = int(iterations), RT_DENOISE_DEMODULATE if demodulate else 0
    p.colorScale, p.sigmaLum, p.sigmaNormal, p.sigmaPlane, p.varianceFloor = float(color_scale), float(sigma_lum), float(sigma_normal), float(sigma_plane), float(variance_floor)
    return p


_filter_contexts = {}


def _filter_context(device):
    """a context of the library for the pure image filter (no scene, no film), one per device, kept until release_filter_contexts()"""
    if device not in _filter_contexts:
        ctx = C.c_void_p()
        r = rtgpu_lib().rtgpu_create(int(device), C.byref(ctx))
        if r != 0:
            raise RuntimeError("rtgpu_create(%d) failed (%d): %s" % (device, r, (rtgpu_lib().rtgpu_last_error() or b"").decode()))
        _filter_contexts[device] = ctx
    return _filter_contexts[device]


def release_filter_contexts():
    """Destroys the contexts atrous_filter created for itself, with their device scratch (64 bytes per pixel of the largest frame filtered, and as much
    again for the staged planes of the NumPy path).  Waits for the filter calls still running on them."""
    while _filter_contexts:
        _, ctx = _filter_contexts.popitem()
        rtgpu_lib().rtgpu_destroy(ctx)


def _run_on_torch_stream(torch, owner, device, tensors, call):
    """call(stream handle) on torch.cuda.current_stream(device); torch's default stream is the null stream, which means the context's own to the async
    entry points: then a side stream of `owner` (device -> stream, one per device, reused) ordered behind the current one, which the current one waits for"""
    current = torch.cuda.current_stream(device)
    if current.cuda_stream != 0:
        return call(C.c_void_p(current.cuda_stream))
    side = owner.get(device)
    if side is None:
        side = owner[device] = torch.cuda.Stream(device)
    side.wait_stream(current)
    r = call(C.c_void_p(side.cuda_stream))
    current.wait_stream(side)
    for t in tensors:
        if t is not None:
            t.record_stream(side)
    return r


_filter_streams = {}

def _image_planes(planes, shapes):
    """The planes (a dict name -> array, "color" first) of atrous_filter / temporal_accumulate held to `shapes` (name -> the shapes allowed): float32 NumPy arrays,
    or contiguous float32 tensors on the colour's ROCm device; a plane named *object_id or *chain_length holds uint32 words, or int32 / int64 in a tensor.  Returns the planes as the
    library reads them (contiguous arrays; int64 ids narrowed to int32), ptr(a name of theirs, an array or None), empty(shape) for an output of their kind, the device
    index (0 for NumPy arrays) and the torch module (None for NumPy arrays)."""
    torch = None
    if any(type(a).__module__.split(".")[0] == "torch" for a in planes.values()):
        import torch
        on_gpu = isinstance(planes["color"], torch.Tensor) and planes["color"].is_cuda
        device = planes["color"].device if on_gpu else None
    for name, a in list(planes.items()):
        ids = name.endswith("object_id") or name.endswith("chain_length")
        if torch is None:
            ok = isinstance(a, np.ndarray) and a.dtype == (np.uint32 if ids else np.float32)
        elif not ids:
            ok = on_gpu and isinstance(a, torch.Tensor) and a.dtype == torch.float32 and a.device == device
        else:
            ok = on_gpu and isinstance(a, torch.Tensor) and a.dtype in (torch.int32, torch.int64) and a.device == device
            if ok and a.dtype == torch.int64:
                planes[name] = a.to(torch.int32)   # (the low words: ids are below 2^32)
        if not ok or a.shape not in shapes[name]:
            raise ValueError("%s must be a %s %s of shape %s%s" % (name, "uint32" if ids else "float32", "NumPy array" if torch is None else "tensor on the colour's ROCm device",
                                                                   " or ".join(str(t) for t in shapes[name]), "" if torch is None else " (all arrays or all tensors)"))
        if torch is not None and not a.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
    if torch is None:
        planes = {name: np.ascontiguousarray(a) for name, a in planes.items()}

        def ptr(a):
            a = planes.get(a) if a.__class__ is str else a
            return None if a is None else C.c_void_p(a.ctypes.data)   # (the arrays outlive the call: in `planes`, or the caller's outputs)
        return planes, ptr, lambda shape: np.zeros(shape, dtype=np.float32), 0, None

    def ptr(a):
        a = planes.get(a) if a.__class__ is str else a
        return None if a is None else C.c_void_p(a.data_ptr())
    return planes, ptr, lambda shape: torch.empty(shape, dtype=torch.float32, device=device), device.index if device.index is not None else torch.cuda.current_device(), torch


def _image_call(torch, index, what, ctx, entry, args, tensors):
    """entry(context, *args) of the library, or with torch entry_async(context, *args, stream) on torch.cuda.current_stream() (`tensors`: what a side stream would
    touch); `ctx`: the caller's context, or None: the module's own of device `index`.  Raises as the status says."""
    lib = rtgpu_lib()
    context = ctx if ctx is not None else _filter_context(index)
    if torch is None:
        r = getattr(lib, entry)(context, *args)
    else:
        entry = getattr(lib, entry + "_async")
        r = _run_on_torch_stream(torch, _filter_streams, index, tensors, lambda stream: entry(context, *args, stream))
    if r != 0:
        err = (lib.rtgpu_last_error() or b"").decode()
        raise (ValueError if r == -1 else RuntimeError)("%s failed (%d): %s" % (what, r, err))


def atrous_filter(color, depth, normal, position, albedo=None, iterations=5, sigma_color=DENOISE_DEFAULTS["sigma_color"],
                  sigma_normal=DENOISE_DEFAULTS["sigma_normal"], sigma_plane=DENOISE_DEFAULTS["sigma_plane"], color_scale=1.0, demodulate=True, ctx=None,
                  color_half=None, sigma_lum=DENOISE_VAR_DEFAULTS["sigma_lum"], variance_floor=DENOISE_VAR_DEFAULTS["variance_floor"], return_variance=False,
                  prepared=False):
    """The edge-avoiding a-trous filter of include/rtgpu.h over a frame: color (H, W, 3), depth (H, W) or (1, H, W), normal, position and albedo (3, H, W)
    -- the layouts of Viewport.sum_buffer() and Viewport.render_aovs() -- as float32 NumPy arrays, or as contiguous float32 torch tensors on a ROCm device
    (then the filter runs on torch.cuda.current_stream() without a host copy and returns a tensor).  Returns the (H, W, 3) image.  albedo is needed with
    demodulate=True only.  `ctx`: a device context to run on (default: one of the module's own per device, which keeps its scratch -- 64 bytes per pixel,
    twice that on the NumPy path -- until release_filter_contexts()).  Not thread-safe: the calls on one context share that scratch and are ordered by the
    library's events from one host thread; callers on several threads serialise their calls or pass contexts of their own.

    color_half (H, W, 3), the sum over half of the samples (Viewport.sum_buffer(secondary=True)[1]), selects the variance-guided filter
    (rtgpu_filter_atrous_var): sigma_lum and variance_floor take sigma_color's place, and return_variance=True returns (image, the (H, W) variance).
    prepared=True (RT_DENOISE_INPUT_PREPARED, with color_half): color and color_half are the accumulated pair (a, b) of temporal_accumulate, taken as they
    are -- no color_scale, no doubling, no division by the albedo; the result is still multiplied by it under demodulate."""
    variance = color_half is not None
    if prepared and not variance:
        raise ValueError("prepared=True needs color_half")
    if return_variance and not variance:
        raise ValueError("return_variance=True needs color_half")
    planes = dict(color=color, depth=depth, normal=normal, position=position)
    if variance:
        planes["color_half"] = color_half
    if demodulate:
        if albedo is None:
            raise ValueError("demodulate=True needs the albedo plane")
        planes["albedo"] = albedo
    if getattr(color, "ndim", 0) != 3 or color.shape[2] != 3:
        raise ValueError("color must be an (H, W, 3) float32 array or tensor")
    h, w = int(color.shape[0]), int(color.shape[1])
    planes, ptr, empty, index, torch = _image_planes(planes, dict(color=((h, w, 3),), color_half=((h, w, 3),), depth=((h, w), (1, h, w)), normal=((3, h, w),),
                                                                 position=((3, h, w),), albedo=((3, h, w),)))
    out, out_variance = empty((h, w, 3)), empty((h, w)) if return_variance else None
    guides = (ptr("depth"), ptr("normal"), ptr("position"), ptr("albedo"), ptr(out))
    tensors = list(planes.values()) + [out, out_variance]
    if variance:
        p = denoise_var_params(iterations, sigma_lum, sigma_normal, sigma_plane, variance_floor, color_scale, demodulate)
        if prepared:
            p.flags |= RT_DENOISE_INPUT_PREPARED
        _image_call(torch, index, "atrous_filter", ctx, "rtgpu_filter_atrous_var",
                    (C.byref(p), C.c_uint32(w), C.c_uint32(h), ptr("color"), ptr("color_half")) + guides + (ptr(out_variance),), tensors)
    else:
        p = denoise_params(iterations, sigma_color, sigma_normal, sigma_plane, color_scale, demodulate)
        _image_call(torch, index, "atrous_filter", ctx, "rtgpu_filter_atrous", (C.byref(p), C.c_uint32(w), C.c_uint32(h), ptr("color")) + guides, tensors)
    return (out, out_variance) if return_variance else out


# ---- temporal accumulation (include/rtgpu.h: rtgpu_temporal_accumulate / rtgpu_denoise_temporal) ------------------------------------------------
class RtTemporalParams(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("colorScale", C.c_float), ("alphaMin", C.c_float), ("maxHistory", C.c_float), ("normalThreshold", C.c_float),
                ("planeTolerance", C.c_float), ("prevSampleOffset", C.c_float * 2), ("prevWorldToScreen", C.c_float * 16)]


# a history of at most 64 frames that never weighs the new frame below a tenth; normals within about 25 degrees; planes within a hundredth of the depth
TEMPORAL_DEFAULTS = dict(alpha_min=0.1, max_history=64.0, normal_threshold=0.9, plane_tolerance=0.01)


def temporal_params(alpha_min=TEMPORAL_DEFAULTS["alpha_min"], max_history=TEMPORAL_DEFAULTS["max_history"], normal_threshold=TEMPORAL_DEFAULTS["normal_threshold"],
                    plane_tolerance=TEMPORAL_DEFAULTS["plane_tolerance"], color_scale=1.0, demodulate=True, prev_world_to_screen=None, prev_sample_offset=(0.0, 0.0)):
    p = RtTemporalParams()
    p.flags = RT_DENOISE_DEMODULATE if demodulate else 0
    p.colorScale, p.alphaMin, p.maxHistory, p.normalThreshold, p.planeTolerance = float(color_scale), float(alpha_min), float(max_history), float(normal_threshold), float(plane_tolerance)
    p.prevSampleOffset[0], p.prevSampleOffset[1] = float(prev_sample_offset[0]), float(prev_sample_offset[1])
    if prev_world_to_screen is not None:
        m = np.asarray(prev_world_to_screen, dtype=np.float32).reshape(-1)
        if m.size != 16:
            raise ValueError("prev_world_to_screen must hold 16 values (RtCamera.worldToScreen)")
        for i in range(16):
            p.prevWorldToScreen[i] = float(m[i])
    return p


HISTORY_KEYS = ("a", "b", "length", "depth", "normal", "position", "object_id")


class RtObjectMotion(C.Structure):
    _fields_ = [("m", C.c_float * 16), ("prevId", C.c_uint32), ("moved", C.c_uint32), ("_pad", C.c_uint32 * 2)]


RT_MOTION_DEFORMED = 2


def object_motion_table(object_motion, deform=None):
    """(matrices (n, 4, 4), prev_ids (n,), moved (n,)) as the (n, 20) word array of RtObjectMotion records.  deform (temporal_accumulate's): moved goes in as it
    is -- RT_MOTION_DEFORMED marks a deformed object -- and first_triangle, num_triangles (n,) fill the last two words."""
    matrices, prev_ids, moved = object_motion
    m = np.ascontiguousarray(matrices, dtype=np.float32).reshape(-1, 16)
    ids, flags = np.asarray(prev_ids).reshape(-1), np.asarray(moved).reshape(-1)
    if m.shape[0] == 0 or ids.shape != (m.shape[0],) or flags.shape != (m.shape[0],):
        raise ValueError("object_motion must be (matrices (n, 4, 4), prev_ids (n,), moved (n,)) with n >= 1")
    table = np.zeros((m.shape[0], 20), dtype=np.uint32)
    table[:, :16] = m.view(np.uint32)
    table[:, 16] = ids.astype(np.uint32)
    table[:, 17] = (flags != 0).astype(np.uint32)
    if deform is not None:
        first, count = np.asarray(deform["first_triangle"]).reshape(-1), np.asarray(deform["num_triangles"]).reshape(-1)
        if first.shape != ids.shape or count.shape != ids.shape:
            raise ValueError("deform's first_triangle and num_triangles must hold one value per record of object_motion")
        table[:, 17], table[:, 18], table[:, 19] = flags.astype(np.uint32), first.astype(np.uint32), count.astype(np.uint32)
    return table


class RtTemporalClip(C.Structure):
    _fields_ = [("radius", C.c_uint32), ("gamma", C.c_float), ("minCount", C.c_uint32), ("_pad", C.c_uint32)]


# history clipping (include/rtgpu.h, "Clipping the history"): the widest window, a box of one standard deviation ("History clipping", says how it
# was chosen), and a pixel clips only where a 3 x 3 patch's worth of its window lies on its own surface
TEMPORAL_CLIP_DEFAULTS = dict(radius=3, gamma=1.0, min_count=9)


class RtTemporalChain(C.Structure):
    _fields_ = [("virtualPosition", C.c_void_p), ("chainLength", C.c_void_p), ("chainDistance", C.c_void_p), ("prevChainLength", C.c_void_p)]


CHAIN_KEYS = ("virtual_position", "chain_length", "chain_distance")


class RtTemporalDeform(C.Structure):
    _fields_ = [("subObjectId", C.c_void_p), ("barycentrics", C.c_void_p), ("prevTriangles", C.c_void_p), ("numPrevTriangles", C.c_uint32), ("_pad", C.c_uint32)]


DEFORM_KEYS = ("sub_object_id", "barycentrics", "prev_triangles", "first_triangle", "num_triangles")


def temporal_clip(clip):
    """The RtTemporalClip of a wrapper's `clip` argument: None (no clip: None comes back), True (TEMPORAL_CLIP_DEFAULTS) or a dict with any of radius, gamma and
    min_count, the rest at their defaults.  The library checks the ranges."""
    if clip is None or clip is False:
        return None
    chosen = dict(TEMPORAL_CLIP_DEFAULTS)
    if clip is not True:
        if not isinstance(clip, dict) or set(clip) - set(chosen):
            raise ValueError("clip must be None, True or a dict with keys among radius, gamma, min_count")
        chosen.update(clip)
    c = RtTemporalClip()
    c.radius, c.gamma, c.minCount = int(chosen["radius"]), float(chosen["gamma"]), int(chosen["min_count"])
    return c


def temporal_accumulate(color, color_half, depth, normal, position, albedo=None, object_id=None, history=None, prev_world_to_screen=None, prev_sample_offset=(0.0, 0.0),
                        alpha_min=TEMPORAL_DEFAULTS["alpha_min"], max_history=TEMPORAL_DEFAULTS["max_history"], normal_threshold=TEMPORAL_DEFAULTS["normal_threshold"],
                        plane_tolerance=TEMPORAL_DEFAULTS["plane_tolerance"], color_scale=1.0, demodulate=True, return_motion=False, ctx=None, object_motion=None,
                        clip=None, return_confidence=False, chain=None, deform=None):
    """Temporal accumulation of include/rtgpu.h over a frame: color, color_half (H, W, 3) -- Viewport.sum_buffer(secondary=True) --, depth (H, W) or (1, H, W),
    normal, position, albedo (3, H, W) float32 and object_id (H, W) or (1, H, W) uint32 (optional) -- Viewport.render_aovs() --, as NumPy arrays or as
    contiguous torch tensors on a ROCm device (object_id: the int64 tensor render_aovs(device=True) returns, or int32 words), then on
    torch.cuda.current_stream() without a host copy, as atrous_filter.  `history`: None (every pixel starts) or the dict a previous call returned, with
    prev_world_to_screen and prev_sample_offset of the pass its guides were rendered with (RtPassParams.camera.worldToScreen, .sampleOffset).  Returns the
    history dict of this frame -- a, b (H, W, 3): the accumulated full and half-sample estimates in history space; length (H, W); and this frame's depth,
    normal, position and object_id (the words the device reads) -- which the next call takes back and whose (a, b) go into atrous_filter(prepared=True);
    return_motion=True: (history, the (2, H, W) motion plane).  albedo is needed with demodulate=True only; the object test needs the ids of both frames.
    object_motion=(matrices (n, 4, 4), prev_ids (n,), moved (n,)): the objects moved between the two frames (rtgpu_temporal_accumulate_moving) -- per current
    object id the matrix that takes a world position to where that surface point was in the previous frame, the id the object had there, and whether it
    moved at all; NumPy arrays whichever way the frame comes.  Both id planes are required with it.
    clip=True or a dict (temporal_clip): the reprojected history is clipped to this frame's local colour statistics and its length cut by how far it was pulled
    (rtgpu_temporal_accumulate_clip), with or without object_motion; return_confidence=True then appends the (H, W) confidence plane -- 1 where nothing clipped
    -- to what is returned.
    chain=dict(virtual_position=(3, H, W) float32, chain_length=(H, W) or (1, H, W) uint32 (or the int64 tensor render_aovs returns), chain_distance=(H, W) or
    (1, H, W) float32) -- Viewport.render_aovs(chain=N) --: the guides are chain guides (rtgpu_temporal_accumulate_chain): the virtual position is reprojected,
    the plane tolerance scales with the chain distance, and histories of different chain lengths stay apart; with object_motion a pixel with a chain starts.
    With or without clip and object_motion.  The returned history then carries chain_length, which a history passed beside chain must have.
    deform=dict(sub_object_id=(H, W) or (1, H, W) uint32 (or the int64 tensor render_aovs returns), barycentrics=(2, H, W) float32 -- this frame's
    Viewport.render_aovs() planes --, prev_triangles=(T, 9) float32: the triangle records deformed meshes had when the history was stored (read_mesh; a NumPy
    array, or beside tensors also a tensor), first_triangle=(n,), num_triangles=(n,)) beside an object_motion whose `moved` may hold RT_MOTION_DEFORMED: a deformed
    object's pixels are followed through their triangle's old record (rtgpu_temporal_accumulate_deform).  For such a record the matrix is the object's transform
    of then and first_triangle / num_triangles its mesh's range of prev_triangles.  With or without clip; not with chain."""
    clip = temporal_clip(clip)
    if deform is not None:
        if not isinstance(deform, dict) or set(deform) != set(DEFORM_KEYS):
            raise ValueError("deform must be a dict with the keys " + ", ".join(DEFORM_KEYS))
        if chain is not None or object_motion is None:
            raise ValueError("deform goes with object_motion and without chain")
    if return_confidence and clip is None:
        raise ValueError("return_confidence=True needs clip")
    if chain is not None:
        if not isinstance(chain, dict) or set(chain) != set(CHAIN_KEYS):
            raise ValueError("chain must be a dict with the keys virtual_position, chain_length and chain_distance")
        if history is not None and history.get("chain_length") is None:
            raise ValueError("chain needs a history with chain_length: one a call with chain returned")
    table = None
    if object_motion is not None:
        table = object_motion_table(object_motion, deform)
        if object_id is None or (history is not None and history.get("object_id") is None):
            raise ValueError("object_motion follows objects by their ids: it needs object_id and a history with one")
    planes = dict(color=color, color_half=color_half, depth=depth, normal=normal, position=position)
    if demodulate:
        if albedo is None:
            raise ValueError("demodulate=True needs the albedo plane")
        planes["albedo"] = albedo
    if object_id is not None:
        planes["object_id"] = object_id
    if history is not None:
        if prev_world_to_screen is None:
            raise ValueError("a history needs prev_world_to_screen")
        for key in HISTORY_KEYS:
            if key not in history:
                raise ValueError("history must be the dict a previous call returned (no %r)" % key)
            if history[key] is not None:
                planes["prev_" + key] = history[key]
        if ("object_id" in planes) != ("prev_object_id" in planes):
            raise ValueError("the object test needs both id planes: give object_id and a history with one, or neither")
        if chain is not None:
            planes["prev_chain_length"] = history["chain_length"]
    if chain is not None:
        planes.update(chain)
    if deform is not None:
        planes.update(sub_object_id=deform["sub_object_id"], barycentrics=deform["barycentrics"])
    if getattr(color, "ndim", 0) != 3 or color.shape[2] != 3:
        raise ValueError("color must be an (H, W, 3) float32 array or tensor")
    h, w = int(color.shape[0]), int(color.shape[1])
    one, three, image = ((h, w), (1, h, w)), ((3, h, w),), ((h, w, 3),)
    # (in the order of the entry's arguments)
    shapes = dict(color=image, color_half=image, depth=one, normal=three, position=three, albedo=three, object_id=one, prev_a=image, prev_b=image, prev_length=one,
                  prev_depth=one, prev_normal=three, prev_position=three, prev_object_id=one)
    planes, ptr, empty, index, torch = _image_planes(planes, dict(shapes, virtual_position=three, chain_length=one, chain_distance=one, prev_chain_length=one,
                                                                 sub_object_id=one, barycentrics=((2, h, w),)))
    p = temporal_params(alpha_min, max_history, normal_threshold, plane_tolerance, color_scale, demodulate, prev_world_to_screen if history is not None else None,
                        prev_sample_offset)
    out = dict(a=empty((h, w, 3)), b=empty((h, w, 3)), length=empty((h, w)))
    motion = empty((2, h, w)) if return_motion else None
    args = [C.byref(p), C.c_uint32(w), C.c_uint32(h)] + [ptr(name) for name in shapes] + [ptr(out["a"]), ptr(out["b"]), ptr(out["length"]), ptr(motion)]
    confidence = empty((h, w)) if return_confidence else None
    tensors = list(planes.values()) + list(out.values()) + [motion, confidence]
    if table is not None and torch is not None:
        with torch.cuda.device(index):
            table = torch.from_numpy(table.view(np.int32)).to(color.device)   # (ordered on the current stream, which the side stream waits for)
    moving = [ptr(table), C.c_uint32(0 if table is None else table.shape[0])]
    if deform is not None:
        triangles = deform["prev_triangles"]
        if torch is None or isinstance(triangles, np.ndarray):
            triangles = np.ascontiguousarray(triangles, dtype=np.float32)
            if torch is not None:
                with torch.cuda.device(index):
                    triangles = torch.from_numpy(triangles).to(color.device)
        elif not (isinstance(triangles, torch.Tensor) and triangles.dtype == torch.float32 and triangles.device == color.device and triangles.is_contiguous()):
            raise ValueError("prev_triangles must be a float32 NumPy array or a contiguous float32 tensor on the colour's ROCm device")
        if triangles.ndim != 2 or triangles.shape[1] != 9:
            raise ValueError("prev_triangles must have the shape (T, 9)")
        block = RtTemporalDeform(ptr("sub_object_id"), ptr("barycentrics"), ptr(triangles) if triangles.shape[0] else None, int(triangles.shape[0]), 0)
        _image_call(torch, index, "temporal_accumulate", ctx, "rtgpu_temporal_accumulate_deform",
                    args + moving + [C.byref(clip) if clip is not None else None, ptr(confidence), C.byref(block)], tensors + [table, triangles])
    elif chain is not None:
        block = RtTemporalChain(*[ptr(name) for name in CHAIN_KEYS + ("prev_chain_length",)])
        _image_call(torch, index, "temporal_accumulate", ctx, "rtgpu_temporal_accumulate_chain",
                    args + moving + [C.byref(clip) if clip is not None else None, ptr(confidence), C.byref(block)], tensors + [table])
    elif clip is not None:
        _image_call(torch, index, "temporal_accumulate", ctx, "rtgpu_temporal_accumulate_clip", args + moving + [C.byref(clip), ptr(confidence)], tensors + [table])
    elif table is None:
        _image_call(torch, index, "temporal_accumulate", ctx, "rtgpu_temporal_accumulate", args, tensors)
    else:
        _image_call(torch, index, "temporal_accumulate", ctx, "rtgpu_temporal_accumulate_moving", args + moving, tensors + [table])
    out.update(depth=planes["depth"], normal=planes["normal"], position=planes["position"], object_id=planes.get("object_id"))
    if chain is not None:
        out["chain_length"] = planes["chain_length"]
    extras = ((motion,) if return_motion else ()) + ((confidence,) if return_confidence else ())
    return (out,) + extras if extras else out


BSDF_NAMES = ("null", "diffuse", "roughDiffuse", "dielectric", "roughDielectric", "metal", "roughMetal", "plastic", "roughPlastic")


def load_blue_noise():
    """128*128*4 uint16 blue-noise table (Data/BlueNoise128_RGBA16.dat of the reference, a data asset)."""
    return np.fromfile(os.path.join(DATA_DIR, "BlueNoise128_RGBA16.dat"), dtype=np.uint16)


def _f(values, n):
    arr = (C.c_float * n)()
    for i, v in enumerate(values):
        arr[i] = float(v)
    return arr


def _color(c):
    c = list(c)
    if len(c) == 3:
        c = c + [0.0]   # Vector4(x, y, z) leaves w = 0, like the reference's constructors / JSON loader
    return _f(c, 4)


def transform_from_euler(translation=(0.0, 0.0, 0.0), orientation_deg=(0.0, 0.0, 0.0)):
    """4x4 row-major local->world matrix from translation + Euler angles in degrees (reference JSON convention)."""
    out = (C.c_float * 16)()
    host_lib().rth_transform_from_euler(_f(translation, 3), _f(orientation_deg, 3), out)
    return out


_IDENTITY = _f([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1], 16)


class Scene:
    """rt::Scene: add objects, BuildBVH(), then hand it to a Viewport (reference: Core/Scene/Scene.h)."""

    def __init__(self):
        self._h = C.c_void_p(host_lib().rth_scene_create())
        self._keep = []
        self.built = False
        self.calls = []     # what was added, in order: ("material", {...}), ("sphere", {...}), ... (plain data; lets a tool rebuild the scene)

    def __del__(self):
        try:
            if self._h:
                host_lib().rth_scene_destroy(self._h)
        except Exception:
            pass

    def add_material(self, bsdf="diffuse", base_color=(0.7, 0.7, 0.7), emission=(0.0, 0.0, 0.0), roughness=0.1, metalness=0.0,
                     ior=1.5, k=4.0):
        mid = host_lib().rth_material_create(self._h, bsdf.encode(), _color(base_color), _color(emission), C.c_float(roughness),
                                             C.c_float(metalness), C.c_float(ior), C.c_float(k))
        if mid < 0:
            raise ValueError("unknown BSDF name %r" % bsdf)
        self.calls.append(("material", dict(bsdf=bsdf, base_color=tuple(base_color)[:3], emission=tuple(emission)[:3], roughness=roughness, metalness=metalness, ior=ior, k=k)))
        return mid

    def add_sphere(self, radius, transform=None, material=-1):
        host_lib().rth_add_sphere(self._h, C.c_float(radius), transform or _IDENTITY, int(material))
        self.calls.append(("sphere", dict(radius=radius, transform=list(transform or _IDENTITY), material=int(material))))

    def add_box(self, size, transform=None, material=-1):
        host_lib().rth_add_box(self._h, _f(size, 3), transform or _IDENTITY, int(material))
        self.calls.append(("box", dict(size=tuple(size), transform=list(transform or _IDENTITY), material=int(material))))

    def add_rect(self, size, transform=None, material=-1, tex_scale=(1.0, 1.0)):
        host_lib().rth_add_rect(self._h, _f(size, 2), _f(tex_scale, 2), transform or _IDENTITY, int(material))
        self.calls.append(("rect", dict(size=tuple(size), tex_scale=tuple(tex_scale), transform=list(transform or _IDENTITY), material=int(material))))

    def add_mesh(self, positions, indices, normals=None, tangents=None, tex_coords=None, material_indices=None, materials=(),
                 transform=None, default_material=-1):
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)

        def opt(a, w):
            if a is None:
                return None, None
            arr = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, w)
            if arr.shape[0] != pos.shape[0]:
                raise ValueError("per-vertex array has the wrong length")
            return arr, arr.ctypes.data_as(C.POINTER(C.c_float))

        nrm, nrm_p = opt(normals, 3)
        tan, tan_p = opt(tangents, 3)
        uv, uv_p = opt(tex_coords, 2)
        mi, mi_p = None, None
        if material_indices is not None:
            mi = np.ascontiguousarray(material_indices, dtype=np.uint32).reshape(-1)
            mi_p = mi.ctypes.data_as(C.POINTER(C.c_uint32))
        mats = (C.c_int * max(1, len(materials)))(*materials)
        r = host_lib().rth_add_mesh(self._h, C.c_uint32(pos.shape[0]), C.c_uint32(idx.shape[0]), pos.ctypes.data_as(C.POINTER(C.c_float)),
                                    nrm_p, tan_p, uv_p, idx.ctypes.data_as(C.POINTER(C.c_uint32)), mi_p, C.c_uint32(len(materials)), mats,
                                    transform or _IDENTITY, int(default_material))
        if r != 0:
            raise ValueError("mesh rejected (code %d)" % r)
        self.calls.append(("mesh", dict(positions=pos, indices=idx, normals=nrm, tangents=tan, tex_coords=uv, material_indices=mi, materials=tuple(materials),
                                        transform=list(transform or _IDENTITY), material=int(default_material))))

    def add_instance(self, object_index, transform=None, default_material=-1):
        """A further object over the shape of the object_index-th add_* call: for a mesh, an instance that shares its triangles and its tree."""
        if host_lib().rth_add_instance(self._h, C.c_uint32(object_index), transform or _IDENTITY, int(default_material)) != 0:
            raise IndexError("object %r has no shape" % (object_index,))
        self.calls.append(("instance", dict(object=int(object_index), transform=list(transform or _IDENTITY), material=int(default_material))))

    def add_area_light(self, shape, params, color, transform=None):
        kind = {"sphere": 0, "box": 1, "rect": 2, "plane": 2}[shape]
        p = list(params) + [0.0] * (4 - len(params))
        if host_lib().rth_add_light_area(self._h, kind, _f(p, 4), _color(color), transform or _IDENTITY) != 0:
            raise ValueError("bad area light")
        self.calls.append(("area_light", dict(shape=kind, params=tuple(p), color=tuple(color)[:3], transform=list(transform or _IDENTITY))))

    def add_background_light(self, color, texture=None):
        if texture is None:
            host_lib().rth_add_light_background(self._h, _color(color))
        elif host_lib().rth_add_light_background_textured(self._h, _color(color), int(texture)) != 0:
            raise ValueError("bad environment map texture")
        self.calls.append(("background_light", dict(color=tuple(color)[:3], texture=texture)))

    # ---- ingestion (helpers::LoadScene / LoadMesh of the reference's Demo, in the C++ host mirror) ------------------
    def load_json(self, path, data_path="", camera=None):
        """helpers::LoadScene: adds the objects / lights of a JSON scene file (and sets `camera`, a Camera, if given).
        data_path is prepended to the mesh / texture paths of the file (Options::dataPath)."""
        if host_lib().rth_load_scene(self._h, camera._h if camera is not None else None, str(path).encode(), str(data_path).encode()) != 0:
            raise ValueError("LoadScene failed: %s" % path)
        return self

    # ---- textures (ITexture of the reference; evaluated on the device) --------------------------------------------
    FORMATS = dict(R8_UNorm=1, R8G8_UNorm=2, B8G8R8_UNorm=3, B8G8R8A8_UNorm=4, R8G8B8A8_UNorm=5, B8G8R8A8_UNorm_Palette=6, B5G6R5_UNorm=7,
                   R16_UNorm=8, R16G16_UNorm=9, R16G16B16A16_UNorm=10, R32_Float=11, R32G32_Float=12, R32G32B32_Float=13,
                   R32G32B32A32_Float=14, R11G11B10_Float=15, R16_Half=16, R16G16_Half=17, R16G16B16_Half=18, R16G16B16A16_Half=19,
                   R9G9B9E5_SharedExp=20, BC1=21, BC4=22, BC5=23)
    FILTERS = dict(nearest=0, bilinear=1, smoothstep=2)

    def add_bitmap_texture(self, pixels, fmt, linear_space=True, filter="smoothstep", palette=None, size=None):
        """pixels: C-contiguous numpy array of shape (height, width[, channels]) whose dtype/channels match `fmt`
        (uint8, uint16, float16 or float32); rows are tightly packed."""
        a = np.ascontiguousarray(pixels)
        if size is not None:            # block-compressed data: `pixels` is the raw block stream, size = (width, height) in texels
            w, h = size
            stride = 0
        else:
            h, w = a.shape[0], a.shape[1]
            stride = a.strides[0]
        tid = host_lib().rth_texture_bitmap(self._h, C.c_uint32(w), C.c_uint32(h), C.c_uint32(self.FORMATS[fmt]), a.ctypes.data_as(C.c_void_p),
                                            C.c_uint32(stride), 1 if linear_space else 0, self.FILTERS[filter])
        if tid < 0:
            raise ValueError("bad bitmap texture")
        self.calls.append(("bitmap_texture", dict(id=int(tid), width=int(w), height=int(h), format=fmt, stride=int(stride), linear_space=bool(linear_space),
                                                  filter=filter, pixels=a, has_palette=palette is not None)))
        if palette is not None:
            pal = np.ascontiguousarray(palette, dtype=np.uint8).reshape(-1, 4)
            if host_lib().rth_texture_set_palette(self._h, tid, pal.ctypes.data_as(C.c_void_p), C.c_uint32(pal.shape[0])) != 0:
                raise ValueError("bad palette")
        return tid

    def add_noise_texture(self, color_a, color_b, octaves=1):
        return host_lib().rth_texture_noise(self._h, _color(color_a), _color(color_b), C.c_uint32(octaves))

    def add_mix_texture(self, texture_a, texture_b, weight):
        tid = host_lib().rth_texture_mix(self._h, int(texture_a), int(texture_b), int(weight))
        if tid < 0:
            raise ValueError("bad mix texture children")
        return tid

    def add_checkerboard_texture(self, color_a, color_b):
        return host_lib().rth_texture_checkerboard(self._h, _color(color_a), _color(color_b))

    def add_const_texture(self, color):
        return host_lib().rth_texture_const(self._h, _color(color))

    def set_material_texture(self, material, slot, texture, strength=1.0):
        """slot: 'baseColor' | 'emission' | 'roughness' | 'metalness' | 'normal' (strength = normalMapStrength)"""
        slots = dict(baseColor=0, emission=1, roughness=2, metalness=3, normal=4)
        if host_lib().rth_material_set_texture(self._h, int(material), slots[slot], int(texture), C.c_float(strength)) != 0:
            raise ValueError("bad material / texture id")
        self.calls.append(("material_texture", dict(material=int(material), slot=slot, texture=int(texture), strength=float(strength))))

    def add_directional_light(self, color, angle_rad=0.2, transform=None):
        host_lib().rth_add_light_directional(self._h, _color(color), C.c_float(angle_rad), transform or _IDENTITY)
        self.calls.append(("directional_light", dict(color=tuple(color)[:3], angle=float(angle_rad), transform=list(transform or _IDENTITY))))

    def add_point_light(self, color, transform=None):
        host_lib().rth_add_light_point(self._h, _color(color), transform or _IDENTITY)
        self.calls.append(("point_light", dict(color=tuple(color)[:3], transform=list(transform or _IDENTITY))))

    def add_spot_light(self, color, angle_rad, transform=None):
        host_lib().rth_add_light_spot(self._h, _color(color), C.c_float(angle_rad), transform or _IDENTITY)
        self.calls.append(("spot_light", dict(color=tuple(color)[:3], angle=float(angle_rad), transform=list(transform or _IDENTITY))))

    def build(self):
        if host_lib().rth_scene_build(self._h) != 0:
            if any(self.mesh_on_device(i) for i in range(self.object_count())):
                raise RuntimeError("Scene::BuildBVH refused: a mesh was deformed on the device (Viewport.update_mesh_device) and the scene's copy of it is "
                                   "stale; give it vertices with set_mesh_vertices first")
            raise RuntimeError("Scene::BuildBVH failed")
        self.built = True
        return self

    # ---- moving objects (ISceneObject::SetTransform + the top-level half of Scene::BuildBVH) ----------------------------------------
    _OBJECT_CALLS = ("sphere", "box", "rect", "mesh", "instance", "area_light", "background_light", "directional_light", "point_light", "spot_light")

    def object_count(self):
        """Objects added so far, shapes and lights alike: the range of set_object_transform's index."""
        return int(host_lib().rth_scene_object_count(self._h))

    def set_object_transform(self, index, transform):
        """ISceneObject::SetTransform of the object the index-th add_* call made (lights count).  Takes effect with update() (or build())."""
        if host_lib().rth_scene_object_set_transform(self._h, C.c_uint32(index), transform) != 0:
            raise IndexError("no object %r" % (index,))
        added = [args for kind, args in self.calls if kind in self._OBJECT_CALLS]
        if len(added) == self.object_count() and "transform" in added[index]:   # (objects of load_json are not in `calls`)
            added[index]["transform"] = list(transform)

    def set_mesh_vertices(self, object_index, positions, normals=None, tangents=None):
        """MeshShape::UpdateVertices of the mesh the object_index-th add_* call made: new positions (and optionally normals / tangents; None: they stay) for
        the same vertices, in add_mesh's order.  The mesh keeps its topology and leaf order; its tree is refitted.  Takes effect with update(); Viewport.
        update_scene() then refits the device's copy from the positions alone (rtgpu_update_mesh).  Instances made from the same arrays are separate meshes."""
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        opt = [None if a is None else np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3) for a in (normals, tangents)]
        if any(a is not None and a.shape != pos.shape for a in opt):
            raise ValueError("per-vertex array has the wrong length")
        ptr = [None if a is None else a.ctypes.data_as(C.POINTER(C.c_float)) for a in opt]
        if host_lib().rth_scene_set_mesh_vertices(self._h, C.c_uint32(object_index), C.c_uint32(pos.shape[0]), pos.ctypes.data_as(C.POINTER(C.c_float)), ptr[0], ptr[1]) != 0:
            raise ValueError("object %r is not a mesh of %d vertices" % (object_index, pos.shape[0]))
        added = [args for kind, args in self.calls if kind in self._OBJECT_CALLS]
        if len(added) == self.object_count() and "positions" in added[object_index]:
            added[object_index]["positions"] = pos.copy()
            for key, a in zip(("normals", "tangents"), opt):
                if a is not None:
                    added[object_index][key] = a.copy()

    def set_mesh_bounds(self, object_index, lo, hi):
        """Scene::SetMeshBounds: the mesh of the object_index-th add_* call was deformed ON THE DEVICE (Viewport.update_mesh_device, which calls this) and
        (lo, hi) is its refitted root box.  update() then builds the top level over it and sends the objects alone.  The mesh is device-owned from here on
        (mesh_on_device): the scene's positions, triangles and tree of it -- `desc`'s share and `calls` -- are stale until set_mesh_vertices gives the scene
        the word again; until then build() and a whole upload (a second viewport, two update() calls without an update_scene() between them) refuse."""
        box = _f(list(lo) + list(hi), 6)
        if host_lib().rth_scene_set_mesh_bounds(self._h, C.c_uint32(object_index), box) != 0:
            raise ValueError("object %r is not a mesh" % (object_index,))

    def mesh_on_device(self, object_index):
        """True while the mesh of the object_index-th add_* call is device-owned: deformed by Viewport.update_mesh_device and not given vertices since."""
        return bool(host_lib().rth_scene_mesh_on_device(self._h, C.c_uint32(object_index)))

    def object_mesh(self, object_index):
        """(flat mesh index, vertex count) of the mesh the object_index-th add_* call made, as of the last build()."""
        mi, nv = C.c_uint32(), C.c_uint32()
        if host_lib().rth_scene_object_mesh(self._h, C.c_uint32(object_index), C.byref(mi), C.byref(nv)) != 0:
            raise ValueError("object %r is not a mesh of the built scene" % (object_index,))
        return int(mi.value), int(nv.value)

    def mesh_update_descs(self):
        """The RtMeshUpdates of the last update() (pointers into the scene, valid until the next build / update / set_mesh_vertices)."""
        out = []
        for i in range(int(host_lib().rth_scene_mesh_update_count(self._h))):
            u = RtMeshUpdate()
            host_lib().rth_scene_mesh_update_desc(self._h, C.c_uint32(i), C.byref(u))
            out.append(u)
        return out

    def update(self):
        """Scene::UpdateBVH: rebuilds the top-level tree over the objects' current boxes and rewrites the flat objects, top nodes and light
        matrices; meshes, materials and textures keep their numbering.  Viewport.update_scene() sends the result to the device."""
        if host_lib().rth_scene_update(self._h) != 0:
            raise RuntimeError("Scene::UpdateBVH failed (it needs a build() first)")
        return self

    def update_desc(self):
        """The RtSceneUpdate of the last update() (pointers into the scene, valid until the next build / update)."""
        u = RtSceneUpdate()
        host_lib().rth_scene_update_desc(self._h, C.byref(u))
        return u

    @property
    def desc(self):
        """Pointer to the flat RtSceneDesc (valid until the scene is rebuilt / destroyed).  Stale for a mesh while mesh_on_device() says so: its nodes,
        triangles and vertex shading are those of the last vertices the scene itself was given."""
        return host_lib().rth_scene_desc(self._h)


class Camera:
    """rt::Camera (reference: Core/Scene/Camera.h)."""

    def __init__(self, translation=(0.0, 0.0, 0.0), orientation_deg=(0.0, 0.0, 0.0), aspect=1.0, fov_deg=20.0):
        self._h = C.c_void_p(host_lib().rth_camera_create())
        self.settings = dict(dof=False, focal_plane_distance=2.0, aperture=0.1)
        self.set_transform(translation, orientation_deg)
        self.set_perspective(aspect, np.float32(fov_deg) / np.float32(180.0) * np.float32(3.14159265359))

    def __del__(self):
        try:
            if self._h:
                host_lib().rth_camera_destroy(self._h)
        except Exception:
            pass

    def set_transform(self, translation, orientation_deg=(0.0, 0.0, 0.0)):
        host_lib().rth_camera_set_transform(self._h, _f(translation, 3), _f(orientation_deg, 3))
        self.settings.update(translation=tuple(translation), orientation_deg=tuple(orientation_deg))

    def set_perspective(self, aspect, fov_rad):
        host_lib().rth_camera_set_perspective(self._h, C.c_float(aspect), C.c_float(fov_rad))
        self.settings.update(aspect=float(aspect), fov_rad=float(fov_rad))

    def set_dof(self, enable, focal_plane_distance=2.0, aperture=0.1):
        host_lib().rth_camera_set_dof(self._h, int(bool(enable)), C.c_float(focal_plane_distance), C.c_float(aperture))
        self.settings.update(dof=bool(enable), focal_plane_distance=float(focal_plane_distance), aperture=float(aperture))

    def set_lens(self, bokeh_shape=0, barrel_const=0.01, barrel_variable=0.0):
        """DOFSettings::bokehShape (0 circle, 1 hexagon, 2 square) and the barrel-distortion factors of rt::Camera."""
        host_lib().rth_camera_set_lens(self._h, C.c_uint32(bokeh_shape), C.c_float(barrel_const), C.c_float(barrel_variable))
        self.settings.update(bokeh_shape=int(bokeh_shape), barrel_const=float(barrel_const), barrel_variable=float(barrel_variable))


def _u32(torch, words):
    """int32 tensor of uint32 words -> int64 tensor of their unsigned values"""
    v = words.to(torch.int64)
    return torch.where(v < 0, v + (1 << 32), v)


class Viewport:
    """rt::Viewport driving the GPU "Path Tracer MIS" renderer (reference: Core/Rendering/Viewport.h)."""

    def __init__(self, width, height, seed=None, dimensions=64, use_blue_noise=True, anti_aliasing_spread=0.5, max_ray_depth=20,
                 min_russian_roulette_depth=1, light_sampling_all=False):
        self._h = C.c_void_p(host_lib().rth_viewport_create())
        self.width, self.height = int(width), int(height)
        self._scene = None
        self.has_renderer = False
        self._track_deformation = False
        self._query_streams, self._denoise_streams = {}, {}   # the side streams of _run_on_torch_stream: ray queries and AOVs, denoise
        if host_lib().rth_viewport_set_params(self._h, C.c_uint32(dimensions), int(bool(use_blue_noise)), C.c_float(anti_aliasing_spread),
                                              C.c_uint32(max_ray_depth), C.c_uint32(min_russian_roulette_depth), int(bool(light_sampling_all))) != 0:
            raise ValueError("invalid rendering params")
        if seed is not None:
            host_lib().rth_viewport_set_seed(self._h, C.c_uint64(seed))
        if host_lib().rth_viewport_resize(self._h, C.c_uint32(width), C.c_uint32(height)) != 0:
            raise ValueError("invalid viewport size")

    def __del__(self):
        try:
            if self._h:
                host_lib().rth_viewport_destroy(self._h)
        except Exception:
            pass

    def set_renderer(self, scene, name="Path Tracer MIS", device=-1, devices=None, intersection_counters=False):
        """CreateRenderer(name, scene) + SetRenderer.  Raises when the GPU renderer cannot be created.  `devices`: a list of HIP device indices
        for ONE renderer over several GPUs of the node (SetRendererDevices -> rtgpu_create_multi; an index may repeat).
        `intersection_counters`: False = the library's (and the reference's, Core/Config.h:4) default; True turns the box / triangle test
        counters on, which routes every ray through the reference's binary walk (parity tests compare those counters too)."""
        self._scene = scene
        if devices is not None:
            arr = (C.c_int * len(devices))(*[int(d) for d in devices])
            host_lib().rth_set_renderer_devices(arr, C.c_uint32(len(devices)))
        try:
            r = host_lib().rth_viewport_set_renderer(self._h, scene._h, name.encode(), int(device))
        finally:
            if devices is not None:
                host_lib().rth_set_renderer_devices(None, C.c_uint32(0))
        if r != 0:
            err = rtgpu_lib().rtgpu_last_error()
            raise RuntimeError("CreateRenderer(%r) failed (%d): %s" % (name, r, err.decode() if err else ""))
        self.has_renderer = True
        if self._track_deformation:
            self.track_deformation(True)
        if intersection_counters:
            rtgpu_lib().rtgpu_set_intersection_counters(self.device_context(), 1)
        self.reset()

    def set_vcm(self, max_path_length=10, use_vertex_connection=True, use_vertex_merging=True, initial_merging_radius=0.02,
                min_merging_radius=0.02, merging_radius_multiplier=1.0, bsdf_weight=1.0, light_weight=1.0, vertex_connecting_weight=1.0,
                camera_connecting_weight=1.0, vertex_merging_weight=1.0):
        """The public members of rt::VertexConnectionAndMerging (renderer name "VCM"); takes effect with the next pass."""
        w = (C.c_float * 5)(bsdf_weight, light_weight, vertex_connecting_weight, camera_connecting_weight, vertex_merging_weight)
        r = host_lib().rth_viewport_set_vcm(self._h, C.c_uint32(max_path_length), int(bool(use_vertex_connection)), int(bool(use_vertex_merging)),
                                            C.c_float(initial_merging_radius), C.c_float(min_merging_radius), C.c_float(merging_radius_multiplier), w)
        if r != 0:
            raise RuntimeError("set_vcm: the viewport's renderer is not \"VCM\"")

    def set_debug_mode(self, mode):
        """DebugRenderer::mRenderingMode (renderer name "Debug"): 0 CameraLight, 1 TriangleID, 2 Depth, 3 Position, 4 Normals, 5 Tangents,
        6 Bitangents, 7 TexCoords, 8 BaseColor, 9 Emission, 10 Roughness, 11 Metalness, 12 IoR."""
        if host_lib().rth_viewport_set_debug_mode(self._h, C.c_uint32(mode)) != 0:
            raise RuntimeError("set_debug_mode: the viewport's renderer is not \"Debug\" or the mode is unknown")

    def vcm_num_photons(self):
        n = C.c_uint32(0)
        ctx = C.c_void_p(host_lib().rth_viewport_device_ctx(self._h))
        if rtgpu_lib().rtgpu_vcm_num_photons(ctx, C.byref(n)) != 0:
            raise RuntimeError(rtgpu_lib().rtgpu_last_error().decode())
        return int(n.value)

    def set_shard(self, rank, world_size):
        if host_lib().rth_viewport_set_shard(self._h, C.c_uint32(rank), C.c_uint32(world_size)) != 0:
            raise RuntimeError("set_shard failed")

    def reset(self):
        host_lib().rth_viewport_reset(self._h)

    def track_deformation(self, enable=True):
        """rtgpu_set_deform_tracking: denoise(temporal=True) follows meshes deformed through Scene.set_mesh_vertices / update_scene() -- pixels on them keep
        their history, reprojected through the triangle records the mesh had a frame ago -- at the price of a device copy of those records per deformed mesh
        and frame and two more guide planes.  Off by default: such pixels then start.  A call before the device context exists is remembered and applied
        when set_renderer makes it."""
        self._track_deformation = bool(enable)
        if self.has_renderer and rtgpu_lib().rtgpu_set_deform_tracking(self.device_context(), C.c_int(int(self._track_deformation))) != 0:
            raise RuntimeError("rtgpu_set_deform_tracking failed: %s" % (rtgpu_lib().rtgpu_last_error() or b"").decode())

    def update_mesh_device(self, object_index, positions, normals=None, tangents=None):
        """rtgpu_update_mesh_device: deforms the mesh of the scene's object_index-th add_* call from tensors that are on the device already -- contiguous
        float32 (V, 3) tensors on the renderer's ROCm device, V the mesh's vertex count; normals / tangents None: they stay.  No host copy: the call runs behind
        torch.cuda.current_stream(), refits the mesh's tables on the device and returns synchronised, so the tensors may be overwritten at once.  The
        scene must be uploaded and in step (no update() the device has not seen).  The scene learns the new box alone (Scene.set_mesh_bounds: the mesh is
        device-owned from here on); where there is a top level the caller follows with scene.update(); vp.update_scene(), exactly as after any move -- a
        one-object scene needs nothing more.  Returns (lo, hi), the refitted root box, as float32 NumPy arrays."""
        import torch
        scene = self._scene
        if not self.has_renderer or scene is None:
            raise RuntimeError("update_mesh_device needs a renderer: call set_renderer first")
        mesh_index, num_vertices = scene.object_mesh(object_index)
        for name, t in (("positions", positions), ("normals", normals), ("tangents", tangents)):
            if t is None and name != "positions":
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or tuple(t.shape) != (num_vertices, 3):
                raise ValueError("%s must be a (%d, 3) float32 tensor" % (name, num_vertices))
            if not t.is_cuda or t.device != positions.device:
                raise ValueError("%s must live on the renderer's ROCm device" % name)
            if not t.is_contiguous():
                raise ValueError("%s must be contiguous" % name)
        ctx = self.device_context()
        if not ctx.value or not host_lib().rth_viewport_scene_in_step(self._h):
            raise RuntimeError("update_mesh_device needs the scene on the device and in step: call update_scene() first (after the scene's last update())")
        device = positions.device
        if (device.index if device.index is not None else torch.cuda.current_device()) != multi_info(ctx)["devices"][0]:
            raise ValueError("the tensors must live on the renderer's device (cuda:%d)" % multi_info(ctx)["devices"][0])
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        status, box = _run_on_torch_stream(torch, self._query_streams, device, (positions, normals, tangents), lambda stream: update_mesh_device(
            ctx, mesh_index, num_vertices, ptr(positions), ptr(normals), ptr(tangents), stream))
        if status != 0:
            err = (rtgpu_lib().rtgpu_last_error() or b"").decode()
            raise (ValueError if status == -1 else RuntimeError)("rtgpu_update_mesh_device failed (%d): %s" % (status, err))
        scene.set_mesh_bounds(object_index, box[0], box[1])
        return box[0].copy(), box[1].copy()

    def update_scene(self):
        """Viewport::UpdateScene: after Scene.update(), sends the new positions of every deformed mesh (Scene.set_mesh_vertices; rtgpu_update_mesh refits its
        tables on the device), then the moved objects and the rebuilt top level (rtgpu_update_objects) -- no triangle is uploaded again.  Passes queued before the call render the scene as it was.  The accumulated
        frame is the caller's to reset()."""
        if host_lib().rth_viewport_update_scene(self._h) != 0:
            raise RuntimeError("Viewport::UpdateScene failed: %s" % (rtgpu_lib().rtgpu_last_error() or b"").decode())

    def render(self, camera, passes=1):
        if host_lib().rth_viewport_render(self._h, camera._h, C.c_uint32(passes)) != 0:
            raise RuntimeError("Viewport::Render failed: %s" % (rtgpu_lib().rtgpu_last_error() or b"").decode())

    def next_pass_params(self, camera):
        """Per-pass constants (Halton seeds, AA offset ...) exactly as Render() would use them; advances the state."""
        p = RtPassParams()
        if host_lib().rth_viewport_next_pass_params(self._h, camera._h, C.byref(p)) != 0:
            raise RuntimeError("NextPassParams failed")
        # copy the seeds: the pointer refers to storage reused by the next call
        seeds = np.ctypeslib.as_array(p.seed, shape=(p.numDimensions,)).copy()
        p._seed_keepalive = seeds
        p.seed = seeds.ctypes.data_as(C.POINTER(C.c_uint32))
        return p

    def render_pass_with(self, params):
        """Submit one pass with explicit constants (used by the parity tests)."""
        if host_lib().rth_viewport_render_pass_with(self._h, C.byref(params)) != 0:
            raise RuntimeError("render pass failed: %s" % (rtgpu_lib().rtgpu_last_error() or b"").decode())

    def set_adaptive(self, enable=True, num_initial_passes=10, min_block_size=4, max_block_size=256, subdivision_treshold=0.005,
                     convergence_treshold=0.0001):
        """RenderingParams::adaptiveSettings (Core/Rendering/Context.h:35-43); resets the viewport."""
        if host_lib().rth_viewport_set_adaptive(self._h, int(bool(enable)), C.c_uint32(num_initial_passes), C.c_uint32(min_block_size),
                                                C.c_uint32(max_block_size), C.c_float(subdivision_treshold), C.c_float(convergence_treshold)) != 0:
            raise ValueError("bad adaptive settings")

    def progress(self):
        """RenderingProgress + the active block list [(minX, maxX, minY, maxY), ...]."""
        err, conv, pixels = C.c_float(), C.c_float(), C.c_uint32()
        n = host_lib().rth_viewport_progress(self._h, C.byref(err), C.byref(conv), C.byref(pixels), None, 0)
        blocks = np.zeros((max(n, 1), 4), dtype=np.uint32)
        host_lib().rth_viewport_progress(self._h, None, None, None, blocks.ctypes.data_as(C.c_void_p), C.c_uint32(n))
        return dict(averageError=err.value, converged=conv.value, activePixels=pixels.value, blocks=[tuple(int(v) for v in b) for b in blocks[:n]])

    def front_buffer(self, exposure=0.0, contrast=0.8, saturation=0.98, dithering=0.005, tonemapper=3, color_filter=(1.0, 1.0, 1.0, 1.0),
                     dither_seed=0, bloom=0.0):
        """Viewport::PostProcessTile on the device (defaults = PostprocessParams(), Core/Rendering/PostProcess.cpp:6-14):
        the (H, W) uint32 0x00RRGGBB front buffer of the passes rendered so far."""
        p = RtPostprocessParams()
        for k in range(4):
            p.colorFilter[k] = color_filter[k]
        p.exposure, p.contrast, p.saturation, p.ditheringStrength, p.bloomFactor = exposure, contrast, saturation, dithering, bloom
        p.tonemapper, p.numPasses, p.ditherSeed = int(tonemapper), max(1, self.passes_finished), int(dither_seed)
        out = np.zeros((self.height, self.width), dtype=np.uint32)
        if rtgpu_lib().rtgpu_postprocess(self.device_context(), C.byref(p), out.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("postprocess failed: %s" % (rtgpu_lib().rtgpu_last_error() or b"").decode())
        return out

    def device_context(self):
        return C.c_void_p(host_lib().rth_viewport_device_ctx(self._h))

    def sum_buffer(self, secondary=False):
        """Accumulated float3 image, shape (H, W, 3); row y as in the reference's sum bitmap.  Synchronises."""
        s = np.zeros((self.height, self.width, 3), dtype=np.float32)
        s2 = np.zeros((self.height, self.width, 3), dtype=np.float32) if secondary else None
        host_lib().rth_viewport_read_sum(self._h, s.ctypes.data_as(C.POINTER(C.c_float)),
                                         s2.ctypes.data_as(C.POINTER(C.c_float)) if secondary else None)
        return (s, s2) if secondary else s

    def counters(self):
        out = (C.c_uint64 * 16)()
        host_lib().rth_viewport_counters(self._h, out)
        d = {n: int(out[i]) for i, n in enumerate(COUNTER_NAMES)}
        if self.has_renderer:   # a statistic of the device library, not part of the reference's RayTracingCounters
            raw = RtCounters()
            if rtgpu_lib().rtgpu_get_counters(self.device_context(), C.byref(raw)) == 0:
                d["numRetracedRays"] = int(raw.numRetracedRays)
                d["numUntrustedRays"], d["numStackOverflowRays"], d["diag2"] = int(raw._reserved[0]), int(raw._reserved[1]), int(raw._reserved[2])
        return d

    # ---- beam lists (include/rtgpu.h: a still camera's per-tile leaf lists) ----------------------------------------------------------------
    def set_beam_margin(self, pixels):
        if rtgpu_lib().rtgpu_set_beam_margin(self.device_context(), float(pixels)) != 0:
            raise RuntimeError(rtgpu_lib().rtgpu_last_error().decode())

    def beam_list_info(self):
        """rtgpu_get_beam_list_info as a dict (synchronises): builds, packetsScanned, packetsWalkedOffset, packetsWalkedNoList, valid, capacity, numTiles, margin, allocations, retiredArrays."""
        info = RtBeamListInfo()
        if rtgpu_lib().rtgpu_get_beam_list_info(self.device_context(), C.byref(info)) != 0:
            raise RuntimeError(rtgpu_lib().rtgpu_last_error().decode())
        return {name: getattr(info, name) for name, _ in RtBeamListInfo._fields_}

    def beam_lists(self, from_host=False):
        """The valid lists as (counts[numTiles], entries[numTiles, capacity, 2] = {leaf reference, bits of dmin}); `from_host`: the pure host builder's for the
        same key instead of the device's arrays."""
        info = self.beam_list_info()
        counts = np.zeros(max(1, info["numTiles"]), dtype=np.uint32)
        entries = np.zeros((max(1, info["numTiles"]), max(1, info["capacity"]), 2), dtype=np.uint32)
        if rtgpu_lib().rtgpu_read_beam_lists(self.device_context(), int(bool(from_host)), counts.ctypes.data_as(C.c_void_p), entries.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError(rtgpu_lib().rtgpu_last_error().decode())
        return counts, entries

    # ---- batched ray queries (include/rtgpu.h: rtgpu_trace_rays / rtgpu_trace_rays_async) -----------------------------------------------
    def trace_rays(self, origins, directions, max_distance=float("inf"), surfaces=False):
        """Scene::Traverse of the renderer's scene for every ray (origin, direction): (N, 3) float32 NumPy arrays, or torch tensors on the
        renderer's ROCm device (then the query runs on torch.cuda.current_stream() without a host copy and the results are tensors on that device).
        max_distance: a scalar or N values (hitPoint.distance before the walk; +inf: unbounded).  Returns RayHits: distance (N,), object_id,
        sub_object_id (N,) (RT_INVALID_OBJECT on a miss), uv (N, 2); with surfaces=True also Scene::EvaluateIntersection's position, normal, tangent
        (N, 3), tex_coord (N, 2) and material (N,).  Ids are uint32 in NumPy and int64 in torch."""
        q = self._query(TRACE_CLOSEST, origins, directions, max_distance, surfaces)
        hits, surf, torch = q["hits"], q["surfaces"], q["torch"]
        if torch is None:
            f, u = hits.view(np.float32), hits
            out = dict(distance=f[:, 0].copy(), object_id=u[:, 1].copy(), sub_object_id=u[:, 2].copy(), uv=f[:, 3:5].copy())
            if surf is not None:
                sf = surf.view(np.float32)
                out.update(position=sf[:, 0:3].copy(), normal=sf[:, 3:6].copy(), tangent=sf[:, 6:9].copy(), tex_coord=sf[:, 9:11].copy(), material=surf[:, 11].copy())
            return RayHits(**out)
        f = hits.view(torch.float32)
        out = dict(distance=f[:, 0], object_id=_u32(torch, hits[:, 1]), sub_object_id=_u32(torch, hits[:, 2]), uv=f[:, 3:5])
        if surf is not None:
            sf = surf.view(torch.float32)
            out.update(position=sf[:, 0:3], normal=sf[:, 3:6], tangent=sf[:, 6:9], tex_coord=sf[:, 9:11], material=_u32(torch, surf[:, 11]))
        return RayHits(**out)

    def occluded(self, origins, directions, max_distance=float("inf")):
        """Scene::Traverse_Shadow (no origin offset) for every ray: a bool array / tensor of N.  Inputs as trace_rays."""
        q = self._query(TRACE_ANY, origins, directions, max_distance, False)
        return q["occluded"] != 0

    def _query(self, mode, origins, directions, max_distance, surfaces):
        torch = None
        if type(origins).__module__.split(".")[0] == "torch" or type(directions).__module__.split(".")[0] == "torch":
            import torch
        if torch is None:
            for name, a in (("origins", origins), ("directions", directions)):
                if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim != 2 or a.shape[1] != 3:
                    raise ValueError("%s must be an (N, 3) float32 NumPy array (or a torch tensor)" % name)
        else:
            for name, a in (("origins", origins), ("directions", directions)):
                if not isinstance(a, torch.Tensor) or a.dtype != torch.float32 or a.dim() != 2 or a.shape[1] != 3:
                    raise ValueError("%s must be an (N, 3) float32 tensor" % name)
                if not a.is_cuda:
                    raise ValueError("%s must live on the renderer's ROCm device" % name)
                if not a.is_contiguous():
                    raise ValueError("%s must be contiguous" % name)
        if origins.shape != directions.shape:
            raise ValueError("origins and directions must have the same shape")
        n = int(origins.shape[0])
        if torch is None:
            md = np.asarray(max_distance, dtype=np.float32)
            if md.ndim not in (0, 1) or (md.ndim == 1 and md.shape[0] != n):
                raise ValueError("max_distance must be a scalar or N values")
        elif isinstance(max_distance, torch.Tensor):
            if max_distance.dtype != torch.float32 or max_distance.dim() != 1 or max_distance.shape[0] != n or max_distance.device != origins.device:
                raise ValueError("max_distance must be a scalar or an (N,) float32 tensor on the rays' device")
        if not self.has_renderer:
            raise RuntimeError("trace_rays / occluded need a renderer: call set_renderer first")
        ctx = self.device_context()
        if not ctx.value or host_lib().rth_viewport_upload_scene(self._h) != 0:
            raise RuntimeError("the viewport's renderer has no device context or its scene could not be uploaded: %s" % (rtgpu_lib().rtgpu_last_error() or b"").decode())
        lib = rtgpu_lib()
        if torch is None:
            rays = np.zeros((n, 8), dtype=np.float32)
            rays[:, 0:3], rays[:, 3], rays[:, 4:7] = origins, md, directions
            hits = np.zeros((n, 8), dtype=np.uint32) if mode == TRACE_CLOSEST else None
            surf = np.zeros((n, 12), dtype=np.uint32) if surfaces else None
            occ = np.zeros(n, dtype=np.uint32) if mode == TRACE_ANY else None
            ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
            r = lib.rtgpu_trace_rays(ctx, C.c_uint32(mode), ptr(rays), C.c_uint32(n), ptr(hits), ptr(surf), ptr(occ), None)
        else:
            device = origins.device
            if directions.device != device:
                raise ValueError("origins and directions must live on the same device")
            if (device.index if device.index is not None else torch.cuda.current_device()) != multi_info(ctx)["devices"][0]:
                raise ValueError("the rays must live on the renderer's device (cuda:%d)" % multi_info(ctx)["devices"][0])
            rays = torch.empty((n, 8), dtype=torch.float32, device=device)
            rays[:, 0:3] = origins
            rays[:, 3] = max_distance
            rays[:, 4:7] = directions
            rays[:, 7] = 0.0
            hits = torch.empty((n, 8), dtype=torch.int32, device=device) if mode == TRACE_CLOSEST else None
            surf = torch.empty((n, 12), dtype=torch.int32, device=device) if surfaces else None
            occ = torch.empty(n, dtype=torch.int32, device=device) if mode == TRACE_ANY else None
            ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
            r = _run_on_torch_stream(torch, self._query_streams, device, (rays, hits, surf, occ), lambda stream: lib.rtgpu_trace_rays_async(
                ctx, C.c_uint32(mode), ptr(rays), C.c_uint32(n), ptr(hits), ptr(surf), ptr(occ), None, stream))
        if r != 0:
            err = (lib.rtgpu_last_error() or b"").decode()
            raise (ValueError if r == -1 else RuntimeError)("ray query failed (%d): %s" % (r, err))
        return dict(hits=hits, surfaces=surf, occluded=occ, torch=torch)

    # ---- the ray source (include/rtgpu.h: rtgpu_set_ray_source / rtgpu_read_camera_rays) ---------------------------------------------------------
    def _ray_source_context(self, what):
        if not self.has_renderer:
            raise RuntimeError("%s needs a renderer: call set_renderer first" % what)
        ctx = self.device_context()
        if not ctx.value:
            raise RuntimeError("%s: the viewport's renderer has no device context" % what)
        return ctx

    def set_ray_source(self, rays=None, directions=None):
        """Passes along caller-supplied primary rays (rtgpu_set_ray_source): pixel (x, y) of every following pass -- and of render_aovs, record_paths,
        denoise() and denoise(variance=True) -- starts at rays[y, x] instead of the camera's ray; row y as in sum_buffer().  `rays`: an (H, W, 8) float32
        array {origin xyz, -, direction xyz, -} (the layout trace_rays packs: words 3 and 7 are not read), or, with `directions`, a pair of (H, W, 3)
        arrays, origins and directions -- what the builders of raytracer_amd.rays return.  Directions need not be unit length; no origin offset is applied.
        Torch tensors on the renderer's ROCm device go in without a host copy, behind torch.cuda.current_stream().  The table is copied: the arrays may be
        changed at once (set a new table between passes for anti-aliasing; every set call ends the batch in flight: 6.05 ms per pass with a table per pass against
        2.32 ms on the 1080p Sponza-class frame, DESIGN.md section 5 -- set_lens_source takes ONE table for all passes instead).  A table with a ray that is not finite
        or has a zero direction raises ValueError and leaves the previous source in place.  None clears the source: the camera renders again.  A resize
        drops the source; the camera and sample offset of the pass constants are not read while one is set; denoise(temporal=True), "VCM" and
        "Light Tracer" passes raise."""
        ctx = self._ray_source_context("set_ray_source")
        if rays is None:
            if directions is not None:
                raise ValueError("directions without origins")
            lib = rtgpu_lib()
            r = lib.rtgpu_set_ray_source(ctx, None, C.c_uint64(0))
            if r != 0:
                raise RuntimeError("set_ray_source failed (%d): %s" % (r, (lib.rtgpu_last_error() or b"").decode()))
            return
        if directions is None:
            parts, words, what = (rays,), 8, "rays must be an (H, W, 8)"
        else:
            parts, words, what = (rays, directions), 3, "origins and directions must be (H, W, 3)"
        self._set_source("set_ray_source", ctx, "rtgpu_set_ray_source", parts, words, what + " float32 NumPy array(s) of the viewport's size (or torch tensors)",
                         what + " float32 tensor(s) of the viewport's size", "tensors")

    def _set_source(self, what, ctx, entry, parts, words, wrong_arrays, wrong_tensors, noun, *settings):
        """set_ray_source and set_lens_source behind their own arguments: `parts` -- one table, or origins and directions -- are (H, W, words) float32 NumPy
        arrays, or torch tensors on the renderer's device (one of them a tensor: all are held to that), and go as one contiguous table to `entry`, tensors to
        `entry`_device behind torch.cuda.current_stream(); `settings` are the entry's arguments behind the count.  A refusal (-1) raises ValueError."""
        lib = rtgpu_lib()
        h, w = self.height, self.width
        shape, count = (h, w, words), C.c_uint64(h * w)
        if any(type(a).__module__.split(".")[0] == "torch" for a in parts):
            import torch
            for a in parts:
                if not isinstance(a, torch.Tensor) or a.dtype != torch.float32 or tuple(a.shape) != shape:
                    raise ValueError(wrong_tensors)
                if not a.is_cuda or a.device != parts[0].device:
                    raise ValueError("the %s must live on the renderer's ROCm device" % noun)
            device = parts[0].device
            if (device.index if device.index is not None else torch.cuda.current_device()) != multi_info(ctx)["devices"][0]:
                raise ValueError("the %s must live on the renderer's device (cuda:%d)" % (noun, multi_info(ctx)["devices"][0]))
            if len(parts) == 1:
                table = parts[0].contiguous()
            else:
                table = torch.zeros((h, w, 8), dtype=torch.float32, device=device)
                table[:, :, 0:3] = parts[0]
                table[:, :, 4:7] = parts[1]
            r = _run_on_torch_stream(torch, self._query_streams, device, (table,), lambda stream: getattr(lib, entry + "_device")(
                ctx, C.c_void_p(table.data_ptr()), count, *settings, stream))
        else:
            for a in parts:
                if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.shape != shape:
                    raise ValueError(wrong_arrays)
            if len(parts) == 1:
                table = np.ascontiguousarray(parts[0])
            else:
                table = np.zeros((h, w, 8), dtype=np.float32)
                table[:, :, 0:3], table[:, :, 4:7] = parts
            r = getattr(lib, entry)(ctx, table.ctypes.data_as(C.c_void_p), count, *settings)
        if r != 0:
            err = (lib.rtgpu_last_error() or b"").decode()
            raise (ValueError if r == -1 else RuntimeError)("%s failed (%d): %s" % (what, r, err))

    def ray_source(self):
        """Whether a ray source is set (rtgpu_get_ray_source)."""
        n = C.c_uint64(0)
        if not self.has_renderer or not self.device_context().value:
            return False
        if rtgpu_lib().rtgpu_get_ray_source(self.device_context(), C.byref(n)) != 0:
            raise RuntimeError("rtgpu_get_ray_source failed: %s" % (rtgpu_lib().rtgpu_last_error() or b"").decode())
        return n.value != 0

    def camera_rays(self, params, device=False):
        """The primary rays the camera of the pass `params` (an RtPassParams from next_pass_params()) generates, one per pixel, in set_ray_source's layout: an
        (H, W, 8) float32 array {origin xyz, 0, direction xyz (not normalised), 0}; device=True: a torch tensor on the renderer's ROCm device, written on
        torch.cuda.current_stream().  Not a pass.  Set as the source they render the camera's frame bit for bit; they are also where a lens model of the
        caller's own starts.  A camera with depth of field or a variable barrel factor raises: a table cannot carry the lens draws.  Always the camera's
        rays, whether or not a source is set."""
        return self._source_export("camera_rays", "rtgpu_read_camera_rays", 8, params, device)

    # ---- the lens source (include/rtgpu.h: rtgpu_set_lens_source / rtgpu_read_lens_source_rays / rtgpu_read_camera_footprints) ---------------------
    def set_lens_source(self, table, lens=False, bokeh_shape=0):
        """Passes along a table of lens rays (rtgpu_set_lens_source): pixel (x, y) of every following pass -- and of render_aovs, record_paths, denoise() and
        denoise(variance=True) -- starts at the ray table[y, x] describes FOR THAT PASS: the stored ray moved by the pass's sample offset along the
        entry's footprint and, with lens=True, through the entry's thin lens, its sample drawn from the pass's sampler as the camera draws it.  One table
        serves every pass: anti-aliasing and depth of field under a source cost no set call.  `table`: an (H, W, 32) float32 array of RtLensRay entries
        {origin xyz, aperture, direction xyz, focalDistance, dOrigin/dsx, -, dOrigin/dsy, -, dDirection/dsx, -, dDirection/dsy, -, lensU, -, lensV, -} -- what
        raytracer_amd.rays.footprints and camera_footprints() return -- or a torch tensor on the renderer's ROCm device, taken without a host copy behind
        torch.cuda.current_stream().  bokeh_shape: 0 circle, 1 hexagon, 2 square.  The table is copied.  A table with a word that is not finite, a zero
        direction or, under lens=True, a focalDistance that is not > 0 raises ValueError and leaves the previous source (plain, lens or the camera) in
        place.  It replaces a ray source and is replaced by one; set_ray_source(None) clears it; a resize drops it.  The camera of the pass constants is
        not read while it is set, their sample offset is; denoise(temporal=True), "VCM" and "Light Tracer" passes raise."""
        ctx = self._ray_source_context("set_lens_source")
        params = RtLensSourceParams(1 if lens else 0, int(bokeh_shape))
        self._set_source("set_lens_source", ctx, "rtgpu_set_lens_source", (table,), 32,
                         "the lens table must be an (H, W, 32) float32 NumPy array of the viewport's size (or a torch tensor)",
                         "the lens table must be an (H, W, 32) float32 tensor of the viewport's size", "tensor", C.byref(params))

    def ray_source_kind(self):
        """What the passes start from (rtgpu_get_ray_source_kind): 0 the camera, 1 a ray source, 2 a lens source."""
        kind = C.c_uint32(0)
        if not self.has_renderer or not self.device_context().value:
            return 0
        if rtgpu_lib().rtgpu_get_ray_source_kind(self.device_context(), C.byref(kind)) != 0:
            raise RuntimeError("rtgpu_get_ray_source_kind failed: %s" % (rtgpu_lib().rtgpu_last_error() or b"").decode())
        return int(kind.value)

    def _source_export(self, what, entry, words, params, device):
        if not isinstance(params, RtPassParams):
            raise TypeError("%s takes the RtPassParams of next_pass_params(camera), not %s" % (what, type(params).__name__))
        lib = rtgpu_lib()
        ctx = self._ray_source_context(what)
        if not device:
            out = np.zeros((self.height, self.width, words), dtype=np.float32)
            r = getattr(lib, entry)(ctx, C.byref(params), out.ctypes.data_as(C.c_void_p))
        else:
            import torch
            dev = torch.device("cuda", multi_info(ctx)["devices"][0])
            out = torch.empty((self.height, self.width, words), dtype=torch.float32, device=dev)
            r = _run_on_torch_stream(torch, self._query_streams, dev, (out,), lambda stream: getattr(lib, entry + "_async")(
                ctx, C.byref(params), C.c_void_p(out.data_ptr()), stream))
        if r != 0:
            err = (lib.rtgpu_last_error() or b"").decode()
            raise (ValueError if r == -1 else RuntimeError)("%s failed (%d): %s" % (what, r, err))
        return out

    def camera_footprints(self, params, device=False):
        """The camera of the pass `params` as a lens table (rtgpu_read_camera_footprints): an (H, W, 32) float32 array of RtLensRay entries -- the camera's
        origin and pinhole direction at params.sampleOffset, the direction's analytic change per unit sample offset, the camera's aperture, focal distance
        and lens axes -- or, device=True, a torch tensor on the renderer's ROCm device written on torch.cuda.current_stream().  Not a pass.  A camera
        with depth of field is accepted: set the table with lens=True and the camera's bokeh shape and a pass at the export's offset renders the camera's
        own frame bit for bit.  A variable barrel factor raises."""
        return self._source_export("camera_footprints", "rtgpu_read_camera_footprints", 32, params, device)

    def lens_source_rays(self, params, device=False):
        """The primary rays a pass with `params` would start from under the lens source that is set (rtgpu_read_lens_source_rays): jitter by
        params.sampleOffset, the lens draws of the pass's sampler and the degenerate-ray guard included, as an (H, W, 8) float32 array in set_ray_source's
        layout {origin xyz, 0, direction xyz (not normalised), 0}; device=True: a torch tensor.  Not a pass: nothing is walked."""
        ctx = self._ray_source_context("lens_source_rays")
        if host_lib().rth_viewport_upload_scene(self._h) != 0:   # (the lens draws take the scene's blue noise, as a pass's do)
            raise RuntimeError("the viewport's scene could not be uploaded: %s" % (rtgpu_lib().rtgpu_last_error() or b"").decode())
        return self._source_export("lens_source_rays", "rtgpu_read_lens_source_rays", 8, params, device)

    # ---- path records (include/rtgpu.h: rtgpu_record_paths) ------------------------------------------------------------------------------
    def record_paths(self, params, pixels, max_vertices=None):
        """The reference's PathDebugData hook for chosen pixels: the vertices of the path the pass `params` traces for each (x, y) of `pixels`
        (sum-buffer coordinates; a pixel may repeat).  Returns a list, in the order of `pixels`, of (vertices, termination_reason, radiance):
        vertices (n, 28) float32 as RtPathVertex lays them out (n = min(the path's vertex count, max_vertices); default: every vertex),
        termination_reason a PathTerminationReason value (PATH_TERMINATION_REASONS names them), radiance (3,) float32 = what the pass adds to the
        pixel.  `params` is an RtPassParams from next_pass_params(): recording it renders nothing and is not a pass, so record before or after
        render_pass_with(params) as you like.  A Camera is not accepted: next_pass_params() is the one place that advances the viewport's sample
        sequence, and a recording that drew from it would shift every later pass."""
        if not isinstance(params, RtPassParams):
            raise TypeError("record_paths takes the RtPassParams of next_pass_params(camera), not %s" % type(params).__name__)
        px = np.asarray(pixels)
        if px.size == 0:
            px = px.reshape(0, 2)
        if px.ndim != 2 or px.shape[1] != 2 or px.dtype.kind not in "iu":
            raise ValueError("pixels must be a sequence of integer (x, y) pairs")
        if (px < 0).any() or (px[:, 0] >= self.width).any() or (px[:, 1] >= self.height).any():
            raise ValueError("a pixel lies outside the %d x %d frame" % (self.width, self.height))
        capacity = int(params.maxRayDepth) + 1 if max_vertices is None else int(max_vertices)
        if capacity < 1:
            raise ValueError("max_vertices must be at least 1")
        if not self.has_renderer:
            raise RuntimeError("record_paths needs a renderer: call set_renderer first")
        ctx = self.device_context()
        if not ctx.value or host_lib().rth_viewport_upload_scene(self._h) != 0:
            raise RuntimeError("the viewport's renderer has no device context or its scene could not be uploaded: %s" % (rtgpu_lib().rtgpu_last_error() or b"").decode())
        n = int(px.shape[0])
        xy = np.ascontiguousarray(px, dtype=np.uint32)
        vertices = np.zeros((max(n, 1), capacity, 28), dtype=np.float32)
        infos = np.zeros((max(n, 1), 8), dtype=np.uint32)
        r = rtgpu_lib().rtgpu_record_paths(ctx, C.byref(params), xy.ctypes.data_as(C.c_void_p), C.c_uint32(n), C.c_uint32(capacity),
                                           vertices.ctypes.data_as(C.c_void_p), infos.ctypes.data_as(C.c_void_p))
        if r != 0:
            err = (rtgpu_lib().rtgpu_last_error() or b"").decode()
            raise (ValueError if r == -1 else RuntimeError)("record_paths failed (%d): %s" % (r, err))
        radiance = infos[:, 2:5].view(np.float32)
        return [(vertices[i, :min(int(infos[i, 0]), capacity)].copy(), int(infos[i, 1]), radiance[i].copy()) for i in range(n)]

    # ---- AOVs (include/rtgpu.h: rtgpu_render_aovs / rtgpu_render_aovs_async) -------------------------------------------------------------
    def render_aovs(self, params, planes=("depth", "normal", "base_color"), device=False, chain=None):
        """What the primary ray of every pixel finds, as raw planes from one call: `planes` names them (AOV_PLANES: first-hit geometry, the
        evaluated material, ids, and the box / triangle tests of the traversal).  Returns a dict name -> array, (H, W) for a one-channel plane and
        (C, H, W) otherwise, row y as in sum_buffer(); float planes are float32, id and cost planes uint32.  device=True: torch tensors on the
        renderer's ROCm device, produced on torch.cuda.current_stream() without a host copy (ids and costs int64, as trace_rays returns them).
        `params` is an RtPassParams from next_pass_params(): the rays are those the pass would trace (the same lens samples), the call renders
        nothing and is not a pass.  A Camera is not accepted, for the reason record_paths gives.
        chain=N (0..16, rtgpu_render_aovs_chain): the planes at the guide vertex of every pixel's path instead -- the first vertex that is not a
        specular event of a mirror or glass material, at most N vertices in -- and the AOV_CHAIN_PLANES beside them; the cost planes have no chain
        form.  With chain=N the name "virtual_position" (AOV_VIRTUAL_PLANES, rtgpu_render_aovs_virtual) is accepted too: where the guide vertex
        appears to be along the primary ray, the point temporal accumulation reprojects inside a reflection.  chain=None is the first-hit call."""
        if not isinstance(params, RtPassParams):
            raise TypeError("render_aovs takes the RtPassParams of next_pass_params(camera), not %s" % type(params).__name__)
        names = [planes] if isinstance(planes, str) else list(planes)
        known = AOV_PLANES if chain is None else collections.OrderedDict(list(AOV_PLANES.items()) + list(AOV_CHAIN_PLANES.items()) + list(AOV_VIRTUAL_PLANES.items()))
        for name in names:
            if name not in known:
                if name in AOV_CHAIN_PLANES or name in AOV_VIRTUAL_PLANES:
                    raise ValueError("AOV plane %r needs chain=N" % (name,))
                raise ValueError("unknown AOV plane %r (AOV_PLANES lists them)" % (name,))
        if chain is not None:
            chain_desc = RtAovChain(int(chain), 0)
            # the virtual entry only where its plane is asked for
            chain_entry = "rtgpu_render_aovs_virtual" if any(name in AOV_VIRTUAL_PLANES for name in names) else "rtgpu_render_aovs_chain"
        if not self.has_renderer:
            raise RuntimeError("render_aovs needs a renderer: call set_renderer first")
        ctx = self.device_context()
        if not ctx.value or host_lib().rth_viewport_upload_scene(self._h) != 0:
            raise RuntimeError("the viewport's renderer has no device context or its scene could not be uploaded: %s" % (rtgpu_lib().rtgpu_last_error() or b"").decode())
        lib = rtgpu_lib()
        n = len(names)
        ids = (C.c_uint32 * max(n, 1))(*[known[name][0] for name in names])
        h, w = self.height, self.width
        shape = lambda name: (h, w) if known[name][1] == 1 else (known[name][1], h, w)   # noqa: E731
        if not device:
            out = collections.OrderedDict((name, np.zeros(shape(name), dtype=known[name][2])) for name in names)
            ptrs = (C.c_void_p * max(n, 1))(*[out[name].ctypes.data for name in names])
            if chain is None:
                r = lib.rtgpu_render_aovs(ctx, C.byref(params), ids, C.c_uint32(n), ptrs)
            else:
                r = getattr(lib, chain_entry)(ctx, C.byref(params), C.byref(chain_desc), ids, C.c_uint32(n), ptrs)
        else:
            import torch
            dev = torch.device("cuda", multi_info(ctx)["devices"][0])
            raw = collections.OrderedDict((name, torch.empty(shape(name), dtype=torch.float32 if known[name][2] is np.float32 else torch.int32, device=dev))
                                          for name in names)
            ptrs = (C.c_void_p * max(n, 1))(*[raw[name].data_ptr() for name in names])
            if chain is None:
                r = _run_on_torch_stream(torch, self._query_streams, dev, raw.values(), lambda stream: lib.rtgpu_render_aovs_async(ctx, C.byref(params), ids, C.c_uint32(n), ptrs, stream))
            else:
                r = _run_on_torch_stream(torch, self._query_streams, dev, raw.values(),
                                         lambda stream: getattr(lib, chain_entry + "_async")(ctx, C.byref(params), C.byref(chain_desc), ids, C.c_uint32(n), ptrs, stream))
        if r != 0:
            err = (lib.rtgpu_last_error() or b"").decode()
            raise (ValueError if r == -1 else RuntimeError)("render_aovs failed (%d): %s" % (r, err))
        if device:
            out = collections.OrderedDict((name, t if t.dtype == torch.float32 else _u32(torch, t)) for name, t in raw.items())
        return out

    def set_guide_chain(self, chain):
        """chain=N (0..16): denoise() and denoise(variance=True) render their guides through render_aovs(chain=N) -- the surface seen in a mirror or through
        glass steers the filter, not the mirror (rtgpu_set_guide_chain).  None: first hit, the default.  While a chain is set, denoise(temporal=True)
        raises: the call that reprojects a reflection takes its chain as an argument, denoise(temporal=True, chain=N)."""
        ctx = self.device_context()
        desc = RtAovChain(int(chain), 0) if chain is not None else None
        if not ctx.value:
            raise RuntimeError("set_guide_chain needs a renderer with a device context: call set_renderer first")
        r = rtgpu_lib().rtgpu_set_guide_chain(ctx, C.byref(desc) if desc is not None else None)
        if r != 0:
            raise (ValueError if r == -1 else RuntimeError)("set_guide_chain failed (%d): %s" % (r, (rtgpu_lib().rtgpu_last_error() or b"").decode()))

    # ---- denoise (include/rtgpu.h: rtgpu_denoise / rtgpu_denoise_async, rtgpu_postprocess_from) ------------------------------------------------------
    def denoise(self, params, iterations=5, sigma_color=DENOISE_DEFAULTS["sigma_color"], sigma_normal=DENOISE_DEFAULTS["sigma_normal"],
                sigma_plane=DENOISE_DEFAULTS["sigma_plane"], color_scale=None, demodulate=True, device=False, variance=False,
                sigma_lum=DENOISE_VAR_DEFAULTS["sigma_lum"], variance_floor=DENOISE_VAR_DEFAULTS["variance_floor"], return_variance=False, temporal=False,
                alpha_min=TEMPORAL_DEFAULTS["alpha_min"], max_history=TEMPORAL_DEFAULTS["max_history"], normal_threshold=TEMPORAL_DEFAULTS["normal_threshold"],
                plane_tolerance=TEMPORAL_DEFAULTS["plane_tolerance"], clip=None, return_confidence=False, chain=None):
        """The frame rendered so far through the a-trous filter of include/rtgpu.h, guided by the depth, normal, position and base-colour planes of the pass
        `params` (an RtPassParams from next_pass_params(), as render_aovs takes it): the (H, W, 3) float32 image, sum_buffer() * color_scale filtered.
        color_scale defaults to 1 / max(1, passes_finished).  device=True: a torch tensor on the renderer's ROCm device, produced on
        torch.cuda.current_stream() without a host copy.  The call is not a pass: film, sum buffers and counters stay as they are.
        variance=True: the variance-guided filter (rtgpu_denoise_var) over the sum and the secondary sum buffer, with sigma_lum and variance_floor in
        sigma_color's place; return_variance=True then returns (image, the (H, W) variance of the filtered luminance).
        temporal=True (rtgpu_denoise_temporal): the frame is first accumulated against the history the renderer keeps from the previous such call --
        reprojected through that call's camera, with alpha_min, max_history, normal_threshold and plane_tolerance -- and becomes the next call's history;
        variance=True then filters the accumulated pair, variance=False returns the accumulated frame unfiltered.  reset() keeps the history (a moving
        camera resets the film every frame); reset_history(), a resize and a new scene drop it.  The reprojection reads params.camera.worldToScreen, which
        Camera.set_perspective computes from the transform of the moment (as the reference's Camera does): after Camera.set_transform call set_perspective again,
        or the history is looked up through the camera's old place.
        clip=True or a dict (temporal_clip), with temporal=True: the history is clipped to this frame's local colour statistics (rtgpu_denoise_temporal_clip) --
        the remedy for lighting that changed under a surface; clip=None is the call without, word for word.  return_confidence=True then appends the (H, W)
        confidence plane to what is returned.
        chain=N (0..16), with temporal=True (rtgpu_denoise_temporal_chain): the guides are the chain guides render_aovs(chain=N) renders and the history is
        reprojected through mirrors and glass by the virtual position; with or without clip.  The chain is this call's own: set_guide_chain does not affect it.
        chain=None is the call without, word for word -- its refusal under set_guide_chain included.
        After track_deformation() the call (without chain) follows meshes deformed since the last such call: their pixels keep their history."""
        clip = temporal_clip(clip)
        if chain is not None and not temporal:
            raise ValueError("chain needs temporal=True (set_guide_chain steers the calls without a history)")
        if clip is not None and not temporal:
            raise ValueError("clip needs temporal=True")
        if return_confidence and clip is None:
            raise ValueError("return_confidence=True needs clip")
        if return_variance and not variance:
            raise ValueError("return_variance=True needs variance=True")
        if not isinstance(params, RtPassParams):
            raise TypeError("denoise takes the RtPassParams of next_pass_params(camera), not %s" % type(params).__name__)
        if not self.has_renderer:
            raise RuntimeError("denoise needs a renderer: call set_renderer first")
        ctx = self.device_context()
        if not ctx.value or host_lib().rth_viewport_upload_scene(self._h) != 0:
            raise RuntimeError("the viewport's renderer has no device context or its scene could not be uploaded: %s" % (rtgpu_lib().rtgpu_last_error() or b"").decode())
        scale = 1.0 / max(1, self.passes_finished) if color_scale is None else color_scale
        # the entry (its _async sibling with device=True) and the arguments in front of the guide params; rtgpu_denoise alone takes no outVariance behind outRGB
        if temporal:
            t = temporal_params(alpha_min, max_history, normal_threshold, plane_tolerance, scale, demodulate)
            v = denoise_var_params(iterations, sigma_lum, sigma_normal, sigma_plane, variance_floor, 1.0, demodulate) if variance else None
            entry, leading = "rtgpu_denoise_temporal", (C.byref(t), C.byref(v) if variance else None)
        elif variance:
            p = denoise_var_params(iterations, sigma_lum, sigma_normal, sigma_plane, variance_floor, scale, demodulate)
            entry, leading = "rtgpu_denoise_var", (C.byref(p),)
        else:
            p = denoise_params(iterations, sigma_color, sigma_normal, sigma_plane, scale, demodulate)
            entry, leading = "rtgpu_denoise", (C.byref(p),)
        lib = rtgpu_lib()
        if not device:
            empty = lambda *shape: np.zeros(shape, dtype=np.float32)   # noqa: E731
            ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
        else:
            import torch
            dev = torch.device("cuda", multi_info(ctx)["devices"][0])
            empty = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
            ptr = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None   # noqa: E731
        out, out_variance = empty(self.height, self.width, 3), empty(self.height, self.width) if return_variance else None
        out_confidence = empty(self.height, self.width) if return_confidence else None
        args = (ctx,) + leading + (C.byref(params), ptr(out)) + ((ptr(out_variance),) if temporal or variance else ())
        if chain is not None:
            chain_desc = RtAovChain(int(chain), 0)
            entry, args = "rtgpu_denoise_temporal_chain", (ctx,) + leading + (C.byref(params), C.byref(chain_desc), ptr(out), ptr(out_variance),
                                                                                C.byref(clip) if clip is not None else None, ptr(out_confidence))
        elif clip is not None:
            entry, args = "rtgpu_denoise_temporal_clip", args + (C.byref(clip), ptr(out_confidence))
        if not device:
            r = getattr(lib, entry)(*args)
        else:
            r = _run_on_torch_stream(torch, self._denoise_streams, dev, [out, out_variance, out_confidence], lambda stream: getattr(lib, entry + "_async")(*(args + (stream,))))
        if r != 0:
            err = (lib.rtgpu_last_error() or b"").decode()
            raise (ValueError if r == -1 else RuntimeError)("denoise failed (%d): %s" % (r, err))
        extras = ((out_variance,) if return_variance else ()) + ((out_confidence,) if return_confidence else ())
        return (out,) + extras if extras else out

    def reset_history(self):
        """Drops the history of denoise(temporal=True) (rtgpu_temporal_reset): the next such call starts every pixel."""
        ctx = self.device_context()
        if ctx.value and rtgpu_lib().rtgpu_temporal_reset(ctx) != 0:
            raise RuntimeError("reset_history failed: %s" % (rtgpu_lib().rtgpu_last_error() or b"").decode())

    def front_buffer_from(self, image, exposure=0.0, contrast=0.8, saturation=0.98, dithering=0.005, tonemapper=3, color_filter=(1.0, 1.0, 1.0, 1.0),
                          dither_seed=0, bloom=0.0, num_passes=1):
        """front_buffer() over `image`, an (H, W, 3) float32 array of the viewport's size, in place of the sum buffer: the tone-mapped (H, W) uint32
        0x00RRGGBB picture of a denoised frame, say.  num_passes scales as front_buffer's pass count does (1: the image is already averaged)."""
        if not isinstance(image, np.ndarray) or image.dtype != np.float32 or image.shape != (self.height, self.width, 3):
            raise ValueError("image must be an (H, W, 3) float32 NumPy array of the viewport's size")
        p = RtPostprocessParams()
        for k in range(4):
            p.colorFilter[k] = color_filter[k]
        p.exposure, p.contrast, p.saturation, p.ditheringStrength, p.bloomFactor = exposure, contrast, saturation, dithering, bloom
        p.tonemapper, p.numPasses, p.ditherSeed = int(tonemapper), max(1, int(num_passes)), int(dither_seed)
        image = np.ascontiguousarray(image)
        out = np.zeros((self.height, self.width), dtype=np.uint32)
        if rtgpu_lib().rtgpu_postprocess_from(self.device_context(), C.byref(p), image.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError("postprocess failed: %s" % (rtgpu_lib().rtgpu_last_error() or b"").decode())
        return out

    @property
    def passes_finished(self):
        return int(host_lib().rth_viewport_passes_finished(self._h))
