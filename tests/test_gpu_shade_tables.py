"""The launch-uniform tables of k_shade_dense read from LDS copies (raytracer_amd/csrc/rt_dense.inl, rt_device_state.h RT_STAGE_*): objects, meshes,
materials, lights and the seed rows of the batch's passes, staged per launch where they fit their capacities -- the scene's tables as a group
(8 objects, 8 meshes, 32 materials, 8 lights), and with them the seed rows (passes x dimensions, rounded up to four, within 2048 words) -- and read
from memory otherwise.  RTGPU_SHADE_STAGE=0 reads everything from memory.

Bar: that of tests/test_gpu_shade_records.py -- BIT-EXACT sum buffers and IDENTICAL ray counters against the CPU oracle.  A scene's oracle image
is computed once and compared with the render under the knob at 1 and at 0.  Small frames; dense path state throughout (the library's default)."""
import numpy as np
import pytest

import oracle_lib
import raytracer_amd as ra
from raytracer_amd import scenes
import scene_zoo
import test_gpu_parity as parity
import test_gpu_shade_records as records
import update_scenes as us

pytestmark = pytest.mark.gpu

# rt_device_state.h
MAX_OBJECTS, MAX_MATERIALS, MAX_LIGHTS, SEED_WORDS, DENSE_MAX_LIGHTS = 8, 32, 8, 2048, 7
KNOB = ("1", "0")
BLUE_NOISE = ra.load_blue_noise()


class Oracle:
    """sum, secondary and counters of the passes fed to it"""

    def __init__(self, w, h):
        self.w, self.h = w, h
        self.sum = np.zeros((h, w, 3), dtype=np.float32); self.secondary = np.zeros((h, w, 3), dtype=np.float32); self.counters = np.zeros(16, dtype=np.uint64)

    def render(self, scene, params):
        scene.desc.contents.blueNoise = BLUE_NOISE.ctypes.data
        oracle_lib.render_pass(scene.desc, params, self.w, self.h, self.sum, self.secondary, self.counters, threads=8)

    def named(self):
        return {n: int(self.counters[i]) for i, n in enumerate(ra.COUNTER_NAMES)}


def viewport(scene, w, h, seed, **vp_args):
    scene.desc.contents.blueNoise = BLUE_NOISE.ctypes.data
    vp = ra.Viewport(w, h, seed=seed, **vp_args)
    vp.set_renderer(scene)
    return vp


def assert_frame(vp, oracle):
    img, img2 = vp.sum_buffer(secondary=True)
    parity.assert_quant_identical(img, img2, vp.counters(), oracle.sum, oracle.secondary, oracle.named())


def check(scene, camera, w, h, passes, monkeypatch, seed=929, **vp_args):
    """`passes` passes in ONE batch under the knob at 1 (explicit per-pass constants, which also go through the oracle) and at 0 (one render call: the
    same seed gives the same constants).  Returns the oracle's counters."""
    monkeypatch.setenv("RTGPU_PASS_BATCH", str(max(passes, 1)))
    oracle = Oracle(w, h)
    for knob in KNOB:
        monkeypatch.setenv("RTGPU_SHADE_STAGE", knob)
        vp = viewport(scene, w, h, seed, **vp_args)
        if knob == KNOB[0]:
            for _ in range(passes):
                p = vp.next_pass_params(camera)
                vp.render_pass_with(p)
                oracle.render(scene, p)
        else:
            vp.render(camera, passes)
        assert_frame(vp, oracle)
    return oracle.named()


def test_a_wave_spans_several_passes(built, monkeypatch):
    """8 x 4 pixels, six passes in one batch, depth 8: 192 vertices at bounce 0, so each of the three waves holds vertices of two passes and the
    staged seed row differs from lane to lane."""
    w, h = 8, 4
    scene, camera = records.small_sponza(w / h)
    counters = check(scene, camera, w, h, 6, monkeypatch, max_ray_depth=8)
    assert counters["numShadowRays"] > 0


def strips(num_materials, lights, emissive=False):
    """A lean single-mesh scene: a floor of `num_materials` strips, a material each, and a wall behind them; `lights` of background, directional, point"""
    mb = scenes.MeshBuilder()
    width = 16.0 / num_materials
    for m in range(num_materials):
        mb.add_grid((-8.0 + m * width, 0.0, 8.0), (width, 0.0, 0.0), (0.0, 0.0, -16.0), 1, 2, m)
    mb.add_grid((-8.0, 0.0, -8.0), (16.0, 0.0, 0.0), (0.0, 6.0, 0.0), 2, 2, 0)
    pos, idx, nrm, tan, uv, mat = mb.arrays()
    scene = ra.Scene()
    mats = [scene.add_material("diffuse", (0.2 + 0.6 * ((7 * m) % num_materials) / num_materials, 0.5, 0.9 - 0.6 * m / num_materials),
                               emission=(0.3, 0.2, 0.1) if emissive and m % 3 == 0 else (0.0, 0.0, 0.0)) for m in range(num_materials)]
    scene.add_mesh(pos, idx, nrm, tan, uv, mat, mats)
    for kind in lights:
        if kind == "background": scene.add_background_light((1.0, 1.5, 2.0))
        elif kind == "directional": scene.add_directional_light((5.0, 5.0, 5.0), 0.02, records.SUN)
        else: scene.add_point_light((30.0, 20.0, 10.0), ra.transform_from_euler((1.0, 3.0, 0.5)))
    scene.build()
    return scene, ra.Camera((0.0, 3.0, 9.0), (20.0, 180.0, 0.0), 1.5, 60.0)


@pytest.mark.parametrize("materials", [MAX_MATERIALS, MAX_MATERIALS + 1])
def test_material_capacity(built, monkeypatch, materials):
    """exactly the staged material capacity, and one more: every table from memory"""
    scene, camera = strips(materials - 1, ("background", "directional"))   # (a scene holds its default material too)
    assert scene.desc.contents.numMaterials == materials
    counters = check(scene, camera, 48, 32, 2, monkeypatch, max_ray_depth=4)
    assert counters["numShadowRays"] > 0


@pytest.mark.parametrize("lights", [0, 1, 2])
def test_light_counts_under_single(built, monkeypatch, lights):
    """0 (no next event estimation: emissive strips light the scene), 1 (no light is drawn) and 2 lights (the per-pixel generator picks one)"""
    scene, camera = strips(6, ("background", "directional")[:lights], emissive=True)
    assert scene.desc.contents.numLights == lights
    counters = check(scene, camera, 48, 32, 2, monkeypatch, max_ray_depth=4)
    assert (counters["numShadowRays"] > 0) == (lights > 0)


def test_most_lights_under_all(built, monkeypatch):
    """LightSamplingStrategy::All with RT_DENSE_MAX_LIGHTS lights: every staged light record is read at every vertex"""
    w, h = 48, 32
    pos, idx, nrm, tan, uv, mat = scenes.sponza_class_mesh(600, 7, refine=True)
    scene = ra.Scene()
    scene.add_mesh(pos, idx, nrm, tan, uv, mat, [scene.add_material("diffuse", c) for _, c in scenes.SPONZA_MATERIALS])
    scene.add_background_light((1.0, 1.5, 2.0))
    scene.add_directional_light((20.0, 19.0, 18.0), 0.02, records.SUN)
    scene.add_point_light((30.0, 20.0, 10.0), ra.transform_from_euler((-8.0, 3.0, 0.5)))
    scene.add_point_light((10.0, 20.0, 30.0), ra.transform_from_euler((-4.0, 1.5, -0.5)))
    for k, angle in enumerate((0.08, 0.15, 0.3)):
        scene.add_spot_light((200.0, 150.0 + 50.0 * k, 100.0), angle, ra.transform_from_euler((-10.0 + 2.0 * k, 4.0, 0.6), (80.0, 30.0 * k, 0.0)))
    scene.build()
    assert scene.desc.contents.numLights == DENSE_MAX_LIGHTS
    camera = ra.Camera((-12.5, 2.2, 0.6), (4.0, 82.0, 0.0), w / h, 65.0)
    counters = check(scene, camera, w, h, 2, monkeypatch, max_ray_depth=4, light_sampling_all=True, dimensions=128)
    assert counters["numShadowRays"] > 2 * w * h and counters["numShadowRaysHit"] > 0


def instances(count):
    """a two-level lean scene: `count` mesh objects (12-triangle boxes, turned and spread over a ground box) under a background and a directional light"""
    scene = ra.Scene()
    pos, idx, nrm, tan, uv, mat = scenes.box_mesh(0.6)
    for k in range(count):
        mats = [scene.add_material("diffuse", (0.3 + 0.07 * k, 0.6, 0.8 - 0.07 * k)), scene.add_material("diffuse", (0.8, 0.4 + 0.05 * k, 0.3))]
        spot = (-4.0 + 2.0 * (k % 5), 0.6 if k else -0.6, -1.5 + 2.5 * (k // 5))
        scene.add_mesh(pos * (np.float32(12.0), np.float32(1.0), np.float32(12.0)) if k == 0 else pos, idx, nrm, tan, uv, mat, mats,
                       transform=ra.transform_from_euler(spot, (0.0, 17.0 * k, 0.0)))
    scene.add_background_light((1.0, 1.5, 2.0))
    scene.add_directional_light((5.0, 5.0, 5.0), 0.02, records.SUN)
    scene.build()
    return scene, ra.Camera((0.0, 3.5, 8.0), (22.0, 180.0, 0.0), 1.5, 60.0)


@pytest.mark.parametrize("objects", [2, MAX_OBJECTS, MAX_OBJECTS + 1])
def test_object_capacity(built, monkeypatch, objects):
    """two mesh objects (two-level: the object decides the mesh and the transform of every hit), exactly the staged object and mesh capacity, and one
    more (every table from memory)"""
    scene, camera = instances(objects)
    assert scene.desc.contents.numObjects == objects and scene.desc.contents.numMeshes == objects
    counters = check(scene, camera, 48, 32, 2, monkeypatch, max_ray_depth=4)
    assert counters["numShadowRays"] > 0 and counters["numShadowRaysHit"] > 0


@pytest.mark.parametrize("blue_noise", [True, False])
@pytest.mark.parametrize("dimensions,passes", [(2, 3), (64, 3), (128, 20)])
def test_dimensions(built, monkeypatch, dimensions, passes, blue_noise):
    """2 dimensions (a staged row of four words; most draws fall through to the per-pixel generator), the default 64, and 20 passes of 128: 2560 words, more
    than the seed rows' 2048 -- the seeds from memory, the tables staged.  Blue-noise dithering (bounce 0 reads the tile behind the staged seed) on and off."""
    assert (passes * dimensions > SEED_WORDS) == (dimensions == 128)
    w, h = (16, 8) if passes == 20 else (48, 32)
    scene, camera = records.small_sponza(w / h)
    counters = check(scene, camera, w, h, passes, monkeypatch, max_ray_depth=8, dimensions=dimensions, use_blue_noise=blue_noise)
    assert counters["numShadowRays"] > 0


_class_scenes = {}


def class_scene(name, aspect):
    if name not in _class_scenes:
        make = {"lean": lambda a: records.small_sponza(a), "simple-bitmaps": lambda a: scenes.sponza_class(a, 600, textured=True),
                "textured": lambda a: scenes.sponza_class(a, 600, textured=True, extra_texture=True), "cornell": scenes.cornell_box,
                "all-lights": scene_zoo.all_lights_scene, "mesh-and-shapes": lambda a: scene_zoo.mesh_scene(a, triangles=600)}[name]
        _class_scenes[name] = make(aspect)
    return _class_scenes[name]


@pytest.mark.parametrize("name", ["lean", "simple-bitmaps", "textured", "cornell", "all-lights", "mesh-and-shapes"])
def test_every_scene_class(built, monkeypatch, name):
    """The scene classes of k_shade_dense: the small Sponza-class mesh (1), its textured variants (4: plain bitmaps; 2: any texture), the Cornell box (3:
    two-level, untextured) and every light type and BSDF on analytic shapes (0).  The last two hold more objects than are staged; a mesh with two
    shapes and an area light (four objects, eleven materials, three lights) is the staged two-level scene with light objects."""
    w, h = 48, 32
    scene, camera = class_scene(name, w / h)
    d = scene.desc.contents
    assert (d.numObjects <= MAX_OBJECTS) == (name not in ("cornell", "all-lights"))
    counters = check(scene, camera, w, h, 3, monkeypatch, max_ray_depth=5)
    assert counters["numRays"] > 0


def test_a_scene_update_between_two_renders(built, monkeypatch):
    """The tables are copied per launch: after rtgpu_update_objects (Viewport.update_scene) the next frame of the same context is the oracle's frame of
    the updated scene.  A mesh, a sphere, a box and a rect light; the sphere and the box move.  (rtgpu_update_objects changes transforms alone -- it
    refuses an update that differs in another field, a default material included -- so the move is what this test can change.)"""
    w, h = 48, 32
    for knob in KNOB:
        monkeypatch.setenv("RTGPU_SHADE_STAGE", knob)
        scene, camera = scene_zoo.mesh_scene(w / h, triangles=600)
        vp = viewport(scene, w, h, 77, max_ray_depth=4)
        first = Oracle(w, h)
        for _ in range(2):
            p = vp.next_pass_params(camera)
            vp.render_pass_with(p)
            first.render(scene, p)
        assert_frame(vp, first)
        before = vp.sum_buffer()
        for index, transform in us.CASES["mesh"][1]:
            scene.set_object_transform(index, transform)
        scene.update()
        vp.update_scene()
        vp.reset()
        second = Oracle(w, h)
        for _ in range(2):
            p = vp.next_pass_params(camera)
            vp.render_pass_with(p)
            second.render(scene, p)
        assert_frame(vp, second)
        assert not np.array_equal(vp.sum_buffer(), before)   # the move shows
