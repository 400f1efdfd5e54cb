"""Scenes shared by the CPU (oracle-only) and GPU parity tests."""
import numpy as np

import raytracer_amd as ra
from raytracer_amd import scenes


def all_lights_scene(aspect):
    """Every light type + every BSDF on analytic shapes (LightSamplingStrategy::All friendly)."""
    s = ra.Scene()
    mats = {name: s.add_material(name, (0.8, 0.6, 0.4) if i % 2 else (0.3, 0.7, 0.9), roughness=0.05 + 0.1 * i, ior=1.3 + 0.05 * i)
            for i, name in enumerate(ra.BSDF_NAMES) if name != "null"}
    emissive = s.add_material("null", (0.0, 0.0, 0.0), emission=(0.5, 0.25, 0.125))
    names = list(mats)
    k = 0
    for iz in range(3):
        for ix in range(3):
            t = ra.transform_from_euler((-3.0 + 3.0 * ix, -1.0, -3.0 + 3.0 * iz), (10.0 * ix, 25.0 * iz, 5.0))
            if k % 2 == 0:
                s.add_sphere(0.9, t, mats[names[k % len(names)]])
            else:
                s.add_box((0.7, 0.9, 0.6), t, mats[names[k % len(names)]])
            k += 1
    s.add_rect((8.0, 8.0), ra.transform_from_euler((0.0, -2.0, 0.0), (-90.0, 0.0, 0.0)), mats["diffuse"])
    s.add_sphere(0.4, ra.transform_from_euler((0.0, 1.5, 0.0)), emissive)
    s.add_area_light("rect", [1.0, 0.5], (6.0, 6.0, 6.0), ra.transform_from_euler((0.0, 4.0, 0.0), (90.0, 0.0, 0.0)))
    s.add_area_light("sphere", [0.5], (4.0, 2.0, 1.0), ra.transform_from_euler((3.5, 2.0, 1.0)))
    s.add_area_light("box", [0.3, 0.2, 0.4], (1.0, 3.0, 5.0), ra.transform_from_euler((-3.5, 2.5, -1.0), (20.0, 30.0, 0.0)))
    s.add_point_light((20.0, 18.0, 15.0), ra.transform_from_euler((2.0, 3.0, -3.0)))
    s.add_spot_light((40.0, 40.0, 60.0), 0.6, ra.transform_from_euler((-2.0, 3.5, 3.0), (0.0, 0.0, 0.0)))
    s.add_directional_light((2.0, 2.0, 1.5), 0.1, ra.transform_from_euler((0.0, 0.0, 0.0), (60.0, 30.0, 0.0)))
    s.add_directional_light((3.0, 2.5, 2.0), 0.001, ra.transform_from_euler((0.0, 0.0, 0.0), (70.0, -40.0, 0.0)))
    s.add_background_light((0.2, 0.3, 0.5))
    s.build()
    cam = ra.Camera((0.5, 2.5, 9.0), (12.0, 180.0, 0.0), aspect, 55.0)
    return s, cam


def edge_materials_scene(aspect):
    """Materials and lights on the branch boundaries tests/golden/edges pins per function, for the shading kernels' own compilation of them:
    roughness exactly SpecularEventRoughnessTreshold = 0.005 (the rough lobe) and its lower neighbour (the specular fall-back) on a rough
    metal, a rough dielectric and a rough plastic; a dielectric with IoR = 1; a metal with IoR = 0, K = 0; a sphere light of radius 0.01 at
    distance > 9 from every surface (cosThetaMax > 0.999999: the FLT_MAX pdf branch of SphereShape::Sample); a rect light coplanar with the
    back wall (cosNormalDir = 0 from the wall, grazing from the floor next to it)."""
    s = ra.Scene()
    threshold = np.float32(0.005)
    below = np.nextafter(threshold, np.float32(0.0))
    white = s.add_material("diffuse", (0.8, 0.8, 0.8))
    kinds = [("roughMetal", dict(roughness=float(threshold), ior=0.2, k=3.0)), ("roughMetal", dict(roughness=float(below), ior=0.2, k=3.0)),
             ("roughDielectric", dict(roughness=float(threshold))), ("roughDielectric", dict(roughness=float(below))),
             ("roughPlastic", dict(roughness=float(threshold))), ("roughPlastic", dict(roughness=float(below))),
             ("dielectric", dict(ior=1.0)), ("metal", dict(ior=0.0, k=0.0))]
    for i, (bsdf, args) in enumerate(kinds):
        m = s.add_material(bsdf, (0.9, 0.7, 0.5) if i % 2 else (0.5, 0.7, 0.9), **args)
        x, z = -3.0 + 2.0 * (i % 4), -1.0 + 2.0 * (i // 4)
        if i % 3 == 2:
            s.add_box((0.6, 0.6, 0.6), ra.transform_from_euler((x, -1.4, z), (0.0, 20.0, 0.0)), m)
        else:
            s.add_sphere(0.6, ra.transform_from_euler((x, -1.4, z)), m)
    s.add_rect((6.0, 6.0), ra.transform_from_euler((0.0, -2.0, 0.0), (-90.0, 0.0, 0.0)), white)        # floor
    s.add_rect((6.0, 4.0), ra.transform_from_euler((0.0, 2.0, -3.0), (0.0, 0.0, 0.0)), white)          # back wall, facing +z
    s.add_area_light("rect", [2.0, 1.0], (6.0, 5.0, 4.0), ra.transform_from_euler((0.0, 1.0, -3.0), (0.0, 0.0, 0.0)))   # in the wall's plane
    s.add_area_light("sphere", [0.01], (4.0e5, 4.0e5, 3.0e5), ra.transform_from_euler((1.0, 9.0, 2.0)))
    s.build()
    cam = ra.Camera((0.3, 1.5, 8.0), (14.0, 180.0, 0.0), aspect, 50.0)
    return s, cam


def mesh_scene(aspect, triangles=20000, with_analytic=True):
    """Sponza-class mesh (small) + a few analytic instances so that both BVH levels are exercised."""
    pos, idx, nrm, tan, uv, mat = scenes.sponza_class_mesh(triangles, seed=5)
    s = ra.Scene()
    mats = [s.add_material("diffuse", c) for _, c in scenes.SPONZA_MATERIALS]
    s.add_mesh(pos, idx, nrm, tan, uv, mat, mats)
    if with_analytic:
        glass = s.add_material("dielectric", (1.0, 1.0, 1.0))
        metal = s.add_material("roughMetal", (0.9, 0.8, 0.6), roughness=0.3)
        s.add_sphere(1.2, ra.transform_from_euler((-4.0, 1.2, 0.5)), glass)
        s.add_box((0.8, 1.5, 0.8), ra.transform_from_euler((3.0, 1.5, -1.0), (0.0, 30.0, 0.0)), metal)
        s.add_area_light("rect", [1.5, 1.5], (30.0, 28.0, 25.0), ra.transform_from_euler((0.0, 11.0, 0.0), (90.0, 0.0, 0.0)))
    s.add_background_light((1.0, 1.5, 2.0))
    s.add_directional_light((20000.0, 19000.0, 18000.0), np.float32(1.0) / np.float32(180.0) * np.float32(3.14159265359),
                            ra.transform_from_euler((0.0, 0.0, 0.0), (80.0, 20.0, 0.0)))
    s.build()
    cam = ra.Camera((-12.5, 2.2, 0.6), (4.0, 82.0, 0.0), aspect, 65.0)
    return s, cam


def textured_scene(aspect, triangles=6000, seed=11, skip=()):
    """Textures on every slot of the shading path: a mesh whose 8 materials carry bitmap base-colour / roughness /
    metalness / emission textures in different texel formats, colour spaces and filters, normal maps (bitmap and
    checkerboard), analytic shapes with checkerboard / const textures, and an HDR environment map on the background
    light (BackgroundLight::mTexture)."""
    rng = np.random.RandomState(seed)
    pos, idx, nrm, tan, uv, mat = scenes.sponza_class_mesh(triangles, seed=5)
    s = ra.Scene()

    def rgba8(h, w):
        return rng.randint(0, 256, size=(h, w, 4)).astype(np.uint8)

    t_albedo = s.add_bitmap_texture(rgba8(32, 48), "B8G8R8A8_UNorm", linear_space=False, filter="smoothstep")
    t_albedo2 = s.add_bitmap_texture(rng.randint(0, 256, size=(7, 5, 3)).astype(np.uint8), "B8G8R8_UNorm", linear_space=False, filter="bilinear")
    t_rough = s.add_bitmap_texture(rng.randint(0, 256, size=(16, 16)).astype(np.uint8), "R8_UNorm", filter="nearest")
    t_metal = s.add_bitmap_texture(rng.randint(0, 65536, size=(9, 13)).astype(np.uint16), "R16_UNorm", filter="bilinear")
    t_emit = s.add_bitmap_texture(rng.uniform(0.0, 1.0, size=(8, 8, 3)).astype(np.float32), "R32G32B32_Float", filter="smoothstep")
    nm = rng.uniform(0.35, 0.65, size=(24, 24, 4)).astype(np.float32)
    t_normal = s.add_bitmap_texture(nm, "R32G32B32A32_Float", filter="smoothstep")
    t_normal_h = s.add_bitmap_texture(rng.uniform(0.3, 0.7, size=(12, 10, 2)).astype(np.float16), "R16G16_Half", filter="bilinear")
    t_check = s.add_checkerboard_texture((0.9, 0.2, 0.1), (0.1, 0.3, 0.9, 1.0))
    t_const = s.add_const_texture((0.5, 0.75, 1.0, 0.0))
    t_noise = s.add_noise_texture((0.9, 0.8, 0.7), (0.2, 0.1, 0.4), octaves=4)
    t_mix = s.add_mix_texture(t_albedo, t_check, t_noise)
    bc1 = rng.randint(0, 256, size=(16 // 4) * (8 // 4) * 8).astype(np.uint8)
    t_bc1 = s.add_bitmap_texture(bc1, "BC1", linear_space=False, filter="bilinear", size=(16, 8))
    env = rng.uniform(0.0, 3.0, size=(16, 32, 4)).astype(np.float16)
    t_env = s.add_bitmap_texture(env, "R16G16B16A16_Half", filter="smoothstep")

    kinds = ["diffuse", "roughDiffuse", "roughPlastic", "roughMetal", "diffuse", "plastic", "roughDielectric", "diffuse"]
    mats = []
    for i, (_, c) in enumerate(scenes.SPONZA_MATERIALS):
        m = s.add_material(kinds[i], c, roughness=0.4, metalness=0.3 if i == 3 else 0.0,
                           emission=(0.6, 0.5, 0.4) if i == 5 else (0.0, 0.0, 0.0))
        mats.append(m)
    if 0 not in skip: s.set_material_texture(mats[0], "baseColor", t_albedo)
    if 1 not in skip: s.set_material_texture(mats[0], "normal", t_normal, 0.8)
    if 2 not in skip: s.set_material_texture(mats[1], "baseColor", t_albedo2)
    if 3 not in skip: s.set_material_texture(mats[1], "roughness", t_rough)
    if 4 not in skip: s.set_material_texture(mats[2], "roughness", t_rough)
    if 5 not in skip: s.set_material_texture(mats[2], "baseColor", t_check)
    if 6 not in skip: s.set_material_texture(mats[3], "metalness", t_metal)
    if 7 not in skip: s.set_material_texture(mats[3], "normal", t_normal_h, 1.0)
    if 8 not in skip: s.set_material_texture(mats[4], "normal", t_check, 0.5)
    if 9 not in skip: s.set_material_texture(mats[5], "emission", t_emit)
    if 10 not in skip: s.set_material_texture(mats[6], "roughness", t_metal)
    if 11 not in skip: s.set_material_texture(mats[7], "baseColor", t_const)
    if 15 not in skip: s.set_material_texture(mats[4], "baseColor", t_mix)
    if 16 not in skip: s.set_material_texture(mats[6], "baseColor", t_bc1)
    if 17 not in skip: s.set_material_texture(mats[5], "roughness", t_noise)
    s.add_mesh(pos, idx, nrm, tan, uv, mat, mats)

    ball = s.add_material("roughPlastic", (0.8, 0.8, 0.8), roughness=0.3)
    if 12 not in skip: s.set_material_texture(ball, "baseColor", t_check)
    if 13 not in skip: s.set_material_texture(ball, "normal", t_normal, 1.0)
    s.add_sphere(1.2, ra.transform_from_euler((-4.0, 1.2, 0.5)), ball)
    crate = s.add_material("diffuse", (1.0, 1.0, 1.0))
    if 14 not in skip: s.set_material_texture(crate, "baseColor", t_albedo)
    s.add_box((0.8, 1.5, 0.8), ra.transform_from_euler((3.0, 1.5, -1.0), (0.0, 30.0, 0.0)), crate)
    s.add_area_light("rect", [1.5, 1.5], (30.0, 28.0, 25.0), ra.transform_from_euler((0.0, 11.0, 0.0), (90.0, 0.0, 0.0)))
    s.add_background_light((1.0, 1.2, 1.5), texture=None if 'env' in skip else t_env)
    s.build()
    cam = ra.Camera((-12.5, 2.2, 0.6), (4.0, 82.0, 0.0), aspect, 65.0)
    return s, cam


def many_lights_scene(aspect, num_point_lights=14):
    """More than 8 lights (under LightSamplingStrategy::All the NEE requests past the eighth take the per-lane append
    path of k_shade), some of them black (zero radiance: no shadow ray), a one-triangle mesh and a mesh-free object."""
    s = ra.Scene()
    grey = s.add_material("roughDiffuse", (0.7, 0.7, 0.7), roughness=0.4)
    s.add_rect((6.0, 6.0), ra.transform_from_euler((0.0, -1.0, 0.0), (-90.0, 0.0, 0.0)), grey)
    s.add_sphere(0.8, ra.transform_from_euler((0.0, -0.2, 0.0)), s.add_material("plastic", (0.9, 0.3, 0.2)))
    pos = np.array([[-2.0, -0.9, 1.0], [2.0, -0.9, 1.0], [0.0, 1.5, -1.5]], dtype=np.float32)
    s.add_mesh(pos, np.array([[0, 1, 2]], dtype=np.uint32), None, None, None, None, [], default_material=grey)
    for i in range(num_point_lights):
        a = 2.0 * np.pi * i / num_point_lights
        color = (0.0, 0.0, 0.0) if i % 5 == 4 else (3.0 + i, 4.0, 12.0 - 0.5 * i)
        s.add_point_light(color, ra.transform_from_euler((3.0 * np.cos(a), 2.0 + 0.1 * i, 3.0 * np.sin(a))))
    s.add_area_light("sphere", [0.3], (5.0, 5.0, 4.0), ra.transform_from_euler((0.0, 3.0, 0.0)))
    s.add_background_light((0.05, 0.06, 0.08))
    s.build()
    return s, ra.Camera((0.0, 1.5, 7.0), (8.0, 180.0, 0.0), aspect, 50.0)


def _look_at_euler(position, target=(0.0, 0.0, 0.0)):
    """Euler angles (degrees, the JSON convention of the reference's cameras: yaw 180 looks down -z, positive pitch looks down) that point a camera at `target`."""
    f = np.asarray(target, np.float64) - np.asarray(position, np.float64)
    f /= np.linalg.norm(f)
    return float(np.degrees(np.arcsin(-f[1]))), float(np.degrees(np.arctan2(f[0], f[2]))), 0.0


def bumpy_patch(rng, n):
    """A height-field patch of 2 n^2 triangles with vertex normals, tangents and texture coordinates (a mesh whose triangles are in general position)."""
    g = np.linspace(-1.0, 1.0, n + 1)
    x, z = np.meshgrid(g, g, indexing="xy")
    a, b, c = rng.uniform(1.0, 4.0, size=3)
    y = 0.25 * np.sin(a * x + 0.3) * np.cos(b * z) + 0.1 * np.sin(c * (x + z)) + rng.uniform(-0.02, 0.02, size=x.shape)
    pos = np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.float32)
    dy_dx = np.gradient(y, g, axis=1); dy_dz = np.gradient(y, g, axis=0)
    nrm = np.stack([-dy_dx, np.ones_like(y), -dy_dz], axis=-1).reshape(-1, 3)
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    tan = np.stack([np.ones_like(y), dy_dx, np.zeros_like(y)], axis=-1).reshape(-1, 3)
    tan = (tan / np.linalg.norm(tan, axis=1, keepdims=True)).astype(np.float32)
    uv = np.stack([(x + 1.0) * 0.5, (z + 1.0) * 0.5], axis=-1).reshape(-1, 2).astype(np.float32)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="xy")
    v0 = (j * (n + 1) + i).reshape(-1); v1 = v0 + 1; v2 = v0 + (n + 1); v3 = v2 + 1
    idx = np.concatenate([np.stack([v0, v2, v1], axis=1), np.stack([v1, v2, v3], axis=1)]).astype(np.uint32)
    return pos, idx, nrm, tan, uv


def random_scene(aspect, seed):
    """A scene drawn from `seed` alone: 3..8 materials over all BSDFs with random parameters, 4..13 analytic shapes and 0..2 bumpy mesh patches under GENERAL rotations,
    a floor, 1..4 lights of random type, transform and parameters, a camera somewhere on a shell around it; in a third of the scenes bitmap textures on random material
    slots (normal maps too) and possibly an environment map.  The fixed scenes of the soaks hold translations and quarter
    turns almost everywhere; the host mirror's differently-rounded matrix inverse (round 6) hid behind exactly that."""
    rng = np.random.RandomState(seed)
    s = ra.Scene()

    def colour(lo=0.05, hi=0.95):
        return tuple(float(v) for v in rng.uniform(lo, hi, size=3))

    def pose(spread=(5.0, 2.5, 5.0), lift=0.5):
        t = (float(rng.uniform(-spread[0], spread[0])), float(lift + rng.uniform(-spread[1], spread[1])), float(rng.uniform(-spread[2], spread[2])))
        r = tuple(float(v) for v in rng.uniform(-180.0, 180.0, size=3)) if rng.randint(5) else (0.0, float(90.0 * rng.randint(4)), 0.0)
        return ra.transform_from_euler(t, r)

    names = [n for n in ra.BSDF_NAMES if n != "null"]
    mats = []
    for _ in range(rng.randint(3, 9)):
        emission = colour(0.0, 0.6) if rng.randint(6) == 0 else (0.0, 0.0, 0.0)
        mats.append(s.add_material(names[rng.randint(len(names))], colour(), emission, roughness=float(rng.choice([0.0, 0.02, rng.uniform(0.03, 1.0)])),
                                   metalness=float(rng.uniform(0.0, 1.0)), ior=float(rng.uniform(1.05, 2.2)), k=float(rng.uniform(0.5, 6.0))))
    if rng.randint(4) == 0:
        mats.append(s.add_material("null", (0.0, 0.0, 0.0), emission=colour(0.1, 0.8)))
    floor = s.add_material("diffuse" if rng.randint(2) else "roughPlastic", colour(0.3, 0.8), roughness=float(rng.uniform(0.05, 0.6)))
    mats_all = mats + [floor]
    # bitmap textures (a draw of their own: geometry, lights and camera of a seed do not depend on it): in a third of the scenes 1..4 bitmaps of assorted texel formats
    # on random slots of random materials -- normal maps among them (Scene.cpp:328-337, the rsqrt site) -- and possibly an environment map for a background light.
    # Default filter, no palette: what the reference's public constructor gives and tests/ref_render.py exports.
    trng = np.random.RandomState((seed * 2654435761 + 12345) % (1 << 31))
    env_map = None
    if trng.randint(3) == 0:
        def bitmap():
            h, w = int(trng.randint(2, 40)), int(trng.randint(2, 40))
            fmt = ["R8G8B8A8_UNorm", "B8G8R8A8_UNorm", "B8G8R8_UNorm", "R8_UNorm", "R16_UNorm", "R32G32B32_Float", "R32G32B32A32_Float"][trng.randint(7)]
            if fmt in ("R8G8B8A8_UNorm", "B8G8R8A8_UNorm"): px = trng.randint(0, 256, size=(h, w, 4)).astype(np.uint8)
            elif fmt == "B8G8R8_UNorm": px = trng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
            elif fmt == "R8_UNorm": px = trng.randint(0, 256, size=(h, w)).astype(np.uint8)
            elif fmt == "R16_UNorm": px = trng.randint(0, 65536, size=(h, w)).astype(np.uint16)
            elif fmt == "R32G32B32_Float": px = trng.uniform(0.0, 1.0, size=(h, w, 3)).astype(np.float32)
            else: px = trng.uniform(0.0, 1.0, size=(h, w, 4)).astype(np.float32)
            return s.add_bitmap_texture(px, fmt, linear_space=bool(trng.randint(2)) or px.dtype != np.uint8)
        for _ in range(trng.randint(1, 5)):
            slot = ["baseColor", "emission", "roughness", "metalness", "normal", "normal"][trng.randint(6)]
            s.set_material_texture(mats_all[trng.randint(len(mats_all))], slot, bitmap(), strength=float(trng.uniform(0.2, 1.5)))
        if trng.randint(2):
            env_map = s.add_bitmap_texture(trng.uniform(0.0, 2.0, size=(int(trng.randint(2, 24)), int(trng.randint(2, 48)), 3)).astype(np.float32), "R32G32B32_Float")
    s.add_rect((12.0, 12.0), ra.transform_from_euler((0.0, -2.5, 0.0), (-90.0, float(rng.uniform(-180.0, 180.0)), 0.0)), floor)
    # a room around it in half of the scenes (a draw of its own again): closed scenes keep paths alive to the depth limit, open ones lose most rays to the sky
    rrng = np.random.RandomState((seed * 40503 + 977) % (1 << 31))
    room = None
    if rrng.randint(2):
        half, turn = float(rrng.uniform(7.0, 9.0)), float(rrng.uniform(-180.0, 180.0))
        room = half
        for t, r in (((0.0, 2.0 * half - 2.5, 0.0), (90.0, turn, 0.0)), ((half, half - 2.5, 0.0), (0.0, -90.0, 0.0)), ((-half, half - 2.5, 0.0), (0.0, 90.0, 0.0)),
                     ((0.0, half - 2.5, half), (0.0, 180.0, 0.0)), ((0.0, half - 2.5, -half), (0.0, 0.0, 0.0))):
            s.add_rect((half, half), ra.transform_from_euler(t, r), mats_all[rrng.randint(len(mats_all))])
    for _ in range(rng.randint(4, 14)):
        m = mats[rng.randint(len(mats))]
        kind = rng.randint(3)
        if kind == 0: s.add_sphere(float(rng.uniform(0.3, 1.4)), pose(), m)
        elif kind == 1: s.add_box(tuple(float(v) for v in rng.uniform(0.2, 1.3, size=3)), pose(), m)
        else: s.add_rect(tuple(float(v) for v in rng.uniform(0.4, 2.0, size=2)), pose(), m, tex_scale=tuple(float(v) for v in rrng.uniform(0.2, 3.0, size=2)))
    for _ in range(rng.randint(3)):
        pos, idx, nrm, tan, uv = bumpy_patch(rng, int(rng.choice([6, 14, 30])))
        pos = pos * np.float32(rng.uniform(1.0, 3.5))
        table = [mats[rng.randint(len(mats))] for _ in range(rng.randint(1, 4))]
        s.add_mesh(pos, idx, nrm, tan, uv, rng.randint(len(table), size=idx.shape[0]).astype(np.uint32), table, pose())
    for _ in range(rng.randint(1, 5)):
        kind = rng.randint(7)
        if kind == 0: s.add_area_light("rect", [float(rng.uniform(0.3, 1.5)), float(rng.uniform(0.3, 1.5))], colour(2.0, 12.0), pose((4.0, 1.0, 4.0), 4.0))
        elif kind == 1: s.add_area_light("sphere", [float(rng.uniform(0.15, 0.8))], colour(2.0, 10.0), pose((4.0, 1.0, 4.0), 3.0))
        elif kind == 2: s.add_area_light("box", [float(v) for v in rng.uniform(0.15, 0.6, size=3)], colour(1.0, 8.0), pose((4.0, 1.0, 4.0), 3.0))
        elif kind == 3: s.add_point_light(colour(8.0, 30.0), pose((4.0, 1.0, 4.0), 3.5))
        elif kind == 4: s.add_spot_light(colour(20.0, 80.0), float(rng.uniform(0.2, 1.2)), pose((4.0, 1.0, 4.0), 4.0))
        elif kind == 5: s.add_directional_light(colour(1.0, 4.0), float(rng.choice([0.001, 0.02, rng.uniform(0.03, 0.3)])), pose())
        else: s.add_background_light(colour(0.05, 0.8), texture=env_map)
    s.build()
    radius, height, turn = rng.uniform(7.0, 13.0), rng.uniform(-1.0, 6.0), rng.uniform(0.0, 2.0 * np.pi)
    if room is not None:
        radius = min(radius, room - 0.75)      # the camera stands inside the room
    position = (float(radius * np.sin(turn)), float(height), float(radius * np.cos(turn)))
    target = tuple(float(v) for v in rng.uniform(-1.5, 1.5, size=3))
    cam = ra.Camera(position, _look_at_euler(position, target), aspect, float(rng.uniform(35.0, 75.0)))
    return s, cam
