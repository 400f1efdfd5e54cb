"""The case stream of the whole-frame integrators' soak (tools/vcm_fuzz.py): renderer "VCM" and renderer "Light Tracer" against the oracle's restatements
(oracle/rto_vcm.h) on random scenes, frame sizes and settings.  Like tools/oracle_fuzz_replay.py for the path tracer: the stream of a seed depends on the generator
alone, so any case can be listed, vetted on the CPU and replayed on its own.
   python tools/vcm_fuzz_replay.py <seed> list [max cases]           prints index + parameters of every case
   python tools/vcm_fuzz_replay.py <seed> oracle <index> [...]       the oracle alone (no GPU): finite words, energy, photons per pass, splats per pixel
   python tools/vcm_fuzz_replay.py <seed> <index> [<index> ...]      renders those cases on the device and the oracle; prints what differs
Test infrastructure (uses the oracle)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import raytracer_amd as ra
from raytracer_amd import scenes
import oracle_lib, scene_zoo

COMPARED = ("numRays", "numShadowRays", "numShadowRaysHit", "numPrimaryRays", "numRayBoxTests", "numPassedRayBoxTests", "numRayTriangleTests",
            "numPassedRayTriangleTests", "numMeshHits", "numAnalyticHits", "numShadowRayBoxTests", "numShadowRayTriangleTests")
NOT_INTERSECTION = ("numRays", "numShadowRays", "numShadowRaysHit", "numPrimaryRays", "numMeshHits", "numAnalyticHits")

SCENE_KINDS = ("random", "zoo", "two", "cornell", "mesh_scene", "sponza", "slab")
SIZES = ((1, 1), (7, 5), (33, 17), (61, 47), (64, 48), (96, 54))
# camera of each fixed scene: position, orientation, field of view, and how far the position is jittered along each axis
CAMERAS = {"zoo": ((0.5, 2.5, 9.0), (12.0, 180.0, 0.0), 55.0, (3.0, 1.5, 2.5)), "two": ((0.5, 2.5, 7.0), (15.0, 180.0, 0.0), 55.0, (2.0, 1.0, 2.0)),
           "cornell": ((0.0, 0.0, 6.0), (0.0, 180.0, 0.0), 40.0, (0.6, 0.6, 1.5)), "mesh_scene": ((-12.5, 2.2, 0.6), (4.0, 82.0, 0.0), 65.0, (2.0, 1.2, 2.0)),
           "slab": ((-2.4, 4.03, 3.49), (40.0, 158.0, 0.0), 45.0, (1.0, 1.0, 1.0))}
# the splats of a pixel are float atomics on the device: two orders of adding n non-negative float32 terms differ by at most about 2 n 2^-24 of their sum, and
# the bound of tests/test_gpu_vcm.py (1e-5 relative + 1e-6) covers that up to n = 80
MAX_SPLATS_PER_PIXEL = 80


def stream(seed, limit=None):
    """The case stream of a seed: dictionaries drawn from RandomState(seed) alone."""
    rng = np.random.RandomState(seed)
    index = -1
    while limit is None or index + 1 < limit:
        index += 1
        kind = SCENE_KINDS[rng.randint(len(SCENE_KINDS))]
        w, h = SIZES[rng.randint(len(SIZES))]
        cam = None
        if kind == "random": make = ("random", int(rng.randint(1, 1 << 30)))
        elif kind == "mesh_scene": make = ("mesh_scene", 2000)
        elif kind == "sponza":
            make = ("sponza", int(rng.choice([300, 3000])), int(rng.randint(1, 1000)), bool(rng.randint(2)), bool(rng.randint(2)))
            cam = ((float(rng.uniform(-13, 13)), float(rng.uniform(0.3, 10)), float(rng.uniform(-5, 5))), (float(rng.uniform(-60, 60)), float(rng.uniform(0, 360)), 0.0), float(rng.uniform(30, 100)))
        else: make = (kind,)
        if kind in CAMERAS:
            base = CAMERAS[kind]
            jitter = [float(rng.uniform(-1.0, 1.0)) for _ in range(6)]
            if rng.randint(4) != 0:
                cam = (tuple(base[0][a] + jitter[a] * base[3][a] for a in range(3)), (base[1][0] + 15.0 * jitter[3], base[1][1] + 30.0 * jitter[4], 0.0), base[2] * (1.0 + 0.4 * jitter[5]))
        if rng.randint(4) != 0:
            radius = float(rng.choice([0.02, 0.1, 0.4]))
            vcm = dict(max_path_length=int(rng.choice([1, 2, 3, 5, 10, 16])), use_vertex_connection=bool(rng.randint(2)), use_vertex_merging=bool(rng.randint(2)),
                       initial_merging_radius=radius, min_merging_radius=radius * float(rng.choice([1.0, 0.5])), merging_radius_multiplier=float(rng.choice([1.0, 0.8])),
                       bsdf_weight=float(rng.choice([1.0, 0.5, 0.0])), light_weight=float(rng.choice([1.0, 0.5, 0.0])),
                       vertex_connecting_weight=float(rng.choice([1.0, 0.5, 0.0])), vertex_merging_weight=float(rng.choice([1.0, 0.5, 0.0])))
            renderer = dict(name="VCM", vcm=vcm, camera_connecting_weight=float(rng.choice([1.0, 0.5])))      # the weight of leg B; leg A renders with 0
            streamed = rng.randint(4) == 0
            passes = int(rng.choice([9, 10, 11])) if streamed else int(rng.choice([1, 2, 3, 4]))
        else:
            renderer = dict(name="Light Tracer", max_ray_depth=int(rng.choice([0, 1, 2, 5, 10, 18])))
            streamed, passes = False, int(rng.randint(1, 5))
        dof = None
        if rng.randint(4) == 0:
            dof = (float(rng.uniform(2.0, 12.0)), float(rng.uniform(0.05, 0.4)), int(rng.randint(3)))      # focal plane distance, aperture, bokeh shape
        yield dict(index=index, kind=kind, make=make, w=w, h=h, cam=cam, renderer=renderer, passes=passes, streamed=bool(streamed), dof=dof,
                   dimensions=int(rng.choice([16, 64, 128])), use_blue_noise=bool(rng.randint(2)), vp_seed=int(rng.randint(1, 1 << 30)), counting=bool(rng.randint(2)))


def case_of(seed, index):
    for case in stream(seed, index + 1):
        if case["index"] == index:
            return case


def two_estimator_scene(aspect):
    from test_vcm_oracle import _two_estimator_scene
    return _two_estimator_scene(aspect)


def build(case):
    make, aspect = case["make"], case["w"] / case["h"]
    if make[0] == "random": scene, camera = scene_zoo.random_scene(aspect, make[1])
    elif make[0] == "zoo": scene, camera = scene_zoo.all_lights_scene(aspect)
    elif make[0] == "two": scene, camera = two_estimator_scene(aspect)
    elif make[0] == "cornell": scene, camera = scenes.cornell_box(aspect)
    elif make[0] == "mesh_scene": scene, camera = scene_zoo.mesh_scene(aspect, triangles=make[1])
    elif make[0] == "sponza": scene, camera = scenes.sponza_class(aspect, make[1], seed=make[2], textured=make[3], extra_texture=make[4])
    else: scene, camera = scenes.rough_glass_slab(aspect)
    if case["cam"]: camera = ra.Camera(case["cam"][0], case["cam"][1], aspect, case["cam"][2])
    if case["dof"]:
        camera.set_dof(True, case["dof"][0], case["dof"][1])
        camera.set_lens(bokeh_shape=case["dof"][2])
    return scene, camera


def accumulate(case, built, device, camera_connecting_weight=None, separate_light=False, splat_counts=None):
    """The passes of a case on the oracle and, with `device`, on the GPU too.  Without it the host mirror's pass counter is advanced the way the tail of
    Viewport::Render does (rth_viewport_finish_pass), so that the oracle gets the per-pass constants the device run would hand it: the CPU vetting of a case
    renders what the GPU test compares against.  `separate_light` (vetting only): light-path splats go to a buffer of their own.
    Returns a dictionary: oracle sums `ref`, `ref2`, (`light`), `ref_counters`, `ref_photons` (after every pass) and, with `device`, `img`, `img2`,
    `counters`, `photons` ((device, oracle) after every synchronised pass)."""
    scene, camera = built
    w, h, r = case["w"], case["h"], case["renderer"]
    desc = scene.desc
    bn = ra.load_blue_noise()
    desc.contents.blueNoise = bn.ctypes.data
    is_vcm = r["name"] == "VCM"
    vp = ra.Viewport(w, h, seed=case["vp_seed"], dimensions=case["dimensions"], use_blue_noise=case["use_blue_noise"], **({} if is_vcm else dict(max_ray_depth=r["max_ray_depth"])))
    vcm = None
    if is_vcm:
        args = dict(r["vcm"], camera_connecting_weight=r["camera_connecting_weight"] if camera_connecting_weight is None else camera_connecting_weight)
        vcm = oracle_lib.Vcm(**args)
        if splat_counts is not None: vcm.set_splat_counts(splat_counts)
    elif splat_counts is not None:
        oracle_lib.light_tracer_set_splat_counts(splat_counts)
    if device:
        vp.set_renderer(scene, name=r["name"], intersection_counters=case["counting"])
        if is_vcm: vp.set_vcm(**args)
    else:
        vp.reset()      # what follows SetRenderer in every caller
    ref = np.zeros((h, w, 3), dtype=np.float32); ref2 = np.zeros((h, w, 3), dtype=np.float32); light = np.zeros((h, w, 3), dtype=np.float32) if separate_light else None
    cnt = np.zeros(16, dtype=np.uint64)
    out = dict(ref=ref, ref2=ref2, light=light, ref_photons=[], photons=[])
    try:
        for i in range(case["passes"]):
            p = vp.next_pass_params(camera)
            if device: vp.render_pass_with(p)
            else: ra.host_lib().rth_viewport_finish_pass(vp._h)
            if is_vcm:
                vcm.render_pass(desc, p, w, h, ref, ref2 if i % 2 == 0 else None, light, cnt)
                out["ref_photons"].append(vcm.num_photons())
                if device and (not case["streamed"] or i == case["passes"] - 1):      # the query synchronises: without it the passes ride in batches
                    out["photons"].append((vp.vcm_num_photons(), vcm.num_photons()))
            else:
                oracle_lib.light_tracer_pass(desc, p, w, h, ref, ref2 if i % 2 == 0 else None, cnt)
    finally:
        if splat_counts is not None:
            if is_vcm: vcm.set_splat_counts(None)
            else: oracle_lib.light_tracer_set_splat_counts(None)
    out["ref_counters"] = {n: int(cnt[i]) for i, n in enumerate(ra.COUNTER_NAMES)}
    if device:
        out["img"], out["img2"] = vp.sum_buffer(secondary=True)
        out["counters"] = vp.counters()
    return out


def oracle_stats(case):
    """The oracle alone on the full-image configuration of a case (no GPU): what tests/test_vcm_fuzz_cases.py and the soak need to know about it."""
    counts = np.zeros((case["h"], case["w"]), dtype=np.uint32)
    is_vcm = case["renderer"]["name"] == "VCM"
    out = accumulate(case, build(case), False, separate_light=is_vcm, splat_counts=counts)
    total = out["ref"] + out["light"] if is_vcm else out["ref"]
    light = out["light"] if is_vcm else out["ref"]
    finite = np.isfinite(total)
    energy = float(total[finite].sum())
    return dict(finite=float(finite.mean()), nonblack=bool(np.any(total[finite] != 0.0)), photons=out["ref_photons"], max_splats=int(counts.max()),
                light_fraction=float(light[np.isfinite(light)].sum()) / energy if energy > 0.0 else 0.0, leg_b=int(counts.max()) <= MAX_SPLATS_PER_PIXEL)


def _counters_differ(case, out):
    names = COMPARED if case["counting"] else NOT_INTERSECTION
    return ["%s gpu %d oracle %d" % (n, out["counters"][n], out["ref_counters"][n]) for n in names if out["counters"][n] != out["ref_counters"][n]]


def _words_differ(got, want):
    """Words that differ; a word counts as equal where both sides hold a NaN."""
    return (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))


def _deviation(got, want):
    """Largest |got - want| relative to the float-atomic bound 1e-5 |want| + 1e-6 (words that are bit-identical or NaN on both sides count as 0)."""
    same = ~_words_differ(got, want)
    with np.errstate(invalid="ignore", over="ignore"):
        dev = np.abs(got.astype(np.float64) - want) / (1e-5 * np.abs(want.astype(np.float64)) + 1e-6)
    dev = np.where(same, 0.0, np.where(np.isnan(dev), np.inf, dev))
    return float(dev.max()) if dev.size else 0.0


def leg_a_problems(case, a):
    """What differs between device and oracle in an accumulation rendered with camera_connecting_weight = 0 (`a`: accumulate(..., device=True))."""
    problems = []
    for name, got, want in (("sum", a["img"], a["ref"]), ("secondary", a["img2"], a["ref2"])):
        diff = np.argwhere(_words_differ(got, want))
        if len(diff):
            problems.append("leg A %s buffer: %d differing words; first " % (name, len(diff)) +
                            "; ".join("pixel (%d, %d) channel %d gpu %.9g oracle %.9g" % (x, y, ch, got[y, x, ch], want[y, x, ch]) for y, x, ch in diff[:4]))
    problems += ["leg A counter " + t for t in _counters_differ(case, a)]
    problems += ["leg A photons after synchronised pass %d: gpu %d oracle %d" % (k, g, o) for k, (g, o) in enumerate(a["photons"]) if g != o]
    return problems


def render(case, quiet=False, leg_b=None, legs="ab"):
    """Device against oracle.  Leg A (VCM): camera_connecting_weight = 0, so every film splat adds zero -- both sum buffers bit-identical, counters and photon
    counts equal.  Leg B (VCM with the case's camera_connecting_weight; the Light Tracer always): counters equal; pixels within 1e-5 |want| + 1e-6, compared only
    when no pixel receives more than MAX_SPLATS_PER_PIXEL splats (`leg_b`: None = ask the oracle's splat counter, False = skip leg B's pixels, True = compare them).
    `legs`: "a" renders leg A alone.
    Returns (agree, report): report["problems"] lists what differs, report["leg_b"] says whether leg B's pixels were compared, report["deviation"] is its largest
    deviation relative to the bound."""
    built = build(case)
    is_vcm = case["renderer"]["name"] == "VCM"
    problems = []
    report = dict(problems=problems, leg_b=False, deviation=0.0, max_splats=None)
    if is_vcm and "a" in legs:
        problems += leg_a_problems(case, accumulate(case, built, True, camera_connecting_weight=0.0))
    counts = np.zeros((case["h"], case["w"]), dtype=np.uint32) if leg_b is None else None
    if "b" not in legs or (is_vcm and leg_b is False):
        pass      # (leg A covers the counters of a VCM case whose leg B pixels are not comparable)
    else:
        b = accumulate(case, built, True, splat_counts=counts)
        if counts is not None:
            report["max_splats"] = int(counts.max())
            leg_b = report["max_splats"] <= MAX_SPLATS_PER_PIXEL
        problems += ["leg B counter " + t for t in _counters_differ(case, b)]
        problems += ["leg B photons after synchronised pass %d: gpu %d oracle %d" % (k, g, o) for k, (g, o) in enumerate(b["photons"]) if g != o]
        if leg_b:
            report["leg_b"] = True
            for name, got, want in (("sum", b["img"], b["ref"]), ("secondary", b["img2"], b["ref2"])):
                dev = _deviation(got, want)
                report["deviation"] = max(report["deviation"], dev)
                if dev > 1.0:
                    problems.append("leg B %s buffer: %.3g times the bound 1e-5 |want| + 1e-6" % (name, dev))
    if not quiet:
        print("case %d: %s; leg B pixels %s, largest deviation %.3g of the bound, most splats on a pixel %s" %
              (case["index"], "agree" if not problems else "DIFFER", "compared" if report["leg_b"] else "not compared", report["deviation"], report["max_splats"]), flush=True)
        for t in problems:
            print("   " + t)
    return not problems, report


if __name__ == "__main__":
    seed = int(sys.argv[1])
    if sys.argv[2] == "list":
        for case in stream(seed, int(sys.argv[3]) if len(sys.argv) > 3 else 1000):
            print(case)
    else:
        oracle_only = sys.argv[2] == "oracle"
        wanted = set(int(a) for a in sys.argv[(3 if oracle_only else 2):])
        for case in stream(seed, max(wanted) + 1):
            if case["index"] in wanted:
                print(case, "env", {k: v for k, v in os.environ.items() if k.startswith("RTGPU_")})
                if oracle_only: print("   oracle:", oracle_stats(case))
                else: render(case)
