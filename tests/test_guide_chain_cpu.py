"""A census of the guide-chain fixtures (tests/guide_chain_ref.py) from the oracle alone, so that the GPU comparison (tests/test_gpu_guide_chain.py) cannot
quietly lose its cases.  These are conditions on the inputs -- camera and props were moved until the oracle met them -- not measurements of the device."""
import numpy as np
import pytest

MIN_CASES = 8


@pytest.fixture(scope="module")
def ref(built):
    import guide_chain_ref
    return guide_chain_ref


def test_the_fold_on_hand_made_recordings(ref):
    """the rule of include/rtgpu.h on three-vertex paths whose material kinds and events are set by hand"""
    desc = ref.scene("hall").desc.contents
    frame = ref.oracle_frame("hall")
    mirror = next(v for v in frame if len(v) >= 3 and ref.is_surface(v[0]) and desc.materials[ref.material_of(v[0], desc)].bsdf == ref.PASSING_BSDFS[2] and ref.is_surface(v[1]))
    v = mirror[:3].copy()
    v[0, 26:27].view(np.uint32)[0] = ref.EV_SPECULAR_REFLECTION
    v[1, 6:8] = v[0, 6:8]                                              # the second vertex on the mirror too
    v[1, 26:27].view(np.uint32)[0] = ref.EV_SPECULAR_REFLECTION
    v[:, 8] = (1.5, 2.25, 1e-3)
    v[0, 22:25], v[1, 22:25] = (0.5, 0.25, 0.125), (0.75, 0.5, 0.25)
    for max_chain, k in ((0, 0), (1, 1), (2, 2), (16, 2)):
        got_k, distance, throughput = ref.fold(v, desc, max_chain)
        assert got_k == k
        want = np.float32(1.5)
        for d in v[1:k + 1, 8]:
            want = np.float32(want + d)
        assert distance == want and distance.dtype == np.float32
        assert np.array_equal(throughput, np.ones(3, np.float32) if k == 0 else v[k - 1, 22:25])
    v[0, 26:27].view(np.uint32)[0] = 4                                  # a glossy event stops the chain at once
    assert ref.fold(v, desc, 16)[0] == 0
    assert ref.fold(v[:1], desc, 16)[0] == 0                            # a closing record is never passed, whatever its stale event word says


def test_hall_has_every_case_the_device_is_compared_on(ref):
    desc = ref.scene("hall").desc.contents
    frame = ref.oracle_frame("hall")
    assert len(frame) == ref.W * ref.H
    c = ref.census(frame, desc, 3)
    print("hall, maxChain 3:", c)
    assert c["k1"] >= 0.15 * c["pixels"] and c["k2"] >= 0.02 * c["pixels"]
    for case in ("diffuse_behind_mirror", "stopped_by_max_chain", "miss_behind_mirror", "light_behind_mirror", "plastic_specular", "sphere_reflection", "sphere_refraction"):
        assert c[case] >= MIN_CASES, case
    # a chain of at most 3 vertices cannot reach the depth limit of 6: that case is counted where the device meets it, at maxChain 16
    deep = ref.census(frame, desc, 16)
    print("hall, maxChain 16:", deep)
    assert c["closed_by_depth"] == 0 and deep["closed_by_depth"] >= MIN_CASES


def test_roulette_cuts_chains_in_the_roulette_variant(ref):
    """without roulette a chain that ends on a mirror or on glass before maxChain ran out of throughput or found no event (a mirror seen from behind, total
    internal reflection); with minRussianRouletteDepth 0 at least 8 more do, and only roulette can have ended those"""
    desc = ref.scene("hall").desc.contents
    plain = ref.census(ref.oracle_frame("hall"), desc, 3)["closed_on_passing_surface"]
    cut = ref.census(ref.oracle_frame("hall", roulette=True), desc, 3)["closed_on_passing_surface"]
    print("chains closed on a passing surface: %d without roulette, %d with" % (plain, cut))
    assert ref.params(roulette=True).minRussianRouletteDepth == 0 and ref.params().minRussianRouletteDepth > ref.MAX_RAY_DEPTH
    assert cut >= plain + MIN_CASES


def test_textured_shows_the_light_in_its_normal_mapped_mirror(ref):
    desc = ref.scene("textured").desc.contents
    frame = ref.oracle_frame("textured")
    c = ref.census(frame, desc, 3)
    print("textured, maxChain 3:", c)
    assert c["light_behind_mirror"] >= MIN_CASES and c["diffuse_behind_mirror"] >= MIN_CASES
    # the stale-material rule bites: the vertex before those light hits has a normal map
    k, _, _, guides, _ = ref.folded_frame(frame, desc, 3)
    lit = [i for i in range(len(frame)) if k[i] >= 1 and guides[i, 7:8].view(np.uint32)[0] == ref.LIGHT_OBJECT]
    mapped = [i for i in lit if desc.materials[ref.material_of(frame[i][k[i] - 1], desc)].normalMapTexture != 0xFFFFFFFF]
    assert len(mapped) >= MIN_CASES


@pytest.mark.parametrize("name, max_chain", [("hall", 1), ("hall", 3), ("hall", 16), ("textured", 3)])
def test_stale_words_are_a_minority_of_the_compared_words(ref, name, max_chain):
    desc = ref.scene(name).desc.contents
    _, _, _, guides, stale = ref.folded_frame(ref.oracle_frame(name), desc, max_chain)
    compared = stale[:, 6:22]
    print("%s, maxChain %d: %d of %d compared words are masked" % (name, max_chain, compared.sum(), compared.size))
    assert compared.sum() * 2 < compared.size
