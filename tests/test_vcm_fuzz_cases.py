"""The pinned cases of tests/vcm_fuzz_cases.py on the oracle alone: they are finite, they are not black, and together they reach the parts of the bidirectional
integrator and the light tracer they were chosen for.  These are conditions on the INPUTS of tests/test_gpu_vcm_fuzz.py, checked without a GPU, so that the GPU
test cannot pass by rendering nothing.  The oracle renders what the GPU test hands it: tools/vcm_fuzz_replay.py advances the host mirror's pass counter through
rth_viewport_finish_pass where no device submits the pass."""
import os
import sys

import pytest

import vcm_fuzz_cases as pinned

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


@pytest.fixture(scope="module")
def vetted(built):
    """[(entry, case, oracle statistics, number of textures of the scene)] of every pinned and every hand case, rendered once."""
    import vcm_fuzz_replay as replay
    out = []
    for entry in pinned.CASES + sorted(pinned.HAND_CASES):
        case = pinned.resolve(entry)
        out.append((entry, case, replay.oracle_stats(case), int(replay.build(case)[0].desc.contents.numTextures) if case["kind"] == "random" else 0))
    return out


def test_the_list_is_a_slice_of_the_stream():
    import vcm_fuzz_replay as replay
    assert 24 <= len(pinned.CASES) <= 32 and len(set(pinned.CASES)) == len(pinned.CASES)
    assert all(e in pinned.CASES for e in pinned.DELIBERATELY_EMPTY) and all(e in pinned.CASES or e in pinned.HAND_CASES for e in pinned.KNOB_CASES)
    # a case is a function of (seed, index) alone: listing the stream twice gives the same cases
    a = list(replay.stream(pinned.SEED, 40)); b = list(replay.stream(pinned.SEED, 40))
    assert a == b and [c["index"] for c in a] == list(range(40))


def test_every_pinned_case_is_finite_and_not_black(vetted):
    for entry, case, stats, _ in vetted:
        assert stats["finite"] >= 0.999, (entry, stats)
        assert stats["nonblack"] != (entry in pinned.DELIBERATELY_EMPTY), (entry, stats)


def test_the_pinned_cases_cover_what_they_were_chosen_for(vetted):
    import vcm_fuzz_replay as replay
    listed = [v for v in vetted if not isinstance(v[0], str)]
    cases = [c for _, c, _, _ in listed]
    vcm = [(c, s) for _, c, s, _ in listed if c["renderer"]["name"] == "VCM"]
    tracer = [(c, s) for _, c, s, _ in listed if c["renderer"]["name"] == "Light Tracer"]
    assert {c["kind"] for c in cases} == set(replay.SCENE_KINDS)
    assert {c["make"][3] for c in cases if c["kind"] == "sponza"} == {True, False}
    assert sum(c["kind"] == "random" for c in cases) >= 6 and sum(t > 0 for _, c, _, t in listed if c["kind"] == "random") >= 2
    assert {1, 2, 3, 16} <= {c["renderer"]["vcm"]["max_path_length"] for c, _ in vcm}
    assert {(c["renderer"]["vcm"]["use_vertex_connection"], c["renderer"]["vcm"]["use_vertex_merging"]) for c, _ in vcm} == {(False, False), (False, True), (True, False), (True, True)}
    for weight in ("bsdf_weight", "light_weight", "vertex_connecting_weight", "vertex_merging_weight"):
        assert {0.5, 0.0} <= {c["renderer"]["vcm"][weight] for c, _ in vcm}, weight
    assert {0.5, 1.0} <= {c["renderer"]["camera_connecting_weight"] for c, _ in vcm}
    assert any(c["streamed"] and c["renderer"]["vcm"]["use_vertex_merging"] and c["renderer"]["vcm"]["merging_radius_multiplier"] < 1.0 and
               c["renderer"]["vcm"]["min_merging_radius"] < c["renderer"]["vcm"]["initial_merging_radius"] and max(s["photons"]) > 0 for c, s in vcm)
    assert {(1, 1), (7, 5), (33, 17)} <= {(c["w"], c["h"]) for c in cases}
    assert {0, 18} <= {c["renderer"]["max_ray_depth"] for c, _ in tracer}
    assert any(c["dof"] for c in cases) and {c["dof"][2] for c in cases if c["dof"]} >= {0, 1}
    assert {c["counting"] for c, _ in vcm} == {True, False} and {c["counting"] for c, _ in tracer} == {True, False}
    merging = [(c, s) for c, s in vcm if c["renderer"]["vcm"]["use_vertex_merging"]]
    # an empty merge set (HashGrid::Build of nothing) followed, in the same accumulation, by passes that do record photons
    assert any(any(n == 0 and max(s["photons"][i + 1:], default=0) > 0 for i, n in enumerate(s["photons"])) for _, s in merging)
    assert any(c["streamed"] and any(n == 0 and max(s["photons"][i + 1:], default=0) > 0 for i, n in enumerate(s["photons"])) for c, s in merging)
    assert any(1 <= sum(s["photons"]) <= 8 for _, s in merging)
    # leg B compares pixels where no pixel receives more than 80 splats; at least three such cases in which the light image is a real part of the estimate
    assert sum(s["leg_b"] and s["light_fraction"] > 0.01 for _, s in vcm) >= 3
    assert sum(s["leg_b"] and s["nonblack"] for _, s in tracer) >= 2


def test_the_knob_cases_are_what_the_knobs_need(vetted):
    by_entry = {e: (c, s, t) for e, c, s, t in vetted}
    two, random_scene, zoo = (by_entry[e] for e in pinned.KNOB_CASES)
    v = two[0]["renderer"]["vcm"]
    assert two[0]["kind"] == "two" and two[0]["streamed"] and two[0]["passes"] == 11 and (v["initial_merging_radius"], v["min_merging_radius"]) == (0.4, 0.2) and v["merging_radius_multiplier"] < 1.0
    assert random_scene[0]["kind"] == "random" and random_scene[2] > 0 and zoo[0]["kind"] == "zoo"
    for case, stats, _ in (two, random_scene, zoo):
        assert case["renderer"]["vcm"]["use_vertex_merging"] and case["passes"] >= 2 and min(stats["photons"]) > 100, stats      # merging happens, on more than a handful of photons
