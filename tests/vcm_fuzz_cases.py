"""The pinned slice of the whole-frame integrators' case stream (tools/vcm_fuzz_replay.py): (seed, index) pairs chosen by running the stream on the oracle alone.
tests/test_vcm_fuzz_cases.py holds the list to the conditions it was chosen for (no GPU needed); tests/test_gpu_vcm_fuzz.py renders every case on the device."""

SEED = 20261017

CASES = [
    # random_scene (textured: 5, 16, 42, 72, 81, 150)
    (SEED, 5), (SEED, 16), (SEED, 19), (SEED, 42), (SEED, 72), (SEED, 81), (SEED, 114), (SEED, 116), (SEED, 117), (SEED, 150),
    # all_lights_scene (32: Light Tracer at depth 18)
    (SEED, 13), (SEED, 44), (SEED, 32),
    # the two-estimator scene
    (SEED, 43), (SEED, 12),
    # Cornell box (9: one pixel, streamed, no photon before the fifth pass; 73: Light Tracer at depth 18; 47: Light Tracer at depth 0)
    (SEED, 3), (SEED, 9), (SEED, 14), (SEED, 98), (SEED, 73), (SEED, 47),
    # mesh + analytic scene (101: Light Tracer at depth 18)
    (SEED, 126), (SEED, 101),
    # Sponza-class mesh, textured and not
    (SEED, 45), (SEED, 158),
    # rough glass slab
    (SEED, 33), (SEED, 38), (SEED, 24),
]

# black on purpose: the Light Tracer at depth 0 connects nothing
DELIBERATELY_EMPTY = [(SEED, 47)]

# Cases that are not in the stream.  The first one is what the "results do not depend on it" knobs of DESIGN.md are held to: the two-estimator scene, 11 streamed
# passes (one full batch of 8 and a partial one whose first merge set comes from the batch before), radius 0.4 shrinking to 0.2.
HAND_CASES = {
    "two_streamed_shrinking": dict(index=-1, kind="two", make=("two",), w=61, h=47, cam=None, passes=11, streamed=True, dof=None, dimensions=64, use_blue_noise=True,
                                   vp_seed=99, counting=False,
                                   renderer=dict(name="VCM", camera_connecting_weight=1.0,
                                                 vcm=dict(max_path_length=10, use_vertex_connection=True, use_vertex_merging=True, initial_merging_radius=0.4,
                                                          min_merging_radius=0.2, merging_radius_multiplier=0.8, bsdf_weight=1.0, light_weight=1.0,
                                                          vertex_connecting_weight=1.0, vertex_merging_weight=1.0))),
}

# what every setting of RTGPU_VCM_CLASS / RTGPU_VCM_MERGE_COOP / RTGPU_VCM_BATCH renders (leg A): the hand case above, a textured random_scene, all_lights_scene
KNOB_CASES = ["two_streamed_shrinking", (SEED, 42), (SEED, 44)]


def resolve(entry):
    """(seed, index) or the name of a hand case -> the case dictionary."""
    if isinstance(entry, str):
        return dict(HAND_CASES[entry])
    import os
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import vcm_fuzz_replay
    return vcm_fuzz_replay.case_of(*entry)


def case_id(entry):
    return entry if isinstance(entry, str) else "%d-%d" % entry
