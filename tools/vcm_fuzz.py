"""Soak test of the whole-frame integrators: renderer "VCM" and renderer "Light Tracer" on the device against the CPU oracle on random scenes, frame sizes and
settings -- camera paths bit-identical (leg A), full images within the float-atomic bound where few splats land on a pixel (leg B), counters and photon counts
equal.  tools/vcm_fuzz_replay.py holds the case stream and renders a single case; tests/test_gpu_vcm_fuzz.py renders a pinned slice under `pytest -m gpu`.
usage: python tools/vcm_fuzz.py [seconds] [seed] [only this scene kind]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))


def run(budget=300.0, seed=1, min_cases=0, log=print, only=None):
    """Random cases until `budget` seconds are used up (and at least `min_cases`).  Returns (cases, mismatches, cases whose leg B pixels were compared, largest
    leg B deviation relative to its bound).  A mismatch line names seed and index: `python tools/vcm_fuzz_replay.py <seed> <index>` replays it."""
    import vcm_fuzz_replay as replay
    t_end = time.time() + budget
    cases = bad = leg_b = 0
    deviation = 0.0
    for case in replay.stream(seed, None):
        if not (time.time() < t_end or cases < min_cases):
            break
        if only and case["kind"] != only:
            continue
        same, report = replay.render(case, quiet=True)
        cases += 1
        leg_b += 1 if report["leg_b"] else 0
        deviation = max(deviation, report["deviation"])
        if not same:
            bad += 1
            log("MISMATCH seed %d index %d" % (seed, case["index"]), case, report["problems"])
    return cases, bad, leg_b, deviation


if __name__ == "__main__":
    t0 = time.time()
    cases, bad, leg_b, deviation = run(float(sys.argv[1]) if len(sys.argv) > 1 else 300.0, int(sys.argv[2]) if len(sys.argv) > 2 else 1,
                                       only=sys.argv[3] if len(sys.argv) > 3 else None)
    print("cases %d (%d with leg B pixels compared, largest deviation %.3g of the bound), mismatches %d; %.0f s" % (cases, leg_b, deviation, bad, time.time() - t0), flush=True)
    sys.exit(1 if bad else 0)
