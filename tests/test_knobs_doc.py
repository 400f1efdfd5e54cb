"""The knob table of DESIGN.md ("Environment knobs") lists exactly the RTGPU_* variables raytracer_amd/csrc/rt_knobs.h reads: a knob that is added,
renamed or retired changes both in the same commit."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_design_knob_table_lists_what_rt_knobs_reads():
    header = open(os.path.join(ROOT, "raytracer_amd", "csrc", "rt_knobs.h")).read()
    read = set(re.findall(r'"(RTGPU_[A-Z0-9_]+)"', header))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design.split("### Environment knobs", 1)[1].split("\n## ", 1)[0]
    rows = re.findall(r"^\| `(RTGPU_[A-Z0-9_]+)` \|", section, flags=re.M)
    assert read and rows
    assert len(rows) == len(set(rows)), sorted(r for r in rows if rows.count(r) > 1)
    assert set(rows) == read, {"only in rt_knobs.h": sorted(read - set(rows)), "only in DESIGN.md": sorted(set(rows) - read)}
