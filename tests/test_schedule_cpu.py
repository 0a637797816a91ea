"""CPU checks of the captured-step plumbing (models/utils/schedule.py) and of the list of environment switches."""
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# switches whose alternatives lost their A/B and were removed with the code they selected (the captured step)
RETIRED = ("MXDET_TUNE_EARLY_ANCHORS", "MXDET_TUNE_DEFER_RPN_WGRAD", "MXDET_TUNE_ROI_FIRST", "MXDET_TUNE_TAIL_AT",
           "MXDET_TUNE_WGRAD_GRAPH", "MXDET_TUNE_OPT_STREAM")


@pytest.mark.parametrize("ranges, size, want", [
    ([], 100, [(0, 100)]),                                      # no bucket updated
    ([(0, 40), (40, 100)], 100, []),                            # everything covered
    ([(0, 30), (50, 100)], 100, [(30, 50)]),                    # a hole in the middle
    ([(0, 60), (20, 40), (50, 80)], 100, [(80, 100)]),          # overlapping ranges (one inside another, one straddling)
    ([(0, 64)], 100, [(64, 100)]),                              # an uncovered tail
    ([(70, 100), (0, 10), (30, 50)], 100, [(10, 30), (50, 70)]),   # ranges given out of order
    ([(10, 20)], 20, [(0, 10)]),                                # an uncovered head
], ids=["none", "all", "hole", "overlap", "tail", "unordered", "head"])
def test_uncovered_ranges(ranges, size, want):
    from mxdetection_amd.models.utils.schedule import uncovered_ranges
    given = list(ranges)
    assert uncovered_ranges(ranges, size) == want
    assert ranges == given                                      # the caller's list is left alone


def _text_files(*dirs):
    for d in dirs:
        for path in glob.glob(os.path.join(ROOT, d, "**", "*"), recursive=True):
            if os.path.isfile(path) and "__pycache__" not in path and "_obj" not in path \
                    and not path.endswith((".so", ".o", ".a", ".npz", ".npy", ".pyc")):
                yield path


def test_every_switch_the_package_reads_is_in_the_readme():
    from mxdetection_amd import _lib
    readme = set(re.findall(r"MXDET_(?:TUNE|ABL)_[A-Z0-9_]*[A-Z0-9]", open(os.path.join(ROOT, "README.md")).read()))
    used = {"MXDET_TUNE_" + k for k in _lib.TUNING_KEYS}
    for path in glob.glob(os.path.join(ROOT, "mxdetection_amd", "**", "*.py"), recursive=True):
        used.update(re.findall(r"MXDET_(?:TUNE|ABL)_[A-Z0-9_]*[A-Z0-9]", open(path).read()))
    assert len(used) > len(_lib.TUNING_KEYS) + 5                # the scan found the Python-side switches too
    assert sorted(used - readme) == []


def test_no_retired_switch_is_named_any_more():
    pat = re.compile(r"\b(?:%s)\b" % "|".join(RETIRED))
    hits = []
    for path in list(_text_files("mxdetection_amd", "tools")) + [os.path.join(ROOT, "README.md")]:
        with open(path, errors="ignore") as f:
            hits += [(os.path.relpath(path, ROOT), m) for m in pat.findall(f.read())]
    assert hits == []
