"""CPU: the reference predicate of the fp16 range guard and the tables of tests/_range.py.

expected_flag against its plain statement on the edge values; SITES and UNGUARDED together are exactly the launching entry points,
and disjoint; every translation unit with reporting sites has at least as many SITES entries as calls of tce_range_report; every
builder's inputs satisfy the condition of _range.check_condition for every target, route and value class it offers; the entries
that are consumed by a split product without a guard are named in DESIGN.md."""
import glob
import os
import re

import numpy as np
import pytest

import _range as R
from tce_rvos_amd import _lib, hazard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tce-rvos_amd", "csrc")


def bits(*words):
    return np.array(words, dtype=np.uint32).view(np.float32)


EDGES = [
    (0x00000000, False), (0x00000001, False), (0x007FFFFF, False),         # +0, smallest and largest denormal
    (0x3F800000, False),                                                   # 1
    (0x476A5FFF, False),                                                   # 59999.996, the fp32 number just below 60000
    (0x476A6000, True),                                                    # 60000
    (0x476A6001, True),
    (0x477FE000, True),                                                    # 65504
    (0x7F7FFFFF, True),                                                    # FLT_MAX
    (0x7F800000, True),                                                    # Inf
    (0x7FC00000, True), (0x7F800001, True), (0x7FFFFFFF, True), (0x7FC12345, True),   # NaN: quiet, signalling, every payload bit
]


def test_edge_words_are_what_they_claim():
    assert float(bits(0x476A6000)[0]) == 60000.0 and float(bits(0x477FE000)[0]) == 65504.0
    assert float(bits(0x476A5FFF)[0]) == float(np.nextafter(np.float32(60000), np.float32(0)))
    assert float(bits(0x7F7FFFFF)[0]) == float(np.finfo(np.float32).max)
    assert R.LIMIT_BITS == 0x476A6000


@pytest.mark.parametrize("word,want", EDGES)
@pytest.mark.parametrize("sign", [0, 0x80000000])
def test_expected_flag_on_edge_values(word, want, sign):
    v = bits(word | sign)
    assert R.expected_flag(v) is want
    assert R.expected_flag_plain(v) is want
    pad = np.concatenate([np.float32([1.0, -2.5]), v, np.float32([0.0])])      # anywhere in an array
    assert R.expected_flag(pad) is want and R.expected_flag_plain(pad) is want


def test_expected_flag_agrees_with_the_plain_statement_on_fp64_values():
    vals = [0.0, -0.0, 1e-45, 59999.996, 59999.999, 60000.0, -60000.0, 60160.0, 59904.0, 65504.0, 3.4e38, 1e39, float("inf"),
            -float("inf"), float("nan")]
    for v in vals:
        with np.errstate(over="ignore"):
            want = not abs(np.float32(v)) < 60000
        assert R.expected_flag(np.float64([v])) == R.expected_flag_plain(np.float64([v])) == want, v
    assert R.expected_flag(np.float64([59999.999]))     # rounds to 60000 in fp32, the format the kernels store


def launching():
    """The launching entry points of the main header and of the three byte-valued output stages (tests/_range.py has rows for these)"""
    stage = set(_lib.VIS_SIGNATURES) | set(_lib.PNGFILE_SIGNATURES) | set(_lib.REFEXP_SIGNATURES)
    unmodelled = stage - set(hazard.MODELS)
    assert all(n.endswith(("_bound", "_ws_bytes")) for n in unmodelled), unmodelled   # queries launch nothing
    return (set(_lib.SIGNATURES) | stage) - hazard.NOT_LAUNCHES


def test_tables_are_complete_and_disjoint():
    sites = {s.entry for s in R.SITES}
    assert not sites & set(R.UNGUARDED), sorted(sites & set(R.UNGUARDED))
    want = launching()
    assert sites | set(R.UNGUARDED) == want, (sorted(want - sites - set(R.UNGUARDED)), sorted((sites | set(R.UNGUARDED)) - want))
    assert all(reason in R.REASONS for reason in R.UNGUARDED.values())
    stage = set(_lib.VIS_SIGNATURES) | set(_lib.PNGFILE_SIGNATURES) | set(_lib.REFEXP_SIGNATURES)
    for name in stage & want:                      # the byte-valued output stages
        assert R.UNGUARDED[name] == R.R_NOT, name
    assert len({s.id for s in R.SITES}) == len(R.SITES)
    for s in R.SITES:
        assert s.kind in ("output", "intermediate") and os.path.exists(os.path.join(CSRC, s.source)), s.id


def test_every_reporting_site_has_a_case():
    """A text count of the one identifier: a new call of tce_range_report cannot arrive without a SITES entry for its file."""
    per_file = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.inc"))):
        text = open(path).read()
        calls = len(re.findall(r"\btce_range_report\s*\(", text)) - len(re.findall(r"void\s+tce_range_report\s*\(", text))
        if calls:
            per_file[os.path.basename(path)] = calls
    assert per_file, "no reporting site found: the identifier was renamed"
    have = {}
    for s in R.SITES:
        have[s.source] = have.get(s.source, 0) + 1
    assert set(per_file) == set(have), (sorted(per_file), sorted(have))
    for name, calls in per_file.items():
        assert have[name] >= calls, f"{name}: {calls} calls of tce_range_report, {have[name]} SITES entries"


@pytest.mark.parametrize("site", R.SITES, ids=[s.id for s in R.SITES])
def test_builder_inputs_satisfy_the_condition(site):
    n = 0
    offered = set()
    for case in site.cases():
        n_off = R.check_condition(case)
        assert case.expect == (n_off > 0)
        offered.add(case.cls)
        n += 1
    assert n > 0 and offered & {"over+", "nan"}, f"{site.id}: no offending class offered"
    for r, c in site.targets:
        assert r >= 0 and c >= 0


def test_open_entries_are_named_in_the_design_notes():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "A + A2" in text
    for name, reason in R.UNGUARDED.items():
        if reason == R.R_OPEN:
            assert name in text, f"{name} is consumed by a split product without a guard: DESIGN.md must say so"
