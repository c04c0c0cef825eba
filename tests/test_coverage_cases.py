"""The depth-of-coverage reference (tests/coverage_cases.py) against the
definition, the planted cases against what they were planted for, and the
coverage entry points of the header, the library and the CLI.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import coverage_cases as cc
from tests.coverage_cases import T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANTED = {c["name"]: c for c in cc.planted_cases()}


def _runs(case):
    return cc.depth_runs(case["contig"], case["start"], case["end"], case["lens"])


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(PLANTED))
def test_depth_runs_equals_brute_force_on_planted(name):
    case = PLANTED[name]
    assert case["lens"].sum() <= 100_000  # every planted genome is small enough
    assert _same(_runs(case), cc.brute_runs(case["contig"], case["start"], case["end"],
                                            case["lens"]))


def test_depth_runs_equals_brute_force_on_random():
    shapes = 0
    for seed in range(300):
        rng = np.random.default_rng(10_000 + seed)
        lens = rng.integers(0, 1200, int(rng.integers(1, 5)))  # (length-0 contigs stay empty)
        if lens.sum() == 0:
            lens[0] = 7
        n = int(rng.integers(1, 400))
        case = cc.random_case(seed, n, lens, int(rng.integers(0, 60)))
        s, e, ln = case["start"], case["end"], case["lens"][case["contig"]]
        shapes += (e == s).any() + 2 * (e == ln).any() + 4 * (len(np.unique(s)) < n)
        got = _runs(case)
        assert _same(got, cc.brute_runs(case["contig"], s, e, case["lens"])), seed
        assert int(((got[2] - got[1]) * got[3]).sum()) == int((e - s).sum()), seed
    assert shapes > 300  # zero widths, rows at contig ends and ties all occur


def test_small_cases_results():
    assert [len(x) for x in _runs(PLANTED["empty"])] == [0] * 4
    assert [x.tolist() for x in _runs(PLANTED["one_row"])] == [[0], [3], [9], [1]]
    assert len(_runs(PLANTED["zero_width_only"])[0]) == 0
    # book-ended rows: the depth does not change at 5
    assert [x.tolist() for x in _runs(PLANTED["book_ended"])] == [[0], [0], [9], [1]]
    assert [x.tolist() for x in _runs(PLANTED["zero_width_inside"])] == [[0], [2], [8], [1]]
    for k in (1, 2, 65, 70000):
        assert [x.tolist() for x in _runs(PLANTED[f"identical_{k}"])] == [[0], [10], [20], [k]]


def test_identical_rows_span_tiles_and_pass_u16():
    c = PLANTED["identical_70000"]
    x, first, last = cc.event_groups(c["start"], c["end"])
    assert x.tolist() == [10, 20]
    # each group holds 70000 events: dozens of tiles, the second reached
    # through whole tiles of one coordinate; the depth does not fit 16 bits
    assert (last - first + 1).tolist() == [70000, 70000]
    assert first[1] // T - first[0] // T >= 30 and 70000 > 1 << 16


def test_tile_sized_cases_have_the_event_counts():
    events = sorted(2 * len(PLANTED[f"tile_sized_{n}"]["start"]) for n in cc.TILE_ROWS)
    for want in (T - 2, T, T + 2, 2 * T, 2 * T + 2, 3 * T - 2):
        assert want in events
    # odd row counts, and heavy ties: most coordinate groups hold many events
    assert {T - 1, T + 1, 2 * T + 1, 3 * T - 1} <= set(cc.TILE_ROWS)
    for n in cc.TILE_ROWS:
        c = PLANTED[f"tile_sized_{n}"]
        x, first, last = cc.event_groups(c["start"], c["end"])
        assert np.median(last - first + 1) >= 10


def test_chain_splits_a_no_change_group_at_the_tile_edge():
    c = PLANTED[f"chain_{T // 2 + 3}"]
    x, first, last = cc.event_groups(c["start"], c["end"])
    k = int(np.nonzero(x == T // 2)[0][0])
    # one start (taken first) and one end at T / 2: positions T - 1 and T
    assert (first[k], last[k]) == (T - 1, T)
    assert (c["start"] == T // 2).sum() == 1 and (c["end"] == T // 2).sum() == 1
    assert [v.tolist() for v in _runs(c)] == [[0], [0], [T // 2 + 3], [1]]


def test_straddle_change_group_positions():
    c = PLANTED["straddle_change"]
    x, first, last = cc.event_groups(c["start"], c["end"])
    k = int(np.nonzero(x == 50)[0][0])
    assert (first[k], last[k]) == (T - 3, T + 5)
    got = _runs(c)
    assert got[1].tolist() == [0, 2, 50] and got[2].tolist() == [1, 50, 60]
    assert got[3].tolist() == [(T - 6) // 2, 3, 6]  # 3 -> 6 at the straddling group


def test_tile_edge_last_event_cases():
    c = PLANTED["edge_is_last"]
    x, first, last = cc.event_groups(c["start"], c["end"])
    assert last[x.tolist().index(1)] == T - 1 and first[x.tolist().index(5)] == T
    c = PLANTED["edge_not_last"]
    x, first, last = cc.event_groups(c["start"], c["end"])
    k = x.tolist().index(1)
    assert first[k] < T - 1 < last[k]


def test_long_over_chain_heads_two_tiles_apart():
    c = PLANTED["long_over_chain"]
    m = T + 5
    got = _runs(c)
    assert [v.tolist() for v in got] == [[0, 0, 0], [0, 5, 5 + m], [5, 5 + m, m + 10], [1, 2, 1]]
    x, first, last = cc.event_groups(c["start"], c["end"])
    xs = x.tolist()
    assert first[xs.index(5 + m)] - last[xs.index(5)] >= 2 * T
    # every interior coordinate: one start and one end, no change
    inner = (x > 5) & (x < 5 + m)
    assert ((last - first)[inner] == 1).all()


def test_staircases_make_every_coordinate_a_head():
    for m, w in ((1500, 7), (1500, 3001)):
        c = PLANTED[f"staircase_{m}_{w}"]
        got = _runs(c)
        x, first, last = cc.event_groups(c["start"], c["end"])
        assert (first == last).all()  # one event per coordinate: each is a head
        assert len(got[0]) == len(x) - 1 == 2 * m - 1  # the run count is 2n - 1
        assert 2 * len(c["start"]) > T  # more than one tile
        assert got[3].max() == min(m, (w + 1) // 2) and got[3][0] == 1 and got[3][-1] == 1


def test_contig_cases_results():
    assert [v.tolist() for v in _runs(PLANTED["contig_touch"])] == \
        [[0, 1], [3, 0], [10, 4], [1, 1]]
    assert [v.tolist() for v in _runs(PLANTED["contig_gap"])] == \
        [[0, 2, 2, 2], [1, 0, 3, 5], [4, 3, 5, 9], [1, 1, 2, 1]]
    assert [v.tolist() for v in _runs(PLANTED["contig_last_end"])] == \
        [[0, 2], [2, 8], [10, 12], [1, 1]]


def test_format_bedgraph():
    runs = _runs(PLANTED["contig_touch"])
    assert cc.format_bedgraph(["a", "b"], runs) == b"a\t3\t10\t1\nb\t0\t4\t1\n"


def test_tile_constant_matches_the_kernel():
    src = open(os.path.join(ROOT, "lime_amd", "csrc", "coverage.hip")).read()
    cvb = int(re.search(r"constexpr int CVB = (\d+);", src).group(1))
    items = int(re.search(r"constexpr int CV_ITEMS = (\d+);", src).group(1))
    assert "CV_TILE = CVB * CV_ITEMS" in src and cvb * items == T


# ---------------------------------------------------- header, library, CLI
def test_header_declares_and_library_exports_coverage():
    import ctypes
    from lime_amd import _ffi
    header = open(os.path.join(ROOT, "include", "lime_amd.h")).read()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("lime_coverage", "lime_result_depths", "lime_result_depth_device",
                 "lime_result_depth_stats"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _ffi.SIGNATURES, name
        assert getattr(lib, name) is not None, name


def test_cli_lists_coverage():
    r = subprocess.run([os.path.join(ROOT, "bin", "lime-submit")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0
    assert re.search(r"^\s*coverage : Compute the coverage over defined intervals$", r.stdout,
                     re.M)
