"""The multiinter reference (tests/multiinter_cases.py) against the per-base
paint, the planted cases against what they were planted for, and the
multiinter entry points of the header, the library and the CLI.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import multiinter_cases as mc
from tests.multiinter_cases import T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANTED = {c["name"]: c for c in mc.planted_cases()}


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _ref(case, m):
    return mc.multiinter_ref(case["sets"], case["lens"], m)


def _lists(runs):
    return [v.tolist() for v in runs]


@pytest.mark.parametrize("name", sorted(PLANTED))
def test_ref_equals_brute_on_planted(name):
    case = PLANTED[name]
    assert case["lens"].sum() <= 100_000  # every planted genome is small enough to paint
    for m in mc.modes(len(case["sets"])):
        assert _same(_ref(case, m), mc.brute(case["sets"], case["lens"], m)), m


def test_ref_equals_brute_on_random():
    shapes = 0
    for seed in range(2500):
        rng = np.random.default_rng(20_000 + seed)
        k = int(rng.integers(1, 7))
        lens = rng.integers(0, 300, int(rng.integers(1, 4)))  # (length-0 contigs stay empty)
        if lens.sum() == 0:
            lens[0] = 7
        case = mc.random_case(seed, k, int(rng.integers(1, 40)), lens, int(rng.integers(1, 50)))
        for c, s, e in case["sets"]:
            shapes += (e == s).any() + 2 * (e == case["lens"][c]).any()
        allrows = [np.concatenate([x[j] for x in case["sets"]]) for j in range(3)]
        shapes += 4 * bool(np.isin(allrows[1], allrows[2]).any())  # book-ends
        for m in mc.modes(k):
            assert _same(_ref(case, m), mc.brute(case["sets"], case["lens"], m)), (seed, m)
        # membership pieces tile the union and sum to the sets' unions
        mem = _ref(case, 0)
        uni = _ref(case, 1)
        assert int((mem[2] - mem[1]).sum()) == int((uni[2] - uni[1]).sum()), seed
        per_set = sum(int((r[2] - r[1]).sum()) for r in
                      (mc.multiinter_ref([x], case["lens"], 1) for x in case["sets"]))
        assert int(((mem[2] - mem[1]) * mc.popcount(mem[3])).sum()) == per_set, seed
    assert shapes > 2500  # zero widths, rows at contig ends and book-ends all occur


def test_small_cases_results():
    assert _lists(_ref(PLANTED["k1"], 0)) == [[0, 0], [3, 20], [9, 31], [1, 1]]
    assert _lists(_ref(PLANTED["k1"], 1)) == [[0, 0], [3, 20], [9, 31]]
    for m in (0, 1, 2, 3):
        assert all(len(v) == 0 for v in _ref(PLANTED["all_empty"], m))
    assert _lists(_ref(PLANTED["one_empty"], 0)) == \
        [[0, 0, 0], [3, 5, 9], [5, 9, 12], [1, 5, 4]]
    assert _lists(_ref(PLANTED["one_empty"], 2)) == [[0], [5], [9]]
    assert all(len(v) == 0 for v in _ref(PLANTED["one_empty"], 3))
    assert all(len(v) == 0 for v in _ref(PLANTED["zero_width_only"], 0))
    assert _lists(_ref(PLANTED["zero_width_inside"], 0)) == [[0], [2], [8], [1]]
    # a book-end inside one set: one run; across sets: two membership runs,
    # one consensus-1 run
    assert _lists(_ref(PLANTED["book_end_inside"], 0)) == [[0], [0], [9], [1]]
    assert _lists(_ref(PLANTED["book_end_across"], 0)) == [[0, 0], [0, 5], [5, 9], [1, 2]]
    assert _lists(_ref(PLANTED["book_end_across"], 1)) == [[0], [0], [9]]
    assert all(len(v) == 0 for v in _ref(PLANTED["book_end_across"], 2))
    full = 0xFFFFFFFF
    assert _lists(_ref(PLANTED["k32_identical"], 0)) == \
        [[0, 0], [10, 30], [20, 31], [full, full]]
    assert _lists(_ref(PLANTED["k32_identical"], 32)) == [[0, 0], [10, 30], [20, 31]]
    assert _lists(_ref(PLANTED["bit31_alone"], 0)) == [[0], [7], [11], [1 << 31]]
    assert mc.popcount([full, 1 << 31, 0, 5]).tolist() == [32, 1, 0, 2]


def test_tile_cases_have_the_event_counts():
    for n_ev in mc.TILE_EVENTS:
        case = PLANTED[f"tile_{n_ev}"]
        key, idx = mc.events(case)
        assert len(key) == n_ev and len(np.unique(key)) == n_ev  # every event a group
        assert set(idx.tolist()) == {0, 1, 2}
        assert len(_ref(case, 0)[0]) == n_ev // 2
    assert set(mc.TILE_EVENTS) == {T - 2, T, T + 2, 2 * T, 2 * T + 2}


def test_straddling_groups():
    case, x = mc._straddle(False)
    first, last = mc.group_span(case, x)
    assert (first, last) == (T - 30, T + 33) and last - first + 1 == 64
    # no class change at x in any mode: one membership run over [A, B)
    mem = _ref(case, 0)
    assert mem[3].tolist()[-1] == 0xFFFFFFFF and mem[1].tolist()[-1] < x < mem[2].tolist()[-1]
    case, x = mc._straddle(True)
    first, last = mc.group_span(case, x)
    assert (first, last) == (T - 30, T + 33)
    mem = _ref(case, 0)
    assert mem[3].tolist()[-2:] == [0xFFFFFFFF, 0x3FFFFFFF]
    assert mem[2].tolist()[-2] == x == mem[1].tolist()[-1]
    assert _ref(case, 32)[2].tolist()[-1] == x  # the 32-way AND ends there


def test_tile_edge_last_event_cases():
    case, a = mc._edge(True)
    assert mc.group_span(case, a) == (T - 2, T - 1)
    assert mc.group_span(case, a + 1) == (T, T)
    case, a = mc._edge(False)
    assert mc.group_span(case, a - 1) == (T - 2, T - 2)
    assert mc.group_span(case, a) == (T - 1, T)


def test_long_over_spans_more_than_three_tiles():
    case = PLANTED["long_over"]
    key, idx = mc.events(case)
    p = np.flatnonzero(idx == 31)
    assert len(p) == 2 and p[0] == 0 and p[1] == len(key) - 1 and p[1] > 3 * T
    mem = _ref(case, 0)
    assert (mem[3] & (1 << 31) != 0).all()  # bit 31 on every run
    assert len(_ref(case, 2)[0]) == (7 * T) // 4


def test_zero_width_group_spans_tiles():
    case = PLANTED["zero_width_5000"]
    first, last = mc.group_span(case, 700)
    assert last - first + 1 == 2 * 5000 + 1 and last // T - first // T >= 4
    assert _lists(_ref(case, 0)) == [[0, 0, 0], [100, 700, 800], [700, 800, 900], [4, 6, 2]]


def test_heads_at_wave_and_thread_edges():
    case, pos = mc._heads_at()
    key, idx = mc.events(case)
    assert np.flatnonzero(idx == 2).tolist() == pos == [63, 64, 511, 512]
    assert len(np.unique(key)) == len(key)
    got = _ref(case, 4)
    assert len(got[0]) == 2 and (got[2] - got[1]).tolist() == [1, 1]


def test_contig_cases_results():
    # never joined across contigs, not even at min_sets = 1
    assert _lists(_ref(PLANTED["contig_touch"], 1)) == [[0, 1, 2], [3, 0, 0], [10, 4, 6]]
    assert _lists(_ref(PLANTED["contig_touch"], 0)) == \
        [[0, 0, 1, 1, 2], [3, 8, 0, 2, 0], [8, 10, 2, 4, 6], [1, 3, 3, 1, 2]]
    assert _lists(_ref(PLANTED["contig_empty"], 2)) == [[0, 2], [2, 2], [4, 3]]
    assert _lists(_ref(PLANTED["contig_last_only"], 0)) == [[3, 3], [2, 9], [9, 12], [1, 3]]
    assert _lists(_ref(PLANTED["contig_last_only"], 2)) == [[3], [9], [12]]


def test_format_multiinter():
    assert mc.format_multiinter(["a"], _ref(PLANTED["book_end_across"], 0)) == \
        b"a\t0\t5\t1\t1\na\t5\t9\t1\t2\n"
    assert mc.format_multiinter(["a"], _ref(PLANTED["book_end_across"], 1)) == b"a\t0\t9\n"
    assert mc.format_multiinter(["a"], _ref(PLANTED["bit31_alone"], 0)) == \
        b"a\t7\t11\t1\t2147483648\n"


def test_tile_constant_matches_the_kernel():
    src = open(os.path.join(ROOT, "lime_amd", "csrc", "multiinter.hip")).read()
    mib = int(re.search(r"constexpr int MIB = (\d+);", src).group(1))
    items = int(re.search(r"constexpr int MI_ITEMS = (\d+);", src).group(1))
    assert "MI_TILE = MIB * MI_ITEMS" in src and mib * items == T


# ---------------------------------------------------- header, library, CLI
def test_header_declares_and_library_exports_multiinter():
    import ctypes
    from lime_amd import _ffi
    header = open(os.path.join(ROOT, "include", "lime_amd.h")).read()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("lime_multiinter", "lime_result_masks", "lime_result_mask_device"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _ffi.SIGNATURES, name
        assert getattr(lib, name) is not None, name
    assert re.search(r"#define LIME_ABI_VERSION 6\b", header)


def test_cli_lists_multiinter():
    r = subprocess.run([os.path.join(ROOT, "bin", "lime-submit")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0
    assert re.search(r"^\s*multiinter : Regions by the input sets that cover them "
                     r"\(membership, or at least -min of them\)$", r.stdout, re.M)
