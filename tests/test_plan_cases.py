"""The plan-edge inputs of tests/plan_cases.py checked on the CPU: the source
lines the restatements quote still stand in intersect.hip, every planted
case lands on the side of its dispatch condition that its name says, and the
restated plan counts (and, where it is listed, emits) exactly what the C
oracle does.  Exact integer equality throughout."""
import re

import numpy as np
import pytest

from oracle import oracle
from tests import plan_cases as pc


def _rows(recs):
    r = np.asarray(recs, np.int64).reshape(-1, 4)
    return r[np.lexsort(r.T[::-1])]


def _oracle_rows(exp):
    return _rows(np.stack([exp[k] for k in ("start", "end", "a_row", "b_row")], axis=1))


def _check_against_oracle(A, B, lens, threshold=0, records=True):
    """restated plan == oracle: the count, and the records as sorted rows"""
    plan = pc.Plan(A, B, lens, threshold)
    exp = oracle.intersect(A, B, threshold)
    assert plan.total == len(exp["start"])
    assert plan.ranges_inside_windows()
    if records:
        assert np.array_equal(_rows(plan.records()), _oracle_rows(exp))
    return plan, exp


# ------------------------------------------------------------------ sources
def test_dispatch_conditions_match_the_sources():
    src = pc._read("lime_amd", "csrc", "intersect.hip")
    for name, pat in pc.SOURCE_LINES.items():
        assert re.search(pat, src), name
    assert pc.fill_wgs() == 2 and pc.fill_cap(1) == 2048 and pc.fill_cap(2) == 2496
    assert pc.overflow_code() == 7
    # the sort's tile geometry the set-statistics tests plant on
    sort = pc._read("lime_amd", "csrc", "sort.hip")
    for pat in (r"constexpr int RB = 512;", r"constexpr int RITEMS = 16;",
                r"constexpr int RTILE = RB \* RITEMS;", r"constexpr int PCMAX = 1024;",
                r"constexpr int WITEMS = RTILE / RWAVES;",
                r"if \(k > 0\) \{\s*\n\s*p0 = l0, p1 = l1, pok = lok;",
                r"if \(p0 > g0 \|\| \(p0 == g0 && p1 > p0 && g1 == g0\)\) uns = 1;"):
        assert re.search(pat, sort), pat


# ------------------------------------------------------- a / b / c: windows
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("k", pc.COUNT_WINDOW_K)
def test_count_window_cases(k, flip):
    case = pc.dense_case(pc.COUNT_WINDOW_N, k)
    A, B = pc.oriented(case, flip)
    plan, _ = _check_against_oracle(A, B, case["lens"])
    assert plan.total == case["pairs"] == 1025 * k
    wl = plan.wlen(flip)  # the stream that owns the pairs
    assert wl[0] == 1023 + k and wl[0] - pc.WCAP == k - pc.COUNT_WINDOW_K[1]
    assert (wl[0] <= pc.WCAP) == (k <= pc.COUNT_WINDOW_K[1])  # in_lds
    assert (wl[1:] <= pc.WCAP).all() and (plan.wlen(1 - flip) <= pc.WCAP).all()
    assert plan.lane == [True, True] and not plan.filtered and plan.tpf == 1
    assert (plan.tile_sums[flip] == [1024 * k, k]).all() and plan.tile_sums[1 - flip].sum() == 0


def test_count_window_lengths():
    assert [1023 + k for k in pc.COUNT_WINDOW_K] == [4095, 4096, 4097]
    assert [1023 + k for k in pc.fill1_window_k()] == [2047, 2048, 2049]
    assert [2047 + k for k in pc.FILL2_WINDOW_K] == [2495, 2496, 2497]


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("k", pc.fill1_window_k())
def test_fill1_window_cases(k, flip):
    case = pc.dense_case(pc.FILL1_WINDOW_N, k)
    A, B = pc.oriented(case, flip)
    plan, _ = _check_against_oracle(A, B, case["lens"])
    cap = pc.fill_cap(1)
    assert plan.tpf == 1 and not plan.filtered
    cw = plan.commit_wlen(flip)
    assert cw[0] == 1023 + k and (cw[0] <= cap) == (k <= cap - 1023)  # par_lds
    assert cw[0] - cap == k - (cap - 1023)
    assert (plan.wlen(flip) <= pc.WCAP).all()


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("k", pc.FILL2_WINDOW_K)
def test_fill2_window_cases(k, flip):
    case = pc.dense_case(pc.FILL2_WINDOW_N, k, pc.FILL2_IDLE)
    A, B = pc.oriented(case, flip)
    plan, _ = _check_against_oracle(A, B, case["lens"])
    assert plan.total == 2049 * k
    assert plan.total < pc.FILL_SPARSE * (plan.own[0] + plan.own[1]) and plan.tpf == 2
    # without the idle rows the same owners take the one-tile fill
    bare = pc.dense_case(pc.FILL2_WINDOW_N, k)
    assert pc.Plan(*pc.oriented(bare, flip), bare["lens"]).tpf == 1
    cw = plan.commit_wlen(flip)
    assert cw[0] == 2047 + k and (cw[0] <= pc.PCAP2) == (k <= pc.FILL2_WINDOW_K[1])
    assert (cw[1:] <= pc.PCAP2).all() and (plan.commit_wlen(1 - flip) <= pc.PCAP2).all()
    # the last, odd, tile is a commit of its own: one owner
    assert len(cw) == 2 and (plan.tile_sums[flip] == [1024 * k, 1024 * k, k]).all()


# ------------------------------------------------- d: the windows kernel switch
@pytest.mark.parametrize("place", sorted(pc.WIDE_PLACES))
@pytest.mark.parametrize("width", [pc.WLANE_MAX, pc.WLANE_MAX + 1])
def test_wide_cases(width, place):
    case = pc.wide_case(width, place)
    A, B = case["A"], case["B"]
    for X, r in zip((A, B), case["wide_rows"]):
        gs, ge, order = pc.canonical(X, case["lens"])
        assert order[case["pos"]] == r and ge[case["pos"]] - gs[case["pos"]] == width
        w = X[2] - X[1]
        assert w[r] == width == w.max() and np.sum(w > 400) == 1
        assert (X[2] <= case["lens"][0]).all()
    for t in pc.WIDE_THRESHOLDS:
        plan, _ = _check_against_oracle(A, B, case["lens"], t)
        assert plan.owmax == [width, width]
        assert plan.lane == [width <= pc.WLANE_MAX] * 2
        assert plan.filtered == (t >= 1)  # zero-width rows in both sets
        # the wide row's own range needs the whole owner-width bound: a window
        # from the other rows' widths alone would cut its partners off
        for st in (0, 1) if place != "set_last" else ():
            i = case["pos"]
            assert plan.hi[st][i] - plan.lo[st][i] > 500
            ogs, _, _ = plan.sets[st]
            pgs = plan.sets[1 - st][0]
            narrow = pc.windows_lane(ogs, pgs, plan.own[st], st, plan.tp, 400)
            assert narrow[i // pc.OT, 1] < plan.hi[st][i]


@pytest.mark.parametrize("maxw", pc.WINDOW_MAXW)
def test_window_cases(maxw):
    case = pc.window_case(maxw)
    assert pc.set_stats(case["A"])[1] == maxw
    owmax = maxw + 2 * case["d"]  # owmax = O->max_width + 2 * reach (stream 0)
    assert owmax == pc.WLANE_MAX + (maxw - pc.WINDOW_MAXW[0])
    assert pc.uses_lane_windows(owmax) == (maxw == pc.WINDOW_MAXW[0])
    exp = oracle.window(case["A"], case["B"], case["d"])
    assert 100_000 < len(exp["start"]) < 1_000_000


# --------------------------------------------- e / f: filtered, owned prefixes
@pytest.mark.parametrize("t", pc.TWO_STREAM_THRESHOLDS)
def test_two_stream_filtered(t):
    case = pc.two_stream_case()
    plan, exp = _check_against_oracle(case["A"], case["B"], case["lens"], t)
    assert plan.filtered and plan.stats[0][2] and plan.stats[1][2]
    assert (plan.total == 0) == (t == 161)
    if t < 161:
        assert 0 < plan.n0 < plan.total and len(plan.sums) == 6
        assert (plan.sums > 0).all()


@pytest.mark.parametrize("t", pc.OWNED_THRESHOLDS)
def test_owned_prefixes_restated(t):
    # the expected answer of an owned plan: the oracle's pairs whose owner's
    # sorted position is below the owned count == the restated plan's records
    case = pc.two_stream_case()
    A, B = case["A"], case["B"]
    exp = oracle.intersect(A, B, t)
    pos = []
    for X in (A, B):
        order = pc.canonical(X, case["lens"])[2]
        inv = np.empty(len(order), np.int64)
        inv[order] = np.arange(len(order))
        pos.append(inv)
    a_owns = B[1][exp["b_row"]] >= A[1][exp["a_row"]]
    full = _oracle_rows(exp)
    for a_own, b_own in [(0, 0), (1, 3000), (1023, 1025), (1024, 0), (3000, 1)]:
        plan = pc.Plan(A, B, case["lens"], t, a_own, b_own)
        keep = np.where(a_owns, pos[0][exp["a_row"]] < a_own, pos[1][exp["b_row"]] < b_own)
        want = _rows(np.stack([exp[k][keep] for k in ("start", "end", "a_row", "b_row")], axis=1))
        assert np.array_equal(_rows(plan.records()), want)
        assert plan.filtered == (t == 40)
    assert len(full) == pc.Plan(A, B, case["lens"], t).total


# ------------------------------------------------------ g: u32 tile offsets
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("m", pc.PILE_M)
def test_pile_cases(m, flip):
    # (the oracle is not affordable at 2^31 pairs: the count is analytic)
    case = pc.pile_case(m)
    A, B = pc.oriented(case, flip)
    plan = pc.Plan(A, B, case["lens"])
    assert plan.total == 1024 * m == case["pairs"]
    assert plan.tile_sums[flip][0] == 1024 * m and plan.tile_sums[flip][1:].sum() == 0
    assert plan.tile_sums[1 - flip].sum() == 0
    want = {2**21 - 1: (2**31 - 1024, False, False), 2**21: (2**31, True, False),
            2**22 - 1: (2**32 - 1024, True, False), 2**22: (2**32, False, True)}[m]
    assert (plan.total, plan.half, plan.overflow) == want
    assert plan.tpf == 1 and not plan.filtered
    assert plan.lane[flip] is False and plan.lane[1 - flip] is True
    assert plan.wlen(flip)[0] == m > pc.WCAP
    # the analytic records are the restated plan's (checked on the first
    # owners: owner i's range is all of the partner set)
    assert (plan.lo[flip] == 0).all() and (plan.hi[flip] == m).all()
    rec = pc.pile_records(m, 5 * m - 2, 4, flip)
    assert rec[:, 2 + flip].tolist() == [4, 4, 5, 5]
    assert rec[:, 3 - flip].tolist() == [m - 2, m - 1, 0, 1]
    assert rec[:, 0].tolist() == [m - 1, m, 1, 2] and (rec[:, 1] == rec[:, 0] + 1).all()
    for first, count in pc.pile_windows(m):
        assert 0 <= first and first + count <= plan.total


def test_pile_records_small():
    # the analytic record formula against the oracle at a size it affords
    # (the same construction with 5 owners and m = 7)
    m = 7
    b_s = np.arange(1, m + 1, dtype=np.int64)
    A = (np.zeros(5, np.int32), np.zeros(5, np.int64), np.full(5, m + 1, np.int64))
    B = (np.zeros(m, np.int32), b_s, b_s + 1)
    for flip, (X, Y) in enumerate([(A, B), (B, A)]):
        exp = oracle.intersect(X, Y)
        assert np.array_equal(_rows(pc.pile_records(m, 0, 5 * m, flip)), _oracle_rows(exp))
        assert np.array_equal(pc.Plan(X, Y, [m + 9]).records(), pc.pile_records(m, 0, 5 * m, flip))
