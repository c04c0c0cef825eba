"""The subtract-edge inputs of tests/subtract_cases.py checked on the CPU: the
source lines the restatements quote still stand in subtract.hip, every planted
case sits on the side of its capacity or dispatch condition that its name
says, and the comb's closed-form record counts are the C oracle's.  Exact
integer equality throughout."""
import re

import numpy as np
import pytest

from oracle import oracle
from tests import subtract_cases as sc


def _closed_matches_oracle(case, t=0):
    """per input row: the comb's closed-form counts == the oracle's"""
    for col, mode in ((0, sc.SET), (1, sc.LIME)):
        exp = sc.expected(case, t, mode)
        got = np.bincount(exp["a_row"], minlength=len(case["A"][1]))
        assert np.array_equal(got, case["closed"][:, col]), mode


def _total(case, t, mode):
    return len(sc.expected(case, t, mode)["start"])


# ------------------------------------------------------------------ sources
def test_conditions_match_the_source():
    src = sc._source()
    for name, pat in sc.SOURCE_LINES.items():
        assert re.search(pat, src), name
    assert (sc.SUB_B, sc.TIE_G, sc.SCAP, sc.BWIN) == (256, 16, 512, 1024)
    assert (sc.CNT_WAVES, sc.CNT_WIN, sc.CNT_ROWS) == (4, 1536, 1024)
    assert (sc.FW, sc.FCAP, sc.FWIN, sc.FROWS, sc.GUESS) == (8, 896, 3072, 2048, 4096)


def test_comb_closed_form_counts():
    # the counts the comb is built on: 1024 rows crossing m teeth give 1024 m
    # records in set mode and 2048 m in lime mode; inside rows none, gap rows
    # one; copies of a tooth and the zero-width row change no count
    for m in (1, 3, 300):
        case = sc.comb(np.arange(1024), np.full(1024, m), 1024 + m + 2)
        case["key"] = ("closed", m)
        assert _total(case, 0, sc.SET) == 1024 * m and _total(case, 0, sc.LIME) == 2048 * m
        _closed_matches_oracle(case)
    copies = np.ones(1030, np.int64)
    copies[::3] = 5
    case = sc.comb(np.arange(1024), sc._pattern(1024), 1030, copies=copies, zw=True)
    case["key"] = ("closed", "mixed")
    for t in (0, -3, 1):
        _closed_matches_oracle(case, t)
    m = sc.Model(case["A"], case["B"])
    assert m.zw and m.runs == 1031 and m.nb == 1031 + 4 * 344 and m.max_group == 5


def test_expected_order_is_the_sorted_sets():
    case = sc.switch_case(64)  # 128 left rows per tooth: ties on start
    A = case["A"]
    order = sc.sorted_rows(A)
    key = list(zip(A[1][order], A[2][order] > A[1][order], order))
    assert key == sorted(key) and sorted(order) == list(range(len(order)))
    raw = oracle.subtract(A, case["B"], 0, sc.LIME)
    exp = sc.expected(case, 0, sc.LIME)
    pos = np.empty(len(order), np.int64)
    pos[order] = np.arange(len(order))
    assert (np.diff(pos[exp["a_row"]]) >= 0).all()  # left rows in sorted order
    for r in (int(exp["a_row"][0]), int(exp["a_row"][len(exp["a_row"]) // 2])):
        for k in ("start", "end", "b_row"):  # a row's records in the oracle's order
            assert np.array_equal(exp[k][exp["a_row"] == r], raw[k][raw["a_row"] == r])
    assert sorted(zip(*[exp[k] for k in ("a_row", "start", "end", "b_row")])) == \
        sorted(zip(*[raw[k] for k in ("a_row", "start", "end", "b_row")]))
    assert not np.array_equal(order, np.arange(len(order)))  # (rows are shuffled)


# --------------------------------------------------------- a. the fused stage
@pytest.mark.parametrize("zw", [False, True])
@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("total", sc.STAGE_T)
def test_stage_cases(total, mode, zw):
    case = sc.stage_case(total, mode, zw)
    m = sc.model(case)
    _closed_matches_oracle(case)
    exp = sc.expected(case, 0, mode)
    assert m.totals(exp, sc.FROWS).tolist() == [total]
    assert (total <= sc.FCAP) == (total != sc.STAGE_T[2]) and total - sc.FCAP in (-1, 0, 1)
    assert m.path(0, total) == ("fused_scan" if zw else "fused_ls")
    assert m.path(0, total, no_ls=True) == "fused_scan"
    assert m.tile_wlen.tolist() == [sc.FROWS + 2] and m.fused_past_stage(0) == 0


@pytest.mark.parametrize("zw", [False, True])
@pytest.mark.parametrize("mode", sc.MODES)
def test_stage3_cases(mode, zw):
    case = sc.stage3_case(mode, zw)
    m = sc.model(case)
    _closed_matches_oracle(case)
    T = m.totals(sc.expected(case, 0, mode), sc.FROWS).tolist()
    assert T == sc.STAGE3_T and T[0] <= sc.FCAP < T[1] and T[2] <= sc.FCAP
    assert m.path(0, sum(T)) == ("fused_scan" if zw else "fused_ls")
    assert m.path(0, sum(T), no_ls=True) == "fused_scan"


# ----------------------------------------- b. local-scan switch, fused window
@pytest.mark.parametrize("W", sc.WINDOW_W + [sc.WINDOW_LONG])
def test_window_cases(W):
    for zw in (False, True):
        case = sc.window_case(W, zw)
        m = sc.model(case)
        _closed_matches_oracle(case)
        total = _total(case, 0, sc.SET)
        assert m.tile_wlen.tolist() == [W] and m.ntiles == 1 and m.zw == zw
        assert m.ls == (not zw and W <= sc.FWIN)
        assert m.path(0, total) == ("fused_ls" if m.ls else "fused_scan")
        assert m.path(0, total, no_ls=True) == "fused_scan"
        # rows whose bounds fall past the stage take the general fold
        past = m.fused_past_stage(0)
        assert (past > 0) == (W > sc.FWIN)
        if W == sc.WINDOW_LONG:
            assert W > 4 * sc.FWIN and past > 700
    assert sc.WINDOW_W == [3071, 3072, 3073]


def test_ends_cases():
    case = sc.ends_case(False)
    m = sc.model(case)
    assert m.ls and m.path(0, 1) == "fused_ls"
    assert int(m.ags[0]) - m.maxw_b < 0 and m.ags[0] < m.bgs[0]  # before every B row
    bl, bh, nst = m.fused_bounds(0)
    assert nst == m.nb == sc.FWIN - 1 and m.tile_wlen.tolist() == [sc.FWIN]
    assert bh[-1] == nst and bl[-1] < nst and (bh[:-1] < nst).all()  # a.e bound exactly nst
    assert m.age[-1] > m.bgs[-1]
    # the first row has no hit; the last one crosses B's last tooth
    exp = sc.expected(case, 0, sc.SET)
    first, last = m.aorder[0], m.aorder[-1]
    assert exp["b_row"][exp["a_row"] == first].tolist() == [-1]
    assert (exp["a_row"] == last).sum() == 2
    z = sc.model(sc.ends_case(True))
    assert z.zw and not z.ls and z.path(0, 1) == "fused_scan" and int(z.ags[0]) - z.maxw_b < 0


# ------------------------------------------------ c. partial and many tiles
@pytest.mark.parametrize("na", sc.TILE_NA)
def test_tiles_cases(na):
    for zw in (False, True):
        case = sc.tiles_case(na, zw)
        m = sc.model(case)
        _closed_matches_oracle(case)
        assert m.na == na and m.ntiles == (na + 2047) // 2048
        assert m.path(0, 1) == ("fused_scan" if zw else "fused_ls")
        assert _total(case, 0, sc.SET) > 0
    assert sc.TILE_NA == [1, 1023, 1024, 1025, 2047, 2048, 2049]


def test_many_tiles_cases():
    for zw in (False, True):
        case = sc.many_tiles_case(zw)
        m = sc.model(case)
        _closed_matches_oracle(case)
        assert m.na == 40 * 1024 + 1 and m.ntiles == 21
        assert m.path(0, 10**6) == ("fused_scan" if zw else "fused_ls")
        for mode, u in ((sc.SET, 1), (sc.LIME, 2)):
            T = m.totals(sc.expected(case, 0, mode), sc.FROWS)
            want = [{"e": 0, "u": 2048 * u}.get(n) if n in "eu" else u * int(n[1:])
                    for n in sc.MANY_PLAN] + [u]
            assert T.tolist() == want
            empty, staged, direct = T == 0, (T > 0) & (T <= sc.FCAP), T > sc.FCAP
            assert empty.sum() == 6 and staged.sum() >= 6 and direct.sum() >= 6
            assert T[0] > 0 and T[-1] > 0          # records in the first and the last tile
            assert empty[1] and empty[2] and T[3] > sc.FCAP  # a look-back across empty tiles
            # a tile behind two with records: its exclusive prefix sums several
            assert T[5] > 0 and T[6] > 0 and T[3] > 0 and T[4] > 0
        lime = m.totals(sc.expected(case, 0, sc.LIME), sc.FROWS)
        assert lime[8] == sc.FCAP and lime[9] == sc.FCAP + 2


# ---------------------------------------------------------- d. output guess
@pytest.mark.parametrize("last", sorted(sc.GUESS_LAST))
@pytest.mark.parametrize("delta", sc.GUESS_DELTA)
def test_guess_cases(delta, last):
    for mode in sc.MODES:
        for zw in (False, True):
            case = sc.guess_case(delta, last, mode, zw)
            m = sc.model(case)
            _closed_matches_oracle(case)
            exp = sc.expected(case, 0, mode)
            T = m.totals(exp, sc.FROWS)
            cap = m.na + sc.GUESS
            assert T.sum() == len(exp["start"]) == cap + delta
            assert T.tolist() == sc.guess_tile_totals(delta, last)
            assert m.path(0, int(T.sum())) == ("fused_scan" if zw else "fused_ls")
            # the tile holding record `cap` (delta > 0: the pass runs again)
            assert (T[2] <= sc.FCAP) == (last == "staged")
            assert T[:2].sum() < cap and (T.sum() > cap) == (delta > 0)
    # every row crossing 5 teeth: exactly na + 4096 in set mode
    case = sc.comb(np.arange(1024), np.full(1024, 5), 1032)
    assert len(oracle.subtract(case["A"], case["B"], 0, sc.SET)["start"]) == 1024 + sc.GUESS


# ------------------------------------------- e. switches of the two-pass side
@pytest.mark.parametrize("runs", sc.SWITCH_RUNS)
def test_switch_cases(runs):
    case = sc.switch_case(runs)
    m = sc.model(case)
    _closed_matches_oracle(case)
    assert m.zw and not m.ls and m.runs == runs and m.na == 4096
    assert (m.runs * 64 >= m.na) == (runs == 64) and abs(m.runs * 64 - m.na) <= 64
    total = _total(case, 0, sc.SET)
    assert m.path(0, total) == ("fused_scan" if runs == 64 else "two_pass")
    assert m.path(1, total) == "walk"


@pytest.mark.parametrize("na", sc.SPARSE_NA)
def test_sparse_cases(na):
    case = sc.sparse_case(na)
    m = sc.model(case)
    _closed_matches_oracle(case)
    for mode in sc.MODES:
        assert _total(case, 0, mode) == 1
    assert m.runs * 64 < m.na and m.nblk == (16 if na == 4096 else 17)
    assert m.sparse(1) == (m.nblk == 17)
    assert m.path(0, 1) == ("two_pass_sweep" if m.nblk == 17 else "two_pass")


# ------------------------------------------------------ f. rcnt saturation
@pytest.mark.parametrize("m_", sc.RCNT_M)
def test_rcnt_cases(m_):
    case = sc.rcnt_case(m_)
    m = sc.model(case)
    _closed_matches_oracle(case)
    assert m.na == sc.rcnt_na(m_) and m.runs * 64 < m.na and m.zw
    for mode, u in ((sc.SET, 1), (sc.LIME, 2)):
        exp = sc.expected(case, 0, mode)
        rc = m.row_counts(exp)
        assert rc.max() == u * m_ and (rc == rc.max()).sum() == 1 and np.sort(rc)[-2] <= 2
        i = int(rc.argmax())
        assert i // sc.SUB_B == 0 and rc[i + 1:sc.SUB_B].sum() > 0  # records placed after it
        assert m.path(0, int(rc.sum())) == "two_pass"
    assert {254, 255, 256} <= set(sc.RCNT_M)             # each of them in set mode,
    assert {254, 256} <= {2 * k for k in sc.RCNT_M}      # the even ones in lime mode too
    assert 2 * 300 > sc.SCAP  # well over the block's stage, in one row


# ------------------------------------------------------------------ g. SCAP
@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("total", sc.SCAP_T)
def test_scap_cases(total, mode):
    case = sc.scap_case(total, mode)
    m = sc.model(case)
    _closed_matches_oracle(case)
    _closed_matches_oracle(case, 1)
    for t in (0, 1):
        T = m.totals(sc.expected(case, t, mode), sc.SUB_B)
        assert T[sc.SCAP_BLOCK] == total and T[sc.SCAP_BLOCK + 1] == 0
        assert (T[:sc.SCAP_BLOCK] > 0).all() and (T[sc.SCAP_BLOCK + 2:] > 0).all()
        assert np.delete(T, sc.SCAP_BLOCK).max() < sc.SCAP
        assert m.path(t, int(T.sum())) == ("walk" if t else "two_pass")
    assert sc.SCAP_T == [511, 512, 513]


# ------------------------------------------------------- h. BWIN and CNT_WIN
@pytest.mark.parametrize("span", sc.BWIN_SPAN)
def test_bwin_walk_cases(span):
    case = sc.bwin_walk_case(span)
    m = sc.model(case)
    _closed_matches_oracle(case, 1)
    _closed_matches_oracle(case, 0)
    assert m.walk_block_window(0, 1) == span and (span <= sc.BWIN) == (span == 1024)
    assert all(m.walk_block_window(b, 1) <= sc.BWIN for b in range(1, m.nblk))
    assert m.nblk == 3 and m.path(0, 1) == "fused_ls"


@pytest.mark.parametrize("c", sc.BWIN_RUNS_COPIES)
def test_bwin_runs_cases(c):
    case = sc.bwin_runs_case(c)
    m = sc.model(case)
    _closed_matches_oracle(case)
    assert m.max_group == sc.TIE_G and m.runs == 71 and m.runs * 64 < m.na
    wlo, need, nst = m.runs_block_window(0)
    assert wlo == 0 and need == 1009 + c and nst == sc.BWIN
    assert (need <= sc.BWIN) == (c == sc.BWIN_RUNS_COPIES[0]) and need - sc.BWIN in (0, 1)
    # the staged starts pass the block's largest end only when it fits
    r0 = m.age[:sc.SUB_B].max()
    assert (m.bgs[nst - 1] >= r0) == (need <= sc.BWIN)
    assert all(m.runs_block_window(b)[1] <= sc.BWIN for b in range(1, m.nblk))
    total = _total(case, 0, sc.SET)
    assert m.path(0, total) == "two_pass"


@pytest.mark.parametrize("c", sc.CNT_WIN_COPIES)
def test_cnt_win_cases(c):
    case = sc.cnt_win_case(c)
    m = sc.model(case)
    _closed_matches_oracle(case)
    wlo, wlen = m.count_windows()
    assert wlo[0] == 0 and wlen[0] == 1521 + c and wlen[0] - sc.CNT_WIN == c - 15
    assert (wlen[1:] <= sc.CNT_WIN).all()
    assert (m.count_past_stage(0) > 0) == (wlen[0] > sc.CNT_WIN)
    assert all(m.count_past_stage(w) == 0 for w in range(1, len(wlo)))
    assert m.max_group == sc.TIE_G and m.runs * 64 < m.na
    assert m.path(0, _total(case, 0, sc.SET)) == "two_pass"


def test_cnt_wide_case():
    case = sc.cnt_wide_case()
    m = sc.model(case)
    assert m.zw and m.runs * 64 < m.na and m.maxw_b == 10 * sc.CNT_WIDE_Q - 7
    assert m.path(0, _total(case, 0, sc.SET)) == "two_pass"
    wlo, wlen = m.count_windows()
    wide = int(np.flatnonzero(m.bge - m.bgs == m.maxw_b)[0])
    assert wide == 2  # early in the set
    # the windows of the workgroups under the wide row start at or before it
    # and grow with every workgroup; past the stage's reach they stage nothing
    # their rows need, and the last workgroup's (past the wide row) reaches
    # back under it
    assert (wlo[:-1] <= wide).all() and (np.diff(wlen[:-1]) == 256).all()
    assert wlen[0] <= sc.CNT_WIN < wlen[-3] and wlen.max() > 2000 and wlen[-1] > sc.CNT_WIN
    past = [m.count_past_stage(w) for w in range(len(wlo))]
    assert past[0] == 0 and past[-3:] == [sc.CNT_ROWS, sc.CNT_ROWS, m.na % sc.CNT_ROWS]
    # left rows under the wide row give nothing, those past it their own records
    exp = sc.expected(case, 0, sc.LIME)
    rc = m.row_counts(exp)
    under = (m.ags > 15) & (m.age < 10 * sc.CNT_WIDE_Q + 8)
    assert under.sum() > 7000 and rc[under].sum() == 0 and rc[~under].sum() > 100


# --------------------------------------------------------------- i. tie index
@pytest.mark.parametrize("place", sc.TIE_PLACES)
@pytest.mark.parametrize("g", sc.TIE_SIZES)
def test_tie_cases(g, place):
    case = sc.tie_case(g, place)
    m = sc.model(case)
    G = sc.tie_tooth(g, place)
    grp = np.flatnonzero(m.bgs == 10 * G)
    assert m.max_group == g == len(grp) and not m.zw and m.ls
    ends = m.bge[grp]
    assert len(set(ends.tolist())) == g and (np.diff(ends) < 0).any()  # shuffled ends
    if place.startswith("last"):
        assert grp[-1] == m.nb - 1 and m.nb % 4 == int(place[-1])
    elif place == "whole":
        assert m.nb == g
    else:
        assert grp[0] > 500 and grp[-1] < m.nb - 500
    # k_tie_detect flags a group past TIE_G rows: gs[j] == gs[j + TIE_G]
    flagged = bool((m.bgs[:-sc.TIE_G] == m.bgs[sc.TIE_G:]).any()) if m.nb > sc.TIE_G else False
    assert flagged == (g > sc.TIE_G)
    row_of = {int((e - 6) // 10 - G): int(r) for e, r in zip(ends, m.border[grp])}
    assert sorted(row_of) == list(range(g))
    for mode in sc.MODES:
        exp = sc.expected(case, 0, mode)

        def heads(p):
            r = m.aorder[np.flatnonzero(m.ags == 10 * p + 2)[0]]
            return exp["b_row"][exp["a_row"] == r].tolist()
        # the group as a spanning block's head: row p - G of it, for every p
        # (set mode names a gap after the block that follows it: lime mode)
        for p in range(G + 1, G + g) if mode == sc.LIME else ():
            assert row_of[p - G] in heads(p), p
        # and as an inside block's head: the row ending first
        assert row_of[0] in heads(G - 2) and row_of[0] in heads(G - 1)
    # the head is the group's first row in device order for few of the probes
    assert row_of[1] != min(row_of.values()) or row_of[2] != min(row_of.values())
