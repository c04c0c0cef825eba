"""The closest-edge inputs of tests/closest_cases.py checked on the CPU: the
source lines the restatement quotes still stand in closest.hip (each exactly
once), every planted case has the property it is named for (computed by the
restatement), the restatement's records are the C oracle's on every case, and
wrong variants of the restated searches, of the window bound and of the fill
filter disturb a planted case.  Exact integer equality throughout."""
import re

import numpy as np
import pytest

from tests import closest_cases as cc
from tests.test_closest import _case, _sorted_rows, decomposed_py


def _records(st):
    return st.a_row.tolist(), st.b_row.tolist()


def _same_as_oracle(case, st=None, mode=0):
    st = st or (cc.state(case) if mode == 0 else cc.single_py(case))
    exp = cc.expected(case, mode)
    assert _records(st) == (exp["a_row"].tolist(), exp["b_row"].tolist())
    return st


def _arms(st, prefix):
    return {k[len(prefix):]: v for k, v in st.trace.items() if k.startswith(prefix) and v}


# ------------------------------------------------------------------ sources
def test_conditions_match_the_source():
    src = cc.source()
    for name, pat in cc.SOURCE_LINES.items():
        assert len(re.findall(pat, src)) == 1, name
    assert len(re.findall(cc.OCAP_STAGE_L, src)) == 6
    assert (cc.CB, cc.MAX_ROUNDS, cc.OCAP, cc.DSH, cc.SWIN) == (256, 32, 4096, 12, 2048)
    assert 1 << cc.DSH == 4096 and cc.NONE == 0xFFFFFFFF


def test_levels_pad_the_tails():
    v = np.full(cc.JAG_NR, cc.NONE, np.int64)
    v[-1] = 7
    l1, l2 = cc.levels(v, True)
    assert (len(l1), len(l2)) == (196, 4) and cc.JAG_NR % 64 and len(l1) % 64
    assert l1[-1] == 7 and l2[-1] == 7 and set(l1[:-1]) == {cc.NONE} == set(l2[:-1])
    l1, l2 = cc.levels(v, True, tail=False)   # the wrong variant loses both tails
    assert l1[-1] == cc.NONE and l2[-1] == cc.NONE
    m1, m2 = cc.levels([5] * 65, False)
    assert m1 == [5, 5] and m2 == [5]         # maxima pad with 0
    assert cc.first_hit([9] * 70, *cc.levels([9] * 70, True), 3, 70, 8, True) == 70


# ------------------------------------------------------------- a. jag skip
@pytest.mark.parametrize("q", cc.JAG_Q)
def test_jag_cases(q):
    case = cc.jag_case(q)
    st = _same_as_oracle(case)
    nr = cc.JAG_NR
    assert st.nR == nr and st.A == [nr] and st.N == [nr]           # every right covers
    assert st.stuck == {0: (0, q)} and st.J == [q] and st.D == [0]
    lo, hi, k, arms = st.stuck_search
    assert (lo, hi, k) == (1, nr, q)
    assert [kk for kk in range(nr) if st.jag[kk] != cc.NONE] == [q]
    assert len(st.a_row) == q                                       # rights 0 .. q - 1
    # the arms the search takes
    if q < 64:
        assert arms == {"hit_head": 1}
    else:
        assert arms["head_to_edge"] == 1 and arms["hit_row_%d" % (q % 64)] == 1
        assert arms.get("skip_4096", 0) == (q >> 12) - (1 if q >= 4096 else 0)
    if q == 8193:   # a whole 4096-block is passed on its l2 entry
        assert st.jmin2[1] == cc.NONE and arms["skip_4096"] == 1
    if q == nr - 1:  # the hit lies in the partial tail of both levels
        assert nr % 64 and len(st.jmin1) % 64
        assert q >> 6 == len(st.jmin1) - 1 and q >> 12 == len(st.jmin2) - 1
        assert st.jmin1[-1] == q + 1 == st.jmin2[-1]
    assert {63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 12287, 12288, nr - 1} == set(cc.JAG_Q)


@pytest.mark.parametrize("u,q,past", cc.JAG2)
def test_jag_second_left_cases(u, q, past):
    case = cc.jag2_case(u, q, past)
    st = _same_as_oracle(case)
    assert st.U[0] == u and st.A == [u, q + 2 if past else q]      # lo = U_0 = u, hi = A_1
    assert st.A[1] % 64 not in (0, 63)                              # hi ends mid-block
    assert st.stuck == ({0: (1, q)} if past else {})
    arms = _arms(st, "jag_")
    assert arms["skip_4096" if u % 4096 == 0 or not past else "skip_64"] >= 1
    assert ("hit_row_%d" % (q % 64) in arms) == past
    assert {a[0] for a in cc.JAG2} == {63, 64, 65, 4095, 4096, 4097}


# ------------------------------------------------------------ b. ends skip
@pytest.mark.parametrize("gap", cc.ENDS_GAP)
def test_ends_cases(gap):
    case = cc.ends_case(gap)
    st = _same_as_oracle(case)
    (i, x, hi, T, k, cur), = [s for s in st.searches if s[0] == 1]
    q = cc.ENDS_X + gap
    assert (x, k) == (cc.ENDS_X, q) and k < hi and st.p == [cc.ENDS_X, q]
    assert all(e < T for e in st.rge[x:q]) and st.rge[q] == T       # every right of [x, q) ends below T
    assert x > st.rb[0] and st.p[0] == x                            # the first left pruned right 0
    # one before-side and one after-side record at the same distance
    assert st.rec_right[st.rec_left == 1].tolist() == [q, q + 1] and st.A[1] == q + 1
    # the fresh head is q already (module docstring: no input needs the round)
    assert cur == q == st.P[1] and st.P0[1] == q and st.rounds == 1
    arms = _arms(st, "ends_")
    assert arms["head_to_edge"] == 1 and arms["hit_row_%d" % (q % 64)] == 1
    assert arms.get("skip_4096", 0) == (1 if gap > 8192 else 0)
    # the same chain in order (LIME_CLOSEST_MAX_ROUNDS=0: k_seq_prune)
    seq = cc.restate(case, cap=0)
    assert seq.sequential and seq.rounds == 0 and _records(seq) == _records(st)
    assert [s[4] for s in seq.searches if s[0] == 1] == [q]
    assert sorted(g + cc.ENDS_X for g in cc.ENDS_GAP)[:4] == [4095, 4096, 4097, 4098]


# ---------------------------------------------------- mutations of first_hit
def _planted_searches():
    return ([cc.jag_case(q) for q in cc.JAG_Q] + [cc.jag2_case(*a) for a in cc.JAG2] +
            [cc.ends_case(g) for g in cc.ENDS_GAP])


@pytest.mark.parametrize("variant", cc.VARIANTS)
def test_wrong_searches_disturb_a_planted_case(variant):
    changed, past_hi, ends_changed = [], 0, []
    for case in _planted_searches():
        good = cc.state(case)
        bad = cc.restate(case, variant=variant)
        if _records(bad) != _records(good):
            changed.append(case["key"])
        past_hi += bad.trace["jag_past_hi"] + bad.trace["ends_past_hi"]
        assert good.trace["jag_past_hi"] + good.trace["ends_past_hi"] == 0
        if [s[4] for s in bad.searches] != [s[4] for s in good.searches]:
            ends_changed.append(case["key"])
    if variant == "no_clamp":
        # no record can change (both callers discard a result at or past hi);
        # the variant is seen reading rows outside [lo, hi)
        assert not changed and past_hi > 0
    else:
        assert changed
        fams = {k[0] for k in changed}
        assert "jag_case" in fams
        if variant == "l2_unaligned":
            assert ("jag_case", 4097) in changed and ("jag2_case", 65, 4100, True) in changed
        else:
            assert ("jag_case", cc.JAG_NR - 1) in changed
    if variant == "l2_unaligned":
        # case b: the search misses q, lands on the after-side right and the
        # before-side record is lost, though the fresh head was exact
        assert {k for k in changed if k[0] == "ends_case"} == \
            {("ends_case", g) for g in cc.ENDS_GAP if g + cc.ENDS_X >= 4096}
        for g in cc.ENDS_GAP[1:]:
            bad = cc.restate(cc.ends_case(g), variant=variant)
            assert bad.p == [cc.ENDS_X, cc.ENDS_X + g + 1] and len(bad.a_row) == 2


# ------------------------------------------------------------------ c. OCAP
@pytest.mark.parametrize("nc", cc.OCAP_NC)
def test_ocap_cases(nc):
    assert (nc + 1 <= cc.OCAP) == (nc == cc.OCAP - 1) and abs(nc - cc.OCAP) <= 1
    for variant in cc.ocap_variants(nc):
        case = cc.ocap_case(nc, variant)
        st = _same_as_oracle(case)
        _same_as_oracle(case, mode=1)
        with_records = sorted(set(np.asarray(st.lc)[st.rec_left].tolist()))
        if variant == "full":
            assert with_records == list(range(nc)) and len(st.a_row) == 2 * nc and st.alive_out
        elif variant.startswith("die"):
            die = nc - 1 if variant == "die_last" else int(variant[3:])
            assert with_records == list(range(die + 1)) and not st.alive_out
            assert st.live == [c <= die for c in range(nc)]
        elif variant == "rights_only_mid":
            assert with_records == list(range(nc // 2)) and st.lb[nc // 2] == st.lb[nc // 2 + 1]
        else:
            assert with_records == [0, nc - 1] and st.nL == 4 and st.alive_out
    assert [len(cc.ocap_variants(n)) for n in cc.OCAP_NC] == [4, 5, 6]


# ------------------------------------------------------------------ d. SWIN
@pytest.mark.parametrize("pre", cc.SWIN_PRE)
@pytest.mark.parametrize("W", cc.SWIN_W)
def test_swin_cases(W, pre):
    st = _same_as_oracle(cc.swin_case(W, pre, 1))
    assert st.windows == [(pre, pre + W, W <= cc.SWIN)] and st.D == [0]
    assert st.J == [pre + W] and st.A == [st.nR] and len(st.a_row) == W   # stuck: j < A
    case = cc.swin_waves_case(W, pre)
    st = _same_as_oracle(case)
    (wlo, whi, win), = st.windows
    assert (wlo, whi - wlo, win) == (pre, W, W <= cc.SWIN)
    D, J, A = np.array(st.D), np.array(st.J), np.array(st.A)
    assert st.nL == 200 and (D[:64] > 0).all()                  # wave 0: no D == 0 left
    assert (D[64:128] == 0).all() and (st.cnt[64:128] == W).all()
    assert (D[128:160] == 0).all() and (D[160:192] > 0).all() and (D[192:] > 0).all()
    assert (J[64:] == pre + W).all() and (J[64:] < A[64:]).all()   # the stuck pointer
    assert st.stuck == {0: (64, pre + W)} and 200 % 64 == 8        # wave 3 runs past L.n
    assert cc.SWIN_W == [2047, 2048, 2049, 4097]


@pytest.mark.parametrize("n", cc.SWIN_LEFTS)
def test_swin_left_counts(n):
    for W, pre in ((cc.SWIN, 1000), (cc.SWIN + 1, 0)):
        st = _same_as_oracle(cc.swin_case(W, pre, n))
        assert st.nL == n and len(st.windows) == (n + 255) // 256 and (np.array(st.D) == 0).all()
        assert st.windows[0] == (pre, pre + W, W <= cc.SWIN)
        if n > 256:   # later blocks: windows of their own, wlo > 0 in both arms
            assert st.windows[1] == (pre + 2, pre + W, True)
            assert all(w[0] > st.windows[0][0] for w in st.windows[1:])
        if n > 512:
            assert st.windows[2] == (pre + 514, pre + W, True)
    assert cc.SWIN_LEFTS == [1, 63, 64, 65, 255, 256, 257, 513]


def test_wrong_window_bound_disturbs_a_planted_case():
    changed = []
    for W in cc.SWIN_W:
        for pre in cc.SWIN_PRE:
            for case in (cc.swin_case(W, pre, 1), cc.swin_waves_case(W, pre)):
                bad = cc.restate(case, swin_bound=cc.SWIN + 1)
                if _records(bad) != _records(cc.state(case)):
                    changed.append(W)
    assert changed and set(changed) == {cc.SWIN + 1}


# ----------------------------------------------------- e. exact-distance runs
def test_end_run_cases():
    st = _same_as_oracle(cc.end_run_case())
    assert st.J == [151, 151] and (np.array(st.A) == 201).all() and st.stuck == {0: (0, 151)}
    assert st.p == [0, 0] and st.cnt.tolist() == [151, 151]
    assert sum(e == cc.END_T for e in st.rge) == 200
    assert sum(e == cc.END_T for e in st.rge[151:]) == 49          # at or above j
    assert st.trace["end_run_past_hb"] == 2 and st.trace["end_run_below_p"] == 0
    st = _same_as_oracle(cc.end_run_below_case())
    assert st.p == [0, 50, 50] and st.D[2] == 201 and st.J == [83, 83, 83] and st.stuck == {}
    assert st.trace["end_run_below_p"] == 1 and st.trace["end_run_both"] == 1
    k = st.rec_right[st.rec_left == 2].tolist()
    assert k == list(range(52, 82)) + [82] and all(st.rge[x] == 1000 + st.off[0] for x in k[:-1])
    assert sum(e == 1000 for e in st.rge[:50]) == 50                # the run's part below p


@pytest.mark.parametrize("g", cc.GROUP_G)
def test_group_cases(g):
    st = _same_as_oracle(cc.group_case(g))
    S = cc.GROUP_S
    assert S >> cc.DSH != (S + 1) >> cc.DSH                       # gs[a] + 1 is the next bucket
    assert st.trace["group_%d" % g] == 2 and st.trace["gs_widest"] >= g
    assert st.cnt.tolist() == [g, g, 1] and st.A[:2] == [1, 1] and st.N[:2] == [1 + g, 1 + g]
    assert cc.GROUP_G == [1, 64, 65, 5000]


def test_lattice_case():
    st = _same_as_oracle(cc.lattice_case())
    for d in ("gs", "pmax", "eg"):
        for low in (0, 1, 4095):   # keys on 4096 m, 4096 m + 1 and 4096 m - 1
            assert st.trace["%s_low_%d" % (d, low)] > 0, (d, low)
    assert st.trace["gs_empty_bucket"] >= 8                        # the stretch without rights
    lows = {x & 4095 for x in st.rgs + st.rge + st.lge}
    assert {0, 1, 4095} <= lows


@pytest.mark.parametrize("span", cc.SPAN)
def test_span_cases(span):
    case = cc.span_case(span)
    st = _same_as_oracle(case)
    assert int(st.off[1]) == span and st.nb == (9 if span == 8 * 4096 else 8)
    ln = span - 1
    assert ln in st.rge and st.lgs[-1] == ln                       # on the last coordinate
    for d in ("gs", "pmax", "eg") if span % 4096 else ("gs", "eg"):
        assert st.trace[d + "_last_entry"] > 0                     # d[nb] is read
    assert st.trace["gs_past_nb"] + st.trace["pmax_past_nb"] + st.trace["eg_past_nb"] == 0


# ------------------------------------------------------ f. coordinate extremes
def test_zero_case():
    case = cc.zero_case()
    st = _same_as_oracle(case)
    assert st.trace["T_eq_0"] >= 1 and st.live == [True] * 3
    off = st.off.tolist()
    for c in range(3):
        i = st.lgs.index(off[c] + 5)                               # the left [5, 8)
        assert st.D[i] == 6 and st.lgs[i] + 1 - st.D[i] == off[c]  # T == the contig's offset
        k = st.rec_right[st.rec_left == i].tolist()
        assert [(st.rgs[x] - off[c], st.rge[x] - off[c]) for x in k] == [(0, 0), (13, 20)]
        z = st.lgs.index(off[c])                                   # a left at coordinate 0
        assert st.D[z] == 1 and st.cnt[z] == 1
    assert off[0] == 0 and st.rge[st.rb[1] - 1] == off[1] - 1      # the neighbour ends one below


def test_far_cases():
    for case, floor in ((cc.far_case(), 2), (cc.far_only_case(), 3)):
        st = _same_as_oracle(case)
        d = [cc.udist(st.lgs[i], st.lge[i], st.rgs[k], st.rge[k])
             for i, k in zip(st.rec_left, st.rec_right)]
        assert sum(x > 2 ** 31 for x in d) >= floor and int(st.off[1]) == 0xFFFFFFFF
        assert sum(x < 200 for x in d) >= 3 - floor
        assert st.nb == 1 << 20
    case = cc.none_distance_case()
    st = _same_as_oracle(case)
    assert st.D == [cc.NONE] and len(st.a_row) == 1 and len(cc.expected(case)["a_row"]) == 1
    assert st.trace["T_eq_0"] >= 1
    assert _records(cc.single_py(case)) == _records(st)
    _same_as_oracle(case, mode=1)


# ------------------------------------------------------------ g. k_seq_single
@pytest.mark.parametrize("n", cc.SINGLE_ADV)
def test_single_advance_cases(n):
    st = _same_as_oracle(cc.single_advance_case(n, False), mode=1)
    assert st.advanced == [n, 0] and st.stop_lane[0] == n % 64 and st.stop_kind[0] == "dist"
    assert st.kept_at == [n - 1, 0]                                # first kept row, past p
    assert {n % 64 for n in cc.SINGLE_ADV} >= {63, 0, 1}
    assert {n - 1 for n in cc.SINGLE_ADV} >= {63, 64, 65}
    if n % 64 == 0:
        st = _same_as_oracle(cc.single_advance_case(n, True), mode=1)
        assert st.advanced == [n, 0] and st.stop_kind == ["r1", "r1"] and st.J == [n, n]
    # (a prune keeps R[j - 1] at the least: kept_at is never None once j > r0)
    assert None not in st.kept_at


@pytest.mark.parametrize("m", cc.SINGLE_DROP)
def test_single_cover_drop_cases(m):
    st = _same_as_oracle(cc.single_cover_drop_case(m), mode=1)
    assert st.advanced[0] == m and st.stop_kind[0] == "cover" and st.stop_lane[0] == m % 64
    assert st.D[0] == 0 and cc.SINGLE_DROP == [63, 64]


# ---------------------------------------------------------------- h. rounds
def test_round_seeds():
    assert len(cc.ROUND_SEEDS) == 13 and cc.ROUND_SEEDS[460] == 7
    for seed, k in cc.ROUND_SEEDS.items():
        nc, A, sa, B, sb = _case(seed)
        assert decomposed_py(_sorted_rows(A, sa), _sorted_rows(B, sb), nc)[1] == k >= 5 and nc > 1
        case = cc.from_seed(seed)
        st = _same_as_oracle(case, cc.restate(case))
        assert st.rounds == 1 and not st.sequential                # global coordinates: exact at once
        for cap in (0, 1):
            capped = cc.restate(case, cap=cap)
            assert (capped.rounds, capped.sequential) == (cap, cap == 0)
            assert _records(capped) == _records(st)


# ------------------------------------------------------------ the fill filter
def _fill_cases():
    return [cc.swin_waves_case(cc.SWIN, 1000), cc.swin_case(cc.SWIN + 1, 0, 65), cc.end_run_case(),
            cc.group_case(65), cc.group_case(5000), cc.lattice_case(), cc.jag_case(4097)]


def test_fill_filter_admits_the_owners():
    one_more = 0
    for case in _fill_cases():
        st = cc.state(case)
        total = int(st.out_off[-1])
        edges = sorted({int(x) for x in st.out_off[st.cnt.nonzero()[0]][:6]} |
                       {int(x) for x in st.out_off[-4:]})
        for e in edges:
            for first in (e - 1, e, e + 1):
                for count in (1, 63, 64, 65, 997):
                    if first < 0 or first + count > total:
                        continue
                    own = cc.fill_owners(st, first, count).tolist()
                    assert cc.fill_admits(st, first, count).tolist() == own
                    wrong = cc.fill_admits(st, first, count, wrong=True).tolist()
                    assert set(own) <= set(wrong)
                    one_more += len(wrong) - len(own)
    assert one_more > 0


# ------------------------------------------------- what could not be planted
@pytest.mark.parametrize("block", range(4))
def test_random_cases_are_exact_at_round_0(block):
    # module docstring: with global coordinates the prefix max of the fresh
    # heads is the chain itself (one round, the confirming one) -- on the very
    # seeds where decomposed_py's contig-local prefix max needs up to 7
    for seed in range(block * 1500, block * 1500 + 1500):
        case = cc.from_seed(seed)
        st = cc.restate(case)
        exp = cc.expected(case)
        cc._EXPECTED.pop((case["key"], 0))   # (6000 oracle results are not kept)
        assert _records(st) == (exp["a_row"].tolist(), exp["b_row"].tolist()), seed
        assert st.rounds == 1 and st.P0 == st.p, seed
