"""The scan-edge inputs of tests/scan_cases.py checked on the CPU: the
builders against the C oracle and an independent restatement of the fold,
the planted rows' sorted positions, the properties the GPU tests rely on
(which edge row starts a run, the run counts that pick subtract's path, the
tie cases' answers depending on the planted row), and the kernels' geometry
constants read from the sources.  Exact integer equality throughout."""
import os
import re

import numpy as np
import pytest

from oracle import oracle
from tests import scan_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------- geometry
def _source(name):
    with open(os.path.join(ROOT, "lime_amd", "csrc", name)) as f:
        return f.read()


def _define(text, name):
    m = re.search(r"#ifndef %s\s*\n#define %s (\d+)" % (name, name), text)
    assert m, name
    return int(m.group(1))


def _constexpr(text, name):
    m = re.search(r"constexpr int %s = (\d+);" % name, text)
    assert m, name
    return int(m.group(1))


def test_geometry_constants_match_the_sources():
    merge, sub = _source("merge.hip"), _source("subtract.hip")
    nt, q = _define(merge, "LIME_MS2_NT"), _define(merge, "LIME_MS2_Q")
    sb = _define(merge, "LIME_MERGE_SB")
    mitems, mb = _constexpr(merge, "MITEMS"), _constexpr(merge, "MB")
    assert (nt, q, sb, mitems, mb) == (1024, 8, 1024, 16, 256)
    assert _constexpr(merge, "MERGE_TIE_G") == 16 and _constexpr(sub, "TIE_G") == 16
    # the derived sizes, as the kernels derive them
    assert re.search(r"RW = RQ \* 256;", merge) and re.search(r"TILE = NW \* RW;", merge)
    assert re.search(r"STILE = SB \* MITEMS;", merge) and re.search(r"MTILE = MB \* MITEMS;", merge)
    assert sc.R == 256 and sc.W == q * 256 and sc.T == nt // 64 * q * 256
    assert sc.ST == sb * mitems and sc.PT == mb * mitems and sc.G == 16
    # subtract's fused tiles and the LS path's window bound
    fw, sub_b = _define(sub, "LIME_SUB_FW"), _constexpr(sub, "SUB_B")
    assert re.search(r"#define LIME_SUB_FWIN \(384 \* LIME_SUB_FW\)", sub)
    assert re.search(r"FROWS = FW \* SUB_B, FWIN = LIME_SUB_FWIN;", sub)
    assert re.search(r"ls = h_wm <= \(unsigned\)FWIN;", sub)
    assert (sc.SUB_FROWS, sc.SUB_FWIN) == (fw * sub_b, 384 * fw) == (2048, 3072)


# ---------------------------------------------- builders == oracle == fold
def _assert_fold_is_oracle(case, stranded):
    exp = oracle.merge(sc.rows(case))
    fd = sc.fold(*sc.rows(case))
    for k in ("contig", "start", "end", "run_of_row"):
        assert fd[k].tolist() == exp[k].tolist(), k
    if stranded:
        assert fd["strand"].tolist() == exp["strand"].tolist()
    return exp


def _assert_row_sorted(case, order):
    if "row_sorted" in case:
        assert order.tolist() == case["row_sorted"].tolist()


@pytest.mark.parametrize("cid", [c[0] for c in sc.PLAIN_CASES])
def test_plain_cases(cid):
    case = sc.case_by_id(sc.PLAIN_CASES, cid)
    exp = _assert_fold_is_oracle(case, False)
    _assert_row_sorted(case, sc.device_order_plain(*sc.rows(case)))
    n = len(case["start"])
    assert (case["end"] <= np.asarray(case["lens"])[case["contig"]]).all()
    if cid == "base":
        assert n == sc.N_BASE == len(exp["start"])
    if "edges" in case:  # A.2: what the oracle says of the planted rows
        kind = cid[:-2]
        assert len(exp["start"]) == sc.PLAIN_RUNS[kind]
        assert (sc.PLAIN_RUNS["bookend"], sc.PLAIN_RUNS["one_base"]) == (98075, 98069)
        rid = exp["run_of_row"][case["row_sorted"]]  # run of every sorted row
        starts_run = rid[case["edges"]] != rid[case["edges"] - 1]
        assert (starts_run == case["edge_starts_run"]).all()
        assert (rid[case["edges"] - 1] == rid[case["edges"] - 40]).all()
    if cid.startswith("one_run"):
        assert len(exp["start"]) == 1
    if cid.startswith("umbrella"):
        q = min(2 * sc.T + sc.T // 2, n - 3)
        assert len(exp["start"]) == n - (q - 1 - 7)  # rows 7 .. q - 1 one run
    if cid.startswith("random_dense"):
        assert 0.05 < np.mean(case["end"] == case["start"]) < 0.25
    if cid == "contig_edges":
        order = sc.device_order_plain(*sc.rows(case))
        c, s, e = (case[k][order] for k in ("contig", "start", "end"))
        at = 0
        for ci, m in enumerate(sc.CONTIG_EDGE_ROWS):
            assert (c[at:at + m] == ci).all() and s[at] == 0
            assert e[at + m - 1] == case["lens"][ci]
            # no run crosses the pad: one ends at the contig's length, the
            # next contig's first starts at 0
            k = exp["contig"] == ci
            assert exp["end"][k][-1] == case["lens"][ci] and exp["start"][k][0] == 0
            at += m
        assert at == n


@pytest.mark.parametrize("cid", [c[0] for c in sc.STRANDED_CASES])
def test_stranded_cases(cid):
    case = sc.case_by_id(sc.STRANDED_CASES, cid)
    exp = _assert_fold_is_oracle(case, True)
    _assert_row_sorted(case, sc.device_order_stranded(*sc.rows(case)))
    assert (case["end"] <= np.asarray(case["lens"])[case["contig"]]).all()
    if "n_runs" in case:
        assert len(exp["start"]) == case["n_runs"]
    if cid.startswith("width-"):
        assert case["max_width"] == int(cid[6:])
        assert int((case["end"] - case["start"]).max()) == case["max_width"]
    if cid.startswith(("uniform", "width")):  # (start, end) ties across strands
        o = sc.device_order_stranded(*sc.rows(case))
        c, s, e, t = (case[k][o] for k in ("contig", "start", "end", "strand"))
        tie = (c[1:] == c[:-1]) & (s[1:] == s[:-1]) & (e[1:] == e[:-1]) & (t[1:] != t[:-1])
        assert tie.sum() > 500


def test_stranded_many_tiles_case():
    case = sc.stranded_many_tiles()
    assert len(case["start"]) == 66 * sc.ST + 3 == 1_081_347
    exp = _assert_fold_is_oracle(case, True)
    _assert_row_sorted(case, sc.device_order_stranded(*sc.rows(case)))
    rid = exp["run_of_row"][case["row_sorted"]]
    for a, m in sc.MANY_TILES_UMBRELLAS:  # one run from a over m tile edges
        b = a + m * sc.ST + 7
        assert rid[a] == rid[b] and rid[a - 1] != rid[a] and rid[b + 1] != rid[b]
        assert b // sc.ST - a // sc.ST >= m
    for a, m in sc.MANY_TILES_CUT:  # cut where the stretch ends, and not resumed
        cut = (a // sc.STRETCH + 1) * sc.STRETCH
        assert cut < a + m and (cut - 1) // sc.ST < (a + m) // sc.ST
        assert rid[a - 1] != rid[a] == rid[cut - 1] != rid[cut]
        assert (np.diff(rid[cut:a + m + 2]) == 1).all()


# ----------------------------------------------------- C. the tie flag
# which of subtract's paths a B set takes (subtract.hip, subtract_run):
#   runs  = threshold <= 0 && B->n > 0 && B->strand_in == nullptr
#   ls    = runs && !B->has_zero_width && !getenv("LIME_SUB_NO_LS") && every
#           fused tile's window within FWIN
#   if (runs && !ls) merge_runs_with_pmax(B, &mb, &tie_big)   // k_merge_scan2<TIE>
#   fused = ls || (runs && mb.n * 64 >= na)
# so under LIME_SUB_NO_LS: k_sub_fused<false> when B's runs * 64 >= na, else
# k_sub_count_runs + k_subtract; threshold > 0: no merge scan, k_tie_detect
def test_subtract_b_run_counts_pick_the_paths():
    for i, g in sc.SUB_POSITIONS:
        runs = {sh: len(oracle.merge(sc.rows(sc.subtract_b(sh, i, g)))["start"])
                for sh in sc.SUB_SHAPES}
        assert runs["sparse"] * 64 >= sc.SUB_NA and runs["sparse"] > 69000
        assert runs["chained"] * 64 < sc.SUB_NA and runs["chained"] > 20


def test_subtract_ls_path_is_taken_only_by_its_own_left_rows():
    # ls (above) = B without zero-width rows and k_sub_window's longest
    # window <= FWIN.  The left rows of part C's other runs spread over the
    # whole contig: their windows hold ~27,000 rows of B, so those runs take
    # the merge scan whether LIME_SUB_NO_LS is set or not; subtract_a_ls's
    # stay under FWIN at every position, and their answers too depend on the
    # planted row
    for i, g in sc.SUB_POSITIONS:
        b = sc.subtract_b("sparse", i, g)
        assert (b["end"] > b["start"]).all()
        assert sc.sub_window_max(sc.subtract_a_ls(i), b) <= sc.SUB_FWIN
        assert sc.sub_window_max(sc.subtract_a(i), b) > sc.SUB_FWIN
        if g < 18:
            continue
        a = sc.rows(sc.subtract_a_ls(i))
        for mode in (oracle.SUB_LIME, oracle.SUB_SET):
            real = oracle.subtract(a, sc.rows(b), 0, mode)
            flat = oracle.subtract(a, sc.rows(sc.subtract_b("sparse", i, g, False)), 0, mode)
            assert any(real[k].tolist() != flat[k].tolist()
                       for k in ("contig", "start", "end", "a_row", "b_row"))


@pytest.mark.parametrize("shape", sc.SUB_SHAPES)
def test_subtract_b_cases(shape):
    for i, g in ((sc.SUB_AT_ROUND[0], 18), (sc.SUB_AT_TILE[2], 18), (sc.SUB_AT_LAST, 18),
                 (sc.T - 7, 17)):
        b = sc.subtract_b(shape, i, g)
        _assert_fold_is_oracle(b, False)
        order = sc.device_order_plain(*sc.rows(b))
        assert order.tolist() == b["row_sorted"].tolist()
        s, e = b["start"][order], b["end"][order]
        # the group sits at sorted rows i .. i + g - 1, its min-end row last
        assert (s[i:i + g] == 10 * i).all() and s[i - 1] < 10 * i < s[i + g:].min(initial=2**40)
        assert e[i + g - 1] == 10 * i + 2000 and (e[i:i + g - 1] == 10 * i + 5000).all()
        assert order[i + g - 1] == b["planted_row"]
        # rows j with start[j] == start[j + G]: exactly the group's first g - G
        hit = np.nonzero(s[:-sc.G] == s[sc.G:])[0]
        assert hit.tolist() == list(range(i, i + g - sc.G))


def test_subtract_positions_sit_in_lanes_60_to_63():
    for i in sc.SUB_AT_ROUND + sc.SUB_AT_WAVE + sc.SUB_AT_TILE:
        assert i % sc.R >= 240 and (i + 1) % sc.R >= 240 and i + sc.SUB_G <= sc.SUB_NB
    assert [i // sc.R % 8 for i in sc.SUB_AT_ROUND] == [3] * 3
    assert [i // sc.W for i in sc.SUB_AT_ROUND] == [2] * 3
    assert [(i // sc.W, i % sc.W // sc.R) for i in sc.SUB_AT_WAVE] == [(3, 7)] * 3
    assert [(i // sc.T, i % sc.T // sc.R) for i in sc.SUB_AT_TILE] == [(0, 127)] * 3 + [(1, 127)] * 3
    assert sc.SUB_NB % sc.T == 4096  # the tile after tile 1 is the partial one


@pytest.mark.parametrize("mode", [oracle.SUB_LIME, oracle.SUB_SET])
@pytest.mark.parametrize("shape", sc.SUB_SHAPES)
@pytest.mark.parametrize("i", [240, 2045, sc.T - 16, sc.T - 7, 40000])
def test_subtract_answer_depends_on_the_planted_row(i, shape, mode):
    # not vacuous: the answer with the planted row's end moved back to the
    # group's (what a walk that never reaches the planted row computes)
    # differs from the real one
    a = sc.rows(sc.subtract_a(i))
    real = oracle.subtract(a, sc.rows(sc.subtract_b(shape, i, sc.SUB_G)), 0, mode)
    flat = oracle.subtract(a, sc.rows(sc.subtract_b(shape, i, sc.SUB_G, False)), 0, mode)
    assert any(real[k].tolist() != flat[k].tolist()
               for k in ("contig", "start", "end", "a_row", "b_row"))


# ------------------------------------------------------ D. prefix max
@pytest.mark.parametrize("n,long_rows", sc.PMAX_CASES)
def test_prefix_case(n, long_rows):
    case = sc.prefix_case(n, long_rows)
    order = sc.device_order_plain(*sc.rows(case))
    e = case["end"][order]
    assert e.max() <= case["lens"][0] < 2**32
    pm = np.maximum.accumulate(e)
    # (zero-width rows: as B of a subtract the set never takes the LS path,
    # so at threshold 0 its prefix max comes out of k_merge_scan2)
    assert (case["end"] == case["start"]).sum() > 1000
    if n > 256 * sc.PT:
        q1, q2 = case["planted"].tolist()
        assert 3 * sc.PT <= q1 < 4 * sc.PT and pm[q1] == e[q1] > pm[q1 - 1]
        assert pm[q2] == e[q2] == case["lens"][0] > pm[q2 - 1]
        # the first planted maximum still stands in tile 256: that tile's
        # prefix is the carry of the tile-maxima scan's first iteration
        assert pm[256 * sc.PT] == e[q1] and e[255 * sc.PT: 256 * sc.PT + 100].max() < e[q1]
        assert q2 > 256 * sc.PT
        # the subtract probe reads the prefix max at the row before a left
        # row's start: for many left rows that row lies in tile 256, where
        # only the carried maximum spans the left row (the tile's own rows
        # up to there end before it starts)
        a = sc.prefix_probe_rows(n, long_rows)
        j = np.searchsorted(case["start"][order], a["start"], "left") - 1
        k = (j >= 256 * sc.PT) & (j < q2)
        local = np.array([e[256 * sc.PT:x + 1].max() for x in j[k]])
        assert (((local <= a["start"][k]) & (pm[j[k]] > a["start"][k] + 1)).sum() >
                (10 if long_rows else 100))  # (of 30 / 300 left rows placed there)
    else:
        assert len(case["planted"]) == 0
    keys = sc.reaching_keys(pm)
    assert len(keys) <= 20000 and keys[0] == 0 and keys[-1] == 2**32 - 1
    idx = [k * t + d for t in (sc.PT, sc.T) for k in range(1, n // t + 1) for d in (-1, 0)
           if k * t + d < n]
    assert np.isin(pm[idx], keys).all() and np.isin(pm[idx] - 1, keys).all()
    # the distinct answers: a dozen or more steps with long rows (fewest
    # under the planted maxima), every third row or better without
    steps = len(np.unique(np.searchsorted(pm, keys, side="right")))
    assert steps > (10 if long_rows else 3000 if len(case["planted"]) else 9000)
