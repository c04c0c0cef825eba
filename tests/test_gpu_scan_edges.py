"""The one-pass scans at their tile, wave and round edges: k_merge_scan2
(plain merge, its prefix max and its same-start flag), k_merge_scan<true>
(stranded merge, full tiles and the segmented carry across them) and the
multi-pass prefix max, on the planted inputs of tests/scan_cases.py (checked
on the CPU by tests/test_scan_cases.py).  Every comparison is exact, on every
row, against the C oracle and the restated fold."""
import functools

import numpy as np
import pytest

from lime_amd import Space, SUBTRACT_LIME, SUBTRACT_SET
from oracle import oracle
from tests import scan_cases as sc

pytestmark = pytest.mark.gpu


def _space(case):
    return Space([f"c{i:02d}" for i in range(len(case["lens"]))], case["lens"])


def _same(got, exp, keys):
    for k in keys:
        assert np.array_equal(np.asarray(got[k], np.int64), np.asarray(exp[k], np.int64)), k


@functools.lru_cache(maxsize=None)
def _merge_refs(cases, cid):
    """oracle and fold of a case, computed once"""
    case = sc.case_by_id(getattr(sc, cases), cid)
    return oracle.merge(sc.rows(case)), sc.fold(*sc.rows(case))


# ------------------------------------------- A. plain merge (k_merge_scan2)
@pytest.mark.parametrize("cid", [c[0] for c in sc.PLAIN_CASES])
def test_plain_merge_edges(ctx, cid):
    case = sc.case_by_id(sc.PLAIN_CASES, cid)
    exp, fd = _merge_refs("PLAIN_CASES", cid)
    n = len(case["start"])
    if "edges" in case:  # the oracle's answer has the planted property
        assert len(exp["start"]) == sc.PLAIN_RUNS[cid[:-2]]
        rid = exp["run_of_row"][case["row_sorted"]]
        assert ((rid[case["edges"]] != rid[case["edges"] - 1]) == case["edge_starts_run"]).all()
    sp = _space(case)
    a = ctx.set_from_host(sp, *sc.rows(case))
    h = a.to_host()
    if "row_sorted" in case:  # the planted rows sit where the case says
        assert np.array_equal(h["row"], case["row_sorted"])
    else:
        assert np.array_equal(h["row"], sc.device_order_plain(*sc.rows(case)))
    res = ctx.merge(a)
    got = res.to_host()
    rid = res.run_of_row(n)
    for ref in (exp, fd):
        _same(got, ref, ("contig", "start", "end"))
        assert np.array_equal(rid, ref["run_of_row"])
    comp = ctx.complement(sp, a).to_host()
    _same(comp, oracle.complement(sc.rows(case), case["lens"]), ("contig", "start", "end"))


# -------------------------------- B. stranded merge (k_merge_scan<true>)
def _check_stranded(ctx, case, a, exp, fd=None):
    n = len(case["start"])
    h = a.to_host()
    order = sc.device_order_stranded(*sc.rows(case))
    assert np.array_equal(h["row"], order)  # (contig, start, end, strand ordinal, row)
    if "row_sorted" in case:
        assert np.array_equal(h["row"], case["row_sorted"])
    _same(h, {k: case[k][order] for k in ("contig", "start", "end")}, ("contig", "start", "end"))
    res = ctx.merge(a)
    got = res.to_host()
    rid = res.run_of_row(n)
    strands = res.run_strands(0, res.n)
    for ref in (exp, fd):
        if ref is None:
            continue
        _same(got, ref, ("contig", "start", "end"))
        assert np.array_equal(rid, ref["run_of_row"])
        assert np.array_equal(strands.astype(np.int64), np.asarray(ref["strand"], np.int64))


@pytest.mark.parametrize("cid", [c[0] for c in sc.STRANDED_CASES])
def test_stranded_merge_tiles(ctx, cid):
    case = sc.case_by_id(sc.STRANDED_CASES, cid)
    exp, fd = _merge_refs("STRANDED_CASES", cid)
    if "n_runs" in case:
        assert len(exp["start"]) == case["n_runs"]
    a = ctx.set_from_host_stranded(_space(case), *sc.rows(case))
    _check_stranded(ctx, case, a, exp, fd)


@pytest.mark.parametrize("strands", ["uniform", "stretches"])
def test_stranded_merge_from_device_rows(ctx, strands):
    import torch
    cid = f"{strands}-{3 * sc.ST + 5}"
    case = sc.case_by_id(sc.STRANDED_CASES, cid)
    exp, fd = _merge_refs("STRANDED_CASES", cid)
    t = [torch.tensor(np.asarray(case[k], np.int32), device="cuda")
         for k in ("contig", "start", "end")]
    t.append(torch.tensor(np.asarray(case["strand"], np.int8), device="cuda"))
    torch.cuda.synchronize()
    a = ctx.set_from_device_stranded(_space(case), len(case["start"]), *[x.data_ptr() for x in t])
    _check_stranded(ctx, case, a, exp, fd)
    del t


def test_stranded_merge_many_tiles(ctx):
    # 67 tiles: more than one 64-wide look-back window (oracle only; the fold
    # agrees with it on this case in tests/test_scan_cases.py)
    case = sc.stranded_many_tiles()
    exp = oracle.merge(sc.rows(case))
    rid = exp["run_of_row"][case["row_sorted"]]
    for a_, m in sc.MANY_TILES_UMBRELLAS:
        assert rid[a_] == rid[a_ + m * sc.ST + 7]
    a = ctx.set_from_host_stranded(_space(case), *sc.rows(case))
    _check_stranded(ctx, case, a, exp)


# ----------------------- C. the same-start flag, through subtract's heads
@functools.lru_cache(maxsize=None)
def _sub_expected(shape, i, g, t, mode, planted=True, nb=sc.SUB_NB, ls=False):
    return oracle.subtract(sc.rows((sc.subtract_a_ls if ls else sc.subtract_a)(i, nb)),
                           sc.rows(sc.subtract_b(shape, i, g, planted, nb)), t, mode)


_COLS = ("contig", "start", "end", "a_row", "b_row")


def _differs(x, y):
    return any(x[k].tolist() != y[k].tolist() for k in _COLS)


def _run_subtract(ctx, shape, i, g, t, mode, nb=sc.SUB_NB, ls=False):
    exp = _sub_expected(shape, i, g, t, mode, True, nb, ls)
    if g > sc.G + 1:
        # not vacuous: a walk that stops short of the planted row (its end
        # taken for the group's) gives another answer
        assert _differs(exp, _sub_expected(shape, i, g, t, mode, False, nb, ls))
    A = (sc.subtract_a_ls if ls else sc.subtract_a)(i, nb)
    B = sc.subtract_b(shape, i, g, True, nb)
    sp = _space(B)
    a = ctx.set_from_host(sp, *sc.rows(A))
    b = ctx.set_from_host(sp, *sc.rows(B))  # fresh: the flag and the index are cached per set
    assert np.array_equal(b.to_host()["row"], B["row_sorted"])
    res = ctx.subtract(a, b, t, mode).to_host()
    og, oe = np.argsort(res["a_row"], kind="stable"), np.argsort(exp["a_row"], kind="stable")
    for k in _COLS:
        assert np.array_equal(res[k][og], exp[k][oe]), k


_MODES = [SUBTRACT_LIME, SUBTRACT_SET]
_POS_IDS = [f"{i}x{g}" for i, g in sc.SUB_POSITIONS]


# (the dispatch: tests/test_scan_cases.py quotes subtract_run's conditions and
# asserts the run counts that send sparse to k_sub_fused<false> and chained to
# k_sub_count_runs + k_subtract; both take k_merge_scan2<true>'s flag)
@pytest.mark.parametrize("mode", _MODES)
@pytest.mark.parametrize("shape", sc.SUB_SHAPES)
@pytest.mark.parametrize("pos", sc.SUB_POSITIONS, ids=_POS_IDS)
def test_tie_flag_merge_scan(ctx, monkeypatch, pos, shape, mode):
    monkeypatch.setenv("LIME_SUB_NO_LS", "1")
    _run_subtract(ctx, shape, pos[0], pos[1], 0, mode)


@pytest.mark.parametrize("mode", _MODES)
@pytest.mark.parametrize("pos", sc.SUB_POSITIONS, ids=_POS_IDS)
def test_tie_flag_ls_deferred(ctx, monkeypatch, pos, mode):
    # the LS path (k_sub_fused<true>): no merge scan; its pass meets the
    # group, flags it, the tie index is built then and the pass runs again.
    # LS is taken only while every fused tile's window of B fits FWIN: the
    # left rows lie within 18k bases round the group (subtract_a_ls), and
    # tests/test_scan_cases.py restates k_sub_window to show they fit -- and
    # that part C's other left rows never do, with or without the variable
    monkeypatch.delenv("LIME_SUB_NO_LS", raising=False)
    assert sc.sub_window_max(sc.subtract_a_ls(pos[0]),
                             sc.subtract_b("sparse", pos[0], pos[1])) <= sc.SUB_FWIN
    _run_subtract(ctx, "sparse", pos[0], pos[1], 0, mode, ls=True)


@pytest.mark.parametrize("mode", _MODES)
@pytest.mark.parametrize("shape", sc.SUB_SHAPES)
@pytest.mark.parametrize("i,nb", [(sc.SUB_AT_LAST, sc.SUB_NB), (sc.SUB_AT_PLAIN, sc.SUB_NB),
                                  (sc.SUB_NB + 2 - sc.SUB_G, sc.SUB_NB + 2)])
def test_tie_flag_detect_kernel(ctx, i, nb, shape, mode):
    # threshold 1: no runs, k_tie_detect decides.  The group ending on the
    # last row of a set of 4 k rows is met by the kernel's last 16-B compare;
    # with 4 k + 2 rows only its scalar tail meets it
    _run_subtract(ctx, shape, i, sc.SUB_G, 1, mode, nb)


# ------------------- D. the prefix max, both producers, first_reachings
@functools.lru_cache(maxsize=None)
def _pmax_reference(n, long_rows):
    case = sc.prefix_case(n, long_rows)
    order = sc.device_order_plain(*sc.rows(case))
    off = np.concatenate([[0], np.cumsum(np.asarray(case["lens"], np.int64) + 1)])
    pm = np.maximum.accumulate(off[case["contig"][order]] + case["end"][order])
    keys = sc.reaching_keys(pm)
    return order, pm, keys, np.searchsorted(pm, keys, side="right")


@functools.lru_cache(maxsize=None)
def _pmax_subtract(n, long_rows, t):
    return oracle.subtract(sc.rows(sc.prefix_probe_rows(n, long_rows)),
                           sc.rows(sc.prefix_case(n, long_rows)), t)


@pytest.mark.parametrize("producer", ["multi_pass", "merge_scan"])
@pytest.mark.parametrize("n,long_rows", sc.PMAX_CASES)
def test_prefix_max_first_reachings(ctx, monkeypatch, n, long_rows, producer):
    case = sc.prefix_case(n, long_rows)
    order, pm, keys, want = _pmax_reference(n, long_rows)
    sp = _space(case)
    b = ctx.set_from_host(sp, *sc.rows(case))  # fresh: the prefix max is cached per set
    h = b.to_host()
    assert np.array_equal(h["row"], order)
    # the reference from the device's own order, as the kernels see the rows
    assert np.array_equal(np.maximum.accumulate(sp.offsets[h["contig"]] + h["end"]), pm)
    A = sc.rows(sc.prefix_probe_rows(n, long_rows))
    a = ctx.set_from_host(sp, *A)

    def subtract_reads_it(t):
        # the spanning-hit test reads the prefix max at the row before every
        # left row's start -- also where a binary search never looks.  (Under
        # long rows B covers every left row whole: the answer is empty)
        res = ctx.subtract(a, b, t).to_host()
        exp = _pmax_subtract(n, long_rows, t)
        og, oe = np.argsort(res["a_row"], kind="stable"), np.argsort(exp["a_row"], kind="stable")
        for k in _COLS:
            assert np.array_equal(res[k][og], exp[k][oe]), k

    if producer == "merge_scan":
        # B of a runs-path subtract: k_merge_scan2 writes the prefix max
        monkeypatch.setenv("LIME_SUB_NO_LS", "1")
        subtract_reads_it(0)
    got = np.asarray(b.first_reachings(keys.tolist()), np.int64)
    assert np.array_equal(got, want)
    if producer == "multi_pass":
        # (built lazily by first_reachings; threshold 1 takes no merge scan)
        subtract_reads_it(1)
