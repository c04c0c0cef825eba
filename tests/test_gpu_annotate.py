"""lime_annotate on the device against tests/annotate_cases.annotate_ref, exact
in every view the handle offers (to_host, fill_host over a sub-range, totals,
to_bed), and against the engine's own operators on the same sets: the pair
count and the pairs of intersect, the pieces of subtract in set mode, the
bit-per-base path.  Shapes: the planted cases of annotate_cases.py (tile edges
of A, the LDS / global switch of the staged windows, empty windows, long rows,
counts past 16 and 32 bits, contig bounds), seeded random sets with heavy
ties, 2e6 device-generated rows, the operator mirror (strands, a genome cut
into several spaces), errors, the allocation-failure sweep and the CLI."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from lime_amd import Context, LimeError, Space, SUBTRACT_SET, _ffi
from lime_amd import set_theory as st
from tests import annotate_cases as ac
from tests.annotate_cases import T, W
from tests.util import GOLDEN, java_key, read_bed_py

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bin", "lime-submit")
PLANTED = {c["name"]: c for c in ac.planted_cases()}
FILL_PAIRS = 5_000_000  # pair counts up to this are filled and compared by a_row


def _space(lens):
    return Space([f"c{i:02d}" for i in range(len(lens))], [int(x) for x in lens])


@functools.lru_cache(maxsize=None)
def _expected(name):
    c = PLANTED[name]
    return ac.annotate_ref(c["A"], c["B"], c["lens"])


def _cross_check(ctx, a, b, hits, cov):
    """hits / cov: the annotation in A's INPUT row order, against intersect
    and subtract (set mode) on the same sets"""
    plan = ctx.intersect(a, b)
    try:
        assert int(hits.sum()) == plan.n
        if 0 < plan.n <= FILL_PAIRS:
            rows = plan.fill_host()["a_row"].astype(np.int64)
            assert np.array_equal(np.bincount(rows, minlength=len(hits)), hits)
    finally:
        plan.close()
    sub = ctx.subtract(a, b, 0, SUBTRACT_SET)
    try:
        h = sub.to_host()
        left = np.bincount(h["a_row"], weights=(h["end"] - h["start"]).astype(np.float64),
                           minlength=len(hits)).astype(np.int64)
    finally:
        sub.close()
    ah = a.to_host()
    width = np.zeros(len(hits), dtype=np.int64)
    width[ah["row"]] = ah["end"] - ah["start"]
    assert np.array_equal(width - cov, left)


def _check(ctx, case, exp=None, cross=True):
    """the annotation of the case == exp in every view"""
    A, B, lens = case["A"], case["B"], case["lens"]
    if exp is None:
        exp = ac.annotate_ref(A, B, lens)
    hits, cov, ov = exp
    sp = _space(lens)
    a, b = ctx.set_from_host(sp, *A), ctx.set_from_host(sp, *B)
    an = ctx.annotate(a, b)
    try:
        n = len(A[0])
        assert an.n == n
        h = an.to_host()
        row = h["row"]
        assert np.array_equal(np.sort(row), np.arange(n))
        # A's sorted order, each entry beside its own row
        for k, col in zip(("contig", "start", "end"), A):
            assert np.array_equal(h[k].astype(np.int64), np.asarray(col, np.int64)[row]), k
        key = sp.offsets[h["contig"]] + h["start"]
        assert (np.diff(key) >= 0).all()
        assert h["n_hits"].dtype == np.uint32 and h["overlap_bases"].dtype == np.uint64
        assert np.array_equal(h["n_hits"].astype(np.int64), hits[row])
        assert np.array_equal(h["covered"].astype(np.int64), cov[row])
        assert np.array_equal(h["overlap_bases"].astype(np.int64), ov[row])
        if n > 2:  # a sub-range
            part = an.fill_host(1, n - 2)
            for k in ("row", "n_hits", "covered", "overlap_bases"):
                assert np.array_equal(part[k], h[k][1:n - 1]), k
        assert an.fill_host(n, 0)["row"].size == 0
        assert an.totals() == (int((hits > 0).sum()), int(hits.sum()), int(cov.sum()),
                               int(ov.sum()))
        assert an.to_bed() == ac.format_annot(sp.names, A, exp, order=row)
        assert all(p for p in an.device_arrays())
        if cross:
            _cross_check(ctx, a, b, hits, cov)
    finally:
        an.close()
        a.close()
        b.close()


# ----------------------------------------------------------- planted cases
@pytest.mark.parametrize("name", ["empty_a", "empty_b", "both_empty", "one_each"])
def test_degenerate(ctx, name):
    _check(ctx, PLANTED[name], _expected(name))


@pytest.mark.parametrize("case,want", ac.edge_cases() + ac.contig_cases(),
                         ids=lambda v: v["name"] if isinstance(v, dict) else "")
def test_edge_semantics(ctx, case, want):
    exp = tuple(np.asarray(v, np.int64) for v in want)
    assert all(np.array_equal(x, y) for x, y in zip(_expected(case["name"]), exp))
    _check(ctx, case, exp)


def test_wide_counts(ctx):
    exp = _expected("wide")
    assert exp[0][0] > 2 ** 16 and exp[2][0] > 2 ** 32
    _check(ctx, PLANTED["wide"], exp)


@pytest.mark.parametrize("name", ["long_b_over_tiles", "long_first_row"])
def test_long_rows(ctx, name):
    _check(ctx, PLANTED[name], _expected(name))


@pytest.mark.parametrize("n", ac.TILE_ROWS)
def test_tile_sized(ctx, n):
    _check(ctx, PLANTED[f"tile_sized_{n}"], _expected(f"tile_sized_{n}"))


@pytest.mark.parametrize("m", ac.WINDOW_ROWS)
def test_window_capacity(ctx, m):
    # m = W - 1, W: tile 0's three windows staged in LDS; W + 1: searched in
    # global memory, the next tile staged again
    c = PLANTED[f"window_{m}"]
    assert ac.tile_windows(c["A"], c["B"], c["lens"])[0].tolist() == [m] * 3
    _check(ctx, c, _expected(f"window_{m}"))


@pytest.mark.parametrize("name", ["b_before_a", "b_after_a", "b_in_gap"])
def test_empty_windows(ctx, name):
    _check(ctx, PLANTED[name], _expected(name))


# ------------------------------------------------------------ random cases
@functools.lru_cache(maxsize=None)
def _random(n):
    # the widths shrink as the rows grow so that the pair records the oracle
    # reference reduces stay in the tens of millions
    c = ac.random_pair(9000 + n, n, {20_000: 40, 60_000: 12, 200_000: 3}[n])
    return c, ac.annotate_ref(c["A"], c["B"], c["lens"])


@pytest.mark.parametrize("n", [20_000, 60_000, 200_000])
def test_random_heavy_ties(ctx, n):
    c, exp = _random(n)
    assert len(np.unique(ac.offsets(c["lens"])[c["B"][0]] + c["B"][1])) < 2300
    assert (c["A"][1] == c["A"][2]).mean() > 0.1
    assert not (c["A"][0] == 1).any()  # a contig without rows
    _check(ctx, c, exp)


def test_stranded_sets_are_read_strand_blind(ctx):
    # a stranded B (its merge runs break at strand changes) gives the same
    c, exp = _random(20_000)
    sp = _space(c["lens"])
    rng = np.random.default_rng(5)
    a = ctx.set_from_host_stranded(sp, *c["A"], rng.integers(0, 4, 20_000).astype(np.int8))
    b = ctx.set_from_host_stranded(sp, *c["B"], rng.integers(0, 4, 20_000).astype(np.int8))
    an = ctx.annotate(a, b)
    h = an.to_host()
    for k, want in zip(("n_hits", "covered", "overlap_bases"), exp):
        assert np.array_equal(h[k].astype(np.int64), want[h["row"]]), k
    for x in (an, a, b):
        x.close()


# --------------------------------------------------- invariants at 2e6 rows
@pytest.mark.parametrize("kind", ["uniform", "pileup"])
def test_invariants_on_device_rows(ctx, kind):
    from tests.test_gpu_configs import dset, device_rows, hg38
    sp = hg38(16)
    n = 2_000_000
    if kind == "uniform":
        da, _ = device_rows(ctx, sp, n, 0xA7, 50, 500)
        db, _ = device_rows(ctx, sp, n, 0xB7, 50, 500)
    else:
        da, _ = device_rows(ctx, sp, n, 0xA8, 100, 1000, pile=(500, 2000))
        db, _ = device_rows(ctx, sp, n, 0xB8, 100, 1000, pile=(700, 2000))
    a, b = dset(ctx, sp, da), dset(ctx, sp, db)
    an = ctx.annotate(a, b)
    h = an.to_host()
    hits = np.zeros(n, np.int64)
    cov = np.zeros(n, np.int64)
    hits[h["row"]] = h["n_hits"]
    cov[h["row"]] = h["covered"]
    rows_hit, pairs, tcov, tov = an.totals()
    assert (rows_hit, pairs, tcov) == (int((hits > 0).sum()), int(hits.sum()), int(cov.sum()))
    assert tov == int(h["overlap_bases"].sum(dtype=np.uint64))
    _cross_check(ctx, a, b, hits, cov)
    # overlap >= covered, with equality where one row of B hits
    ovl = h["overlap_bases"].astype(np.int64)
    assert (ovl >= h["covered"]).all()
    one = h["n_hits"] == 1
    assert np.array_equal(ovl[one], h["covered"][one].astype(np.int64))
    if kind == "uniform":
        assert one.sum() > 1000
    # a MERGED A is disjoint: its covered bases are the bits A and B share
    m = ctx.merge(a)
    gs, ge = m.device_arrays()
    import torch
    rid = torch.arange(m.n, dtype=torch.int32, device="cuda")
    ma = ctx.set_from_global(sp, m.n, gs, ge, rid.data_ptr())
    am = ctx.annotate(ma, b)
    ba, bb = ctx.bitset(a), ctx.bitset(b)
    both = ctx.bitset_and([ba, bb])
    bh = both.to_host()
    assert am.totals()[2] == int((bh["end"] - bh["start"]).sum())
    for x in (both, ba, bb, am, ma, m, an, a, b):
        x.close()


# ------------------------------------------------------ the operator mirror
def _golden_rdd(k):
    chrom, s, e, name = read_bed_py(os.path.join(GOLDEN, f"intersect_with_overlap_0{k}.bed"))
    return [(st.ReferenceRegion(c, a, b), f"{k}:{i}") for i, (c, a, b) in
            enumerate(zip(chrom, s.tolist(), e.tolist()))]


def _rdd_ref(left, right):
    """the definition over ReferenceRegions: same contig, same strand"""
    out = []
    for r, _ in left:
        hits = [q for q, _ in right if q.referenceName == r.referenceName and
                q.strand == r.strand and q.start < r.end and q.end > r.start]
        ov = sum(min(r.end, q.end) - max(r.start, q.start) for q in hits)
        bases = set()
        for q in hits:
            bases.update(range(max(r.start, q.start), min(r.end, q.end)))
        out.append((len(hits), len(bases), ov))
    return out


def _ordered(left):
    return sorted(range(len(left)), key=lambda i: (
        java_key(left[i][0].referenceName), left[i][0].start, left[i][0].end,
        st._STRAND_ORD[left[i][0].strand], i))


def test_distributed_annotate_on_golden_files(ctx):
    left, right = _golden_rdd(0), _golden_rdd(1)
    got = st.DistributedAnnotate(left, right, ctx=ctx).compute()
    ref = _rdd_ref(left, right)
    assert got == [(left[i][0], (left[i][1],) + ref[i]) for i in _ordered(left)]
    assert len(got) == len(left)  # every left row once, in order
    pairs = st.DistributedIntersection(left, right, ctx=ctx).compute()
    assert sum(v[1] for _, v in got) == len(pairs) > 0


def test_distributed_annotate_strands_and_spaces(ctx, monkeypatch):
    c = ac.random_pair(77, 800, 300, lens=(9000, 7000, 8000, 9500, 6000))
    names = [f"c{i}" for i in range(5)]
    ls, rs = ("FORWARD", "REVERSE", "INDEPENDENT"), ("FORWARD", "INDEPENDENT")

    def rdd(rows, strands, tag):
        return [(st.ReferenceRegion(names[ci], si, ei, strands[k % len(strands)]), (tag, k))
                for k, (ci, si, ei) in enumerate(zip(*(v.tolist() for v in rows)))]
    left, right = rdd(c["A"], ls, "l"), rdd(c["B"], rs, "r")
    ref = _rdd_ref(left, right)
    want = [(left[i][0], (left[i][1],) + ref[i]) for i in _ordered(left)]
    # a left strand absent on the right: zeros
    assert all(ref[i] == (0, 0, 0) for i in range(len(left)) if left[i][0].strand == "REVERSE")
    assert sum(r[0] for r in ref) > 300
    regs = [r for r, _ in left + right]
    assert len(st._space_for(regs).spaces) == 1
    assert st.DistributedAnnotate(left, right, ctx=ctx).compute() == want
    monkeypatch.setattr(st, "SPAN_CAP", 20_000)
    assert len(st._space_for(regs).spaces) >= 2
    assert st.DistributedAnnotate(left, right, ctx=ctx).compute() == want


# ------------------------------------------------- error and memory behaviour
def test_sets_of_two_contexts_are_rejected(ctx):
    other = Context(0)
    try:
        c = PLANTED["one_each"]
        sp = _space(c["lens"])
        a, b = ctx.set_from_host(sp, *c["A"]), other.set_from_host(sp, *c["B"])
        for x, y in ((a, b), (b, a)):
            with pytest.raises(LimeError) as ei:
                ctx.annotate(x, y)
            assert ei.value.code == 1  # LIME_ERR_ARG
        a.close()
        b.close()
    finally:
        other.close()


def test_sets_of_two_spaces_are_rejected(ctx):
    c = PLANTED["one_each"]
    a = ctx.set_from_host(_space([30]), *c["A"])
    b = ctx.set_from_host(_space([31]), *c["B"])
    with pytest.raises(LimeError) as ei:
        ctx.annotate(a, b)
    assert ei.value.code == 1
    a.close()
    b.close()


def test_fill_host_out_of_range_is_an_argument_error(ctx):
    c = PLANTED["empty_b"]
    sp = _space(c["lens"])
    a, b = ctx.set_from_host(sp, *c["A"]), ctx.set_from_host(sp, *c["B"])
    an = ctx.annotate(a, b)
    lib = _ffi.load()
    buf = (C.c_uint32 * 8)()
    assert an.n == 3
    for first, count in ((0, 4), (3, 1), (-1, 1), (0, -1), (2, 2)):
        assert lib.lime_annot_fill_host(an._h, first, count, None, buf, None, None) == 1
    assert lib.lime_annot_fill_host(an._h, 1, 2, None, buf, None, None) == 0
    with pytest.raises(LimeError) as ei:
        an.fill_host(2, 5)
    assert ei.value.code == 1
    for x in (an, a, b):
        x.close()


@functools.lru_cache(maxsize=None)
def _sweep_case():
    c = ac.random_pair(905, 6000, 200, lens=(20000, 15000))
    return _space(c["lens"]), c, ac.annotate_ref(c["A"], c["B"], c["lens"])


def test_sweep_annotate(monkeypatch):
    from tests.test_gpu_pool_ownership import _put, sweep
    sp, c, exp = _sweep_case()
    assert 6000 > 2 * T  # several tiles

    def read(ctx, st_):
        h = st_["an"].to_host()
        for k, want in zip(("n_hits", "covered", "overlap_bases"), exp):
            assert np.array_equal(h[k].astype(np.int64), want[h["row"]]), k

    def totals(ctx, st_):
        assert st_["an"].totals() == (int((exp[0] > 0).sum()), int(exp[0].sum()),
                                      int(exp[1].sum()), int(exp[2].sum()))

    def bed(ctx, st_):
        row = st_["an"].fill_host()["row"]
        assert st_["an"].to_bed() == ac.format_annot(sp.names, c["A"], exp, order=row)

    sweep(monkeypatch, "annotate", [sp],
          [_put("a", lambda ctx, st_: ctx.set_from_host(sp, *c["A"])),
           _put("b", lambda ctx, st_: ctx.set_from_host(sp, *c["B"])),
           _put("an", lambda ctx, st_: ctx.annotate(st_["a"], st_["b"])), read, totals, bed])


# ------------------------------------------------------------------------ CLI
def test_cli_annotate_on_golden_files():
    paths = [os.path.join(GOLDEN, f"intersect_with_overlap_0{k}.bed") for k in (0, 1)]
    (ca, sa, ea, na), (cb, sb, eb, _) = (read_bed_py(p) for p in paths)
    names = sorted(set(ca) | set(cb), key=java_key)
    idx = {n: i for i, n in enumerate(names)}
    lens = [max([e for c, e in zip(ca + cb, ea.tolist() + eb.tolist()) if c == n]) for n in names]
    A = (np.array([idx[c] for c in ca]), sa, ea)
    B = (np.array([idx[c] for c in cb]), sb, eb)
    ref = ac.annotate_ref(A, B, lens)
    r = subprocess.run([CLI, "annotate"] + paths, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == ac.format_annot(names, A, ref, fields=na)
    assert ref[0].sum() > 0
