"""lime_coverage on the device against tests/coverage_cases.depth_runs: the
runs (to_host), their depths, the bedGraph text and the depth statistics, all
exact.  Shapes: the planted cases of coverage_cases.py (tile edges of k_cov's
merged event order, coordinate groups straddling tiles, staircases, contig
bounds), seeded random sets with heavy ties, the operator mirror (one space
and a genome cut into several), invariants on 2e6 device-generated rows
against the bit-per-base path, error and allocation-failure behaviour, and
the CLI."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from lime_amd import Context, LimeError, Space, _ffi
from lime_amd import set_theory as st
from tests import coverage_cases as cc
from tests.coverage_cases import T
from tests.util import GOLDEN, java_key, read_bed_py

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bin", "lime-submit")
PLANTED = {c["name"]: c for c in cc.planted_cases()}


def _space(lens):
    return Space([f"c{i:02d}" for i in range(len(lens))], [int(x) for x in lens])


@functools.lru_cache(maxsize=None)
def _expected(name):
    c = PLANTED[name]
    return cc.depth_runs(c["contig"], c["start"], c["end"], c["lens"])


def _check(ctx, case, exp=None, strand=None):
    """coverage of the case == exp in every view the result offers"""
    if exp is None:
        exp = cc.depth_runs(case["contig"], case["start"], case["end"], case["lens"])
    sp = _space(case["lens"])
    rows = (case["contig"], case["start"], case["end"])
    a = (ctx.set_from_host_stranded(sp, *rows, strand) if strand is not None
         else ctx.set_from_host(sp, *rows))
    r = ctx.coverage(a)
    try:
        assert r.n == len(exp[0])
        h, d = r.to_host(), r.depths()
        for k, want in zip(("contig", "start", "end"), exp):
            assert np.array_equal(h[k].astype(np.int64), want), k
        assert np.array_equal(d.astype(np.int64), exp[3])
        assert (h["a_row"] == -1).all() and (h["b_row"] == -1).all()
        assert r.to_bed() == cc.format_bedgraph(sp.names, exp)
        w = exp[2] - exp[1]
        assert r.depth_stats() == (int(w.sum()), int((w * exp[3]).sum()),
                                   int(exp[3].max()) if len(w) else 0)
        # the check at scale: width x depth sums to the input widths
        assert r.depth_stats()[1] == int((case["end"] - case["start"]).sum())
        if r.n > 1:  # a range of the depths
            assert np.array_equal(r.depths(1, r.n - 1), d[1:])
    finally:
        r.close()
        a.close()


# ------------------------------------------------- degenerate and small shapes
@pytest.mark.parametrize("name", ["empty", "one_row", "zero_width_only", "book_ended",
                                  "zero_width_inside"])
def test_small(ctx, name):
    _check(ctx, PLANTED[name], _expected(name))


def test_book_ended_is_one_run_where_merge_gives_two(ctx):
    case = PLANTED["book_ended"]
    sp = _space(case["lens"])
    a = ctx.set_from_host(sp, case["contig"], case["start"], case["end"])
    r, m = ctx.coverage(a), ctx.merge(a)
    assert r.n == 1 and m.n == 2
    assert r.depths().tolist() == [1]
    for h in (r, m, a):
        h.close()


@pytest.mark.parametrize("k", [1, 2, 65, 70000])
def test_identical_rows(ctx, k):
    # k = 70000: a depth past 2^16, and both coordinate groups span dozens of
    # tiles -- the second is closed from lower bounds over all rows before it
    name = f"identical_{k}"
    assert _expected(name)[3].tolist() == [k]
    _check(ctx, PLANTED[name], _expected(name))


# ------------------------------------------------------------------ tile edges
@pytest.mark.parametrize("n", cc.TILE_ROWS)
def test_tile_sized(ctx, n):
    _check(ctx, PLANTED[f"tile_sized_{n}"], _expected(f"tile_sized_{n}"))


@pytest.mark.parametrize("name", [f"chain_{T // 2 + 3}", "straddle_change", "edge_is_last",
                                  "edge_not_last", "long_over_chain"])
def test_tile_edge_groups(ctx, name):
    _check(ctx, PLANTED[name], _expected(name))


@pytest.mark.parametrize("name", ["staircase_1500_7", "staircase_1500_3001"])
def test_staircase(ctx, name):
    assert len(_expected(name)[0]) == 2 * 1500 - 1
    _check(ctx, PLANTED[name], _expected(name))


# --------------------------------------------------------------------- contigs
@pytest.mark.parametrize("name", ["contig_touch", "contig_gap", "contig_last_end"])
def test_contigs(ctx, name):
    _check(ctx, PLANTED[name], _expected(name))


# --------------------------------------------------- random and operator paths
@pytest.mark.parametrize("n,stranded", [(20_000, False), (60_000, True), (200_000, False)])
def test_random_heavy_ties(ctx, n, stranded):
    # coordinates from ~2100 values for up to 2e5 rows; contig 1 has no rows
    case = cc.random_case(7000 + n, n, [800, 0, 600, 700], 40)
    case["lens"][1] = 500
    assert not (case["contig"] == 1).any() and len(np.unique(case["start"])) < n // 4
    strand = np.random.default_rng(n).integers(0, 4, n).astype(np.int8) if stranded else None
    _check(ctx, case, strand=strand)


@functools.lru_cache(maxsize=None)
def _cpg():
    chrom, s, e, _ = read_bed_py(os.path.join(GOLDEN, "cpg.bed"))
    names = sorted(set(chrom), key=java_key)
    idx = {n: i for i, n in enumerate(names)}
    c = np.array([idx[x] for x in chrom], np.int64)
    lens = np.array([e[c == i].max() for i in range(len(names))], np.int64)
    exp = cc.depth_runs(c, s, e, lens)
    rdd = [(st.ReferenceRegion(x, a, b), k) for k, (x, a, b) in
           enumerate(zip(chrom, s.tolist(), e.tolist()))]
    want = [(st.ReferenceRegion(names[ci], si, ei), di)
            for ci, si, ei, di in zip(*(v.tolist() for v in exp))]
    return names, exp, rdd, want


def test_distributed_coverage_on_cpg(ctx):
    names, exp, rdd, want = _cpg()
    got = st.DistributedCoverage(rdd, ctx=ctx).compute()
    assert got == want and len(got) > 20_000
    assert all(r.strand == "INDEPENDENT" for r, _ in got[:100])


def test_distributed_coverage_across_spaces(ctx, monkeypatch):
    case = cc.random_case(811, 3000, [9000, 7000, 8000, 9500, 6000], 300)
    names = [f"c{i}" for i in range(5)]
    exp = cc.depth_runs(case["contig"], case["start"], case["end"], case["lens"])
    want = [(st.ReferenceRegion(names[ci], si, ei), di)
            for ci, si, ei, di in zip(*(v.tolist() for v in exp))]
    strands = ("FORWARD", "REVERSE", "INDEPENDENT")  # ignored
    rdd = [(st.ReferenceRegion(names[ci], si, ei, strands[k % 3]), k) for k, (ci, si, ei) in
           enumerate(zip(case["contig"].tolist(), case["start"].tolist(), case["end"].tolist()))]
    regs = [r for r, _ in rdd]
    assert len(st._space_for(regs).spaces) == 1
    assert st.DistributedCoverage(rdd, ctx=ctx).compute() == want
    monkeypatch.setattr(st, "SPAN_CAP", 20_000)
    assert len(st._space_for(regs).spaces) >= 2
    assert st.DistributedCoverage(rdd, ctx=ctx).compute() == want


# --------------------------------------------------- invariants at 2e6 rows
@pytest.mark.parametrize("kind", ["uniform", "pileup"])
def test_invariants_on_device_rows(ctx, kind):
    from tests.test_gpu_configs import assert_runs_equal, coalesce, dset, device_rows, hg38
    sp = hg38(16)
    n = 2_000_000
    dev, (hc, hs, he) = (device_rows(ctx, sp, n, 0xC0, 50, 500) if kind == "uniform" else
                         device_rows(ctx, sp, n, 0xC1, 100, 1000, pile=(500, 2000)))
    a = dset(ctx, sp, dev)
    r = ctx.coverage(a)
    cov, depth_bases, mx = r.depth_stats()
    widths = he.astype(np.int64) - hs.astype(np.int64)
    assert depth_bases == int(widths.sum())
    bits = ctx.bitset(a)
    assert cov == bits.popcount()
    # numpy's maximum depth: after the i-th sorted start, i + 1 rows have
    # started and those with end <= it have ended
    gs = np.sort(sp.offsets[hc] + hs.astype(np.int64))
    ge = np.sort(sp.offsets[hc] + he.astype(np.int64))
    depth_at = np.arange(1, n + 1) - np.searchsorted(ge, gs, "right")
    assert mx == int(depth_at.max()) and mx == int(r.depths().max())
    if kind == "pileup":
        assert mx > 50
    h = r.to_host()
    assert (h["end"] > h["start"]).all() and r.depths().min() >= 1
    b = ctx.bitset_runs(0, bits).to_host()
    assert_runs_equal(coalesce(h["contig"], h["start"], h["end"]),
                      coalesce(b["contig"], b["start"], b["end"]))
    for x in (r, bits, a):
        x.close()


# ------------------------------------------------- error and memory behaviour
def test_depths_of_a_merge_result_is_an_argument_error(ctx):
    case = PLANTED["one_row"]
    a = ctx.set_from_host(_space(case["lens"]), case["contig"], case["start"], case["end"])
    m = ctx.merge(a)
    lib = _ffi.load()
    buf = (C.c_uint32 * 4)()
    assert lib.lime_result_depths(m._h, 0, 1, buf) == 1  # LIME_ERR_ARG
    with pytest.raises(LimeError) as ei:
        m.depth_stats()
    assert ei.value.code == 1
    with pytest.raises(LimeError):
        m.depth_device()
    assert m.to_bed() == b"c00\t3\t9\n"  # other results keep three columns
    m.close()
    a.close()


def test_set_of_another_context_is_rejected(ctx):
    other = Context(0)
    try:
        case = PLANTED["one_row"]
        a = other.set_from_host(_space(case["lens"]), case["contig"], case["start"],
                                case["end"])
        with pytest.raises(LimeError) as ei:
            ctx.coverage(a)
        assert ei.value.code == 1
        a.close()
    finally:
        other.close()


@functools.lru_cache(maxsize=None)
def _sweep_case():
    case = cc.random_case(905, 6000, [20000, 15000], 200)
    return _space(case["lens"]), case, cc.depth_runs(case["contig"], case["start"], case["end"],
                                                     case["lens"])


def test_sweep_coverage(monkeypatch):
    from tests.test_gpu_pool_ownership import _put, sweep
    sp, case, exp = _sweep_case()
    assert 2 * 6000 > 2 * T  # several tiles

    def read(ctx, st_):
        h = st_["r"].to_host()
        for k, want in zip(("contig", "start", "end"), exp):
            assert np.array_equal(h[k].astype(np.int64), want), k
        assert np.array_equal(st_["r"].depths().astype(np.int64), exp[3])

    def stats(ctx, st_):
        w = exp[2] - exp[1]
        assert st_["r"].depth_stats() == (int(w.sum()), int((w * exp[3]).sum()),
                                          int(exp[3].max()))

    def bed(ctx, st_):
        assert st_["r"].to_bed() == cc.format_bedgraph(sp.names, exp)

    sweep(monkeypatch, "coverage", [sp],
          [_put("a", lambda ctx, st_: ctx.set_from_host(sp, case["contig"], case["start"],
                                                         case["end"])),
           _put("r", lambda ctx, st_: ctx.coverage(st_["a"])), read, stats, bed])


# ------------------------------------------------------------------------ CLI
def test_cli_coverage_is_the_bedgraph():
    names, exp, _, _ = _cpg()
    r = subprocess.run([CLI, "coverage", os.path.join(GOLDEN, "cpg.bed")], capture_output=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == cc.format_bedgraph(names, exp)
