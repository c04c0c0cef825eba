"""lime_multiinter on the device against tests/multiinter_cases.multiinter_ref,
exact, in every view the result offers (to_host, masks, depths, to_bed,
depth_stats) and in every mode of multiinter_cases.modes.  Shapes: the planted
cases (tile, wave and thread edges of the sorted event order, coordinate groups
straddling and spanning tiles, contig bounds), stranded sets, seeded random sets
with heavy ties, invariants on 2e6 device-generated rows against the
bit-per-base path, the operator mirror (one space and a genome cut into
several), error and allocation-failure behaviour, and the CLI."""
import functools
import os
import subprocess

import numpy as np
import pytest

from lime_amd import Context, LimeError, Space
from lime_amd import set_theory as st
from tests import multiinter_cases as mc
from tests.multiinter_cases import T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bin", "lime-submit")
PLANTED = {c["name"]: c for c in mc.planted_cases()}
ARG = 1  # LIME_ERR_ARG


def _space(lens):
    return Space([f"c{i:02d}" for i in range(len(lens))], [int(x) for x in lens])


@functools.lru_cache(maxsize=None)
def _expected(name, m):
    c = PLANTED[name]
    return mc.multiinter_ref(c["sets"], c["lens"], m)


def _compare(r, sp, exp, widths_per_set=None, bed=True):
    """the result r == exp in every view (bed=False: all but the text, whose
    Python-side formatting takes many seconds for millions of runs)"""
    member = len(exp) == 4
    assert r.n == len(exp[0])
    h = r.to_host()
    for k, want in zip(("contig", "start", "end"), exp):
        assert np.array_equal(h[k].astype(np.int64), want), k
    assert (h["a_row"] == -1).all() and (h["b_row"] == -1).all()
    if bed:
        assert r.to_bed() == mc.format_multiinter(sp.names, exp)
    if not member:
        for view in (r.masks, r.depths, r.depth_stats, r.mask_device):
            with pytest.raises(LimeError) as ei:
                view()
            assert ei.value.code == ARG
        return
    ns = mc.popcount(exp[3])
    assert np.array_equal(r.masks().astype(np.int64), exp[3])
    assert np.array_equal(r.depths().astype(np.int64), ns)
    w = exp[2] - exp[1]
    assert r.depth_stats() == (int(w.sum()), int((w * ns).sum()), int(ns.max()) if len(w) else 0)
    if widths_per_set is not None:  # the check at scale
        assert r.depth_stats()[1] == widths_per_set
    if r.n > 1:  # a range of the masks
        assert np.array_equal(r.masks(1, r.n - 1).astype(np.int64), exp[3][1:])
    assert r.mask_device()


def _check(ctx, case, expected=None, strands=None, modes=None):
    sp = _space(case["lens"])
    k = len(case["sets"])
    sets = [ctx.set_from_host_stranded(sp, *rows, strands[i]) if strands is not None
            else ctx.set_from_host(sp, *rows) for i, rows in enumerate(case["sets"])]
    per_set = sum(int((u[2] - u[1]).sum()) for u in
                  (mc.multiinter_ref([x], case["lens"], 1) for x in case["sets"]))
    try:
        for m in (mc.modes(k) if modes is None else modes):
            exp = expected(m) if expected else mc.multiinter_ref(case["sets"], case["lens"], m)
            r = ctx.multiinter(sets, m)
            try:
                _compare(r, sp, exp, per_set)
            finally:
                r.close()
    finally:
        for s in sets:
            s.close()


def _planted(ctx, name):
    _check(ctx, PLANTED[name], lambda m: _expected(name, m))


# ------------------------------------------------- degenerate and small shapes
@pytest.mark.parametrize("name", ["k1", "all_empty", "one_empty", "zero_width_only",
                                  "zero_width_inside", "book_end_inside", "book_end_across",
                                  "k32_identical", "bit31_alone"])
def test_small(ctx, name):
    _planted(ctx, name)


def test_book_end_is_one_run_where_merge_gives_two(ctx):
    case = PLANTED["book_end_inside"]
    a = ctx.set_from_host(_space(case["lens"]), *case["sets"][0])
    r, m = ctx.multiinter([a]), ctx.merge(a)
    assert r.n == 1 and m.n == 2 and r.masks().tolist() == [1]
    for h in (r, m, a):
        h.close()


def test_same_set_twice_holds_two_bits(ctx):
    case = PLANTED["one_empty"]
    sp = _space(case["lens"])
    a, b = ctx.set_from_host(sp, *case["sets"][0]), ctx.set_from_host(sp, *case["sets"][2])
    twice = [case["sets"][0], case["sets"][2], case["sets"][0]]
    for m in (0, 1, 2, 3):
        r = ctx.multiinter([a, b, a], m)
        _compare(r, sp, mc.multiinter_ref(twice, case["lens"], m))
        r.close()
    r = ctx.multiinter([a, b, a])
    assert r.masks().tolist() == [5, 7, 2]
    for h in (r, a, b):
        h.close()


# ------------------------------------- tile, wave and thread edges of the events
@pytest.mark.parametrize("n_ev", mc.TILE_EVENTS)
def test_tile_sized(ctx, n_ev):
    _planted(ctx, f"tile_{n_ev}")


@pytest.mark.parametrize("name", ["straddle_same", "straddle_change", "edge_is_last",
                                  "edge_not_last", "long_over", "zero_width_5000",
                                  "heads_at_wave_and_thread_edges"])
def test_tile_edge_groups(ctx, name):
    _planted(ctx, name)


def test_heads_only_at_the_planted_events(ctx):
    case, pos = mc._heads_at()
    assert pos == [63, 64, 511, 512]
    _check(ctx, case, modes=[4])


# --------------------------------------------------------------------- contigs
@pytest.mark.parametrize("name", ["contig_touch", "contig_empty", "contig_last_only"])
def test_contigs(ctx, name):
    _planted(ctx, name)


# -------------------------------------------------------------------- stranded
def test_stranded_rows_of_one_set_join(ctx):
    case = {"sets": [mc._rows([0, 0], [0, 5], [10, 15]), mc._rows([0], [12], [20])],
            "lens": np.array([30])}
    strands = [np.array([1, 2], np.int8), np.array([0], np.int8)]
    exp = mc.multiinter_ref(case["sets"], case["lens"], 0)
    assert [v.tolist() for v in exp] == [[0, 0, 0], [0, 12, 15], [12, 15, 20], [1, 3, 2]]
    _check(ctx, case, strands=strands)
    # the first set alone: one run [0, 15)
    sp = _space(case["lens"])
    a = ctx.set_from_host_stranded(sp, *case["sets"][0], strands[0])
    r, m = ctx.multiinter([a], 1), ctx.merge(a)
    h = r.to_host()
    assert (h["start"].tolist(), h["end"].tolist()) == ([0], [15]) and m.n == 2
    for x in (r, m, a):
        x.close()


def test_random_stranded(ctx):
    case = mc.random_case(4100, 3, 4000, [9000, 0, 7000], 60, values=500)
    rng = np.random.default_rng(41)
    strands = [rng.integers(0, 4, len(s[0])).astype(np.int8) for s in case["sets"]]
    strands[2][:] = 1  # a uniform strand
    _check(ctx, case, strands=strands)


# ----------------------------------------------------------- random heavy ties
@functools.lru_cache(maxsize=None)
def _ties_case():
    # 4 sets of 5e4 rows, coordinates from ~2000 values per contig; contig 1
    # has no rows
    case = mc.random_case(7300, 4, 50_000, [400_000, 0, 300_000], 30, values=1000)
    case["lens"][1] = 500
    assert all(len(np.unique(s[1])) < 2100 for s in case["sets"])
    return case


@pytest.mark.parametrize("m", [0, 1, 2, 3, 4])
def test_random_heavy_ties(ctx, m):
    _check(ctx, _ties_case(), modes=[m])


# ----------------------------------------------- invariants on 2e6 device rows
def test_invariants_on_device_rows(ctx):
    import torch
    from tests.test_gpu_configs import assert_runs_equal, coalesce, dset, device_rows, hg38
    sp = hg38(16)
    n = 500_000
    devs, hosts = zip(*(device_rows(ctx, sp, n, 0xD0 + i, 50, 500) for i in range(4)))
    sets = [dset(ctx, sp, d) for d in devs]
    rows = [(hc.astype(np.int64), hs.astype(np.int64), he.astype(np.int64))
            for hc, hs, he in hosts]
    lens = np.asarray(sp.lengths, np.int64)
    bits = [ctx.bitset(a) for a in sets]
    pops = [b.popcount() for b in bits]
    # membership: exact, and the sum over the sets of each set's bases
    r = ctx.multiinter(sets)
    _compare(r, sp, mc.multiinter_ref(rows, lens, 0), sum(pops), bed=False)
    assert r.depth_stats()[1] == sum(pops) and r.depth_stats()[2] <= 4
    covered = r.depth_stats()[0]
    r.close()
    # min_sets = 4: the runs of the bit-per-base 4-way AND
    r = ctx.multiinter(sets, 4)
    h = r.to_host()
    _compare(r, sp, mc.multiinter_ref(rows, lens, 4), bed=False)
    both = ctx.bitset_and(bits)
    b = both.to_host()
    assert_runs_equal((h["contig"], h["start"], h["end"]),
                      coalesce(b["contig"], b["start"], b["end"]))
    r.close()
    both.close()
    # min_sets = 1: the bases of the concatenated rows
    r = ctx.multiinter(sets, 1)
    h = r.to_host()
    _compare(r, sp, mc.multiinter_ref(rows, lens, 1), bed=False)
    cat = tuple(torch.cat([d[j] for d in devs]) for j in range(3))
    torch.cuda.synchronize()
    call = dset(ctx, sp, cat)
    ball = ctx.bitset(call)
    assert int((h["end"] - h["start"]).sum()) == ball.popcount() == covered
    for x in [r, ball, call] + bits + sets:
        x.close()


# ------------------------------------------------------------ operator mirror
def _rdds(case, names):
    strands = ("FORWARD", "REVERSE", "INDEPENDENT")  # ignored
    return [[(st.ReferenceRegion(names[ci], si, ei, strands[j % 3]), j) for j, (ci, si, ei) in
             enumerate(zip(c.tolist(), s.tolist(), e.tolist()))] for c, s, e in case["sets"]]


def _want(exp, names):
    if len(exp) == 4:
        return [(st.ReferenceRegion(names[ci], si, ei), (bin(mi).count("1"), mi))
                for ci, si, ei, mi in zip(*(v.tolist() for v in exp))]
    return [st.ReferenceRegion(names[ci], si, ei) for ci, si, ei in
            zip(*(v.tolist() for v in exp))]


def test_distributed_multiintersection(ctx, monkeypatch):
    case = mc.random_case(812, 3, 2500, [9000, 7000, 8000, 9500, 6000], 300)
    assert all(len(s[0]) for s in case["sets"])
    names = [f"c{i}" for i in range(5)]
    rdds = _rdds(case, names)
    regs = [r for rdd in rdds for r, _ in rdd]
    want = {m: _want(mc.multiinter_ref(case["sets"], case["lens"], m), names) for m in (0, 2)}
    assert len(st._space_for(regs).spaces) == 1
    for m in (0, 2):
        assert st.DistributedMultiIntersection(rdds, m, ctx=ctx).compute() == want[m]
    assert all(r.strand == "INDEPENDENT" for r, _ in want[0][:50])
    monkeypatch.setattr(st, "SPAN_CAP", 20_000)
    assert len(st._space_for(regs).spaces) >= 2
    for m in (0, 2):
        assert st.DistributedMultiIntersection(rdds, m, ctx=ctx).compute() == want[m]


# ------------------------------------------------- error and memory behaviour
def test_argument_errors(ctx):
    case = PLANTED["one_empty"]
    sp = _space(case["lens"])
    a = ctx.set_from_host(sp, *case["sets"][0])

    def fails(sets, m=0):
        with pytest.raises(LimeError) as ei:
            ctx.multiinter(sets, m)
        assert ei.value.code == ARG

    fails([])
    fails([a] * 33)
    fails([a, a], 3)
    fails([a, a], -1)
    other = Context(0)
    try:
        b = other.set_from_host(sp, *case["sets"][2])
        fails([a, b])
        b.close()
    finally:
        other.close()
    # sets of different spaces
    c = ctx.set_from_host(_space([41]), *case["sets"][2])
    fails([a, c])
    # the mask accessors on a merge and on a consensus result
    m, r = ctx.merge(a), ctx.multiinter([a, a], 2)
    for res in (m, r):
        for view in (res.masks, res.mask_device):
            with pytest.raises(LimeError) as ei:
                view()
            assert ei.value.code == ARG
    assert r.to_bed() == b"c00\t3\t9\n"
    ok = ctx.multiinter([a] * 32)
    assert ok.masks().tolist() == [0xFFFFFFFF]
    for x in (ok, m, r, c, a):
        x.close()


@functools.lru_cache(maxsize=None)
def _sweep_case():
    case = mc.random_case(906, 3, 2500, [20000, 15000], 4, exact=True)
    exp = {m: mc.multiinter_ref(case["sets"], case["lens"], m) for m in (0, 2)}
    assert len(mc.events(case)[0]) > 2 * T  # three tiles
    return _space(case["lens"]), case, exp


@pytest.mark.parametrize("m", [0, 2])
def test_sweep_multiinter(monkeypatch, m):
    from tests.test_gpu_pool_ownership import _put, sweep
    sp, case, exp = _sweep_case()

    def read(ctx, st_):
        _compare(st_["r"], sp, exp[m])

    steps = [_put(f"s{i}", lambda ctx, st_, i=i: ctx.set_from_host(sp, *case["sets"][i]))
             for i in range(3)]
    steps.append(_put("r", lambda ctx, st_: ctx.multiinter([st_["s0"], st_["s1"], st_["s2"]], m)))
    sweep(monkeypatch, f"multiinter/{m}", [sp], steps + [read])


# ------------------------------------------------------------------------ CLI
def test_cli_multiinter(tmp_path):
    case = mc.random_case(907, 3, 300, [5000, 4000], 80)
    names = ["chrA", "chrB"]
    # every contig's extent is reached, so the CLI's space equals the case's
    for c, ln in enumerate(case["lens"].tolist()):
        case["sets"][0] = tuple(np.append(v, x) for v, x in zip(case["sets"][0], (c, 0, ln)))
    paths = []
    for i, (c, s, e) in enumerate(case["sets"]):
        p = tmp_path / f"in{i}.bed"
        p.write_text("".join(f"{names[ci]}\t{si}\t{ei}\n" for ci, si, ei in
                             zip(c.tolist(), s.tolist(), e.tolist())))
        paths.append(str(p))
    for m in (0, 2):
        args = [CLI, "multiinter"] + paths + (["-min", str(m)] if m else [])
        r = subprocess.run(args, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout == mc.format_multiinter(
            names, mc.multiinter_ref(case["sets"], case["lens"], m))
