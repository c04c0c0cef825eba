"""The bit-per-base build and run extraction (lime_amd/csrc/bitset.hip) at
their bin, tile and slot edges, on the planted inputs of tests/bitset_cases.py
(checked on the CPU by tests/test_bitset_cases.py, which also shows the arm
each case takes):

  a. row pieces: every length 0 .. 513 on word bits 0, 63 and 64, starts and
     ends around paint-tile and bin bounds, the packed row that looks like
     SLAB_PAD, cross pieces over 0 .. 4 tiles, a row covering the window, a
     tile wholly covered as a, as the b of a & ~b and as the a of ~a;
  b. 0 .. 2 STEP + 5 rows and 17 chunks in 16 uneven groups, 8191 / 8192 /
     8193 / 16385 rows in one (bin, chunk group) and one paint tile, empty
     tiles and bins, an empty operand of a k-way AND, 1024 / 1025 contigs,
     global rows around windows of one and two bins;
  c. optimistic binning on 8 bins and one chunk: a region of exactly rcap and
     of rcap + 1 rows, the SLAB_PAD look-alike, 7 / 96 / 97 bins, the counted
     builds after an overflow, an overflow in the middle of a 3-way AND;
  d. the word paths: runs on bits 0 and 63 and across word, thread, wave and
     tile bounds, runs reaching the window's end, 2048 / 2049 / 2050 events
     in a tile (one pass, two passes), every op on the two-pass path;
  e. the fused path: runs joined and not joined across paint tiles, a tile of
     exactly its slot's events and of two more, NOT past hi_bit;
  f. NOT over spaces of short contigs: 63 / 64 / 65 / 130 pads in a tile of
     either word path, 64 / 65 / 128 / 129 in a paint tile, pads on bit 63
     before a tile and on its first bit.

Every result is compared with the reference of tests/bitset_cases.py run for
run in output order (whole-array integer equality) and every bitset by its
popcount, on every path the case can take -- binned, words after drop_bins,
from the sorted set, mixed -- and the path the engine reports
(LIME_TRACE_RUNS) is the one the arm counter predicts.  The pool's live bytes
return to their value once the bitsets and results are closed."""
import numpy as np
import pytest

import lime_amd
from lime_amd import Space
from tests import bitset_cases as bc

pytestmark = pytest.mark.gpu

C = bc.CASES
Z32, Z64, Z8 = np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int8)
_SPACES = {}


@pytest.fixture(autouse=True)
def _trace(monkeypatch):
    monkeypatch.setenv("LIME_TRACE_RUNS", "1")


def _space(ctx, case):
    """the case's space, made once, and primed: the context keeps the device
    offsets of the last few spaces it met, so an empty set is made (and
    closed) in the space before the live bytes are read"""
    key = case["lens"]
    if key not in _SPACES:
        _SPACES[key] = Space(["c%05d" % i for i in range(len(key))], list(key))
    ctx.set_from_host_stranded(_SPACES[key], Z32, Z64, Z64, Z8).close()
    return _SPACES[key]


def _dev(cols):
    """u32 device columns (one element at least: an empty set still has a pointer)"""
    import torch
    out = []
    for x in cols:
        x = np.asarray(x, np.int64).astype(np.uint32).view(np.int32)
        out.append(torch.from_numpy(x if len(x) else np.zeros(1, np.int32)).cuda())
    torch.cuda.synchronize()
    return out


def _same(got, exp, what):
    for k, e in zip(("contig", "start", "end"), exp[:3]):
        g = np.asarray(got[k]).astype(np.int64)
        assert len(g) == len(e), (what, k, len(g), len(e))
        if not np.array_equal(g, e):
            i = int(np.flatnonzero(g != e)[0])
            raise AssertionError((what, k, i, int(g[i]), int(e[i])))


class _Run:
    """the bitsets of a case on each path, its ops against the reference;
    closing gives the pool back"""

    def __init__(self, ctx, case, capfd):
        self.ctx, self.case, self.capfd = ctx, case, capfd
        self.sp = _space(ctx, case)
        self.before = ctx.pool_live_bytes()[0]
        self.bits, self.rows = {}, {}

    def dev_rows(self, i):
        if i not in self.rows:
            self.rows[i] = _dev(self.case["sets"][i])
        return self.rows[i]

    def bitset(self, i, path):
        if (i, path) in self.bits:
            return self.bits[i, path]
        case, ctx = self.case, self.ctx
        n = len(case["sets"][i][0])
        if path == "sorted":
            c, s, e = bc.contig_rows(case, i)
            st = ctx.set_from_host(self.sp, c.astype(np.int32), s, e)
            b = ctx.bitset(st)
            st.close()
        else:
            ptrs = [t.data_ptr() for t in self.dev_rows(i)]
            if len(ptrs) == 3:
                b = ctx.bitset_from_device(self.sp, n, *ptrs)
            else:
                b = ctx.bitset_from_global(self.sp, *bc.window(case), n, *ptrs)
            if path == "words":
                b.drop_bins()
        self.bits[i, path] = b
        return b

    def op(self, op, idx, paths):
        """op over operands idx, operand j on paths[j]; the path taken"""
        if isinstance(paths, str):
            paths = (paths,) * len(idx)
        a = [self.bitset(i, p) for i, p in zip(idx, paths)]
        self.capfd.readouterr()
        if op == 4:
            res = self.ctx.bitset_and(a)
        else:
            res = self.ctx.bitset_runs(op, a[0], a[1] if len(a) > 1 else None)
        got = res.to_host()
        res.close()
        lines = [x for x in self.capfd.readouterr().err.splitlines()
                 if x.startswith("lime: bitset_runs")]
        assert len(lines) == 1, lines
        took = lines[0].split(" ", 4)[4]
        what = (self.case["key"], op, idx, paths)
        binned = all(p == "binned" for p in paths) and len(idx) <= bc.MAXK
        assert took == bc.path(self.case, op, idx, binned), what
        _same(got, bc.reference(self.case, op, idx), what)
        return took

    def fused_and(self, idx):
        """the AND of row sets idx kept binned (one k_paint_ev over all)"""
        rows = [(len(self.case["sets"][i][0]), *(t.data_ptr() for t in self.dev_rows(i)))
                for i in idx]
        if len(rows[0]) == 4:
            b = self.ctx.bitset_and_from_device(self.sp, rows)
        else:
            b = self.ctx.bitset_and_from_global(self.sp, *bc.window(self.case), rows)
        exp = bc.reference(self.case, 4, idx)
        for _ in range(2):      # binned, then from the words its popcount painted
            res = self.ctx.bitset_runs(0, b)
            _same(res.to_host(), exp, (self.case["key"], "fused and", idx))
            res.close()
            assert b.popcount() == exp[3]
            b.drop_bins()
        b.close()

    def all_ops(self, paths=("binned", "words", "sorted")):
        took = set()
        for op, idx in self.case["ops"]:
            for p in paths:
                if p == "sorted" and not bc.sortable(self.case, idx):
                    continue
                took.add(self.op(op, idx, p))
            if len(idx) == 2:   # one binned and one word operand in the same op
                took.add(self.op(op, idx, ("words", "binned")))
                took.add(self.op(op, idx, ("binned", "words")))
        return took

    def close(self):
        for (i, p), b in self.bits.items():
            assert b.popcount() == bc.reference(self.case, 0, (i,))[3], (self.case["key"], i, p)
            b.close()
        self.bits = {}
        self.ctx.synchronize()
        assert self.ctx.pool_live_bytes()[0] == self.before, self.case["key"]


def _check(ctx, capfd, key, **kw):
    r = _Run(ctx, C[key], capfd)
    took = r.all_ops(**kw)
    r.close()
    return took


# ------------------------------------------------------------ a. row pieces
def test_row_pieces(ctx, capfd):
    r = _Run(ctx, C["pieces"], capfd)
    assert r.all_ops() == {"fused", "words one-pass"}
    r.fused_and((0, 1))
    r.close()


def test_row_covering_the_window(ctx, capfd):
    assert _check(ctx, capfd, "whole") == {"fused", "words one-pass"}


# -------------------------------------------------- b. row counts and skew
@pytest.mark.parametrize("n", bc.COUNTS)
def test_row_counts(ctx, capfd, n):
    _check(ctx, capfd, "count_%d" % n)


@pytest.mark.parametrize("key", ["in_tile_%d" % n for n in bc.IN_TILE] + ["chunks_17"])
def test_rows_in_one_tile(ctx, capfd, key):
    assert "fused" in _check(ctx, capfd, key)


def test_and_with_an_empty_operand(ctx, capfd):
    r = _Run(ctx, C["and_empty"], capfd)
    r.all_ops()
    r.fused_and((0, 1, 2))
    r.fused_and((0, 2))
    r.fused_and((1,))
    r.close()


@pytest.mark.parametrize("nc", [bc.CMAX, bc.CMAX + 1])
def test_contig_table(ctx, capfd, nc):
    _check(ctx, capfd, "contigs_%d" % nc)


@pytest.mark.parametrize("bins", [1, 2])
def test_global_rows_around_a_window(ctx, capfd, bins):
    r = _Run(ctx, C["window_%d" % bins], capfd)
    r.all_ops()
    r.fused_and((0, 1))
    r.close()


# ------------------------------------------------- c. optimistic binning
class _Opt:
    """a fresh context with optimistic binning on and its trace: after an
    overflow a context prefers the counted path, which must not leak"""

    def __init__(self, monkeypatch, capfd):
        monkeypatch.setenv("LIME_TRACE_BINNING", "1")
        monkeypatch.setenv("LIME_BIN_OPTIMISTIC", "1")
        self.ctx, self.capfd = lime_amd.Context(0), capfd

    def build(self, key):
        """the case's op over freshly built bitsets -> the binning trace"""
        r = _Run(self.ctx, C[key], self.capfd)
        self.capfd.readouterr()
        (op, idx), = C[key]["ops"]
        if op == 4:
            rows = [(len(C[key]["sets"][i][0]), *(t.data_ptr() for t in r.dev_rows(i))) for i in idx]
            b = self.ctx.bitset_and_from_device(r.sp, rows)
        else:
            b = r.bitset(0, "binned")
        log = self.capfd.readouterr().err.splitlines()
        exp = bc.reference(C[key], op, idx)
        for _ in range(2):      # fused, then words
            res = self.ctx.bitset_runs(0, b)
            _same(res.to_host(), exp, key)
            res.close()
            assert b.popcount() == exp[3]
            b.drop_bins()
        if op == 4:
            b.close()
        r.close()
        rows = [x.split()[3] for x in log if x.startswith("lime: bin_rows")]
        return rows, sum("region overflow, counted again" in x for x in log)

    def close(self):
        self.ctx.close()


@pytest.fixture
def opt(monkeypatch, capfd):
    o = _Opt(monkeypatch, capfd)
    yield o
    o.close()


@pytest.mark.parametrize("key", ["opt_exact", "opt_lookalike", "opt_two_chunks", "opt_96_bins"])
def test_optimistic_regions_that_fit(opt, key):
    assert opt.build(key) == (["optimistic"], 0)


@pytest.mark.parametrize("key", ["opt_over", "opt_one_bin"])
def test_optimistic_region_overflows(opt, key):
    assert opt.build(key) == (["optimistic", "counted"], 1)


@pytest.mark.parametrize("key", ["opt_7_bins", "opt_97_bins"])
def test_optimistic_gate(opt, key):
    assert opt.build(key) == (["counted"], 0)


def test_counted_builds_after_an_overflow(opt):
    # the overflow sets bin_pessimism to 32 and the counted rerun of the same
    # set spends one: the next 31 builds are counted, the 32nd optimistic
    assert opt.build("opt_over") == (["optimistic", "counted"], 1)
    for i in range(bc.PESSIMISM - 1):
        assert opt.build("opt_exact") == (["counted"], 0), i
    assert opt.build("opt_exact") == (["optimistic"], 0)


def test_overflow_in_the_middle_of_an_and(opt):
    # (set 2 is binned before set 1's flags are read: still optimistic)
    assert opt.build("opt_and") == (["optimistic", "optimistic", "optimistic", "counted"], 1)


# ------------------------------------------------------ d. the word paths
def test_word_path_run_edges(ctx, capfd):
    assert _check(ctx, capfd, "w_edges") == {"fused", "words one-pass"}


@pytest.mark.parametrize("nw", [bc.EV_TW, 2 * bc.BT, bc.BT + 77, 2 * bc.EV_TW + 1])
def test_run_reaching_the_window_end(ctx, capfd, nw):
    assert _check(ctx, capfd, "w_end_%d" % nw) == {"fused", "words one-pass"}


@pytest.mark.parametrize("nw", [bc.BT + 77, 2 * bc.EV_TW + 1])
def test_odd_last_word_on_the_two_pass_path(ctx, capfd, nw):
    assert _check(ctx, capfd, "w_end2_%d" % nw) == {"fused", "words one-pass", "words two-pass"}


@pytest.mark.parametrize("ev", [2048, 2049, 2050])
def test_events_of_a_word_tile(ctx, capfd, ev):
    took = _check(ctx, capfd, "w_dense_%d" % ev)
    assert took == {"fused", "words one-pass", "words two-pass"}


# ------------------------------------------------------ e. the fused path
def test_fused_run_edges(ctx, capfd):
    assert _check(ctx, capfd, "f_edges") == {"fused", "words one-pass"}


@pytest.mark.parametrize("ev,want", [(4096, "fused"), (4098, "fused overflow, words two-pass")])
def test_events_of_a_paint_tile(ctx, capfd, ev, want):
    assert _check(ctx, capfd, "f_slot_%d" % ev) == {want, "words two-pass"}


def test_not_past_the_window(ctx, capfd):
    assert _check(ctx, capfd, "f_not_window") == {"fused", "words one-pass"}


# ------------------------------------------------------ f. pads under NOT
PAD_CASES = ["%s_%d" % (tag, n) for tag, table in (("p1", bc.PAD_WORDS), ("p2", bc.PAD_WORDS2),
                                                   ("pf", bc.PAD_PAINT)) for n in table]


@pytest.mark.parametrize("key", PAD_CASES + ["pad_bit63", "pad_bit0"])
def test_pads_under_not(ctx, capfd, key):
    words = "words two-pass" if key.startswith("p2") else "words one-pass"
    assert _check(ctx, capfd, key) == {"fused", words}
