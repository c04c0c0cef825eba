"""Pool blocks have one owner: a failed call leaves the context's live bytes
as it found them, and nothing half built behind.

Failure sweep.  LIME_TEST_ALLOC_FAIL=N (read once by lime_ctx_create) makes
that context's N-th pool allocation fail, once, on the host: the operator
returns LIME_ERR_NOMEM before any launch sees the pointer.  Every operator
sequence below is run step by step -- one engine call per step -- in a fresh
context for N = 1, 2, ...  When a step raises:

  - the error is the out-of-memory one;
  - the live bytes equal the value recorded just before the step;
  - the same call repeated on the same context succeeds, and the sequence's
    results equal the oracle (no half-built prefix max, tie index or bins);
  - once the results are destroyed the live bytes are back at the value the
    sequence started from.

The sweep of a sequence ends at the first N for which nothing raises; reaching
N = 400 fails the test (no sequence makes that many allocations; the final N
of each is printed).

A space's device offsets and lengths are cached by the context at first use
and stay its own for its lifetime (lime_ctx::spaces: two blocks of n_contigs +
1 words, rounded to the pool's 256 bytes).  Each sequence therefore begins
with a checked step that creates (and destroys) an empty set in its space;
the value the sequence starts from is taken after that step.  If that first
step is the one that fails, the context may already have cached the space:
its live bytes are then unchanged or larger by exactly that entry.

The inputs are made once (host arrays or torch device tensors) and shared by
the contexts; the references are computed once per sequence.

The second part needs no hook: the validation errors of the sort, the
subtract's LIME_TEST_SUB_SKEW failure and the BED parse errors leave the live
bytes unchanged too."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from lime_amd import Context, LimeError, Space, SUBTRACT_LIME
from lime_amd import _ffi
from oracle import oracle
from tests.scan_cases import device_order_plain, device_order_stranded
from tests.util import GOLDEN, as_sorted_tuples, random_sets, read_bed_py

pytestmark = pytest.mark.gpu

NOMEM = 4  # LIME_ERR_NOMEM
CAP = 400
Z32, Z64 = np.zeros(0, np.int32), np.zeros(0, np.int64)


def _space(n_contigs, contig_len):
    return Space([f"c{i:02d}" for i in range(n_contigs)], [contig_len] * n_contigs)


def _live(ctx):
    return ctx.pool_live_bytes()[0]


def _close_all(st):
    for h in reversed(list(st.values())):
        if hasattr(h, "close"):
            h.close()
    st.clear()


def sweep(monkeypatch, name, spaces, steps):
    """steps: callables (ctx, st), one engine call each; what a step creates
    goes into the dict st (destroyed in reverse order at the end)."""
    sp, = spaces
    cached = 2 * ((4 * (len(sp.names) + 1) + 255) // 256 * 256)  # the context's entry

    def prime(ctx, st):
        ctx.set_from_host(sp, Z32, Z64, Z64).close()

    for n in range(1, CAP + 1):
        monkeypatch.setenv("LIME_TEST_ALLOC_FAIL", str(n))
        ctx = Context(0)
        monkeypatch.delenv("LIME_TEST_ALLOC_FAIL")
        st, raised, base = {}, 0, None
        try:
            for i, step in enumerate([prime] + list(steps)):
                before = _live(ctx)
                try:
                    step(ctx, st)
                except LimeError as e:
                    raised += 1
                    assert e.code == NOMEM, (name, n, i, str(e))
                    if i == 0:
                        assert _live(ctx) in (before, before + cached), (name, n)
                    else:
                        assert _live(ctx) == before, (name, n, i)
                    step(ctx, st)  # the same call on the same context
                if i == 0:
                    base = _live(ctx)
            _close_all(st)
            assert _live(ctx) == base, (name, n)
        finally:
            _close_all(st)
            ctx.close()
        assert raised <= 1, (name, n)  # the hook fires once
        if not raised:
            print(f"{name}: {n - 1} allocations swept")
            return
    pytest.fail(f"{name}: an allocation still failed at N = {CAP}")


def _dev(*cols):
    import torch
    t = [torch.from_numpy(np.ascontiguousarray(x).astype(np.int64).astype(np.int32)).cuda()
         for x in cols]
    torch.cuda.synchronize()
    return t


def _rows(res, keys):
    """the records as one array, rows in sorted order"""
    arr = np.stack([np.asarray(res[k]).astype(np.int64) for k in keys], axis=1)
    return arr[np.lexsort(arr.T[::-1])] if len(arr) else arr


def _put(key, make):
    def step(ctx, st):
        st[key] = make(ctx, st)
    return step


# ----------------------------------------------------------- set creation
@functools.lru_cache(maxsize=None)
def _digit_case(kind):
    # span 40002: 16 key bits, no bucket candidate -- the digit passes
    rng = np.random.default_rng(600)
    (c, s, e), _ = random_sets(rng, 3000, 1, n_contigs=2, contig_len=20000, max_len=300,
                               zero_frac=0.1 if kind == "zero_width" else 0.0, dup_frac=0.05)
    strand = rng.integers(0, 4, 3000).astype(np.int8) if kind == "stranded" else None
    order = (device_order_stranded(c, s, e, strand) if kind == "stranded"
             else device_order_plain(c, s, e))
    return _space(2, 20000), (c, s, e), strand, order


@pytest.mark.parametrize("kind", ["plain", "stranded", "zero_width"])
def test_sweep_set_digit_passes(monkeypatch, kind):
    sp, A, strand, order = _digit_case(kind)
    if kind == "zero_width":
        assert (A[2] == A[1]).any()

    def create(ctx, st):
        return (ctx.set_from_host_stranded(sp, *A, strand) if kind == "stranded"
                else ctx.set_from_host(sp, *A))

    def read(ctx, st):
        h = st["a"].to_host()
        assert (h["row"] == order).all()
        for k, x in zip(("contig", "start", "end"), A):
            assert (h[k] == x[order]).all(), k

    sweep(monkeypatch, f"set/digit/{kind}", [sp], [_put("a", create), read])


@functools.lru_cache(maxsize=None)
def _bucket_case(wide):
    # one contig of 131000 (wide: 262000) bases: 17 (18) key bits, TB 16,
    # 2.2e6 rows over 65501 buckets -- ~33 per bucket, just over LMIN; widths
    # under 300 take the u16-width prep and the packed second pass, one width
    # of 70000 the unpacked one
    L = 262_000 if wide else 131_000
    rng = np.random.default_rng(601)
    n = 2_200_000
    s = rng.integers(0, L - 300, n)
    e = s + rng.integers(0, 300, n)
    if wide:
        s[12345], e[12345] = 1000, 71_000
    c = np.zeros(n, np.int32)
    return _space(1, L), n, _dev(c, s, e), (s, e), device_order_plain(c, s, e)


@pytest.mark.parametrize("wide", [False, True], ids=["packed", "unpacked"])
def test_sweep_set_bucketed(monkeypatch, wide):
    sp, n, dev, (s, e), order = _bucket_case(wide)

    def create(ctx, st):
        return ctx.set_from_device(sp, n, *(t.data_ptr() for t in dev))

    def read(ctx, st):
        h = st["a"].to_host()
        assert (h["row"] == order).all()
        assert (h["start"] == s[order]).all() and (h["end"] == e[order]).all()

    sweep(monkeypatch, f"set/bucketed/{'unpacked' if wide else 'packed'}", [sp],
          [_put("a", create), read])


# ------------------------------------------------------------------ merge
@functools.lru_cache(maxsize=None)
def _merge_case(stranded):
    rng = np.random.default_rng(602)
    A = random_sets(rng, 4000, 1, n_contigs=2, contig_len=60000, max_len=300, zero_frac=0.05,
                    dup_frac=0.05, book_frac=0.1)[0]
    strand = rng.integers(0, 4, 4000).astype(np.int8) if stranded else None
    exp = oracle.merge((*A, strand) if stranded else A)
    return _space(2, 60000), A, strand, exp


@pytest.mark.parametrize("stranded", [False, True], ids=["plain", "stranded"])
def test_sweep_merge(monkeypatch, stranded):
    sp, A, strand, exp = _merge_case(stranded)
    keys = ("contig", "start", "end")

    def create(ctx, st):
        return (ctx.set_from_host_stranded(sp, *A, strand) if stranded
                else ctx.set_from_host(sp, *A))

    def read(ctx, st):
        assert as_sorted_tuples(st["m"].to_host(), keys) == as_sorted_tuples(exp, keys)

    def checksum(ctx, st):
        assert st["m"].checksum()[:2] == oracle.result_checksum({k: exp[k] for k in keys})

    sweep(monkeypatch, f"merge/{'stranded' if stranded else 'plain'}", [sp],
          [_put("a", create), _put("m", lambda ctx, st: ctx.merge(st["a"])), read, checksum])


# --------------------------------------------------------------- subtract
@functools.lru_cache(maxsize=None)
def _subtract_case(kind):
    if kind == "two_pass":
        # (test_subtract_one_pass_and_two_pass, deep B: count + write passes)
        rng = np.random.default_rng(4242)
        L = 200_000
        A = random_sets(rng, 8000, 1, n_contigs=2, contig_len=L, max_len=400, zero_frac=0.05,
                        dup_frac=0.05, book_frac=0.1)[0]
        B = random_sets(rng, 4000, 1, n_contigs=2, contig_len=L, max_len=100, zero_frac=0.05,
                        dup_frac=0.05, book_frac=0.1)[0]
        B = [x.copy() for x in B]
        B[0][:30], B[1][:30] = B[0][40], B[1][40]
        B[2][:30] = B[1][40] + rng.integers(1, 300, 30)
        k = 300
        c = rng.integers(0, 2, k).astype(B[0].dtype)
        st = rng.integers(0, L - 30_000, k)
        B = [np.concatenate([B[0], c]), np.concatenate([B[1], st]),
             np.concatenate([B[2], st + rng.integers(5_000, 30_000, k)])]
        t = 0
    else:
        # (test_subtract_total_disagreement_fails: 4000 x 3000)
        rng = np.random.default_rng(5200)
        L = 240_000
        A, B = random_sets(rng, 4000, 3000, n_contigs=2, contig_len=L, max_len=300)
        keep = B[2] > B[1]
        B = [x[keep].copy() for x in B]
        if kind == "tie_index":  # one same-start group of 30 rows, past TIE_G = 16
            B[0][:30], B[1][:30] = B[0][40], B[1][40]
            B[2][:30] = B[1][40] + rng.integers(1, 30, 30)
        t = 1 if kind == "walk" else 0
    return _space(2, L), tuple(A), tuple(B), t, oracle.subtract(A, B, t, SUBTRACT_LIME)


@pytest.mark.parametrize("kind", ["fused", "no_ls", "two_pass", "walk", "tie_index"])
def test_sweep_subtract(monkeypatch, kind):
    sp, A, B, t, exp = _subtract_case(kind)
    if kind == "no_ls":
        monkeypatch.setenv("LIME_SUB_NO_LS", "1")
    else:
        monkeypatch.delenv("LIME_SUB_NO_LS", raising=False)

    def read(ctx, st):
        res = st["r"].to_host()
        og = np.argsort(res["a_row"], kind="stable")
        oe = np.argsort(exp["a_row"], kind="stable")
        for key in ("contig", "start", "end", "a_row", "b_row"):
            assert list(res[key][og]) == list(exp[key][oe]), key

    def checksum(ctx, st):
        assert st["r"].checksum()[:2] == oracle.result_checksum(exp)

    sweep(monkeypatch, f"subtract/{kind}", [sp],
          [_put("a", lambda ctx, st: ctx.set_from_host(sp, *A)),
           _put("b", lambda ctx, st: ctx.set_from_host(sp, *B)),
           _put("r", lambda ctx, st: ctx.subtract(st["a"], st["b"], t, SUBTRACT_LIME)),
           read, checksum])


# ------------------------------------------------------------------ pairs
@functools.lru_cache(maxsize=None)
def _pairs_case(kind):
    rng = np.random.default_rng(603)
    A, B = random_sets(rng, 3000, 3000, n_contigs=2, contig_len=90000, max_len=400,
                       zero_frac=0.05, dup_frac=0.05, book_frac=0.05)
    sa = rng.integers(0, 4, 3000).astype(np.int8)
    sb = rng.integers(0, 4, 3000).astype(np.int8)
    if kind == "intersect":
        exp = oracle.intersect(A, B)
    elif kind == "window":
        exp = oracle.window(A, B, 200)
    else:
        exp = oracle.closest((*A, sa), (*B, sb), 0)
    return _space(2, 90000), A, sa, B, sb, exp


@pytest.mark.parametrize("kind", ["intersect", "window", "closest", "closest_recursion"])
def test_sweep_pairs(monkeypatch, kind):
    sp, A, sa, B, sb, exp = _pairs_case(kind.split("_")[0])
    closest = kind.startswith("closest")
    if kind == "closest_recursion":  # (one Jacobi round, then the in-order recursion)
        monkeypatch.setenv("LIME_CLOSEST_MAX_ROUNDS", "1")
    else:
        monkeypatch.delenv("LIME_CLOSEST_MAX_ROUNDS", raising=False)
    want = _rows(exp, ("start", "end", "a_row", "b_row"))

    def make(X, sx):
        return lambda ctx, st: (ctx.set_from_host_stranded(sp, *X, sx) if closest
                                else ctx.set_from_host(sp, *X))

    def count(ctx, st):
        if kind == "intersect":
            return ctx.intersect(st["a"], st["b"])
        if kind == "window":
            return ctx.window(st["a"], st["b"], 200)
        return ctx.closest(st["a"], st["b"], 0)

    def fill(ctx, st):
        assert st["p"].n == len(exp["start"])
        p = st["p"].fill_host()
        assert np.array_equal(_rows(p, ("start", "end", "a_row", "b_row")), want)

    def checksum(ctx, st):
        assert st["p"].checksum() == oracle.checksum_pairs(exp)

    sweep(monkeypatch, f"pairs/{kind}", [sp],
          [_put("a", make(A, sa)), _put("b", make(B, sb)), _put("p", count), fill, checksum])


# ------------------------------------------------------------- complement
@functools.lru_cache(maxsize=None)
def _complement_case():
    rng = np.random.default_rng(604)
    A = random_sets(rng, 3000, 1, n_contigs=3, contig_len=50000, max_len=300, zero_frac=0.05,
                    book_frac=0.1)[0]
    return _space(3, 50000), A, oracle.complement(A, [50000] * 3)


def test_sweep_complement(monkeypatch):
    sp, A, exp = _complement_case()

    def read(ctx, st):
        got = st["r"].to_host()
        for k in ("contig", "start", "end"):
            assert list(got[k]) == list(exp[k]), k

    sweep(monkeypatch, "complement", [sp],
          [_put("a", lambda ctx, st: ctx.set_from_host(sp, *A)),
           _put("r", lambda ctx, st: ctx.complement(sp, st["a"])), read])


# ---------------------------------------------------------------- bitsets
@functools.lru_cache(maxsize=None)
def _bitset_case():
    from tests.test_gpu_configs import coalesce
    rng = np.random.default_rng(605)
    A, B = random_sets(rng, 3000, 3000, n_contigs=2, contig_len=200000, max_len=2000)
    ma, mb = oracle.merge(A), oracle.merge(B)
    ix = oracle.intersect((ma["contig"], ma["start"], ma["end"]),
                          (mb["contig"], mb["start"], mb["end"]))
    order = np.lexsort((ix["start"], ix["contig"]))
    exp = coalesce(*(np.asarray(ix[k])[order] for k in ("contig", "start", "end")))
    return _space(2, 200000), len(A[0]), _dev(*A), len(B[0]), _dev(*B), exp


def test_sweep_bitset_and_runs(monkeypatch):
    from tests.test_gpu_configs import coalesce
    sp, na, da, nb, db, exp = _bitset_case()

    def read(ctx, st):
        got = st["r"].to_host()
        got = coalesce(got["contig"], got["start"], got["end"])
        for x, y in zip(got, exp):
            assert np.asarray(x).tolist() == np.asarray(y).tolist()

    sweep(monkeypatch, "bitset/and_runs", [sp],
          [_put("x", lambda ctx, st: ctx.bitset_from_device(sp, na, *(t.data_ptr() for t in da))),
           _put("y", lambda ctx, st: ctx.bitset_from_device(sp, nb, *(t.data_ptr() for t in db))),
           _put("r", lambda ctx, st: ctx.bitset_and([st["x"], st["y"]])), read])


# ------------------------------------------------------------------ route
@functools.lru_cache(maxsize=None)
def _route_case():
    import torch
    lens = [300_000, 200_000, 250_000]
    sp = Space(["c0", "c1", "c2"], lens)
    rng = np.random.default_rng(606)
    n, nsh = 20_003, 5
    c = rng.integers(0, 3, n).astype(np.int32)
    L = np.array(lens)[c]
    s = (rng.random(n) * (L - 1)).astype(np.int64)
    e = np.minimum(s + rng.integers(0, 4000, n), L)
    g0, g1 = sp.offsets[c] + s, sp.offsets[c] + e
    span = int(sp.span)
    cuts = np.sort(rng.choice(np.arange(1, span), nsh - 1, replace=False))
    splits = [0] + [int(x) for x in cuts] + [span]
    dest = np.searchsorted(np.array(splits, np.int64), g0, side="right") - 1
    order = np.argsort(dest, kind="stable")  # by shard, input order kept
    want = np.stack([g0[order], g1[order], 7 + order], 1).astype(np.int64)
    buf = torch.empty((n, 3), dtype=torch.int32, device="cuda")
    cols = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3)]
    return sp, n, _dev(c, s, e), splits, np.bincount(dest, minlength=nsh).tolist(), want, buf, cols


def test_sweep_route_interleaved(monkeypatch):
    import torch
    sp, n, dev, splits, counts, want, buf, cols = _route_case()

    def route(ctx, st):
        got = ctx.route_rows_interleaved(sp, n, *(t.data_ptr() for t in dev), splits, 3,
                                         buf.data_ptr(), cap=n, row_base=7)
        torch.cuda.synchronize()
        assert got == counts
        assert np.array_equal(buf.cpu().numpy().view(np.uint32).astype(np.int64), want)

    def split(ctx, st):
        ctx.deinterleave(n, 3, buf.data_ptr(), *(t.data_ptr() for t in cols))
        ctx.synchronize()
        got = np.stack([t.cpu().numpy().view(np.uint32).astype(np.int64) for t in cols], 1)
        assert np.array_equal(got, want)

    sweep(monkeypatch, "route/interleaved", [sp], [route, split])


# -------------------------------------------------------------------- BED
@functools.lru_cache(maxsize=None)
def _bed_case(name):
    path = os.path.join(GOLDEN, name)
    with open(path, "rb") as f:
        text = f.read()
    chrom, s, e, nm = read_bed_py(path)
    ext = {}
    for cname, x in zip(chrom, e):
        ext[cname] = max(ext.get(cname, 0), int(x))
    sp = Space(list(ext), list(ext.values()))
    c = np.array([sp.index[x] for x in chrom], np.int32)
    order = device_order_plain(c, s, e)
    bed = "".join(f"{sp.names[a]}\t{b}\t{x}\n"
                  for a, b, x in zip(c[order], s[order], e[order])).encode()
    return text, chrom, s, e, nm, sp, bed


@pytest.mark.parametrize("name", ["cpg.bed", "intersect_with_overlap_00.bed"])
def test_sweep_bed_parse_and_format(monkeypatch, name):
    text, chrom, s, e, nm, sp, bed = _bed_case(name)

    def read(ctx, st):
        h, names = st["d"].to_host(), st["d"].names
        assert [names[k] for k in h["contig"]] == chrom
        assert (h["start"] == s).all() and (h["end"] == e).all() and h["name"] == nm

    def remap(ctx, st):
        d = st["d"]
        ids = np.array([sp.index[x] for x in d.names], np.int32)
        _ffi.check(_ffi.load().lime_dbed_remap_contigs(
            d._h, ids.ctypes.data_as(C.POINTER(C.c_int32)), len(ids)))

    def to_set(ctx, st):
        c, ds, de, _ = st["d"].device_arrays()
        return ctx.set_from_device(sp, st["d"].n, c, ds, de)

    def fmt(ctx, st):
        assert st["a"].to_bed() == bed

    sweep(monkeypatch, f"bed/{name}", [sp],
          [_put("d", lambda ctx, st: ctx.parse_bed(text)), read, remap, _put("a", to_set), fmt])


# ------------------------------------- existing failures leave nothing behind
@pytest.fixture(scope="module")
def own():
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("bad,code", [("contig", "LIME_ERR_CONTIG"), ("order", "LIME_ERR_RANGE"),
                                      ("beyond", "LIME_ERR_RANGE")])
def test_sort_validation_errors_leave_nothing(own, bad, code):
    sp = _space(2, 20000)
    own.set_from_host(sp, Z32, Z64, Z64).close()  # (the space's cached offsets)
    rng = np.random.default_rng(607)
    (c, s, e), _ = random_sets(rng, 3000, 1, n_contigs=2, contig_len=20000, max_len=300)
    c, s, e = c.copy(), s.copy(), e.copy()
    if bad == "contig":
        c[1234] = 2  # outside the space
    elif bad == "order":
        s[1234], e[1234] = 500, 400  # end < start
    else:
        e[1234] = 20001  # end beyond the contig
    dev = _dev(c, s, e)
    before = _live(own)
    with pytest.raises(LimeError) as ei:
        own.set_from_device(sp, 3000, *(t.data_ptr() for t in dev))
    assert code in str(ei.value)
    assert _live(own) == before


def test_subtract_skew_failure_leaves_nothing(own, monkeypatch):
    sp, A, B, t, exp = _subtract_case("fused")
    a, b = own.set_from_host(sp, *A), own.set_from_host(sp, *B)
    before = _live(own)
    monkeypatch.setenv("LIME_TEST_SUB_SKEW", "1")
    with pytest.raises(LimeError, match="record total changed"):
        own.subtract(a, b, 0, SUBTRACT_LIME)
    monkeypatch.delenv("LIME_TEST_SUB_SKEW")
    assert _live(own) == before
    r = own.subtract(a, b, 0, SUBTRACT_LIME)
    assert r.checksum()[:2] == oracle.result_checksum(exp)
    for h in (r, b, a):
        h.close()


@pytest.mark.parametrize("text,code", [
    (b"chr1\t1\t2\nchr1\tx\t5\n", "LIME_ERR_IO"),
    (b"chr1\t1\n", "LIME_ERR_IO"),
    (b"chr1\t1\t2\nchr1\t3\t4\nchr1\t0\t4294967296\n", "LIME_ERR_RANGE"),
    (b"chr1\t-5\t2\n", "LIME_ERR_RANGE"),
])
def test_bed_parse_errors_leave_nothing(own, text, code):
    before = _live(own)
    with pytest.raises(LimeError) as ei:
        own.parse_bed(text)
    assert code in str(ei.value)
    assert _live(own) == before
