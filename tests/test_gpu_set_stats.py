"""The per-set statistics (min width, max width, any zero width) and the
"already in canonical order" check that k_prep gathers per tile and k_stats
reduces (lime_amd/csrc/sort.hip), through every set builder, with the one
row that decides the answer planted on the seams of the reduction: k_prep's
tile is 8192 rows, a wave's chunk 1024, a full chunk is read in four
iterations of 256 rows (4 consecutive rows per lane), a short last chunk row
by row.

max_width bounds every partner window of the intersect plan, min_width picks
the filtered count and fill, the zero-width flag the skip of zero-width
partners, and `unsorted` whether the set is sorted at all: one lost row is a
silently wrong answer downstream.  Truth is plain numpy on the input rows;
every comparison is exact."""
import numpy as np
import pytest

from lime_amd import Space
from oracle import oracle
from tests import plan_cases as pc
from tests import scan_cases as sc
from tests.test_gpu_fill_edges import check_plan
from tests.test_gpu_sort import _expected

pytestmark = pytest.mark.gpu

TILE, CHUNK = 8192, 1024
N = 2 * TILE + CHUNK + 7  # two full tiles, one full wave chunk, a 7-row tail
POSITIONS = [0, 3, 4, 255, 256, 1023, 1024, TILE - 1, TILE, 2 * TILE + 1023, 2 * TILE + 1024, N - 1]
KINDS = {"widest": 70_000, "narrowest": 1, "zero": 0}
LENS3 = [400_000, 300_000, 200_000]


def _space(lens):
    return Space([f"c{i:04d}" for i in range(len(lens))], lens)


def _base(seed, n, lens):
    """n random rows over the contigs, every width in [10, 500]"""
    rng = np.random.default_rng(seed)
    ln = np.asarray(lens, np.int64)
    c = rng.integers(0, len(lens), n).astype(np.int32)
    w = rng.integers(10, 501, n)
    s = (rng.random(n) * (ln[c] - 500)).astype(np.int64)
    return c, s, s + w


def _plant(base, kind, pos, lens):
    """the base rows with row `pos` made the set's only row of the kind"""
    c, s, e = (x.copy() for x in base)
    w = KINDS[kind]
    s[pos] = min(int(s[pos]), lens[c[pos]] - w)
    e[pos] = s[pos] + w
    return c, s, e


def _truth(X, kind):
    lo, hi, z = pc.set_stats(X)
    w = X[2] - X[1]
    # the planted row alone decides its statistic
    if len(w) > 1:
        assert {"widest": np.sum(w == hi) == 1 and hi == 70_000,
                "narrowest": np.sum(w == lo) == 1 and lo == 1,
                "zero": np.sum(w == 0) == 1 and z}[kind]
    return lo, hi, z


def _check_rows(S, X, order, rows=None):
    """S holds the input rows in the given order"""
    h = S.to_host()
    want = order if rows is None else rows[order]
    assert np.array_equal(h["row"], want)
    for k, x in zip(("contig", "start", "end"), X):
        assert np.array_equal(h[k], np.asarray(x)[order]), k


def _device(X, dtype=np.int32):
    import torch
    t = [torch.tensor(np.ascontiguousarray(x).astype(dtype).view(np.int32), device="cuda")
         for x in X]
    torch.cuda.synchronize()  # (the engine reads on its own stream)
    return t


def _global(X, lens):
    off = pc.offsets(lens)
    return off[X[0]] + X[1], off[X[0]] + X[2]


# builders: (ctx, space, lens, X, strand) -> (set, expected order, row ids or None)
def _b_host(ctx, sp, lens, X, strand):
    return ctx.set_from_host(sp, *X), _expected(*_global(X, lens)), None


def _b_host_stranded(ctx, sp, lens, X, strand):
    return (ctx.set_from_host_stranded(sp, *X, strand),
            sc.device_order_stranded(*X, strand), None)


def _b_device(ctx, sp, lens, X, strand):
    t = _device(X)
    S = ctx.set_from_device(sp, len(X[1]), *(x.data_ptr() for x in t))
    ctx.synchronize()  # (the rows are consumed before the tensors go)
    return S, _expected(*_global(X, lens)), None


def _b_device_stranded(ctx, sp, lens, X, strand):
    import torch
    t = _device(X)
    st = torch.tensor(strand, device="cuda")
    torch.cuda.synchronize()
    S = ctx.set_from_device_stranded(sp, len(X[1]), *(x.data_ptr() for x in t), st.data_ptr())
    ctx.synchronize()
    return S, sc.device_order_stranded(*X, strand), None


def _b_device_no_codes(ctx, sp, lens, X, strand):
    t = _device(X)
    S = ctx.set_from_device_stranded(sp, len(X[1]), *(x.data_ptr() for x in t), None)
    ctx.synchronize()
    return S, sc.device_order_stranded(*X, np.zeros(len(X[1]), np.int8)), None


def _row_ids(n):
    return (3 * np.arange(n, dtype=np.int64) + 7)


def _b_global(ctx, sp, lens, X, strand):
    gs, ge = _global(X, lens)
    rows = _row_ids(len(gs))
    t = _device((gs, ge, rows), np.uint32)
    S = ctx.set_from_global(sp, len(gs), *(x.data_ptr() for x in t))
    ctx.synchronize()
    return S, _expected(gs, ge), rows


def _b_global_stranded(ctx, sp, lens, X, strand):
    import torch
    gs, ge = _global(X, lens)
    rows = _row_ids(len(gs))
    t = _device((gs, ge, rows), np.uint32)
    st = torch.tensor(strand, device="cuda")
    torch.cuda.synchronize()
    S = ctx.set_from_global_stranded(sp, len(gs), *(x.data_ptr() for x in t), st.data_ptr())
    ctx.synchronize()
    return S, sc.device_order_stranded(*X, strand), rows


def _b_bed(ctx, sp, lens, X, strand):
    names = sp.names
    text = "".join(f"{names[c]}\t{s}\t{e}\n" for c, s, e in zip(*(x.tolist() for x in X)))
    bed = ctx.parse_bed(text.encode())
    assert bed.n == len(X[1])
    S = bed.to_set(sp)
    ctx.synchronize()
    bed.close()
    return S, _expected(*_global(X, lens)), None


BUILDERS = {"host": _b_host, "host_stranded": _b_host_stranded, "device": _b_device,
            "device_stranded": _b_device_stranded, "device_stranded_no_codes": _b_device_no_codes,
            "global": _b_global, "global_stranded": _b_global_stranded, "bed": _b_bed}


def _sweep(ctx, build, lens, seed, n=N, positions=POSITIONS):
    sp = _space(lens)
    base = _base(seed, n, lens)
    strand = np.random.default_rng(seed + 1).integers(0, 4, n).astype(np.int8)
    for kind in KINDS:
        for pos in positions:
            X = _plant(base, kind, pos, lens)
            S, order, rows = build(ctx, sp, lens, X, strand)
            assert S.n == n
            assert S.stats() == _truth(X, kind), (kind, pos)
            _check_rows(S, X, order, rows)
            S.close()


# ------------------------------------------- a. statistics at reduction seams
@pytest.mark.parametrize("builder", sorted(BUILDERS))
def test_stats_at_seams(ctx, builder):
    _sweep(ctx, BUILDERS[builder], LENS3, 500 + sorted(BUILDERS).index(builder))


@pytest.mark.parametrize("builder", ["host", "device"])
def test_stats_at_seams_many_contigs(ctx, builder):
    # 1500 contigs: more than PCMAX (1024), the contig table stays in global
    # memory (k_prep's LC = false branch)
    _sweep(ctx, BUILDERS[builder], [80_000] * 1500, 520)


@pytest.mark.parametrize("builder", ["host", "device", "global"])
def test_stats_small_sets(ctx, builder):
    sp = _space(LENS3)
    z = np.zeros(0, np.int64)
    S, _, _ = BUILDERS[builder](ctx, sp, LENS3, (np.zeros(0, np.int32), z, z), None)
    assert S.n == 0 and S.stats() == (0, 0, False) and len(S.to_host()["row"]) == 0
    for n in (1, 63, 64, 65):
        _sweep(ctx, BUILDERS[builder], LENS3, 530 + n, n=n, positions=sorted({0, n - 1}))


# --------------------------------------------------------- b. the large preps
# 2.2e6 rows over one 200 000-base contig: 32 or more rows per 4-base bucket,
# so the set is a candidate for the bucketed sort and its prep is the one
# that writes (gs, u16 width) for caller rows (set_from_host / set_from_device)
# or only validates (set_from_global)
BIG_N = 2_200_000
BIG_LEN = [200_000]
BIG_POSITIONS = [0, 134 * TILE, BIG_N - 1]


@pytest.fixture(scope="module")
def big_base():
    base = _base(540, BIG_N, BIG_LEN)
    for x in base:
        x.flags.writeable = False
    return base


@pytest.mark.parametrize("builder", ["host", "device", "global"])
def test_stats_large_preps(ctx, big_base, builder):
    sp = _space(BIG_LEN)
    for kind in KINDS:
        for pos in BIG_POSITIONS:
            X = _plant(big_base, kind, pos, BIG_LEN)
            S, _, _ = BUILDERS[builder](ctx, sp, BIG_LEN, X, None)
            assert S.n == BIG_N
            assert S.stats() == _truth(X, kind), (kind, pos)
            S.close()


# ------------------------------------- c. set_extend_sorted / set_concat_sorted
def _halo(gs, ge, rows):
    t = _device((gs, ge, rows), np.uint32)
    return t, (len(gs),) + tuple(x.data_ptr() for x in t)


def test_extend_and_concat_stats(ctx):
    lens = [400_000]
    sp = _space(lens)
    n = 3000
    rng = np.random.default_rng(550)
    s = np.sort(rng.integers(100_000, 200_000, n))
    X = (np.zeros(n, np.int32), s, s + rng.integers(10, 501, n))
    own = pc.set_stats(X)
    S = ctx.set_from_host(sp, *X)
    assert S.stats() == own and own[0] >= 10 and own[1] <= 500 and not own[2]
    # three rows past S's last, one of them 90 000 wide; two rows before its first
    after = (np.array([200_000, 200_010, 200_020]), np.array([200_003, 290_010, 200_025]))
    before = (np.array([50, 60]), np.array([57, 60]))
    ta, ha = _halo(*after, np.arange(n, n + 3))
    tb, hb = _halo(*before, np.arange(n + 3, n + 5))
    E = ctx.set_extend_sorted(S, *ha, 3, 90_000, False)
    assert E.n == n + 3 and E.stats() == (3, 90_000, False)
    # the caller's bounds are taken as given: looser ones, and the zero flag
    assert ctx.set_extend_sorted(S, *ha, 2, 95_000, True).stats() == (2, 95_000, True)
    assert ctx.set_extend_sorted(S, *ha, 40, 300, False).stats() == (own[0], own[1], False)
    # nothing added: the set's own statistics whatever the bounds say
    assert ctx.set_extend_sorted(S, 0, None, None, None, 0, 99_999, True).stats() == own
    C = ctx.set_concat_sorted(hb, S, ha, 0, 90_000, True)
    assert C.n == n + 5 and C.stats() == (0, 90_000, True)
    h = C.to_host()
    assert np.array_equal(h["row"],
                          np.concatenate([[n + 3, n + 4], np.arange(n), [n, n + 1, n + 2]]))
    assert np.array_equal(h["start"], np.concatenate([before[0], X[1], after[0]]))
    assert np.array_equal(h["end"], np.concatenate([before[1], X[2], after[1]]))
    # an empty set takes the bounds alone
    Z = ctx.set_from_host(sp, np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert ctx.set_extend_sorted(Z, *ha, 3, 90_000, False).stats() == (3, 90_000, False)
    ctx.synchronize()
    del ta, tb


@pytest.mark.parametrize("flip", [0, 1])
def test_extended_set_finds_wide_halo_pairs(ctx, flip):
    # the halo row [200 010, 290 010) is the extended set's widest by far: its
    # pairs with rows starting up to 90 000 bases into it are found only
    # through the max width the caller declared
    lens = [400_000]
    sp = _space(lens)
    n = 3000
    rng = np.random.default_rng(551)
    s = np.sort(rng.integers(100_000, 200_000, n))
    X = (np.zeros(n, np.int32), s, s + rng.integers(10, 501, n))
    after = (np.array([200_000, 200_010, 200_020]), np.array([200_003, 290_010, 200_025]))
    t, ha = _halo(*after, np.arange(n, n + 3))
    E = ctx.set_extend_sorted(ctx.set_from_host(sp, *X), *ha, 3, 90_000, False)
    ys = rng.integers(150_000, 300_000, 2500)
    Y = (np.zeros(2500, np.int32), ys, ys + rng.integers(0, 300, 2500))
    full = (np.zeros(n + 3, np.int32), np.concatenate([X[1], after[0]]),
            np.concatenate([X[2], after[1]]))
    Ys = ctx.set_from_host(sp, *Y)
    A, B = (Y, full) if flip else (full, Y)
    exp = oracle.intersect(A, B)
    wide = exp["a_row" if not flip else "b_row"] == n + 1
    assert wide.sum() > 1000
    plan = ctx.intersect(Ys, E) if flip else ctx.intersect(E, Ys)
    check_plan(ctx, sp, A, B, plan=plan, exp=exp)
    ctx.synchronize()
    del t


# ---------------------------------------------------------- d. the order check
ORDER_POSITIONS = [1, 4, 256, 1024, TILE, TILE + 1024, 2 * TILE + 1024, N - 1]
ORDER_KINDS = ["inversion", "tie", "legal_zero_first", "legal_equal", "legal_contig"]


def _order_case(kind, i, n=N):
    """rows in canonical order (starts 10 apart, 3 wide) except the pair
    (i - 1, i): -> (lens, (contig, start, end), must the set reorder)"""
    s = 10 * np.arange(n, dtype=np.int64) + 5
    e = s + 3
    c = np.zeros(n, np.int32)
    lens = [10 * n + 100] * 2
    if kind == "inversion":  # row i - 1 starts past row i
        s[i - 1] = s[i] + 1
        e[i - 1] = s[i - 1] + 3
    elif kind == "tie":  # a non-zero-width row directly before a zero-width one, one start
        s[i] = e[i] = s[i - 1]
    elif kind == "legal_zero_first":
        s[i] = e[i - 1] = s[i - 1]
        e[i] = s[i] + 3
    elif kind == "legal_equal":
        s[i], e[i] = s[i - 1], e[i - 1]
    elif kind == "legal_contig":  # contig 0 ends high, contig 1 starts at local 0
        c[i:] = 1
        s[i:] -= s[i]
        e[i:] = s[i:] + 3
    return lens, (c, s, e), not kind.startswith("legal")


def _check_order(ctx, builder, lens, X, reorder):
    sp = _space(lens)
    S, order, rows = BUILDERS[builder](ctx, sp, lens, X, None)
    n = len(X[1])
    assert np.array_equal(order, np.arange(n)) != reorder  # the case is what its name says
    _check_rows(S, X, order, rows)
    got = ctx.merge(S).to_host()
    exp = oracle.merge(X)
    for k in ("contig", "start", "end"):
        assert np.array_equal(got[k], exp[k]), k
    S.close()


@pytest.mark.parametrize("kind", ORDER_KINDS)
@pytest.mark.parametrize("builder", ["host", "device", "global"])
def test_order_check_at_seams(ctx, builder, kind):
    for i in ORDER_POSITIONS:
        lens, X, reorder = _order_case(kind, i)
        _check_order(ctx, builder, lens, X, reorder)


@pytest.mark.parametrize("builder", ["host", "global"])
def test_order_check_large_preps(ctx, builder):
    # the u16-width prep (host rows) and the validate-only prep (global
    # rows) of b: 2.2e6 rows in order but for one inversion at a 256-row seam
    rng = np.random.default_rng(560)
    s = np.sort(rng.integers(0, BIG_LEN[0] - 600, BIG_N))
    i = 100 * TILE + 256
    s[i - 1] = s[i] + 1
    X = (np.zeros(BIG_N, np.int32), s, s + rng.integers(1, 501, BIG_N))
    _check_order(ctx, builder, BIG_LEN, X, True)
