"""The packed owner words between k_count and k_fill, at the edges of what a
tile may pack.  A 1024-owner tile hands the fill its owners' (lo, off, gs, ge)
in two words per owner when its partner window is at most 2048 rows, its pair
total below 2^20, and every owner starts within 65535 of the tile's first
owner and is at most 65535 wide; any other tile, and every tile of a window
plan, keeps the plain (lo, off) words.  Every case stands on one side of one
of those limits, compares the whole fill with the CPU oracle (as
test_gpu_fill_edges.py does), then fills again in chunks that start mid-tile.
Each shape runs as (A, B) and as (B, A), so both streams own it once.

`tile_forms` is the packing rule written out in numpy: every case asserts
with it that its tiles have the forms the case is about.

The shapes are those of test_gpu_fill_edges.py: partners [s, s + 1) on a grid
of 4, owners that start at 2 mod 4 and hold the k grid starts after them."""
import numpy as np
import pytest

from lime_amd import Space
from oracle import oracle
from tests.test_gpu_fill_edges import check_plan, dense_block, oriented, space1
from tests.util import random_sets

pytestmark = pytest.mark.gpu

TILE = 1024
PK_WIN, PK_TOTAL, PK_SPAN = 2048, 1 << 20, 1 << 16
WLANE_MAX = 65536  # owner sets at most this wide take their windows from first / last starts


def tile_forms(O, P, lo_off):
    """1 (packed) / 0 per owner tile of sorted one-contig owners O = (s, e)
    against partners P = (s, e), for threshold 0."""
    os_, oe = (np.asarray(x, np.int64) for x in O)
    order = np.lexsort((oe, os_))
    os_, oe = os_[order], oe[order]
    ps, pe = (np.asarray(x, np.int64) for x in P)
    porder = np.lexsort((pe, ps))
    ps, pe = ps[porder], pe[porder]
    owmax = int((oe - os_).max())
    forms = []
    for t in range(0, len(os_), TILE):
        s, e = os_[t:t + TILE], oe[t:t + TILE]
        hkey = s[-1] + owmax if owmax <= WLANE_MAX else e.max()
        hkey = max(hkey, s[-1] + lo_off)
        wlo, whi = np.searchsorted(ps, s[0] + lo_off), np.searchsorted(ps, hkey)
        lo = np.searchsorted(ps, s + lo_off)
        hi = np.maximum(np.searchsorted(ps, e), lo)
        if lo_off == 0:  # zero-width partners at exactly the owner's start are skipped
            for i in np.nonzero(lo < len(ps))[0]:
                while lo[i] < whi and ps[lo[i]] == s[i] and pe[lo[i]] == s[i]:
                    lo[i] += 1
            hi = np.maximum(hi, lo)
        forms.append(int(whi - wlo <= PK_WIN and (hi - lo).sum() < PK_TOTAL and
                         (s - s[0]).max() < PK_SPAN and (e - s).max() < PK_SPAN))
    return forms


def rows(a_s, a_e, b_s, b_e=None):
    """(A, B, length) on one contig; B rows one wide unless b_e is given"""
    a_s, a_e, b_s = (np.asarray(x, np.int64) for x in (a_s, a_e, b_s))
    b_e = b_s + 1 if b_e is None else np.asarray(b_e, np.int64)
    A = (np.zeros(len(a_s), np.int32), a_s, a_e)
    B = (np.zeros(len(b_s), np.int32), b_s, b_e)
    return A, B, int(max(a_e.max(), b_e.max())) + 8


def run(ctx, A, B, top, flip, forms=None, sparse=None):
    """whole fill == oracle, chunks that start mid-tile == the whole fill;
    forms: the owner tiles' expected forms (A's, which own every pair)"""
    if forms is not None:
        assert tile_forms(A[1:], B[1:], flip) == forms
    X, Y = oriented(A, B, flip)
    plan, whole = check_plan(ctx, space1(top), X, Y)
    if sparse is not None:  # fewer than 16 pairs per owner row: two-tile commits
        assert (plan.n < 16 * (len(A[0]) + len(B[0]))) == sparse
    n = plan.n
    cuts = sorted({0, min(n, 1), n // 7 + 1, n // 3 + 65, n // 2 + 3, n - n // 5, n})
    cuts = [c for c in cuts if c <= n]
    parts = [plan.fill_host(f, l - f) for f, l in zip(cuts[:-1], cuts[1:]) if l > f]
    if parts:
        assert np.array_equal(np.concatenate(parts), whole)
    return plan


def block(n, k, base, last_at=None, wide=None):
    """n owners with k partners each from grid coordinate base; last_at: the
    last owner starts there instead (its own k partners after it); wide =
    (i, width): owner i is that wide.  -> (a_s, a_e, b_s)"""
    a_s, a_l, b_s = dense_block(n, k, base)
    a_e = a_s + a_l
    if last_at is not None:
        a_s[-1] = last_at
        a_e[-1] = last_at + 4 * k
        far = (last_at + 3) // 4 * 4 + 4 * np.arange(k + 1, dtype=np.int64)
        b_s = np.concatenate([b_s[b_s < a_s[-2] + 4 * k + 4], far])
    if wide is not None:
        a_e[wide[0]] = a_s[wide[0]] + wide[1]
    return a_s, a_e, b_s


# ------------------------------------------------------------------ owner span
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("k", [3, 40])
@pytest.mark.parametrize("span", [65535, 65536])
def test_owner_span(ctx, span, k, flip):
    # the tile's last owner starts at g0 + 65535 (packed) / g0 + 65536 (plain)
    a_s, a_e, b_s = block(TILE, k, 0, last_at=2 + span)
    A, B, top = rows(a_s, a_e, b_s)
    plan = run(ctx, A, B, top, flip, forms=[int(span < PK_SPAN)], sparse=k == 3)
    assert plan.n == TILE * k


# ----------------------------------------------------------------- owner width
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("k", [3, 40])
@pytest.mark.parametrize("width", [65535, 65536])
def test_owner_width(ctx, width, k, flip):
    # one owner of width 65535 (packed) / 65536 (plain) among narrow ones; it
    # holds every grid row after its start
    a_s, a_e, b_s = block(TILE, k, 0, wide=(500, width))
    A, B, top = rows(a_s, a_e, b_s)
    run(ctx, A, B, top, flip, forms=[int(width < PK_SPAN)], sparse=k == 3)


# --------------------------------------------------------------- window length
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("width", [4, 256])
@pytest.mark.parametrize("wlen", [2048, 2049])
def test_window_length(ctx, wlen, width, flip):
    # owners every 8, partners every 4 up to the last owner's start: 2046 grid
    # rows, and wlen - 2046 more between them.  The last owner, one wide, starts
    # past every partner: its lo is the window's end (lo - wlo = wlen).
    # width 4: one pair per owner (two-tile commits); 256: 64 pairs (one-tile)
    i = np.arange(TILE, dtype=np.int64)
    a_s = 8 * i + 2
    a_e = a_s + width
    a_e[-1] = a_s[-1] + 1
    b_s = np.concatenate([4 * np.arange(1, 2047, dtype=np.int64),
                          40 * np.arange(1, wlen - 2046 + 1, dtype=np.int64) + 1])
    A, B, top = rows(a_s, a_e, b_s)
    assert len(b_s) == wlen and b_s.max() < a_s[-1]
    run(ctx, A, B, top, flip, forms=[int(wlen <= PK_WIN)], sparse=width == 4)


# ------------------------------------------------------------------ tile total
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("k", [1023, 1024])
def test_tile_total(ctx, k, flip):
    # 1024 owners of k partners: 2^20 - 1024 pairs (packed), 2^20 (plain)
    a_s, a_e, b_s = block(TILE, k, 0)
    A, B, top = rows(a_s, a_e, b_s)
    plan = run(ctx, A, B, top, flip, forms=[int(TILE * k < PK_TOTAL)], sparse=False)
    assert plan.n == TILE * k


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("k", [3, 40])
def test_empty_owners_at_tile_ends(ctx, k, flip):
    # the first and the last owner of a packed tile have no pair (one wide,
    # between two grid rows); a second tile follows
    a_s, a_e, b_s = block(TILE + 300, k, 0)
    a_e[0], a_e[TILE - 1], a_e[TILE] = a_s[0] + 1, a_s[TILE - 1] + 1, a_s[TILE] + 1
    A, B, top = rows(a_s, a_e, b_s)
    plan = run(ctx, A, B, top, flip, forms=[1, 1], sparse=k == 3)
    assert plan.n == (TILE + 300 - 3) * k


# ------------------------------------------------------------ mixed neighbours
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("k", [3, 40])
@pytest.mark.parametrize("forms", [[1, 0], [0, 1], [0, 1, 1, 0, 1]])
def test_mixed_neighbours(ctx, forms, k, flip):
    # packed and plain tiles side by side (a plain tile's last owner starts
    # 70000 past its first): k = 40 one tile per commit, k = 3 two tiles per
    # commit, in both orders
    a_s, a_e, b_s, base = [], [], [], 0
    for f in forms:
        s, e, b = block(TILE, k, base, last_at=None if f else base + 70002)
        a_s.append(s), a_e.append(e), b_s.append(b)
        base = (int(b.max()) // 4 + 8) * 4
    A, B, top = rows(np.concatenate(a_s), np.concatenate(a_e), np.concatenate(b_s))
    plan = run(ctx, A, B, top, flip, forms=forms, sparse=k == 3)
    assert plan.n == len(forms) * TILE * k


# --------------------------------------------------------------- partial tiles
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("k", [3, 40])
@pytest.mark.parametrize("n", [1, 1023, 1025])
def test_partial_tiles(ctx, n, k, flip):
    a_s, a_e, b_s = block(n, k, 0)
    A, B, top = rows(a_s, a_e, b_s)
    plan = run(ctx, A, B, top, flip, forms=[1] * ((n + TILE - 1) // TILE))
    assert plan.n == n * k


# ------------------------------------------------------------- contig boundary
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("k", [3, 40])
def test_contig_boundary(ctx, k, flip):
    # 700 owners on each of two short contigs: the first tile's owners span the
    # boundary (its contig offset is looked up per owner), 4 * 760 coordinates
    # apart at most, so both tiles pack
    n = 700
    a_s, a_e, b_s = block(n, k, 0)
    length = int(b_s.max()) + 8
    assert 2 * length < PK_SPAN
    A = (np.repeat([0, 1], n).astype(np.int32), np.tile(a_s, 2), np.tile(a_e, 2))
    B = (np.repeat([0, 1], len(b_s)).astype(np.int32), np.tile(b_s, 2), np.tile(b_s + 1, 2))
    X, Y = oriented(A, B, flip)
    sp = Space(["c0", "c1"], [length, length])
    plan, whole = check_plan(ctx, sp, X, Y)
    assert plan.n == 2 * n * k
    # across the contig boundary, from the first tile into the second, nearly all
    for first, count in [(n * k - 100, 200), (TILE * k - 33, (2 * n - TILE) * k), (5, plan.n - 10)]:
        assert np.array_equal(plan.fill_host(first, count), whole[first:first + count])


# --------------------------------------------------------- zero-width partners
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("k", [3, 40])
def test_zero_width_partners(ctx, k, flip):
    # zero-width partner rows at exactly an owner's start (one, two or none
    # per owner) are skipped: the packed lo is the skipped one (the same rows
    # inside an earlier owner do pair with it)
    a_s, a_e, b_s = block(TILE + 100, k, 0)
    zw = np.concatenate([a_s[::3], a_s[::6]])
    b_all = np.concatenate([b_s, zw])
    A, B, top = rows(a_s, a_e, b_all, np.concatenate([b_s + 1, zw]))
    run(ctx, A, B, top, flip, forms=[1, 1])


# ------------------------------------------------- plans that keep plain words
@pytest.mark.parametrize("d", [1, 150])
def test_window_plan_stays_plain(ctx, d):
    # a window plan's records carry the unwidened rows: never packed
    rng = np.random.default_rng(79)
    n, length = 2500, 7000
    A, B = random_sets(rng, n, n, n_contigs=1, contig_len=length, max_len=160, dup_frac=0.05,
                       book_frac=0.05)
    sp = space1(length)
    plan = ctx.window(ctx.set_from_host(sp, *A), ctx.set_from_host(sp, *B), d)
    _, whole = check_plan(ctx, sp, A, B, plan=plan, exp=oracle.window(A, B, d))
    for first, count in [(1000, 65), (plan.n // 2 - 5000, 10001)]:
        assert np.array_equal(plan.fill_host(first, count), whole[first:first + count])


@pytest.mark.parametrize("flip", [0, 1])
def test_filtered_plan_stays_plain(ctx, flip):
    # threshold 5 with partners narrower than it: the filtered count and fill
    rng = np.random.default_rng(80)
    n, length = 2500, 7000
    A, B = random_sets(rng, n, n, n_contigs=1, contig_len=length, max_len=160, dup_frac=0.05,
                       book_frac=0.05)
    A, B = oriented(A, B, flip)
    sp = space1(length)
    plan = ctx.intersect(ctx.set_from_host(sp, *A), ctx.set_from_host(sp, *B), 5)
    _, whole = check_plan(ctx, sp, A, B, plan=plan, exp=oracle.intersect(A, B, 5))
    for first, count in [(1000, 65), (plan.n // 2 - 5000, 10001)]:
        assert np.array_equal(plan.fill_host(first, count), whole[first:first + count])
