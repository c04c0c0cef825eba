"""Edges of the intersect fill (k_fill): owner-tile counts, empty owner
tiles, one owner wider than the LDS partner window, workgroup shares that end
on tile boundaries, and output windows of odd sizes.  Every case compares the
stored records exactly with the CPU oracle (as sorted rows, like
test_gpu_parity.py) and the device checksum with the hash of the stored
records.

The built plans put B on a grid: B_j = [4 j, 4 j + 1) and A_i = [4 i + 2,
4 i + 2 + 4 K) holds exactly the K grid starts 4 (i + 1) .. 4 (i + K), none of
them tied with its own.  Taken as (A, B) every pair belongs to an A owner
(the first stream's owner tiles; every B-owner tile is empty); taken as
(B, A) every pair belongs to a stream-1 owner.  An owner tile is 1024 owners,
a workgroup's share at these sizes 4096 records, the LDS partner window 2048
rows; plans of 16 or more pairs per owner row take the one-tile fill."""
import numpy as np
import pytest

from lime_amd import PAIR_DTYPE, Space
from oracle import oracle
from tests.util import random_sets

pytestmark = pytest.mark.gpu

TILE = 1024


def space1(length):
    return Space(["c0"], [int(length)])


def sorted_rows(res, contig):
    cols = [np.asarray(contig, dtype=np.int64)] + [
        np.asarray(res[k]).astype(np.int64) for k in ("start", "end", "a_row", "b_row")]
    arr = np.stack(cols, axis=1)
    return arr[np.lexsort(arr.T[::-1])]


def check_plan(ctx, sp, A, B, plan=None, exp=None):
    """whole fill == oracle (sorted rows); device checksum == hash of the
    stored records.  Returns (plan, whole)."""
    if plan is None:
        plan = ctx.intersect(ctx.set_from_host(sp, *A), ctx.set_from_host(sp, *B))
    if exp is None:
        exp = oracle.intersect(A, B)
    assert plan.n == len(exp["start"])
    whole = plan.fill_host()
    got = sorted_rows(whole, np.asarray(A[0])[whole["a_row"]] if plan.n else [])
    want = sorted_rows(exp, exp["contig"])
    assert np.array_equal(got, want)
    assert plan.checksum() == oracle.checksum_pairs(whole)
    return plan, whole


def grid_plan(a_starts, a_lens, b_starts):
    """(A, B, length): A rows [s, s + len), B rows [s, s + 1), one contig."""
    a_s = np.asarray(a_starts, dtype=np.int64)
    a_e = a_s + np.asarray(a_lens, dtype=np.int64)
    b_s = np.asarray(b_starts, dtype=np.int64)
    A = (np.zeros(len(a_s), np.int32), a_s, a_e)
    B = (np.zeros(len(b_s), np.int32), b_s, b_s + 1)
    top = max([int(a_e.max()) if len(a_e) else 0, int(b_s.max()) + 1 if len(b_s) else 0])
    return A, B, top + 8


def oriented(A, B, flip):
    return (B, A) if flip else (A, B)


def dense_block(n, k, base):
    """n owners with exactly k partners each, from grid coordinate `base`
    (a multiple of 4): (a_starts, a_lens, b_starts)."""
    i = np.arange(n, dtype=np.int64)
    j = np.arange(n + k + 1, dtype=np.int64)
    return base + 4 * i + 2, np.full(n, 4 * k, np.int64), base + 4 * j


# ---------------------------------------------------------------- owner counts
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("k", [3, 80])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_owner_counts(ctx, n, k, flip):
    # n owners of one stream with exactly k pairs each (k = 3: the two-tile
    # sparse fill; k = 80: one-tile commits)
    a_s, a_l, b_s = dense_block(n, k, 0)
    A, B, top = grid_plan(a_s, a_l, b_s)
    A, B = oriented(A, B, flip)
    plan, _ = check_plan(ctx, space1(top), A, B)
    assert plan.n == n * k


@pytest.mark.parametrize("k_len", [(3, 12), (80, 320)])
@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049])
def test_owner_counts_both_streams(ctx, n, k_len):
    # random rows: both streams own pairs, about k per owner row
    k, mean_len = k_len
    rng = np.random.default_rng(1000 * n + k)
    length = n * mean_len // k  # 2 k pairs per A row = k per owner row
    A, B = random_sets(rng, n, n, n_contigs=1, contig_len=length, max_len=2 * mean_len,
                       dup_frac=0.05, book_frac=0.05)
    check_plan(ctx, space1(length), A, B)


@pytest.mark.parametrize("flip", [0, 1])
def test_one_set_empty(ctx, flip):
    a_s, a_l, b_s = dense_block(TILE, 80, 0)
    A, B, top = grid_plan(a_s, a_l, [])
    A, B = oriented(A, B, flip)
    plan, whole = check_plan(ctx, space1(top), A, B)
    assert plan.n == 0 and len(whole) == 0 and plan.checksum() == (0, 0)


# ----------------------------------------------------------------- empty tiles
@pytest.mark.parametrize("flip", [0, 1])
def test_empty_tiles(ctx, flip):
    # owner tiles: empty, dense, empty x 3, dense, dense, empty; a region
    # holds exactly one tile of owners, an empty one no grid row at all
    k, span = 100, 4 * 2048
    a_s, a_l, b_s = [], [], []
    for r, dense in enumerate([0, 1, 0, 0, 0, 1, 1, 0]):
        if dense:
            s, l, b = dense_block(TILE, k, r * span)
            b = b[b < (r + 1) * span]
        else:
            s = r * span + 4 * np.arange(TILE, dtype=np.int64) + 2
            l, b = np.ones(TILE, np.int64), np.zeros(0, np.int64)
        a_s.append(s), a_l.append(l), b_s.append(b)
    A, B, top = grid_plan(np.concatenate(a_s), np.concatenate(a_l), np.concatenate(b_s))
    A, B = oriented(A, B, flip)
    plan, whole = check_plan(ctx, space1(top), A, B)
    assert plan.n == 3 * TILE * k
    # windows that run from a dense tile over the empty ones into the next
    # dense tile, and one that starts on the tile boundary itself
    edge = TILE * k
    for first, count in [(edge - 5000, 10000), (edge, 4097), (edge - 1, 2), (0, edge + 1),
                         (2 * edge - 70, 3 * 4096 + 11)]:
        part = plan.fill_host(first, count)
        assert np.array_equal(part, whole[first:first + count])


# -------------------------------------------------------------- one huge owner
@pytest.mark.parametrize("flip", [0, 1])
def test_one_huge_owner(ctx, flip):
    # 1500 ordinary owners, ONE owner with 30000 partners (15 LDS windows, 8
    # workgroup shares), 1500 ordinary owners: the middle tile's window is
    # past the LDS image (global-partner path), the tiles around it are not
    # (k = 200 keeps the plan at 16 or more pairs per owner row, grid rows
    # under the huge owner included: the one-tile fill)
    k, big = 200, 30000
    s0, l0, b0 = dense_block(1500, k, 0)
    base1 = 4 * 2048
    s1, l1 = np.array([base1 + 2], np.int64), np.array([4 * big], np.int64)
    b1 = base1 + 4 * np.arange(1, big + 1, dtype=np.int64)
    base2 = base1 + 4 * (big + 64)
    s2, l2, b2 = dense_block(1500, k, base2)
    A, B, top = grid_plan(np.concatenate([s0, s1, s2]), np.concatenate([l0, l1, l2]),
                          np.concatenate([b0, b1, b2]))
    A, B = oriented(A, B, flip)
    plan, whole = check_plan(ctx, space1(top), A, B)
    assert plan.n == 3000 * k + big
    # windows cut inside the huge owner's records
    h0 = 1500 * k
    for first, count in [(h0 - 3, 7), (h0 + 4095, 4098), (h0 + big - 65, 130),
                         (h0 + 1000, big - 2000)]:
        part = plan.fill_host(first, count)
        assert np.array_equal(part, whole[first:first + count])


# ---------------------------------------------------------- boundary alignment
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("k", [127, 128, 129])
def test_share_and_tile_boundaries(ctx, k, flip):
    # k = 128: a tile is 131072 records = 32 shares of 4096, so every
    # workgroup share of the whole fill ends on a tile boundary or inside
    # one tile; 127 / 129: the same plan with the boundaries off by 1024
    n = 4 * TILE
    a_s, a_l, b_s = dense_block(n, k, 0)
    A, B, top = grid_plan(a_s, a_l, b_s)
    A, B = oriented(A, B, flip)
    plan, whole = check_plan(ctx, space1(top), A, B)
    assert plan.n == n * k
    tile = TILE * k
    for first, count in [(tile, 2 * tile), (tile - 4096, 8192), (2 * tile, 4096),
                         (3 * tile - 64, 64), (3 * tile, tile)]:
        part = plan.fill_host(first, count)
        assert np.array_equal(part, whole[first:first + count])


# --------------------------------------------------------------- chunk windows
@pytest.fixture(scope="module")
def two_stream_plan(ctx):
    """~30 pairs per owner row, both streams: (plan, whole fill, records of
    the first stream), checked against the oracle once."""
    rng = np.random.default_rng(77)
    n, length = 3000, 8000
    A, B = random_sets(rng, n, n, n_contigs=1, contig_len=length, max_len=160, dup_frac=0.05,
                       book_frac=0.05)
    plan, whole = check_plan(ctx, space1(length), A, B)
    # the first stream's records: b starts inside a (ties to a)
    n0 = int(np.sum(B[1][whole["b_row"]] >= A[1][whole["a_row"]]))
    assert 0 < n0 < plan.n
    first_stream = B[1][whole["b_row"]] >= A[1][whole["a_row"]]
    assert first_stream[:n0].all() and not first_stream[n0:].any()
    return plan, whole, n0


@pytest.mark.parametrize("count", [1, 63, 64, 65])
def test_small_windows(ctx, two_stream_plan, count):
    import torch
    plan, whole, n0 = two_stream_plan
    buf = torch.zeros((count + 2, 4), dtype=torch.int32, device="cuda")
    # mid-tile, mid-share, across a share end (4096), across the streams, the
    # plan's last records
    for first in [0, 1000, 4096 - 32, 40 * TILE + 17, n0 - count // 2 - 1, n0 - count, n0,
                  plan.n - count]:
        buf.fill_(-1)
        torch.cuda.synchronize()  # (the engine fills on its own stream)
        plan.fill_device(first, count, buf[1:].data_ptr())
        ctx.synchronize()
        got = buf.cpu().numpy().view(np.uint32)
        assert (got[0] == 0xffffffff).all() and (got[-1] == 0xffffffff).all()
        part = np.ascontiguousarray(got[1:-1]).reshape(-1).view(PAIR_DTYPE)
        assert np.array_equal(part, whole[first:first + count])


def test_window_across_streams(ctx, two_stream_plan):
    plan, whole, n0 = two_stream_plan
    for first, count in [(n0 - 5000, 10000), (n0 - 1, 2), (n0 - 4096, 4096 + 1), (0, n0 + 1)]:
        part = plan.fill_host(first, count)
        assert np.array_equal(part, whole[first:first + count])


def test_odd_windows_make_the_whole(ctx, two_stream_plan):
    plan, whole, _ = two_stream_plan
    sizes = [1, 63, 64, 65, 777, 4095, 4097, 10007, 65, 30011, 1, 8191]
    parts, f, i = [], 0, 0
    while f < plan.n:
        k = min(sizes[i % len(sizes)], plan.n - f)
        parts.append(plan.fill_host(f, k))
        f, i = f + k, i + 1
    assert np.array_equal(np.concatenate(parts), whole)


# ---------------------------------------------------------------- window plans
@pytest.mark.parametrize("d", [1, 150])
def test_window_plan(ctx, d):
    # DistributedWindow (the WIN fill) over the two-stream shape
    rng = np.random.default_rng(78)
    n, length = 3000, 8000
    A, B = random_sets(rng, n, n, n_contigs=1, contig_len=length, max_len=160, dup_frac=0.05,
                       book_frac=0.05)
    sp = space1(length)
    plan = ctx.window(ctx.set_from_host(sp, *A), ctx.set_from_host(sp, *B), d)
    _, whole = check_plan(ctx, sp, A, B, plan=plan, exp=oracle.window(A, B, d))
    for first, count in [(1000, 65), (4096 - 32, 64), (plan.n // 2 - 5000, 10001)]:
        part = plan.fill_host(first, count)
        assert np.array_equal(part, whole[first:first + count])
