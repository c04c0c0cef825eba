"""The intersect plan at the switches between its code paths
(lime_amd/csrc/intersect.hip), on the planted inputs of tests/plan_cases.py
(checked on the CPU by tests/test_plan_cases.py):

  a. k_count searches an LDS image of the tile's partner window up to WCAP
     (4096) rows and global memory past it: windows of 4095 / 4096 / 4097;
  b. k_fill<1> stages the window in LDS up to its cap (2048): 2047 / 2048 /
     2049;
  c. k_fill<2> (plans below 16 pairs per owner row) stages the union of two
     tiles' windows up to 2496: 2495 / 2496 / 2497;
  d. k_windows_lane bounds a tile's window by the owners' max width up to
     65536, k_windows reads every owner's end past it: one owner of 65536 /
     65537 bases, and window plans whose widened owners are that wide;
  e. k_fill_filtered with output windows [first, first + count);
  f. owned prefixes (a_owned / b_owned) at tile edges, plain and filtered;
  g. the u32 tile-local offsets: one owner tile of 2^31 - 1024, 2^31 and
     2^32 - 1024 pairs fills correctly, 2^32 is refused.  (The 2^31 flag also
     keeps two such tiles out of one k_fill<2> commit; a plan sparse enough to
     take k_fill<2> with a tile that large needs more than 1.3e8 owner rows,
     which is out of this suite's reach.)

Every case runs in both orientations (the pairs owned by stream 0, then by
stream 1) and is compared exactly: plan.n with the oracle's count, the whole
fill with the oracle as sorted rows, the device checksum with the hash of the
stored records."""
import numpy as np
import pytest

from lime_amd import LimeError, PAIR_DTYPE, Space
from oracle import oracle
from tests import plan_cases as pc
from tests.test_gpu_fill_edges import check_plan, dense_block, grid_plan, oriented

pytestmark = pytest.mark.gpu


def _space(case):
    return Space(["c0"], case["lens"])


def _windows_equal(plan, whole, windows):
    for first, count in windows:
        first = max(0, min(first, plan.n - count))
        part = plan.fill_host(first, count)
        assert np.array_equal(part, whole[first:first + count]), (first, count)


def _as_records(rec):
    out = np.zeros(len(rec), PAIR_DTYPE)
    for j, k in enumerate(("start", "end", "a_row", "b_row")):
        out[k] = rec[:, j]
    return out


# ------------------------------------------------ a. count pass: LDS / global
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("k", pc.COUNT_WINDOW_K)
def test_count_window_switch(ctx, k, flip):
    case = pc.dense_case(pc.COUNT_WINDOW_N, k)
    # the shared builders make the same rows
    A, B, top = grid_plan(*dense_block(pc.COUNT_WINDOW_N, k, 0))
    assert all(np.array_equal(x, y) for x, y in zip(A + B, case["A"] + case["B"]))
    A, B = oriented(case["A"], case["B"], flip)
    plan, _ = check_plan(ctx, _space(case), A, B)
    assert plan.n == 1025 * k


# ------------------------------------------------- b. one-tile fill: LDS window
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("k", pc.fill1_window_k())
def test_fill_window_switch_one_tile(ctx, k, flip):
    case = pc.dense_case(pc.FILL1_WINDOW_N, k)
    A, B = oriented(case["A"], case["B"], flip)
    plan, whole = check_plan(ctx, _space(case), A, B)
    assert plan.n == 1025 * k
    # records in fill order: owners in sorted order, their partners in order
    assert np.array_equal(whole, _as_records(pc.Plan(A, B, case["lens"]).records()))
    _windows_equal(plan, whole, [(1024 * k - 70, 140), (k - 1, 2), (1024 * k, k)])


# ------------------------------------------------- c. two-tile fill: LDS window
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("k", pc.FILL2_WINDOW_K)
def test_fill_window_switch_two_tiles(ctx, k, flip):
    case = pc.dense_case(pc.FILL2_WINDOW_N, k, pc.FILL2_IDLE)
    A, B = oriented(case["A"], case["B"], flip)
    plan, whole = check_plan(ctx, _space(case), A, B)
    assert plan.n == 2049 * k
    assert np.array_equal(whole, _as_records(pc.Plan(A, B, case["lens"]).records()))
    # across the two tiles of the first commit, across the commit's end into
    # the last (odd, one-owner) tile, that tile alone, and odd cuts of it
    edge1, edge2 = 1024 * k, 2048 * k
    _windows_equal(plan, whole, [(edge1 - 70, 140), (edge1, 4097), (edge2 - 65, 130),
                                 (edge2 - 4096, 4096 + k), (edge2, k), (edge2 + 1, k - 2),
                                 (edge2 - 1, 2), (0, edge2 + 1)])


# ------------------------------------------------- d. the windows kernel switch
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("place", sorted(pc.WIDE_PLACES))
@pytest.mark.parametrize("width", [pc.WLANE_MAX, pc.WLANE_MAX + 1])
def test_windows_kernel_switch(ctx, width, place, flip):
    case = pc.wide_case(width, place)
    A, B = oriented(case["A"], case["B"], flip)
    sp = _space(case)
    a, b = ctx.set_from_host(sp, *A), ctx.set_from_host(sp, *B)
    assert a.stats()[1] == width and b.stats()[1] == width
    for t in pc.WIDE_THRESHOLDS:
        exp = oracle.intersect(A, B, t)
        plan, whole = check_plan(ctx, sp, A, B, plan=ctx.intersect(a, b, t), exp=exp)
        assert np.array_equal(whole, _as_records(pc.Plan(A, B, case["lens"], t).records()))


@pytest.mark.parametrize("maxw", pc.WINDOW_MAXW)
def test_window_plan_kernel_switch(ctx, maxw):
    # window(A, B, d): stream 0's owners are A's rows widened by d on either
    # side, max_width + 2 d = 65536 / 65537
    case = pc.window_case(maxw)
    A, B, d = case["A"], case["B"], case["d"]
    sp = _space(case)
    a, b = ctx.set_from_host(sp, *A), ctx.set_from_host(sp, *B)
    assert a.stats()[1] + 2 * d == pc.WLANE_MAX + (maxw - pc.WINDOW_MAXW[0])
    plan = ctx.window(a, b, d)
    check_plan(ctx, sp, A, B, plan=plan, exp=oracle.window(A, B, d))


# ------------------------------------------ e. filtered fill, output windows
@pytest.fixture(scope="module", params=pc.TWO_STREAM_THRESHOLDS)
def filtered_plan(ctx, request):
    """(plan, whole fill, restated plan) of the two-stream case at one
    threshold, checked against the oracle once"""
    t = request.param
    case = pc.two_stream_case()
    A, B = case["A"], case["B"]
    sp = _space(case)
    a, b = ctx.set_from_host(sp, *A), ctx.set_from_host(sp, *B)
    assert a.stats()[0] == 0 == b.stats()[0]  # zero-width rows: the filtered path
    model = pc.Plan(A, B, case["lens"], t)
    assert model.filtered
    plan, whole = check_plan(ctx, sp, A, B, plan=ctx.intersect(a, b, t),
                             exp=oracle.intersect(A, B, t))
    assert plan.n == model.total and (plan.n == 0) == (t == 161)
    assert np.array_equal(whole, _as_records(model.records()))
    return plan, whole, model


def test_filtered_windows(ctx, filtered_plan):
    plan, whole, model = filtered_plan
    if plan.n == 0:
        assert len(plan.fill_host()) == 0 and plan.checksum() == (0, 0)
        return
    # an owner with 5 or more records, cut inside them
    cnt = model.count[0]
    q = int(np.flatnonzero(cnt >= 5)[10])
    o = int(model.toff[q // pc.OT] + cnt[q // pc.OT * pc.OT:q].sum())
    n0, t1 = model.n0, int(model.toff[1])
    assert 0 < t1 < n0 < plan.n
    _windows_equal(plan, whole, [
        (o + 1, 3), (o + 2, int(cnt[q]) + 4),                 # inside / out of one owner
        (t1 - 33, 66), (t1, 1), (t1 - 1, 1), (t1 - 5000, 10000),  # a 1024-owner tile's end
        (n0 - 33, 66), (n0 - 1, 2), (n0, 777), (0, n0 + 1),   # the stream boundary
        (plan.n - 1, 1), (plan.n - 63, 63), (plan.n - 4097, 4097)])  # the last records


def test_filtered_odd_windows_make_the_whole(ctx, filtered_plan):
    plan, whole, _ = filtered_plan
    sizes = [1, 63, 64, 65, 777, 4095, 4097, 10007, 65, 30011, 1, 8191]
    parts, f, i = [], 0, 0
    while f < plan.n:
        k = min(sizes[i % len(sizes)], plan.n - f)
        parts.append(plan.fill_host(f, k))
        f, i = f + k, i + 1
    assert plan.n == 0 or np.array_equal(np.concatenate(parts), whole)


@pytest.mark.parametrize("count", [1, 63, 64, 65])
def test_filtered_small_windows_guarded(ctx, filtered_plan, count):
    import torch
    plan, whole, model = filtered_plan
    if plan.n == 0:
        return
    n0, t1 = model.n0, int(model.toff[1])
    buf = torch.zeros((count + 2, 4), dtype=torch.int32, device="cuda")
    for first in [0, 1000, t1 - count // 2 - 1, t1, n0 - count // 2 - 1, n0 - count, n0,
                  plan.n - count]:
        buf.fill_(-1)
        torch.cuda.synchronize()  # (the engine fills on its own stream)
        plan.fill_device(first, count, buf[1:].data_ptr())
        ctx.synchronize()
        got = buf.cpu().numpy().view(np.uint32)
        assert (got[0] == 0xffffffff).all() and (got[-1] == 0xffffffff).all()
        part = np.ascontiguousarray(got[1:-1]).reshape(-1).view(PAIR_DTYPE)
        assert np.array_equal(part, whole[first:first + count])


# -------------------------------------------- f. owned prefixes on one GPU
@pytest.mark.parametrize("t", pc.OWNED_THRESHOLDS)
def test_owned_prefixes(ctx, t):
    case = pc.two_stream_case()
    A, B = case["A"], case["B"]
    sp = _space(case)
    a, b = ctx.set_from_host(sp, *A), ctx.set_from_host(sp, *B)
    exp = oracle.intersect(A, B, t)
    # sorted position of every input row: the inverse of the set's row ids
    pos = []
    for S in (a, b):
        row = S.to_host()["row"]
        inv = np.empty(len(row), np.int64)
        inv[row] = np.arange(len(row))
        pos.append(inv)
    a_owns = B[1][exp["b_row"]] >= A[1][exp["a_row"]]  # (b starts inside a, ties to a)
    pa, pb = pos[0][exp["a_row"]], pos[1][exp["b_row"]]
    for a_own in pc.OWNED:
        for b_own in pc.OWNED:
            keep = np.where(a_owns, pa < a_own, pb < b_own)
            want = {k: exp[k][keep] for k in exp}
            plan = ctx.intersect(a, b, t, a_own, b_own)
            check_plan(ctx, sp, A, B, plan=plan, exp=want)
            plan.close()
    # -1: every row owns; a count past the set's size is refused
    assert ctx.intersect(a, b, t, -1, -1).n == len(exp["start"])
    with pytest.raises(LimeError) as ei:
        ctx.intersect(a, b, t, 3001, 3000)
    assert ei.value.code == 1  # LIME_ERR_ARG


# ------------------------------------------------- g. u32 tile-local offsets
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("m", pc.PILE_M)
def test_tile_offsets_u32(ctx, m, flip):
    # expected records are analytic (record p: owner p // m, partner p % m),
    # read in windows of 130 records: no whole fill, no checksum at 2^31 pairs.
    # Out of scope: the 2^31 flag's two-tile side (two such tiles in one
    # k_fill<2> commit) -- a plan that sparse needs more than 1.3e8 owner rows
    case = pc.pile_case(m)
    A, B = oriented(case["A"], case["B"], flip)
    sp = _space(case)
    a, b = ctx.set_from_host(sp, *A), ctx.set_from_host(sp, *B)
    if 1024 * m > 0xffffffff:
        with pytest.raises(LimeError) as ei:
            ctx.intersect(a, b)
        assert ei.value.code == pc.overflow_code()
        return
    plan = ctx.intersect(a, b)
    assert plan.n == 1024 * m == case["pairs"]
    for first, count in pc.pile_windows(m):
        got = plan.fill_host(first, count)
        assert np.array_equal(got, _as_records(pc.pile_records(m, first, count, flip))), first
    plan.close()
