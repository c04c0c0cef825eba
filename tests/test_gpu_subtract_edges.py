"""Subtract at the capacities of its LDS stages and the switches between its
launches (lime_amd/csrc/subtract.hip), on the planted inputs of
tests/subtract_cases.py (checked on the CPU by tests/test_subtract_cases.py,
which also shows the launch each case takes):

  a. k_sub_fused stages a tile's records up to FCAP (896): tiles of 895 / 896
     / 897 records, and an unstaged tile between two staged ones;
  b. the local scan runs while every tile's window of B is within FWIN (3072):
     windows of 3071 / 3072 / 3073 rows, one of four stages' length on the
     merge-scan path, a left row whose end bound is exactly the staged count,
     a left row before every B row;
  c. 1, 1023, 1024, 1025, 2047, 2048 and 2049 left rows (a tile is 2048), and
     40 x 1024 + 1 with empty, staged and unstaged tiles;
  d. the output guess na + 4096: totals one below, at and one past it, the
     tile across the guess staged or not -- the second pass's result exact;
  e. runs * 64 against na at equality and one run below; one record in 16 and
     in 17 blocks (the sweeping write pass);
  f. the count pass's uint8 per-row count: a row of 254 / 255 / 256 records
     and one of 600;
  g. the write passes' record stage SCAP (512): a block of 511 / 512 / 513;
  h. the B-row stages: a walked block's window of 1024 / 1025 rows, a runs
     write block needing 1024 / 1025, a count workgroup's window of 1535 /
     1536 / 1537 and windows reaching back to one wide row;
  i. a same-start group of 16 / 17 / 18 rows of B (the walks reach 17) mid
     set, as B's last rows with len(B) % 4 = 0 .. 3, and as all of B;
  j. the cases of a, b and i again on the merge-scan path (LIME_SUB_NO_LS).

Every case runs in both modes and is compared with the oracle's records in
the engine's output order (tests/subtract_cases.py expected_in_order) by
whole-array equality: nothing is sorted on either side."""
import numpy as np
import pytest

from lime_amd import Space, SUBTRACT_LIME, SUBTRACT_SET
from tests import subtract_cases as sc

pytestmark = pytest.mark.gpu

COLS = ("contig", "start", "end", "a_row", "b_row")
RUNS_T = [0, -3]


def test_modes_are_the_oracles():
    assert (SUBTRACT_LIME, SUBTRACT_SET) == (sc.LIME, sc.SET)


def _sets(ctx, case):
    sp = Space(["c0"], case["lens"])
    a, b = ctx.set_from_host(sp, *case["A"]), ctx.set_from_host(sp, *case["B"])
    m = sc.model(case)  # the set statistics the dispatch reads
    assert a.stats()[1] == m.maxw_a and b.stats()[1:] == (m.maxw_b, m.zw)
    return a, b


def _same(res, exp):
    assert len(res["start"]) == len(exp["start"])
    for k in COLS:
        if not np.array_equal(res[k], exp[k]):
            i = int(np.flatnonzero(res[k] != exp[k])[0])
            raise AssertionError((k, i, {c: (int(res[c][i]), int(exp[c][i])) for c in COLS}))


def _check(ctx, case, ts, mode, sets=None):
    """subtract at every threshold of ts == the oracle, record for record"""
    a, b = sets or _sets(ctx, case)
    out = None
    for t in ts:
        out = ctx.subtract(a, b, t, mode).to_host()
        _same(out, sc.expected(case, t, mode))
    return out


def _check_both_paths(ctx, case, ts, mode, monkeypatch):
    """j: the case on its own path, then (fresh sets) on the merge-scan path"""
    own = _check(ctx, case, ts, mode)
    monkeypatch.setenv("LIME_SUB_NO_LS", "1")
    other = _check(ctx, case, ts, mode)
    monkeypatch.delenv("LIME_SUB_NO_LS")
    for k in COLS:
        assert np.array_equal(own[k], other[k]), k


# --------------------------------------------------------- a. the fused stage
@pytest.mark.parametrize("zw", [False, True])
@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("total", sc.STAGE_T)
def test_fused_record_stage(ctx, total, mode, zw, monkeypatch):
    case = sc.stage_case(total, mode, zw)
    assert len(sc.expected(case, 0, mode)["start"]) == total
    _check_both_paths(ctx, case, RUNS_T, mode, monkeypatch)


@pytest.mark.parametrize("zw", [False, True])
@pytest.mark.parametrize("mode", sc.MODES)
def test_fused_unstaged_tile_between_staged(ctx, mode, zw, monkeypatch):
    _check_both_paths(ctx, sc.stage3_case(mode, zw), RUNS_T, mode, monkeypatch)


# ----------------------------------------- b. local-scan switch, fused window
@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("W,zw", [(w, False) for w in sc.WINDOW_W] +
                         [(sc.WINDOW_W[2], True), (sc.WINDOW_LONG, True)])
def test_fused_window_switch(ctx, W, zw, mode, monkeypatch):
    _check_both_paths(ctx, sc.window_case(W, zw), RUNS_T, mode, monkeypatch)


@pytest.mark.parametrize("zw", [False, True])
@pytest.mark.parametrize("mode", sc.MODES)
def test_fused_window_ends(ctx, mode, zw, monkeypatch):
    _check_both_paths(ctx, sc.ends_case(zw), RUNS_T + [1], mode, monkeypatch)


# ------------------------------------------------ c. partial and many tiles
@pytest.mark.parametrize("zw", [False, True])
@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("na", sc.TILE_NA)
def test_partial_tiles(ctx, na, mode, zw):
    _check(ctx, sc.tiles_case(na, zw), RUNS_T + [1], mode)


@pytest.mark.parametrize("zw", [False, True])
@pytest.mark.parametrize("mode", sc.MODES)
def test_many_tiles(ctx, mode, zw):
    _check(ctx, sc.many_tiles_case(zw), RUNS_T, mode)


# ---------------------------------------------------------- d. output guess
@pytest.mark.parametrize("zw", [False, True])
@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("last", sorted(sc.GUESS_LAST))
@pytest.mark.parametrize("delta", sc.GUESS_DELTA)
def test_output_guess(ctx, delta, last, mode, zw):
    case = sc.guess_case(delta, last, mode, zw)
    out = _check(ctx, case, RUNS_T, mode)
    assert len(out["start"]) == sc.GUESS_NA + sc.GUESS + delta


# ------------------------------------------- e. switches of the two-pass side
@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("runs", sc.SWITCH_RUNS)
def test_one_pass_two_pass_switch(ctx, runs, mode):
    case = sc.switch_case(runs)
    a, b = _sets(ctx, case)
    assert ctx.merge(b).n == runs == sc.model(case).runs  # mb.n * 64 >= na
    _check(ctx, case, RUNS_T + [1], mode, (a, b))


@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("na", sc.SPARSE_NA)
def test_sweeping_write_switch(ctx, na, mode):
    out = _check(ctx, sc.sparse_case(na), RUNS_T + [1], mode)
    assert len(out["start"]) == 1


# ------------------------------------------------------ f. rcnt saturation
@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("m", sc.RCNT_M)
def test_row_count_saturation(ctx, m, mode):
    _check(ctx, sc.rcnt_case(m), RUNS_T, mode)


# ------------------------------------------------------------------ g. SCAP
@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("total", sc.SCAP_T)
def test_block_record_stage(ctx, total, mode):
    _check(ctx, sc.scap_case(total, mode), RUNS_T + [1], mode)


# ------------------------------------------------------- h. BWIN and CNT_WIN
@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("span", sc.BWIN_SPAN)
def test_walk_block_window(ctx, span, mode):
    _check(ctx, sc.bwin_walk_case(span), [1, 0], mode)


@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("c", sc.BWIN_RUNS_COPIES)
def test_runs_block_window(ctx, c, mode):
    _check(ctx, sc.bwin_runs_case(c), RUNS_T + [1], mode)


@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("c", sc.CNT_WIN_COPIES)
def test_count_window(ctx, c, mode):
    _check(ctx, sc.cnt_win_case(c), RUNS_T, mode)


@pytest.mark.parametrize("mode", sc.MODES)
def test_count_window_wide_row(ctx, mode):
    _check(ctx, sc.cnt_wide_case(), RUNS_T + [1], mode)


# --------------------------------------------------------------- i. tie index
@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("place", sc.TIE_PLACES)
@pytest.mark.parametrize("g", sc.TIE_SIZES)
def test_same_start_group(ctx, g, place, mode, monkeypatch):
    case = sc.tie_case(g, place)
    # the local scan, twice on the same sets: the first call meets the group
    # without B's tie index (past 17 rows: defers, builds it, runs again),
    # the second finds it built
    sets = _sets(ctx, case)
    first = _check(ctx, case, [0], mode, sets)
    again = _check(ctx, case, [0, -3], mode, sets)
    # the merge-scan path on fresh sets (its scan tells of the group), and
    # the walk
    monkeypatch.setenv("LIME_SUB_NO_LS", "1")
    scan = _check(ctx, case, [0], mode)
    monkeypatch.delenv("LIME_SUB_NO_LS")
    for k in COLS:
        assert np.array_equal(first[k], again[k]) and np.array_equal(first[k], scan[k]), k
    _check(ctx, case, [1], mode)
