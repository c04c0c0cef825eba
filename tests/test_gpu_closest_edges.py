"""closest at the edges of its block skips, staging windows, directories and
fill ranges (lime_amd/csrc/closest.hip), on the planted inputs of
tests/closest_cases.py (checked on the CPU by tests/test_closest_cases.py,
which also shows the arm each case takes):

  a. first_hit<true> in k_stuck: the jag in the last row of a head loop, the
     first and last row of a 64- and a 4096-row block, behind a block passed
     on its l2 entry and in the partial tail of both levels; the search
     starting at 63 / 64 / 65 and 4095 / 4096 / 4097 and ending mid-block;
  b. first_hit<false>: a head 4095 .. 4098 and 8201 rows past p_{i-1}, whose
     miss loses the before-side record; by rounds and by k_seq_prune;
  c. 4095 / 4096 / 4097 contigs (the contig table in LDS up to 4096 entries,
     read from global memory past that), the sweep live into every contig,
     dying on one, crossing thousands of empty ones; both modes;
  d. a covering window of 2047 / 2048 / 2049 / 4097 rights (staged up to
     2048), from right 0 and from right 1000, a block with a wave without
     D == 0 lefts, one with a stuck pointer and one past L.n, blocks with
     windows of their own, 1 .. 513 lefts;
  e. runs on one end below p, inside [p, hb) and at or above j; a same-start
     group of 1 / 64 / 65 / 5000 rights; coordinates on 4096 m - 1, 4096 m,
     4096 m + 1; spans of 8 * 4096 and one less; empty directory buckets;
  f. T == 0, lefts at coordinate 0, a contig of 0xFFFFFFFE bases with
     distances above 2^31, and the distance 0xFFFFFFFF itself;
  g. k_seq_single: advances of 63 .. 129 rights, stops on lane 63 and 0 and
     at r1, a prune keeping row 63 / 64 / 65, a covered length that drops;
  h. the seeds on which the Python decomposition needs 5 to 7 rounds: the
     engine, whose prefix max of ends is over global coordinates, needs one.

Every case is compared with the oracle record for record in output order
(whole-array integer equality) and by checksum; the pool's live bytes return
to their value once the plan and the sets are closed.  Cases of a, d, e and g
are also filled in parts."""
import numpy as np
import pytest

from lime_amd import PAIR_DTYPE, LimeError, Space
from oracle import oracle
from tests import closest_cases as cc

pytestmark = pytest.mark.gpu

COLS = ("a_row", "b_row", "start", "end")
Z32, Z64, Z8 = np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int8)
_SPACES = {}


def _space(ctx, case):
    """the case's space, made once, and primed: the context keeps the device
    offsets of the last few spaces it met and drops unused ones when a new one
    comes, so an empty set is made (and closed) in the space before the live
    bytes are read"""
    key = tuple(case["lens"])
    if key not in _SPACES:
        _SPACES[key] = Space(["c%05d" % i for i in range(len(key))], list(key))
    ctx.set_from_host_stranded(_SPACES[key], Z32, Z64, Z64, Z8).close()
    return _SPACES[key]


def _same(got, exp):
    assert len(got) == len(exp["start"])
    for k in COLS:
        g, e = np.asarray(got[k]).astype(np.int64), np.asarray(exp[k]).astype(np.int64)
        if not np.array_equal(g, e):
            i = int(np.flatnonzero(g != e)[0])
            raise AssertionError((k, i, int(g[i]), int(e[i])))


class _Run:
    """sets and plan of a case, compared with the oracle; closing gives the
    pool back"""

    def __init__(self, ctx, case, mode=0):
        self.ctx = ctx
        sp = _space(ctx, case)
        self.before = ctx.pool_live_bytes()[0]
        self.a = ctx.set_from_host_stranded(sp, *case["A"], case["sa"])
        self.b = ctx.set_from_host_stranded(sp, *case["B"], case["sb"])
        self.plan, self.alive_out = ctx.closest_chained(self.a, self.b, mode)
        exp = cc.expected(case, mode)
        assert self.plan.n == len(exp["start"])
        self.whole = self.plan.fill_host()
        _same(self.whole, exp)
        assert self.plan.checksum() == oracle.checksum_pairs(exp)

    def close(self):
        for h in (self.plan, self.a, self.b):
            h.close()
        assert self.ctx.pool_live_bytes()[0] == self.before


def _check(ctx, case, mode=0):
    r = _Run(ctx, case, mode)
    rounds = r.plan.closest_rounds()
    r.close()
    return rounds


# ------------------------------------------------------ a / b. block skips
@pytest.mark.parametrize("cap", [None, "0"])
def test_jag_skip(ctx, monkeypatch, cap):
    if cap is not None:
        monkeypatch.setenv("LIME_CLOSEST_MAX_ROUNDS", cap)
    want = (1, False) if cap is None else (0, True)
    for q in cc.JAG_Q:
        assert _check(ctx, cc.jag_case(q)) == want, q
    for args in cc.JAG2:
        assert _check(ctx, cc.jag2_case(*args)) == want, args


@pytest.mark.parametrize("cap", [None, "0", "1"])
def test_ends_skip(ctx, monkeypatch, cap):
    if cap is not None:
        monkeypatch.setenv("LIME_CLOSEST_MAX_ROUNDS", cap)
    want = (0, True) if cap == "0" else (1, False)
    for gap in cc.ENDS_GAP:
        assert _check(ctx, cc.ends_case(gap)) == want, gap


# ------------------------------------------------------------------ c. OCAP
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("nc", cc.OCAP_NC)
def test_contig_table(ctx, nc, mode):
    for variant in cc.ocap_variants(nc):
        case = cc.ocap_case(nc, variant)
        r = _Run(ctx, case, mode)
        assert r.alive_out == cc.state(case).alive_out, variant
        r.close()


# ------------------------------------------------------------------ d. SWIN
@pytest.mark.parametrize("pre", cc.SWIN_PRE)
@pytest.mark.parametrize("W", cc.SWIN_W)
def test_covering_window(ctx, W, pre):
    _check(ctx, cc.swin_case(W, pre, 1))
    _check(ctx, cc.swin_waves_case(W, pre))


@pytest.mark.parametrize("n", cc.SWIN_LEFTS)
def test_covering_window_left_counts(ctx, n):
    _check(ctx, cc.swin_case(cc.SWIN, 1000, n))
    _check(ctx, cc.swin_case(cc.SWIN + 1, 0, n))


# ------------------------------------------- e / f. exact runs and extremes
def test_exact_distance_runs(ctx):
    for case in [cc.end_run_case(), cc.end_run_below_case(), cc.lattice_case()] + \
            [cc.group_case(g) for g in cc.GROUP_G] + [cc.span_case(s) for s in cc.SPAN]:
        assert _check(ctx, case) == (1, False), case["key"]


def test_coordinate_extremes(ctx):
    for case in (cc.zero_case(), cc.far_case(), cc.far_only_case()):
        for mode in (0, 1):
            _check(ctx, case, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_distance_0xffffffff(ctx, mode):
    # a zero-width left at 0xFFFFFFFE and a zero-width right at 0: the
    # distance is the value that used to mark "no output" in dd[]
    case = cc.none_distance_case()
    assert len(cc.expected(case, mode)["start"]) == 1
    _check(ctx, case, mode)


# ------------------------------------------------------------ g. k_seq_single
def test_single_overlap_ballots(ctx):
    for n in cc.SINGLE_ADV:
        _check(ctx, cc.single_advance_case(n, False), 1)
        _check(ctx, cc.single_advance_case(n, False), 0)
        if n % 64 == 0:
            _check(ctx, cc.single_advance_case(n, True), 1)
    for m in cc.SINGLE_DROP:
        _check(ctx, cc.single_cover_drop_case(m), 1)
    # the window and group cases through the in-order chain as well
    _check(ctx, cc.swin_waves_case(cc.SWIN + 1, 1000), 1)
    _check(ctx, cc.group_case(65), 1)
    _check(ctx, cc.end_run_case(), 1)


# ---------------------------------------------------------------- h. rounds
@pytest.mark.parametrize("cap", [None, "K", "K-1"])
def test_round_counts(ctx, monkeypatch, cap):
    for seed in cc.ROUND_SEEDS:
        case = cc.from_seed(seed)
        st = cc.restate(case)
        K = st.rounds
        assert K == 1   # (tests/closest_cases.py ROUND_SEEDS: exact at round 0)
        if cap is None:
            monkeypatch.delenv("LIME_CLOSEST_MAX_ROUNDS", raising=False)
            want = (K, False)
        else:
            forced = K if cap == "K" else K - 1
            monkeypatch.setenv("LIME_CLOSEST_MAX_ROUNDS", str(forced))
            want = (K, False) if forced >= K else (forced, True)
        got = _check(ctx, case)
        print(seed, cap, got)
        assert got == want, seed


# ------------------------------------------------------------- partial fills
def _fill_cases():
    return [(cc.swin_waves_case(cc.SWIN, 1000), 0), (cc.swin_waves_case(cc.SWIN + 1, 0), 0),
            (cc.swin_case(cc.SWIN, 1000, 257), 0), (cc.end_run_case(), 0),
            (cc.end_run_below_case(), 0), (cc.group_case(65), 0), (cc.group_case(5000), 0),
            (cc.lattice_case(), 0), (cc.span_case(cc.SPAN[0]), 0), (cc.jag_case(4097), 0),
            (cc.single_cover_drop_case(64), 1)]


def _offsets(whole):
    """(first record, count) of each left with records, in output order"""
    a = np.asarray(whole["a_row"])
    cut = np.flatnonzero(np.diff(a) != 0) + 1
    first = np.concatenate([[0], cut])
    return first, np.diff(np.concatenate([first, [len(a)]]))


@pytest.mark.parametrize("idx", range(11))
def test_partial_fills(ctx, idx):
    import torch
    case, mode = _fill_cases()[idx]
    r = _Run(ctx, case, mode)
    plan, whole, n = r.plan, r.whole, r.plan.n
    first, cnt = _offsets(whole)
    if mode == 0:   # the engine's off[] is the restatement's
        st = cc.state(case)
        assert np.array_equal(first, st.out_off[:-1][st.cnt > 0]) and st.out_off[-1] == n

    def part(f, c):
        got = plan.fill_host(f, c)
        assert np.array_equal(got, whole[f:f + c]), (f, c)
    # chunks of 1, 63, 64, 65 and 997 records that make up the whole (the
    # small sizes over at most 2200 records from 100 before the largest left)
    big = int(np.argmax(cnt))
    for size in (1, 63, 64, 65, 997):
        lo = 0 if n <= 2200 or size == 997 else max(int(first[big]) - 100, 0)
        hi = n if n <= 2200 or size == 997 else min(lo + 2200, n)
        parts = [plan.fill_host(f, min(size, hi - f)) for f in range(lo, hi, size)]
        assert np.array_equal(np.concatenate(parts), whole[lo:hi]), size
    # chunks starting on a left's off[i], one before and one after it, and
    # inside its run: 63 / 64 / 65 records in (a D == 0 run cut inside a
    # 64-candidate ballot), in the middle, one before its end
    lefts = sorted({0, 1, big, len(first) - 1} & set(range(len(first))))
    for i in lefts:
        f0, c0 = int(first[i]), int(cnt[i])
        for f in {f0 - 1, f0, f0 + 1, f0 + 63, f0 + 64, f0 + 65, f0 + c0 // 2, f0 + c0 - 1}:
            for c in (1, 2, 63, 64, 65, 997):
                if 0 <= f and f + c <= n:
                    part(f, c)
    # one fill into a device buffer with sentinel records on both sides
    f = int(first[big]) + min(1, int(cnt[big]) - 1)
    c = min(65, n - f)
    buf = torch.full((c + 2, 4), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # (the engine fills on its own stream)
    plan.fill_device(f, c, buf[1:].data_ptr())
    ctx.synchronize()
    got = buf.cpu().numpy().view(np.uint32)
    assert (got[0] == 0xffffffff).all() and (got[-1] == 0xffffffff).all()
    assert np.array_equal(np.ascontiguousarray(got[1:-1]).reshape(-1).view(PAIR_DTYPE),
                          whole[f:f + c])
    # ranges outside the plan
    for f, c in ((n, 1), (0, n + 1), (-1, 1), (n - 1, 2)):
        with pytest.raises(LimeError):
            plan.fill_host(f, c)
    assert len(plan.fill_host(n, 0)) == 0
    del buf
    r.close()
