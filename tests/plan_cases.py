"""Inputs planted on the dispatch edges of the intersect plan, and the plan's
dispatch conditions restated in numpy -- shared by tests/test_plan_cases.py
(CPU: every case has the property it is named for, and the restated plan
counts what the oracle counts) and tests/test_gpu_plan_edges.py (the engine
against the oracle on the same inputs).

The plan (lime_amd/csrc/intersect.hip): both sets sorted in canonical order;
stream 0's owners are A's rows (partners: B rows starting in [a.s, a.e)),
stream 1's owners B's rows (partners: A rows starting in (b.s, b.e)); owners
are taken in tiles of OT = 1024, every tile has a partner window [lo, hi)
(k_windows_lane or k_windows), k_count finds every owner's range inside it
(searching an LDS image of the window or global memory) and the tile's pair
sum, and k_fill / k_fill_filtered write the records.  Each restatement below
quotes the source line it restates; tests/test_plan_cases.py checks that the
quoted lines still stand in the source.

Every builder is cached and returns read-only arrays.
"""
import functools
import os
import re

import numpy as np

from tests.test_gpu_fill_edges import dense_block, grid_plan
from tests.util import random_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OT = 1024            # constexpr int OT = IB * OPT;  (256 x 4 owners per tile)
WCAP = 4096          # constexpr int WCAP = 4096;
WLANE_MAX = 65536    # constexpr int64_t WLANE_MAX = 65536;
PCAP2 = 2496         # constexpr int PCAP2 = 2496;
FILL_SPARSE = 16     # #define LIME_FILL_SPARSE 16

# the source lines the restatements below stand for (regular expressions over
# lime_amd/csrc/intersect.hip)
SOURCE_LINES = {
    "OT": r"constexpr int IB = 256;\s*\n\s*constexpr int OPT = 4;[^\n]*\n"
          r"\s*constexpr int OT = IB \* OPT;",
    "WCAP": r"constexpr int WCAP = 4096;",
    "WLANE_MAX": r"constexpr int64_t WLANE_MAX = 65536;",
    "PCAP": r"constexpr int PCAP = LIME_FILL_WGS >= 3 \? 1792 : 2048;",
    "PCAP2": r"constexpr int PCAP2 = 2496;",
    "CAP": r"static constexpr int CAP = TPF == 1 \? PCAP : PCAP2;",
    "FILL_SPARSE": r"#ifndef LIME_FILL_SPARSE\n[^\n]*\n#define LIME_FILL_SPARSE 16\n",
    "lane_switch": r"if \(owmax <= WLANE_MAX\)\s*\n\s*hipLaunchKernelGGL\(k_windows_lane,",
    "owmax": r"const int64_t owmax = \(int64_t\)O->max_width \+ "
             r"\(st == 0 && reach > 0 \? 2 \* reach : 0\);",
    "lane_lkey": r"const int64_t lkey = \(int64_t\)g0 \+ sa\.lo_off;",
    "lane_hkey": r"int64_t hkey = \(int64_t\)g1 \+ owmax - tp \+ 1;",
    "lane_hkey_floor": r"const int64_t lkey_last = \(int64_t\)g1 \+ sa\.lo_off;[^\n]*\n"
                       r"\s*if \(hkey < lkey_last\) hkey = lkey_last;",
    "exact_hmax": r"hmax = max\(hmax, \(int64_t\)sa\.oge\[j\] - tp \+ 1\);",
    "exact_floor": r"if \(hmax < lkey_last\) hmax = lkey_last;",
    "owner_keys": r"lo_key = \(int64_t\)og \+ lo_off;\s*\n\s*hi_key = \(int64_t\)oe - tp \+ 1;",
    "tp": r"pl->tp = threshold > 1 \? threshold : 1;",
    "zw_skip": r"s\.zw_skip = \(st == 0 && threshold <= 0 && P->has_zero_width\) \? 1 : 0;",
    "in_lds": r"const bool in_lds = wlen <= WCAP;",
    "par_lds": r"const bool par_lds = \(int64_t\)whi - wlo <= CAP;",
    "filtered": r"pl->filtered = threshold >= 1 && "
                r"\(int64_t\)std::min\(A->min_width, B->min_width\) < threshold &&\s*\n"
                r"\s*A->n > 0 && B->n > 0;",
    "filter_test": r"c \+= \(int64_t\)\(sa\.pge\[p\] - sa\.pgs\[p\]\) >= threshold;",
    "oflow": r"if \(s > 0xffffffffull && oflow\)\s*\n\s*atomicOr\(oflow, 1u\);\s*\n"
             r"\s*else if \(s > 0x7fffffffull && oflow\)\s*\n\s*atomicOr\(oflow, 2u\);",
    "oflow_fail": r"if \(tot\[1\] & 1\)\s*\n\s*return fail\(LIME_ERR_OVERFLOW,",
    "tpf": r"pl->tpf = !\(tot\[1\] & 2\) && "
           r"pl->total < \(int64_t\)LIME_FILL_SPARSE \* \(a_own \+ b_own\) \? 2 : 1;",
    "filtered_window": r"if \(pos >= fa\.first && pos < wend\) \{",
}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def fill_wgs():
    """LIME_FILL_WGS of the library build: the Makefile's HIPFLAGS when they
    set it, else the source's default"""
    flags = re.search(r"^HIPFLAGS\s*=((?:.*\\\n)*.*)$", _read("Makefile"), re.M).group(1)
    m = re.search(r"-DLIME_FILL_WGS=(\d+)", flags)
    if m:
        return int(m.group(1))
    m = re.search(r"#ifndef LIME_FILL_WGS\n#define LIME_FILL_WGS (\d+)",
                  _read("lime_amd", "csrc", "intersect.hip"))
    return int(m.group(1))


def fill_cap(tpf=1):
    """rows of k_fill<tpf>'s LDS partner window (FillShape<TPF>::CAP)"""
    if tpf == 2:
        return PCAP2
    m = re.search(r"constexpr int PCAP = LIME_FILL_WGS >= (\d+) \? (\d+) : (\d+);",
                  _read("lime_amd", "csrc", "intersect.hip"))
    return int(m.group(2)) if fill_wgs() >= int(m.group(1)) else int(m.group(3))


def overflow_code():
    """LIME_ERR_OVERFLOW of include/lime_amd.h"""
    m = re.search(r"#define LIME_ERR_OVERFLOW (\d+)", _read("include", "lime_amd.h"))
    return int(m.group(1))


# -------------------------------------------------------------- restatements
def offsets(lens):
    """global offset of every contig: contigs are laid out with one pad base
    between them (lime_space_create: o += lengths[c] + 1)"""
    return np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64) + 1)])


def canonical(X, lens):
    """(gs, ge, order) of a plain set: (global start, zero-width first, input
    row)"""
    c, s, e = (np.asarray(x) for x in X)
    off = offsets(lens)
    gs, ge = off[c] + s, off[c] + e
    order = np.lexsort((np.arange(len(gs)), ge > gs, gs))
    return gs[order].astype(np.int64), ge[order].astype(np.int64), order


def set_stats(X):
    """(min width, max width, any zero width); (0, 0, False) when empty"""
    w = np.asarray(X[2], np.int64) - np.asarray(X[1], np.int64)
    return (int(w.min()), int(w.max()), bool((w == 0).any())) if len(w) else (0, 0, False)


def is_filtered(threshold, stats_a, stats_b, na, nb):
    # pl->filtered = threshold >= 1 && (int64_t)std::min(A->min_width, B->min_width) < threshold &&
    #                A->n > 0 && B->n > 0;
    return threshold >= 1 and min(stats_a[0], stats_b[0]) < threshold and na > 0 and nb > 0


def uses_lane_windows(owmax):
    # if (owmax <= WLANE_MAX) hipLaunchKernelGGL(k_windows_lane, ...
    return owmax <= WLANE_MAX


def windows_lane(ogs, pgs, no, lo_off, tp, owmax):
    """k_windows_lane: per owner tile [lo, hi), both lower bounds in the
    partner starts:
        lkey = g0 + lo_off
        hkey = g1 + owmax - tp + 1;  if (hkey < lkey_last) hkey = lkey_last
    with g0 / g1 the tile's first / last owner start, lkey_last = g1 + lo_off"""
    out = []
    for o0 in range(0, no, OT):
        o1 = min(o0 + OT, no)
        g0, g1 = int(ogs[o0]), int(ogs[o1 - 1])
        lkey = g0 + lo_off
        hkey = max(g1 + owmax - tp + 1, g1 + lo_off)
        out.append((int(np.searchsorted(pgs, lkey, "left")),
                    int(np.searchsorted(pgs, hkey, "left"))))
    return np.array(out, np.int64).reshape(-1, 2)


def windows_exact(ogs, oge, pgs, no, lo_off, tp):
    """k_windows: hkey is the exact max of oe - tp + 1 over the tile's owners
    (hmax = max(hmax, (int64_t)sa.oge[j] - tp + 1)), floored at lkey_last"""
    out = []
    for o0 in range(0, no, OT):
        o1 = min(o0 + OT, no)
        lkey = int(ogs[o0]) + lo_off
        hkey = max(int(oge[o0:o1].max()) - tp + 1, int(ogs[o1 - 1]) + lo_off)
        out.append((int(np.searchsorted(pgs, lkey, "left")),
                    int(np.searchsorted(pgs, hkey, "left"))))
    return np.array(out, np.int64).reshape(-1, 2)


def owner_ranges(ogs, oge, pgs, pge, no, st, threshold):
    """k_count: per owner (lo, hi, count).  lo_key = og + lo_off, hi_key =
    oe - tp + 1, the range empty when hi_key <= lo_key; stream 0 with
    threshold <= 0 skips the zero-width partners at exactly og (canonical
    order puts them first); under the width filter count is the number of
    partners in [lo, hi) with width >= threshold, else hi - lo."""
    tp = max(threshold, 1)
    lo_off = 0 if st == 0 else 1
    og, oe = ogs[:no], oge[:no]
    lk, hk = og + lo_off, oe - tp + 1
    lo = np.searchsorted(pgs, lk, "left")
    hi = np.where(hk > lk, np.searchsorted(pgs, hk, "left"), lo)
    if st == 0 and threshold <= 0 and (pge == pgs).any():  # zw_skip
        key = 2 * pgs + (pge > pgs)
        lo = np.maximum(lo, np.searchsorted(key, 2 * og + 1, "left"))
        hi = np.maximum(hi, lo)
    return lo.astype(np.int64), hi.astype(np.int64)


class Plan:
    """the restated plan of intersect(A, B, threshold, a_own, b_own) over one
    space (contig lengths `lens`)"""

    def __init__(self, A, B, lens, threshold=0, a_own=-1, b_own=-1):
        self.sets = [canonical(A, lens), canonical(B, lens)]
        self.stats = [set_stats(A), set_stats(B)]
        na, nb = len(A[1]), len(B[1])
        self.own = [na if a_own < 0 or a_own > na else a_own,
                    nb if b_own < 0 or b_own > nb else b_own]
        self.threshold = threshold
        self.tp = max(threshold, 1)  # pl->tp = threshold > 1 ? threshold : 1;
        self.filtered = is_filtered(threshold, self.stats[0], self.stats[1], na, nb)
        self.owmax, self.lane, self.win, self.win_exact = [], [], [], []
        self.lo, self.hi, self.keep, self.count, self.tile_sums = [], [], [], [], []
        for st in (0, 1):
            ogs, oge, _ = self.sets[st]
            pgs, pge, _ = self.sets[1 - st]
            no = self.own[st] if na and nb else 0
            # const int64_t owmax = (int64_t)O->max_width + ...
            owmax = self.stats[st][1]
            self.owmax.append(owmax)
            self.lane.append(uses_lane_windows(owmax))
            ex = windows_exact(ogs, oge, pgs, no, st, self.tp)
            self.win_exact.append(ex)
            self.win.append(windows_lane(ogs, pgs, no, st, self.tp, owmax) if self.lane[st] else ex)
            lo, hi = owner_ranges(ogs, oge, pgs, pge, no, st, threshold)
            # c += (int64_t)(sa.pge[p] - sa.pgs[p]) >= threshold;
            keep = (pge - pgs >= threshold) if self.filtered else np.ones(len(pgs), bool)
            cum = np.concatenate([[0], np.cumsum(keep)])
            cnt = cum[hi] - cum[lo]
            self.lo.append(lo), self.hi.append(hi), self.keep.append(keep), self.count.append(cnt)
            self.tile_sums.append(np.add.reduceat(cnt, np.arange(0, no, OT)) if no
                                  else np.zeros(0, np.int64))
        self.sums = np.concatenate(self.tile_sums).astype(np.int64)
        self.toff = np.concatenate([[0], np.cumsum(self.sums)])  # per tile, stream 0 first
        self.total = int(self.sums.sum())
        self.n0 = int(self.tile_sums[0].sum())  # records of stream 0
        # if (s > 0xffffffffull && oflow) atomicOr(oflow, 1u);
        # else if (s > 0x7fffffffull && oflow) atomicOr(oflow, 2u);
        self.overflow = bool((self.sums > 0xffffffff).any())
        self.half = bool(((self.sums > 0x7fffffff) & (self.sums <= 0xffffffff)).any())
        # pl->tpf = !(tot[1] & 2) &&
        #           pl->total < (int64_t)LIME_FILL_SPARSE * (a_own + b_own) ? 2 : 1;
        self.tpf = 2 if not self.half and self.total < FILL_SPARSE * (self.own[0] + self.own[1]) \
            else 1

    def wlen(self, st):
        """window lengths of stream st's tiles (k_count: wlen = whi - wlo;
        in_lds = wlen <= WCAP)"""
        return self.win[st][:, 1] - self.win[st][:, 0]

    def commit_wlen(self, st):
        """window lengths of k_fill<tpf>'s commits: the union of the first
        and the last tile's windows (r.wlo = min(...), r.whi = max(...));
        par_lds = whi - wlo <= CAP"""
        w = self.win[st]
        out = []
        for t in range(0, len(w), self.tpf):
            t1 = min(t + self.tpf, len(w))
            out.append(max(w[t, 1], w[t1 - 1, 1]) - min(w[t, 0], w[t1 - 1, 0]))
        return np.array(out, np.int64)

    def ranges_inside_windows(self):
        """every owner's [lo, hi) lies inside its tile's window, and the lane
        window holds the exact one"""
        for st in (0, 1):
            t = np.arange(len(self.lo[st])) // OT
            w, ex = self.win[st], self.win_exact[st]
            if not ((w[t, 0] <= self.lo[st]) & (self.hi[st] <= w[t, 1])).all():
                return False
            if not ((w[:, 0] == ex[:, 0]) & (w[:, 1] >= ex[:, 1])).all():
                return False
        return True

    def records(self):
        """the plan's records in fill order as a (total, 4) array (start,
        end, a_row, b_row), coordinates local to the single contig: stream 0's
        owners in sorted order, then stream 1's; an owner's partners in sorted
        order"""
        out = []
        for st in (0, 1):
            ogs, oge, orow = self.sets[st]
            pgs, pge, prow = self.sets[1 - st]
            lo, hi = self.lo[st], self.hi[st]
            cand = hi - lo
            owner = np.repeat(np.arange(len(lo)), cand)
            first = np.concatenate([[0], np.cumsum(cand)])[:-1]
            p = np.repeat(lo, cand) + np.arange(int(cand.sum())) - np.repeat(first, cand)
            k = self.keep[st][p]
            owner, p = owner[k], p[k]
            rec = np.stack([np.maximum(ogs[owner], pgs[p]), np.minimum(oge[owner], pge[p]),
                            (orow[owner], prow[p])[st], (prow[p], orow[owner])[st]], axis=1)
            out.append(rec.astype(np.int64))
        return np.concatenate(out)


# --------------------------------------------------------------------- cases
def _freeze(case):
    for v in case.values():
        for x in (v if isinstance(v, tuple) else (v,)):
            if isinstance(x, np.ndarray):
                x.flags.writeable = False
    return case


def _case(A, B, length, **extra):
    case = {"A": A, "B": B, "lens": [int(length)]}
    case.update(extra)
    return _freeze(case)


def oriented(case, flip):
    """(A, B) of the case, or (B, A): every pair then belongs to the other
    stream"""
    return (case["B"], case["A"]) if flip else (case["A"], case["B"])


@functools.lru_cache(maxsize=None)
def dense_case(n, k, idle=0):
    """dense_block(n, k, 0): n owners [4 i + 2, 4 i + 2 + 4 k) with exactly k
    partners each on the grid [4 j, 4 j + 1); a full owner tile's window is
    1023 + k partner rows, two tiles' union 2047 + k.  idle: that many more
    grid rows past every owner's end (they pair with nothing)"""
    a_s, a_l, b_s = dense_block(n, k, 0)
    if idle:
        b_s = np.concatenate([b_s, b_s[-1] + 4 * (k + 8) + 4 * np.arange(1, idle + 1)])
    A, B, top = grid_plan(a_s, a_l, b_s)
    return _case(A, B, top, n=n, k=k, pairs=n * k)


# a. k_count's LDS / global switch: the first tile's window 4095 / 4096 / 4097
COUNT_WINDOW_K = [WCAP - 1023 - 1, WCAP - 1023, WCAP - 1023 + 1]
COUNT_WINDOW_N = OT + 1


def fill1_window_k():
    """b. k_fill<1>'s LDS partner window: CAP - 1 / CAP / CAP + 1 rows"""
    cap = fill_cap(1)
    return [cap - 1023 - 1, cap - 1023, cap - 1023 + 1]


FILL1_WINDOW_N = OT + 1

# c. k_fill<2>'s LDS partner window: the union of two tiles' windows 2495 /
# 2496 / 2497 rows; 60 000 idle rows keep the plan below 16 pairs per owner
FILL2_WINDOW_K = [PCAP2 - 2047 - 1, PCAP2 - 2047, PCAP2 - 2047 + 1]
FILL2_WINDOW_N = 2 * OT + 1
FILL2_IDLE = 60_000

# d. the windows kernel switch: one owner row of width WLANE_MAX / WLANE_MAX + 1
WIDE_N = 3000
WIDE_PLACES = {"tile_first": OT, "tile_last": 2 * OT - 1, "set_last": WIDE_N - 1}
WIDE_THRESHOLDS = [0, 1, 30]
WIDE_LEN = 100_000  # starts below it; the contig leaves room for the wide rows


@functools.lru_cache(maxsize=None)
def wide_case(width, place):
    """3000 x 3000 random rows (max_len 400, zero-width rows, duplicates,
    book-ends); in each set the row at sorted position WIDE_PLACES[place]
    is made `width` bases wide (the set's widest by far)"""
    rng = np.random.default_rng(4100 + sorted(WIDE_PLACES).index(place))
    A, B = random_sets(rng, WIDE_N, WIDE_N, n_contigs=1, contig_len=WIDE_LEN, max_len=400,
                       zero_frac=0.05, dup_frac=0.05, book_frac=0.05)
    length = WIDE_LEN + WLANE_MAX + 8
    rows = []
    for X in (A, B):
        _, _, order = canonical(X, [length])
        r = int(order[WIDE_PLACES[place]])
        X[2][r] = X[1][r] + width
        rows.append(r)
    return _case(A, B, length, wide_rows=tuple(rows), width=width, pos=WIDE_PLACES[place])


# d (window plans): the widened owners are max_width + 2 d wide
WINDOW_D = 32_568
WINDOW_MAXW = [WLANE_MAX - 2 * WINDOW_D, WLANE_MAX - 2 * WINDOW_D + 1]  # 400, 401


@functools.lru_cache(maxsize=None)
def window_case(maxw):
    """1200 x 600 random rows narrower than 400 on one contig of 100 000, A's
    input row 0 made exactly `maxw` wide: window(A, B, WINDOW_D)'s stream-0
    owners are up to maxw + 2 WINDOW_D wide"""
    rng = np.random.default_rng(4200)
    A, B = random_sets(rng, 1200, 600, n_contigs=1, contig_len=WIDE_LEN, max_len=400,
                       zero_frac=0.05, dup_frac=0.05, book_frac=0.05)
    A[2][0] = A[1][0] + maxw
    return _case(A, B, WIDE_LEN, maxw=maxw, d=WINDOW_D)


# e / f. the two-stream shape of test_gpu_fill_edges.py with zero-width rows
TWO_STREAM_THRESHOLDS = [1, 40, 161]
OWNED = [0, 1, OT - 1, OT, OT + 1, 3000]
OWNED_THRESHOLDS = [0, 40]


@functools.lru_cache(maxsize=None)
def two_stream_case():
    """3000 x 3000 rows on one contig of 8000, widths below 160, 5 % of them
    zero: ~30 pairs per owner row in both streams"""
    rng = np.random.default_rng(79)
    A, B = random_sets(rng, 3000, 3000, n_contigs=1, contig_len=8000, max_len=160,
                       zero_frac=0.05, dup_frac=0.05, book_frac=0.05)
    return _case(A, B, 8000)


# g. u32 tile-local offsets: one owner tile with 1024 m pairs
PILE_M = [2**21 - 1, 2**21, 2**22 - 1, 2**22]


@functools.lru_cache(maxsize=4)
def pile_case(m):
    """A: 1024 identical rows [0, m + 1); B: m unit rows at starts 1 .. m.
    Every A row holds every B start: 1024 m pairs, all of one stream-0 owner
    tile; record p pairs owner p // m with partner p % m"""
    A = (np.zeros(OT, np.int32), np.zeros(OT, np.int64), np.full(OT, m + 1, np.int64))
    b_s = np.arange(1, m + 1, dtype=np.int64)
    B = (np.zeros(m, np.int32), b_s, b_s + 1)
    return _case(A, B, m + 9, m=m, pairs=OT * m)


def pile_records(m, first, count, flip):
    """records [first, first + count) of pile_case(m): (start, end, a_row,
    b_row) as a (count, 4) array"""
    p = np.arange(first, first + count, dtype=np.int64)
    owner, partner = p // m, p % m
    return np.stack([partner + 1, partner + 2, partner if flip else owner,
                     owner if flip else partner], axis=1)


def pile_windows(m):
    """(first, count) windows of 130 records: the start, an owner boundary,
    across 2^31 where the plan has it, the last records"""
    total = OT * m
    w = [(0, 130), (5 * m - 65, 130), (total - 130, 130)]
    if total > 2**31 + 65:
        w.append((2**31 - 65, 130))
    return w
