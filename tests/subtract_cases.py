"""Inputs planted on the staging capacities and dispatch switches of subtract
(lime_amd/csrc/subtract.hip), and those conditions restated in numpy --
shared by tests/test_subtract_cases.py (CPU: every case has the property it is
named for, the quoted source lines still stand, the comb's closed-form counts
are the oracle's) and tests/test_gpu_subtract_edges.py (the engine against the
oracle, record for record in output order, on the same inputs).

subtract_run takes one of five launches:
    t >= 1                               the walking k_subtract<_, false>
    t <= 0, ls                           k_sub_fused<true>   (local scan)
    t <= 0, !ls, runs * 64 >= na         k_sub_fused<false>  (merge scan)
    t <= 0, !ls, else                    k_sub_count_runs + k_subtract<true, true>,
                                         the sweeping <true, true, true> when
                                         total * 16 < nblk
and inside each, every LDS stage has a capacity with a global-memory form
behind it.  Each restatement below quotes the source line it restates
(SOURCE_LINES); the constants are read from the source (and from the
Makefile's HIPFLAGS where they override it).

The comb.  B is disjoint teeth [10 j, 10 j + 6) on one contig.  A left row at
tooth p is one of
    inside    [10 p + 1, 10 p + 5)          0 records in both modes
    crossing  [10 p + 2, 10 (p + m) + 2)    m records (set), 2 m (lime)
    gap       [10 p + 7, 10 p + 9)          1 record, no hit: (L, None)
so every tile's and block's record total is chosen row by row.  Exact copies
of a tooth lengthen a window of B without changing B's runs or any record but
its b_row; one zero-width B row far past A's last row sets has_zero_width,
which keeps subtract off the local-scan path without an environment variable.
Input rows of both sets are stored in a fixed shuffled order, so a_row and
b_row are not sorted positions.

Every builder is cached and returns read-only arrays.
"""
import functools
import math
import os
import re

import numpy as np

from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LIME, SET = oracle.SUB_LIME, oracle.SUB_SET
MODES = [LIME, SET]

# the source lines the restatements below stand for (regular expressions over
# lime_amd/csrc/subtract.hip)
SOURCE_LINES = {
    "SUB_B": r"constexpr int SUB_B = 256;",
    "TIE_G": r"constexpr int TIE_G = 16;",
    "CNT_WAVES": r"#ifndef LIME_SUB_CNT_WAVES\n#define LIME_SUB_CNT_WAVES 4\n",
    "CNT_WIN": r"#ifndef LIME_SUB_CNT_WIN\n#define LIME_SUB_CNT_WIN 1536\n",
    "CNT_ROWS": r"constexpr int CNT_ROWS = CNT_WAVES \* SUB_B;",
    "SCAP": r"constexpr int SCAP = 512;",
    "BWIN": r"constexpr int BWIN = 1024;",
    "FW": r"#ifndef LIME_SUB_FW\n#define LIME_SUB_FW 8\n",
    "FCAP": r"#ifndef LIME_SUB_FCAP\n#define LIME_SUB_FCAP \(112 \* LIME_SUB_FW\)\n",
    "FWIN": r"#ifndef LIME_SUB_FWIN\n#define LIME_SUB_FWIN \(384 \* LIME_SUB_FW\)\n",
    "FROWS": r"constexpr int FW = LIME_SUB_FW, FROWS = FW \* SUB_B, FWIN = LIME_SUB_FWIN;",
    # k_sub_window
    "window_key": r"const int64_t key = \(int64_t\)ags\[b \* SUB_B \* stride\] - maxw;",
    "window_hkey": r"wend \? \(int64_t\)ags\[min\(\(b \+ 1\) \* SUB_B \* stride, na\) - 1\] "
                   r"\+ maxwa",
    "window_search": r"if \(r \+ step <= nb && \(int64_t\)bgs\[r \+ step - 1\] < key\) "
                     r"r \+= step;\s*\n"
                     r"\s*if \(wend && h \+ step <= nb && \(int64_t\)bgs\[h \+ step - 1\] < hkey\) "
                     r"h \+= step;",
    "window_len": r"dev::wave_reduce_max\(\(uint32_t\)min\(h \+ 1 - r, \(int64_t\)0xffffffff\)\);",
    # subtract_run
    "runs": r"const bool runs = threshold <= 0 && B->n > 0 && B->strand_in == nullptr;",
    "ls_gate": r"if \(runs && !B->has_zero_width && !getenv\(\"LIME_SUB_NO_LS\"\)\) \{",
    "ls_tiles": r"const int64_t nt = blocks_for\(na, FROWS\);",
    "ls": r"ls = h_wm <= \(unsigned\)FWIN;",
    "fused": r"const bool fused = ls \|\| \(runs && mb\.n \* 64 >= na\);",
    "stride": r"const int stride = fused \? FW : inl \? CNT_WAVES : 1;",
    "sparse": r"sparse = runs && \(int64_t\)total \* 16 < nblk;",
    "nblk": r"const int64_t nblk = \(na \+ SUB_B - 1\) / SUB_B;",
    "cap": r"uint64_t cap = \(uint64_t\)na \+ 4096, total = 0;",
    "rerun": r"if \(total <= cap\) break;",
    "rerun_cap": r"cap = total;\s*\n\s*\}",
    # k_sub_fused
    "fused_nst": r"\(int\)min\(min\(\(int64_t\)FWIN, sa\.nb - wlo\),\s*\n"
                 r"\s*\(int64_t\)wend\[tile\] \+ 1 - wlo\)\);",
    "fused_staged": r"const bool staged = T <= \(uint64_t\)FCAP;",
    "fused_cap_staged": r"if \(at >= fa\.cap\) break;",
    "fused_cap_direct": r"\} else if \(at < fa\.cap\) \{",
    "fused_local": r"return !sa\.zw && \(blk < nst \|\| tail\) && "
                   r"\(a_e <= a_s \|\| bhk < nst \|\| tail\);",
    "fused_pack": r"v_b = __shfl\(\(uint32_t\)bl\[k\] \| \(uint32_t\)bh\[k\] << 16, src\);",
    # k_sub_count_runs
    "cnt_nst": r"const int nst = \(int\)min\(\(int64_t\)CNT_WIN, sa\.nb - wlo\);",
    "cnt_lo": r"int64_t lo1 = bl\[k\] < nst \? wlo \+ bl\[k\] : "
              r"dev::lower_bound\(sa\.bgs, whi, sa\.nb, \(int64_t\)a_s\);",
    "rcnt": r"sa\.rcnt\[base \+ k \* 64 \+ lane\] = \(uint8_t\)\(n_out < 255 \? n_out : 255\);",
    "rcnt_fold": r"n_out = rc < 255u \? rc : fold\(false\);",
    "bwlo_key": r"const int64_t key = max\(\(int64_t\)as\[0\] - \(int64_t\)sa\.maxw, "
                r"\(int64_t\)0\);",
    # sub_block
    "block_stage": r"const int cap = \(int\)min\(\(int64_t\)BWIN, sa\.nb - wlo\);",
    "block_stage_stop": r"nst = min\(k0 \+ SUB_B, cap\);\s*\n\s*__syncthreads\(\);\s*\n"
                        r"\s*if \(w_gs\[nst - 1\] >= amax\) break;",
    "block_whi": r"if \(i < sa\.na\) h = sa\.olo\[i\] \+ sa\.ocnt\[i\];",
    "block_win": r"const bool win = whi - wlo <= BWIN;",
    "walk_staged": r"staged = bend - bbase <= SCAP;",
    "runs_staged": r"staged = total <= \(uint64_t\)SCAP;",
    "skip_empty": r"if \(RUNS && WRITE && sa\.off\[blk \+ 1\] == sa\.off\[blk\]\) return;",
    # the same-start walks and the tie index
    "tie_walk_span": r"for \(; j < lo1 && j <= j0 \+ TIE_G && Bgs\(j\) == bs; \+\+j\) \{",
    "tie_walk_run": r"for \(; k < nx && k <= j \+ TIE_G && Bgs\(k\) == bs; \+\+k\) \{",
    "tie_walk_fused": r"for \(; q < nx && q <= j \+ TIE_G && gsf\(q\) == bs; \+\+q\) \{",
    "tie_defer": r"if \(sa\.tn < 0\)\s*\n\s*atomicOr\(sa\.err, 4u\);",
    "tie_rerun": r"if \(fe & 4u\) \{",
    "tie_small": r"if \(n <= TIE_G \|\| known == 0\) \{",
    "tie_detect_skip": r"if \(j \+ TIE_G >= n\) return;",
    "tie_detect_vector": r"if \(j \+ TIE_G \+ 4 <= n\) \{",
    "tie_detect_tail": r"for \(int64_t q = j; q \+ TIE_G < n && q < j \+ 4; \+\+q\) "
                       r"hit \|= gs\[q\] == gs\[q \+ TIE_G\];",
}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _source():
    return _read("lime_amd", "csrc", "subtract.hip")


def _macro(name):
    """value of the macro `name` in the library build: the Makefile's HIPFLAGS
    when they define it, else the source's #ifndef default"""
    flags = re.search(r"^HIPFLAGS\s*=((?:.*\\\n)*.*)$", _read("Makefile"), re.M).group(1)
    m = re.search(r"-D%s=(\S+)" % name, flags)
    text = m.group(1) if m else re.search(r"#ifndef %s\n#define %s ([^\n]+)\n" % (name, name),
                                          _source()).group(1)
    text = re.sub(r"LIME_SUB_\w+", lambda k: str(_macro(k.group(0))), text)
    assert re.fullmatch(r"[\d\s()*+]+", text), text
    return int(eval(text))  # (digits, parentheses, * and + only)


def _constexpr(name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, _source()).group(1))


SUB_B = _constexpr("SUB_B")
TIE_G = _constexpr("TIE_G")
SCAP = _constexpr("SCAP")
BWIN = _constexpr("BWIN")
CNT_WAVES = _macro("LIME_SUB_CNT_WAVES")
CNT_WIN = _macro("LIME_SUB_CNT_WIN")
CNT_ROWS = CNT_WAVES * SUB_B
FW = _macro("LIME_SUB_FW")
FCAP = _macro("LIME_SUB_FCAP")
FWIN = _macro("LIME_SUB_FWIN")
FROWS = FW * SUB_B
GUESS = int(re.search(r"uint64_t cap = \(uint64_t\)na \+ (\d+),", _source()).group(1))
RCNT_MAX = 255


# -------------------------------------------------------------- restatements
def canonical(X):
    """(gs, ge, order) of a set on one contig: (start, zero-width first, input
    row), the order test_sorted_set_order pins"""
    c, s, e = (np.asarray(x) for x in X)
    assert not c.any()
    order = np.lexsort((np.arange(len(s)), e > s, s))
    return s[order].astype(np.int64), e[order].astype(np.int64), order


def sorted_rows(A):
    """A's input rows in the engine's order (contig, start, zero-width first,
    row)"""
    c, s, e = (np.asarray(x) for x in A)
    return np.lexsort((np.arange(len(s)), e > s, s, c))


def expected_in_order(A, B, t, mode):
    """the oracle's records regrouped into the engine's output order: left
    rows in the set's sorted order, each row's records in the oracle's own
    order"""
    exp = oracle.subtract(A, B, t, mode)
    order = sorted_rows(A)
    pos = np.empty(len(order), np.int64)
    pos[order] = np.arange(len(order))
    k = np.argsort(pos[exp["a_row"]], kind="stable")
    return {key: np.ascontiguousarray(v[k]) for key, v in exp.items()}


def sub_windows(ags, bgs, stride, maxw_b, maxw_a):
    """k_sub_window, per tile of SUB_B * stride left rows: (start, end), both
    lower bounds among B's starts
        key  = ags[b * SUB_B * stride] - maxw
        hkey = ags[min((b + 1) * SUB_B * stride, na) - 1] + maxwa
    the window's length is end + 1 - start"""
    na, rows = len(ags), SUB_B * stride
    first = np.arange(0, na, rows)
    last = np.minimum(first + rows, na) - 1
    start = np.searchsorted(bgs, ags[first] - maxw_b, "left")
    end = np.searchsorted(bgs, ags[last] + maxw_a, "left")
    return start.astype(np.int64), end.astype(np.int64)


class Model:
    """subtract(A, B, t <= 0 or t >= 1) restated: the dispatch of subtract_run
    and the windows, stages and totals its launches see"""

    def __init__(self, A, B):
        self.A, self.B = A, B
        self.ags, self.age, self.aorder = canonical(A)
        self.bgs, self.bge, self.border = canonical(B)
        self.na, self.nb = len(self.ags), len(self.bgs)
        self.maxw_a = int((self.age - self.ags).max())
        self.maxw_b = int((self.bge - self.bgs).max())
        self.zw = bool((self.bge == self.bgs).any())
        # B's merge runs (mb.n): the oracle's merge
        self.runs = len(oracle.merge(B)["start"])
        # const int64_t nblk = (na + SUB_B - 1) / SUB_B;
        self.nblk = (self.na + SUB_B - 1) // SUB_B
        self.ntiles = (self.na + FROWS - 1) // FROWS
        self.tile_win = sub_windows(self.ags, self.bgs, FW, self.maxw_b, self.maxw_a)
        self.tile_wlen = self.tile_win[1] + 1 - self.tile_win[0]
        # ls = h_wm <= (unsigned)FWIN;  behind  runs && !B->has_zero_width
        self.ls = not self.zw and int(self.tile_wlen.max()) <= FWIN
        # largest same-start group of B
        _, cnt = np.unique(self.bgs, return_counts=True)
        self.max_group = int(cnt.max())

    def fused(self, no_ls=False):
        # const bool fused = ls || (runs && mb.n * 64 >= na);
        return (self.ls and not no_ls) or self.runs * 64 >= self.na

    def sparse(self, total):
        # sparse = runs && (int64_t)total * 16 < nblk;
        return total * 16 < self.nblk

    def path(self, t, total, no_ls=False):
        """the launch subtract_run takes"""
        if t >= 1:
            return "walk"
        if self.ls and not no_ls:
            return "fused_ls"
        if self.fused(no_ls):
            return "fused_scan"
        return "two_pass_sweep" if self.sparse(total) else "two_pass"

    def row_counts(self, exp):
        """records of every left row, in sorted order, from the oracle's
        result"""
        return np.bincount(exp["a_row"], minlength=self.na)[self.aorder].astype(np.int64)

    def totals(self, exp, rows):
        """record totals per `rows` sorted left rows (FROWS: a fused tile's T,
        SUB_B: a block's)"""
        return np.add.reduceat(self.row_counts(exp), np.arange(0, self.na, rows))

    # -- the fused pass
    def fused_stage(self, tile):
        """(wlo, nst) of k_sub_fused's tile: nst = min(FWIN, nb - wlo,
        wend + 1 - wlo)"""
        wlo, wend = int(self.tile_win[0][tile]), int(self.tile_win[1][tile])
        return wlo, min(FWIN, self.nb - wlo, wend + 1 - wlo)

    def _bounds(self, r0, r1, wlo, nst):
        w = self.bgs[wlo:wlo + nst]
        a_s, a_e = self.ags[r0:r1], self.age[r0:r1]
        return np.searchsorted(w, a_s, "left"), np.searchsorted(w, a_e, "left"), a_e > a_s

    def fused_bounds(self, tile):
        """(bl, bh, nst) of the tile's rows: lower bounds of a.s and a.e among
        the staged starts; a bound equal to nst lies past the stage"""
        wlo, nst = self.fused_stage(tile)
        bl, bh, wide = self._bounds(tile * FROWS, min((tile + 1) * FROWS, self.na), wlo, nst)
        return bl, np.where(wide, bh, bl), nst

    def fused_past_stage(self, tile):
        """rows of the tile that take the general fold on the merge-scan
        path: a bound at nst, unless the stage reaches B's end (tail)"""
        wlo, nst = self.fused_stage(tile)
        bl, bh, _ = self.fused_bounds(tile)
        if wlo + nst == self.nb:
            return 0
        return int(((bl == nst) | (bh == nst)).sum())

    # -- the two-pass side
    def count_windows(self):
        """k_sub_count_runs' workgroups (CNT_ROWS rows): (wlo, window length
        end + 1 - start of k_sub_window at stride CNT_WAVES)"""
        s, e = sub_windows(self.ags, self.bgs, CNT_WAVES, self.maxw_b, self.maxw_a)
        return s, e + 1 - s

    def count_past_stage(self, wg):
        """rows of the workgroup with a bound past its stage of nst =
        min(CNT_WIN, nb - wlo) rows"""
        wlo = int(self.count_windows()[0][wg])
        nst = min(CNT_WIN, self.nb - wlo)
        bl, bh, wide = self._bounds(wg * CNT_ROWS, min((wg + 1) * CNT_ROWS, self.na), wlo, nst)
        return int(((bl == nst) | (wide & (bh == nst))).sum())

    def runs_block_window(self, blk):
        """the runs write pass's block: (bwlo, rows needed = lb(amax) + 1 -
        bwlo, nst staged): staged SUB_B at a time up to BWIN until the last
        staged start reaches amax, the block's largest end"""
        r0, r1 = blk * SUB_B, min((blk + 1) * SUB_B, self.na)
        # key = max(as[0] - sa.maxw, 0)
        wlo = int(np.searchsorted(self.bgs, max(int(self.ags[r0]) - self.maxw_b, 0), "left"))
        amax = int(self.age[r0:r1].max())
        need = int(np.searchsorted(self.bgs, amax, "left")) + 1 - wlo
        cap = min(BWIN, self.nb - wlo)
        nst = 0
        for k0 in range(0, cap, SUB_B):
            nst = min(k0 + SUB_B, cap)
            if self.bgs[wlo + nst - 1] >= amax:
                break
        return wlo, need, nst

    def walk_block_window(self, blk, t):
        """the walking pass's block at threshold t >= 1: whi - wlo, with wlo
        k_sub_window's start at stride 1 and whi the largest olo + ocnt of its
        rows (owner_ranges, stream 0: lo = lb(a.s), hi = lb(a.e - tp + 1))"""
        assert t >= 1
        r0, r1 = blk * SUB_B, min((blk + 1) * SUB_B, self.na)
        wlo = int(np.searchsorted(self.bgs, int(self.ags[r0]) - self.maxw_b, "left"))
        lk, hk = self.ags[r0:r1], self.age[r0:r1] - t + 1
        lo = np.searchsorted(self.bgs, lk, "left")
        hi = np.where(hk > lk, np.searchsorted(self.bgs, hk, "left"), lo)
        return max(int(hi.max()), wlo) - wlo


# --------------------------------------------------------------------- cases
_CASES, _MODELS, _EXPECTED = {}, {}, {}


def _freeze(case):
    for v in case.values():
        for x in (v if isinstance(v, tuple) else (v,)):
            if isinstance(x, np.ndarray):
                x.flags.writeable = False
    return case


def _cached(fn):
    @functools.wraps(fn)
    def wrapper(*args):
        key = (fn.__name__,) + args
        if key not in _CASES:
            case = fn(*args)
            case["key"] = key
            _CASES[key] = _freeze(case)
        return _CASES[key]
    return wrapper


def model(case):
    if case["key"] not in _MODELS:
        _MODELS[case["key"]] = Model(case["A"], case["B"])
    return _MODELS[case["key"]]


def expected(case, t, mode):
    """expected_in_order of the case, computed once (read-only)"""
    key = (case["key"], t, mode)
    if key not in _EXPECTED:
        exp = expected_in_order(case["A"], case["B"], t, mode)
        for v in exp.values():
            v.flags.writeable = False
        _EXPECTED[key] = exp
    return _EXPECTED[key]


def _shuffle(n, salt):
    """a fixed permutation of range(n): k -> (k * P + salt) mod n"""
    p = next(q for q in (7919, 104729, 1299709, 15485863) if math.gcd(q, n) == 1) if n > 1 else 1
    return (np.arange(n, dtype=np.int64) * p + salt) % max(n, 1)


def comb(p, kind, n_teeth, copies=None, zw=False, first_tooth=0, group=None, wide_b=None,
         strict=True):
    """The comb (module docstring).  p, kind: per left row its tooth and
    -1 gap / 0 inside / m > 0 crossing m teeth, in the order wanted in the
    sorted set (rows at one tooth: inside, crossing, gap).  B: teeth
    first_tooth .. n_teeth - 1, tooth j in copies[j] exact copies; zw: one
    zero-width row far past everything; group = (G, g): tooth G replaced by g
    rows [10 G, 10 (G + i) + 6), i < g (one start, distinct ends); wide_b =
    (s, e): one more B row.  strict: every row's teeth exist and B is the
    plain comb, so the closed-form counts hold (case["closed"], per input
    row: [set, lime])."""
    p, kind = np.asarray(p, np.int64), np.asarray(kind, np.int64)
    na = len(p)
    off = np.where(kind < 0, 7, np.where(kind == 0, 1, 2))
    a_s = 10 * p + off
    a_e = np.where(kind < 0, 10 * p + 9, np.where(kind == 0, 10 * p + 5, 10 * (p + kind) + 2))
    assert (np.diff(a_s) >= 0).all(), "rows are given in sorted order"
    copies = np.ones(n_teeth, np.int64) if copies is None else np.asarray(copies, np.int64)
    assert len(copies) == n_teeth
    copies = copies.copy()
    copies[:first_tooth] = 0
    if group:
        copies[group[0]] = 0
    j = np.repeat(np.arange(n_teeth), copies)
    b_s, b_e = 10 * j, 10 * j + 6
    if group:
        G, g = group
        ends = 10 * (G + np.arange(g)) + 6
        b_s, b_e = np.concatenate([b_s, np.full(g, 10 * G)]), np.concatenate([b_e, ends])
    if wide_b:
        b_s, b_e = np.append(b_s, wide_b[0]), np.append(b_e, wide_b[1])
    top = int(max(a_e.max(), b_e.max() if len(b_e) else 0))
    if zw:
        z = top + 1000
        b_s, b_e = np.append(b_s, z), np.append(b_e, z)
        top = z
    plain = strict and not group and not wide_b
    if plain:
        assert (p >= first_tooth).all() and (p + np.maximum(kind, 0) < n_teeth).all()
    pa, pb = _shuffle(na, 5), _shuffle(len(b_s), 11)
    A = (np.zeros(na, np.int32), np.empty(na, np.int64), np.empty(na, np.int64))
    A[1][pa], A[2][pa] = a_s, a_e
    B = (np.zeros(len(b_s), np.int32), np.empty(len(b_s), np.int64), np.empty(len(b_s), np.int64))
    B[1][pb], B[2][pb] = b_s, b_e
    case = {"A": A, "B": B, "lens": [top + 100]}
    if plain:
        closed = np.empty((na, 2), np.int64)
        closed[pa, 0] = np.where(kind < 0, 1, kind)
        closed[pa, 1] = np.where(kind < 0, 1, 2 * kind)
        case["closed"] = closed
    return case


PATTERN = np.array([1, 0, -1, 0, 0, 2, 0, 0])    # 5 records (set) / 7 (lime) per 8 rows
PATTERN1 = np.array([1, 0, -1, 0, 0, 1, 0, 0])   # crossing one tooth at most


def _pattern(n, pat=PATTERN):
    return pat[np.arange(n) % len(pat)]


def _tooth_order(p, kind):
    """rows in sorted order: by tooth, at one tooth inside, crossing, gap
    (stable)"""
    return np.lexsort((np.where(kind < 0, 2, np.minimum(kind, 1)), p))


def kinds_for_total(n, total, mode):
    """kinds of n rows with `total` records in `mode`: crossing rows one tooth
    each (spread evenly) while they suffice, else every row crossing; an odd
    total in lime mode takes one gap row"""
    u = 2 if mode == LIME else 1
    g = total % u
    s = (total - g) // u  # teeth crossed in all
    kind = np.zeros(n, np.int64)
    if s + g <= n:
        at = (np.arange(s) * n) // max(s, 1)
        kind[at] = 1
        if g:
            kind[np.flatnonzero(kind == 0)[0]] = -1
    else:
        rows = n - g
        kind[:] = s // rows
        kind[(np.arange(s % rows) * rows) // max(s % rows, 1)] += 1
        if g:
            kind[n - 1] = -1
    assert np.where(kind < 0, 1, u * kind).sum() == total
    return kind


# a. the fused record stage (staged = T <= FCAP): one tile of 1024 rows with
# FCAP - 1 / FCAP / FCAP + 1 records; three tiles, the middle one FCAP + 1
STAGE_T = [FCAP - 1, FCAP, FCAP + 1]
STAGE3_T = [600, FCAP + 1, 300]


@_cached
def stage_case(total, mode, zw):
    kind = kinds_for_total(FROWS, total, mode)
    return comb(np.arange(FROWS), kind, FROWS + 3, zw=zw)


@_cached
def stage3_case(mode, zw):
    kind = np.concatenate([kinds_for_total(FROWS, t, mode) for t in STAGE3_T])
    return comb(np.arange(3 * FROWS), kind, 3 * FROWS + 3, zw=zw)


# b. the local-scan switch and the fused window: one tile whose window is W
# rows of B (first row at tooth 0, last at tooth W - 4, the widest row crossing
# 2 teeth: end = tooth W - 1, length W)
WINDOW_NA = 1024  # (one partial tile: a tile is FROWS = 2048 left rows)
WINDOW_W = [FWIN - 1, FWIN, FWIN + 1]
WINDOW_LONG = 4 * FWIN + 1015  # several times the stage


@_cached
def window_case(W, zw):
    pitch = -(-(W - 4) // (WINDOW_NA - 1))
    p = pitch * np.arange(WINDOW_NA)
    p[-1] = W - 4
    assert p[-1] > p[-2]
    kind = _pattern(WINDOW_NA)
    kind[-1] = 2  # (the widest: its own a.e bound is the window's last row)
    return comb(p, kind, W + 3, zw=zw)


@_cached
def ends_case(zw):
    """B starts at tooth 2: the first left row [1, 5) lies before every B row
    (a.s - maxw < 0), the second crosses into the first tooth; the last row
    at tooth FWIN - 1 crosses 2 teeth and ends past B's last start (tooth FWIN),
    so (without the zero-width row) the stage is all FWIN - 1 rows of B and the
    row's a.e bound is exactly nst"""
    p = 3 * np.arange(WINDOW_NA)
    kind = _pattern(WINDOW_NA)
    kind[0], kind[1], kind[-1] = 0, 1, 2
    p[1], p[-1] = 1, FWIN - 1
    return comb(p, kind, FWIN + 1, zw=zw, first_tooth=2, strict=False)


# c. partial and many tiles
TILE_NA = [1, 1023, 1024, 1025, FROWS - 1, FROWS, FROWS + 1]
MANY_NA = 40 * 1024 + 1  # 20 tiles of FROWS rows and one row more
# per tile: e empty, sN: N rows crossing one tooth (N records in set mode, 2 N
# in lime mode: s448 is FCAP exactly in lime mode, s449 one past it), u: every
# row crossing (2048 / 4096: unstaged in both modes)
MANY_PLAN = ["s100", "e", "e", "u", "s300", "u", "u", "e", "s448", "s449"] * 2


@_cached
def tiles_case(na, zw):
    return comb(np.arange(na), _pattern(na), na + 4, zw=zw)


@_cached
def many_tiles_case(zw):
    kinds = []
    for name in MANY_PLAN:
        k = np.zeros(FROWS, np.int64)
        if name == "u":
            k[:] = 1
        elif name != "e":
            n = int(name[1:])
            k[(np.arange(n) * FROWS) // n] = 1
        kinds.append(k)
    kinds.append(np.array([1]))  # the last tile: one row, one or two records
    kind = np.concatenate(kinds)
    assert len(kind) == MANY_NA
    return comb(np.arange(len(kind)), kind, len(kind) + 3, zw=zw)


# d. the output guess cap = na + GUESS: three tiles, na + GUESS + delta records;
# the last tile (the one straddling cap when delta > 0) staged or not
GUESS_NA = 3 * FROWS
GUESS_DELTA = [-1, 0, 1]
GUESS_LAST = {"staged": 700, "unstaged": 1500}


def guess_tile_totals(delta, last):
    total = GUESS_NA + GUESS + delta
    t = [3000, 0, GUESS_LAST[last]]
    t[1] = total - t[0] - t[2]
    return t


@_cached
def guess_case(delta, last, mode, zw):
    kind = np.concatenate([kinds_for_total(FROWS, t, mode)
                           for t in guess_tile_totals(delta, last)])
    return comb(np.arange(GUESS_NA), kind, GUESS_NA + 8, zw=zw)


# e. the switches of the two-pass side (B with its zero-width row): 128 left
# rows per tooth, so B's runs stay far below A's rows
PER_TOOTH = 128
SWITCH_NA = 4096
SWITCH_RUNS = [64, 63]        # runs * 64 >= na: 4096 / 4032
SPARSE_NA = [16 * SUB_B, 16 * SUB_B + 1]  # nblk 16 / 17, one record


@_cached
def switch_case(runs):
    p = np.arange(SWITCH_NA) // PER_TOOTH
    kind = _pattern(SWITCH_NA, PATTERN1)
    o = _tooth_order(p, kind)
    return comb(p[o], kind[o], runs - 1, zw=True)


@_cached
def sparse_case(na):
    kind = np.zeros(na, np.int64)
    kind[2000] = -1
    p = np.arange(na) // PER_TOOTH
    o = _tooth_order(p, kind)
    return comb(p[o], kind[o], 40, zw=True)


# f. the uint8 per-row count: one left row crossing m teeth
RCNT_M = [127, 128, 254, 255, 256, 300]
RCNT_ROW = PER_TOOTH + 2  # (block 0, tooth 1; rows with records follow it)


def rcnt_na(m):
    return 17408 if m <= 256 else 20480


@_cached
def rcnt_case(m):
    na = rcnt_na(m)
    p = np.arange(na) // PER_TOOTH
    kind = _pattern(na, np.array([0, 0, 1, 0, 0, -1, 0, 0]))
    assert kind[RCNT_ROW] == 1
    kind[RCNT_ROW] = m
    o = _tooth_order(p, kind)
    return comb(p[o], kind[o], max(m + 3, int(p[-1]) + 3), zw=True)


# g. the write passes' record stage: block 5's total SCAP - 1 / SCAP / SCAP + 1
SCAP_T = [SCAP - 1, SCAP, SCAP + 1]
SCAP_NA = 4096
SCAP_BLOCK = 5


@_cached
def scap_case(total, mode):
    p = np.arange(SCAP_NA) // PER_TOOTH
    kind = _pattern(SCAP_NA, PATTERN1)
    kind[(SCAP_BLOCK + 1) * SUB_B:(SCAP_BLOCK + 2) * SUB_B] = 0
    kind[SCAP_BLOCK * SUB_B:(SCAP_BLOCK + 1) * SUB_B] = kinds_for_total(SUB_B, total, mode)
    o = _tooth_order(p, kind)
    # (blocks are whole teeth: the reorder stays inside each block)
    return comb(p[o], kind[o], int(p[-1]) + 5, zw=True)


# h. the B-row stages of the two-pass side and of the walk
BWIN_SPAN = [BWIN, BWIN + 1]
BWIN_WALK_NA = 600


@_cached
def bwin_walk_case(span):
    """rows 4 teeth apart; block 0's last row (tooth 1020) crosses span - 1021
    teeth: its hit range ends at tooth span, whi - wlo = span"""
    p = 4 * np.arange(BWIN_WALK_NA)
    kind = _pattern(BWIN_WALK_NA)
    kind[SUB_B - 1] = span - (4 * (SUB_B - 1) + 1)
    return comb(p, kind, int(p[-1]) + 8)


BWIN_RUNS_NA = 5120
BWIN_RUNS_COPIES = [TIE_G - 1, TIE_G]  # block 0 needs BWIN / BWIN + 1 rows


@_cached
def bwin_runs_case(c):
    """teeth 0 .. 62 in 16 copies, tooth 63 in c: block 0 (teeth 0 and 1)
    holds a row crossing 62 teeth, whose end lies before tooth 64 at sorted
    index 1008 + c"""
    p = np.arange(BWIN_RUNS_NA) // PER_TOOTH
    kind = _pattern(BWIN_RUNS_NA, np.array([0, 0, 1, 0, 0, -1, 0, 0]))
    kind[PER_TOOTH + 2] = 62
    o = _tooth_order(p, kind)
    n_teeth = 70
    copies = np.ones(n_teeth, np.int64)
    copies[:63], copies[63] = TIE_G, c
    return comb(p[o], kind[o], n_teeth, copies=copies, zw=True)


CNT_WIN_COPIES = [TIE_G - 2, TIE_G - 1, TIE_G]  # CNT_WIN - 1 / CNT_WIN / CNT_WIN + 1
CNT_WIN_NA = CNT_ROWS + 88 * PER_TOOTH


@_cached
def cnt_win_case(c):
    """workgroup 0: 1024 rows on teeth 0 .. 63 (16 per tooth), the last one
    crossing 32 teeth (A's widest): its end, and the window's, at tooth 96;
    teeth 0 .. 94 in 16 copies and tooth 95 in c: 1521 + c rows"""
    k = np.arange(CNT_WIN_NA)
    p = np.where(k < CNT_ROWS, k // 16, 64 + (k - CNT_ROWS) // PER_TOOTH)
    kind = _pattern(CNT_WIN_NA, PATTERN1)
    kind[CNT_ROWS - 16:CNT_ROWS] = 0  # (tooth 63: the workgroup's last sorted row is the wide one)
    kind[CNT_ROWS - 1] = 32
    o = _tooth_order(p, kind)
    n_teeth = int(p[-1]) + 34
    copies = np.ones(n_teeth, np.int64)
    copies[:95], copies[95] = TIE_G, c
    return comb(p[o], kind[o], n_teeth, copies=copies, zw=True)


CNT_WIDE_Q = 2000


@_cached
def cnt_wide_case():
    """one B row [15, 10 Q + 8) early in the set: B's max width reaches back
    to it from every left row below tooth Q, so those workgroups' windows start
    at it and their staged rows end far before the rows' own bounds; it merges
    teeth 1 .. Q into one run"""
    q = CNT_WIDE_Q
    na = 4 * (q + 64)
    p = np.arange(na) // 4
    kind = _pattern(na)
    o = _tooth_order(p, kind)
    return comb(p[o], kind[o], q + 64 + 4, zw=True, wide_b=(15, 10 * q + 8))


# i. the tie index: one same-start group of g rows of B
TIE_SIZES = [TIE_G, TIE_G + 1, TIE_G + 2]
TIE_PLACES = ["mid", "last0", "last1", "last2", "last3", "whole"]


def tie_tooth(g, place):
    if place == "mid":
        return 600
    if place == "whole":
        return 5
    r = int(place[-1])
    return 600 + (r - 600 - g) % 4  # B = teeth 0 .. G - 1 and the group: (G + g) % 4 == r


@_cached
def tie_case(g, place):
    """the group at tooth G: rows [10 G, 10 (G + i) + 6), i < g, in shuffled
    input order.  The left row at tooth p in G + 1 .. G + g - 1 starts under
    the group's rows i >= p - G only and ends two teeth past the group: its
    spanning block's head is row p - G (the one ending first past the left
    row's start, not the group's first row).  The left rows at teeth G - 2 and
    G - 1 cross into the group: it is an inside block's head there (row 0).
    mid: teeth on both sides; lastR: the group is B's last g rows and
    len(B) % 4 == R; whole: B is the group"""
    G = tie_tooth(g, place)
    na = 1300 if place == "mid" else G + 40
    n_teeth = 1304 if place == "mid" else G + 1
    first = G if place == "whole" else 0
    kind = _pattern(na)
    kind[G + 1:G + g] = G + g + 1 - np.arange(G + 1, G + g)  # spanned, ending past the group
    kind[G - 2], kind[G - 1] = 3, 2                          # crossing into the group
    return comb(np.arange(na), kind, n_teeth, first_tooth=first, group=(G, g), strict=False)
