"""Inputs that plant rows on the tile, wave and round edges of the merge
scans, the same-start (tie) flag and the prefix max -- pure numpy, shared by
tests/test_scan_cases.py (CPU: the builders against the oracle and the fold
below) and tests/test_gpu_scan_edges.py (the engine against both).

Geometry (asserted against the kernel sources by test_scan_cases.py, so a
retune fails loudly instead of moving every planted row off its edge):

  k_merge_scan2 (plain sets)     round R = 256 rows (64 lanes x 4), wave
                                 W = LIME_MS2_Q x 256 = 2048, tile
                                 T = LIME_MS2_NT / 64 x W = 32768
  k_merge_scan<true> (stranded)  tile ST = LIME_MERGE_SB x MITEMS = 16384,
                                 thread = MITEMS = 16 rows, wave = 1024 rows
  k_prefix_max                   tile PT = MB x MITEMS = 4096; k_scan_max
                                 takes MB = 256 tile maxima per iteration
  TIE_G / MERGE_TIE_G            G = 16

Every builder is cached and returns read-only arrays: a case is built once
per process and shared by the tests that use it.
"""
import functools

import numpy as np

R, W, T = 256, 2048, 32768
ST = 16384
PT = 4096
G = 16

N_BASE = 3 * T + 5  # A.1 / B.2 staircase rows (= 6 ST + 5)

# strand codes: 0 independent, 1 forward, 2 reverse, 3 unknown; RegionOrdering
# compares the enum ordinal FORWARD < REVERSE < INDEPENDENT < UNKNOWN
STRAND_ORD = np.array([2, 0, 1, 3], np.int64)


# ------------------------------------------------------------ references
def fold(contig, start, end, strand=None):
    """The merge fold restated: rows in (contig, start, end, strand ordinal,
    input row) order, a running hull; a row opens a new run unless it has the
    hull's contig and strand and strictly overlaps it (book-ended rows do
    not merge).  -> {"contig", "start", "end", "strand"} per run and
    "run_of_row" per input row."""
    contig = np.asarray(contig, np.int64)
    start = np.asarray(start, np.int64)
    end = np.asarray(end, np.int64)
    n = len(contig)
    code = np.zeros(n, np.int64) if strand is None else np.asarray(strand, np.int64)
    order = np.lexsort((np.arange(n), STRAND_ORD[code], end, start, contig))
    rc, rs, re_, rt = [], [], [], []
    rid = [0] * n
    hc = hs = he = ht = None
    k = 0
    for c, s, e, t in zip(contig[order].tolist(), start[order].tolist(), end[order].tolist(),
                          code[order].tolist()):
        if hc == c and ht == t and s < he and e > hs:
            if e > he:
                he = e
        else:
            if hc is not None:
                rc.append(hc), rs.append(hs), re_.append(he), rt.append(ht)
            hc, hs, he, ht = c, s, e, t
        rid[k] = len(rc)
        k += 1
    if hc is not None:
        rc.append(hc), rs.append(hs), re_.append(he), rt.append(ht)
    run_of_row = np.zeros(n, np.int64)
    run_of_row[order] = rid
    return {"contig": np.array(rc, np.int64), "start": np.array(rs, np.int64),
            "end": np.array(re_, np.int64), "strand": np.array(rt, np.int64),
            "run_of_row": run_of_row}


def device_order_plain(contig, start, end):
    """input rows in a plain set's device order: (global start -- contig,
    start --, zero-width first, input row)"""
    n = len(contig)
    return np.lexsort((np.arange(n), np.asarray(end) > np.asarray(start), start, contig))


def device_order_stranded(contig, start, end, strand):
    """input rows in a stranded set's device order: (contig, start, end,
    strand ordinal, input row)"""
    n = len(contig)
    return np.lexsort((np.arange(n), STRAND_ORD[np.asarray(strand, np.int64)], end, start,
                       contig))


# ------------------------------------------------------------- plumbing
def _freeze(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return case


def _staircase(n):
    s = 4 * np.arange(n, dtype=np.int64)
    return s, s + 2


def _shuffled(seed, lens, s, e, strand=None, contig=None, **extra):
    """A case from rows given in device order with all-distinct sort keys:
    shuffled (seeded); "row_sorted"[k] = the input row at sorted index k."""
    n = len(s)
    perm = np.random.default_rng(seed).permutation(n)  # input row j = sorted row perm[j]
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    case = {"contig": (np.zeros(n, np.int32) if contig is None else contig[perm].astype(np.int32)),
            "start": s[perm].copy(), "end": e[perm].copy(), "lens": list(lens),
            "row_sorted": inv}
    if strand is not None:
        case["strand"] = strand[perm].astype(np.int8)
    case.update(extra)
    return _freeze(case)


def rows(case):
    """(contig, start, end[, strand]) as the engine and the oracle take them"""
    t = (case["contig"], case["start"], case["end"])
    return t + (case["strand"],) if "strand" in case else t


# ------------------------------------------------ A. plain merge, planted
PLAIN_KINDS = ("bookend", "one_base", "zw_bookend", "zw_inside")
PLAIN_DELTAS = (-1, 0, 1)
# runs of a planted staircase: every planted hull swallows rows p-39 .. p-1,
# and row p too unless it is book-ended (6 planted rows)
PLAIN_RUNS = {"bookend": N_BASE - 6 * 39, "zw_bookend": N_BASE - 6 * 39,
              "one_base": N_BASE - 6 * 40, "zw_inside": N_BASE - 6 * 40}


def plain_edges(delta):
    n = N_BASE
    return [x + delta for x in (R, W, T, 2 * T, 2 * T + W)] + [n - 1]


@functools.lru_cache(maxsize=None)
def plain_base():
    """A.1: one contig, s_k = 4 k, e_k = s_k + 2 -- every row its own run"""
    s, e = _staircase(N_BASE)
    return _shuffled(100, [4 * N_BASE + 8], s, e)


@functools.lru_cache(maxsize=None)
def plain_planted(kind, delta):
    """A.2: the staircase with, for every edge row p, row p - 40 stretched to
    end at s[p] (bookend, zw_bookend: row p starts a run) or at s[p] + 1
    (one_base, zw_inside: row p merges); zw_*: row p zero-width.  "edges":
    the rows p; "edge_starts_run": what the oracle must say of them."""
    n = N_BASE
    s, e = _staircase(n)
    ps = plain_edges(delta)
    for p in ps:
        e[p - 40] = s[p] + (1 if kind in ("one_base", "zw_inside") else 0)
        if kind.startswith("zw_"):
            e[p] = s[p]
    return _shuffled(200 + 10 * PLAIN_KINDS.index(kind) + delta, [4 * n + 8], s, e,
                     edges=np.array(ps), edge_starts_run=kind in ("bookend", "zw_bookend"))


PLAIN_SHAPES = ("umbrella", "one_run", "random_dense")
PLAIN_SHAPE_N = (T, T + 1, 2 * T, 2 * T + 1, 3 * T - 1)


@functools.lru_cache(maxsize=None)
def plain_shape(shape, n):
    """A.3.  umbrella: e[7] = s[2 T + T / 2] (where the set is shorter: its
    row n - 3) -- the carry exceeds every local maximum of the tiles under
    it; one_run: e = s + 5, one run (the result's copy path: runs * 2 <= n);
    random_dense: starts U[0, 4 n), widths U[0, 8), 10 % zero-width"""
    if shape == "random_dense":
        rng = np.random.default_rng(300 + n)
        s = rng.integers(0, 4 * n, n).astype(np.int64)
        ln = rng.integers(0, 8, n).astype(np.int64)
        ln[rng.random(n) < 0.1] = 0
        return _freeze({"contig": np.zeros(n, np.int32), "start": s, "end": s + ln,
                        "lens": [4 * n + 8]})
    s, e = _staircase(n)
    if shape == "umbrella":
        e[7] = s[min(2 * T + T // 2, n - 3)]
    elif shape == "one_run":
        e = s + 5
    else:
        raise ValueError(shape)
    return _shuffled(310 + n, [4 * n + 8], s, e)


CONTIG_EDGE_ROWS = (T, W, 777)


@functools.lru_cache(maxsize=None)
def plain_contig_edges():
    """A.4: contig 0 holds exactly T rows and contig 1 exactly W, so contig
    1 opens on a tile edge and contig 2 on a wave edge; the last row of each
    contig ends at the contig's length and the next contig's first row starts
    at 0: one base (the pad between contigs) apart in global coordinates"""
    rng = np.random.default_rng(400)
    cs, ss, es, lens = [], [], [], []
    for c, m in enumerate(CONTIG_EDGE_ROWS):
        L = 4 * m + 8
        s = np.sort(rng.integers(1, 4 * m, m)).astype(np.int64)
        e = s + rng.integers(0, 8, m)
        s[0], e[0] = 0, 3
        s[m - 1], e[m - 1] = 4 * m + 2, L  # past every other start: sorted last
        cs.append(np.full(m, c)), ss.append(s), es.append(e), lens.append(L)
    c, s, e = np.concatenate(cs), np.concatenate(ss), np.concatenate(es)
    perm = rng.permutation(len(s))
    return _freeze({"contig": c[perm].astype(np.int32), "start": s[perm], "end": e[perm],
                    "lens": lens})


# --------------------------------------------------- B. stranded merge
STRETCH = 20000  # "stretches": one strand per STRETCH consecutive sorted rows
_STRETCH_CODES = np.array([1, 2, 0, 3], np.int8)
STRANDED_N = (ST, ST + 1, 2 * ST, 3 * ST + 5)
STRANDED_WIDTHS = (255, 256, 65535, 65536, (1 << 24) + 5)


@functools.lru_cache(maxsize=None)
def stranded_random(n, strands, wmax=0):
    """B.1 / B.4: three contigs, starts dense enough for many (start, end)
    ties across strands, widths U[0, 8).  strands: "uniform" (codes U{0..3}),
    "stretches", "equal" (the sort skips its strand pass).  wmax > 0: 2 % of
    the rows get widths U[0, wmax] and one row exactly wmax (the sort's
    width-digit passes: 1 digit up to 255, 2 up to 65535, 3, 4)."""
    rng = np.random.default_rng(500 + n + wmax % 1000 + len(strands))
    L = max(n // 2, wmax + 16)
    c = rng.integers(0, 3, n).astype(np.int32)
    s = rng.integers(0, n // 2 - 8, n).astype(np.int64)
    ln = rng.integers(0, 8, n).astype(np.int64)
    if wmax:
        k = rng.random(n) < 0.02
        ln[k] = rng.integers(0, wmax + 1, int(k.sum()))
        ln[n // 2] = wmax
    s = np.minimum(s, L - ln)
    e = s + ln
    if strands == "uniform":
        st = rng.integers(0, 4, n).astype(np.int8)
    elif strands == "equal":
        st = np.ones(n, np.int8)
    elif strands == "stretches":
        order = np.lexsort((np.arange(n), e, s, c))
        st = np.empty(n, np.int8)
        st[order] = _STRETCH_CODES[(np.arange(n) // STRETCH) % 4]
    else:
        raise ValueError(strands)
    return _freeze({"contig": c, "start": s, "end": e, "strand": st, "lens": [L, L, L],
                    "max_width": int(ln.max())})


STRANDED_SINGLE_AT = (ST, ST - 1, 2 * ST, 16 * 3, 1024 * 3)


@functools.lru_cache(maxsize=None)
def stranded_planted(kind, p=0):
    """B.2: the A.1 staircase, all rows strand 1, and
    single:       row p strand 2, under a hull e[p - 3] = s[p + 3] + 1 that it
                  cuts (rows p-3..p-1 | p | p+1.. each on their own again: the
                  hull must not resume when the strand returns)
    umbrella_cut: e[5] = s[p + ST + 100] + 1 over the tile edges up to one past
                  row p, cut by a strand-2 row at p (ST unless given): the
                  tile holding p must pass on its maximum since p only
    umbrella:     the same umbrella, no strand change: one run over 2 tiles,
                  carried through tiles that hold no segment start
    alternate:    strands alternate row by row under e = s + 6 (neighbours
                  overlap, yet every row is its own run)"""
    n = N_BASE
    s, e = _staircase(n)
    st = np.ones(n, np.int8)
    if kind == "umbrella_cut":
        p = p or ST
        e[5] = s[p + ST + 100] + 1
        st[p] = 2
        n_runs = n - (p - 1 - 5)  # rows 5 .. p - 1 one run
    elif kind == "single":
        st[p] = 2
        e[p - 3] = s[p + 3] + 1
        n_runs = n - 2  # p-3..p-1 one run, every other row its own
    elif kind == "umbrella":
        e[5] = s[2 * ST + 100] + 1
        n_runs = n - (2 * ST + 100 - 5)  # rows 5 .. 2 ST + 100 one run
    elif kind == "alternate":
        st = (1 + np.arange(n) % 2).astype(np.int8)
        e = s + 6
        n_runs = n
    else:
        raise ValueError(kind)
    return _shuffled(600 + p % 997 + len(kind), [4 * n + 8], s, e, strand=st, n_runs=n_runs)


MANY_TILES_N = 66 * ST + 3
MANY_TILES_UMBRELLAS = ((3 * ST + 11, 5), (10 * ST - 1, 40), (52 * ST + 100, 13))  # (row, tiles)
# (row, rows reached): umbrellas left to the stretches, which cut them
MANY_TILES_CUT = ((100, 2 * ST + 5000), (8 * ST + 200, ST + 10000), (50 * ST + 500, ST + 5000))


@functools.lru_cache(maxsize=None)
def stranded_many_tiles():
    """B.3: 66 ST + 3 staircase rows (more tiles than one 64-wide look-back
    window), "stretches" strands, and umbrellas of 5, 40 and 13 tiles whose
    rows all take the strand of the umbrella's first row -- the tiles under
    an umbrella hold no segment start and carry its end along -- and three
    more that the next stretch cuts: the rows after the cut are their own
    runs again, also in the tiles that follow"""
    n = MANY_TILES_N
    s, e = _staircase(n)
    st = _STRETCH_CODES[(np.arange(n) // STRETCH) % 4].copy()
    for a, m in MANY_TILES_UMBRELLAS:
        b = a + m * ST + 7
        e[a] = s[b] + 1
        st[a:b + 1] = st[a]
    for a, m in MANY_TILES_CUT:
        e[a] = s[a + m] + 1
    return _shuffled(700, [4 * n + 8], s, e, strand=st)


# -------------------------------------- C. the same-start flag (subtract)
SUB_NB = 2 * T + 4096
SUB_NA = 6000
SUB_SHAPES = ("sparse", "chained")
SUB_G = 18
# group starts i whose rows i and i + 1 (the two rows with gs[j] == gs[j + G]
# in a group of 18) both lie in the rows 240..255 (mod 256) of lanes 60-63
SUB_AT_ROUND = tuple(2 * W + 3 * R + x for x in (240, 247, 254))      # round 3 of wave 2
SUB_AT_WAVE = tuple(3 * W + x for x in (2032, 2039, 2046))            # -> the next wave's rows
SUB_AT_TILE = tuple(t * T + x for t in (0, 1) for x in (32752, 32759, 32766))  # -> next tile
SUB_AT_LAST = SUB_NB - SUB_G                                          # ends on the last row
SUB_AT_PLAIN = 40000
SUB_POSITIONS = (tuple((i, SUB_G) for i in SUB_AT_ROUND + SUB_AT_WAVE + SUB_AT_TILE +
                       (SUB_AT_LAST, SUB_AT_PLAIN)) + ((T - 7, 17), (T - 7, 16)))


@functools.lru_cache(maxsize=None)
def subtract_b(shape, i, g, planted=True, nb=SUB_NB):
    """C.1 / C.2: nb rows on one contig, starts 10 k (sorted index == k), and
    one group of g rows sharing start 10 i at sorted indices i .. i + g - 1,
    ends 10 i + 5000 -- but (planted) the group's row of the largest input
    position ends at 10 i + 2000: the head of every block the group opens,
    last of the group in device order, out of a 17-row walk's reach when
    g >= 18.  sparse: the other rows 3 wide (~nb runs); chained: 25 wide and
    chaining, except rows k % 3000 >= 2997 and i - 3 .. i - 1 (3 wide)."""
    k = np.arange(nb, dtype=np.int64)
    s = 10 * k
    if shape == "sparse":
        e = s + 3
    elif shape == "chained":
        e = s + 25
        narrow = k % 3000 >= 2997
        narrow[i - 3:i] = True
        e[narrow] = s[narrow] + 3
    else:
        raise ValueError(shape)
    s[i:i + g] = 10 * i
    e[i:i + g] = 10 * i + 5000
    perm = np.random.default_rng(800 + i + g).permutation(nb)
    inv = np.empty(nb, np.int64)
    inv[perm] = k
    s_in, e_in = s[perm].copy(), e[perm].copy()
    grp = np.sort(inv[i:i + g])  # the group's input rows, in device order
    if planted:
        e_in[grp[-1]] = 10 * i + 2000
    row_sorted = inv.copy()
    row_sorted[i:i + g] = grp
    return _freeze({"contig": np.zeros(nb, np.int32), "start": s_in, "end": e_in,
                    "lens": [10 * nb + 6000], "row_sorted": row_sorted,
                    "planted_row": int(grp[-1])})


@functools.lru_cache(maxsize=None)
def subtract_a(i, nb=SUB_NB):
    """C.3: 6000 rows of width U[1, 3000): 5400 uniform over the contig, 600
    starting within [10 i - 2500, 10 i + 5500)"""
    rng = np.random.default_rng(900 + i)
    L = 10 * nb + 6000
    s = np.concatenate([rng.integers(0, L - 3000, SUB_NA - 600),
                        rng.integers(10 * i - 2500, 10 * i + 5500, 600)]).astype(np.int64)
    s = np.clip(s, 0, L - 3000)
    e = s + rng.integers(1, 3000, SUB_NA)
    return _freeze({"contig": np.zeros(SUB_NA, np.int32), "start": s, "end": e, "lens": [L]})


# subtract's LS path (k_sub_fused<true>): B without zero-width rows and every
# fused tile (FW x SUB_B = 2048 left rows) with a window of B of at most FWIN
# = 3072 rows.  subtract_a's 6000 rows lie 700k bases wide over a B with a row
# every 10 bases (windows of ~27,000 rows): they never take it.
SUB_FROWS, SUB_FWIN = 2048, 3072
SUB_NA_LS = 3000


@functools.lru_cache(maxsize=None)
def subtract_a_ls(i, nb=SUB_NB):
    """Left rows that keep subtract on its LS path against subtract_b: 3000
    rows (two fused tiles) of width U[1, 3000) starting within
    [10 i - 8000, 10 i + 10000) -- 18k bases of starts, + B's widest row
    (5000) + the widest left row (< 3000) = under 2600 rows of B per window"""
    rng = np.random.default_rng(950 + i)
    L = 10 * nb + 6000
    s = np.clip(rng.integers(10 * i - 8000, 10 * i + 10000, SUB_NA_LS), 0, L - 3000)
    e = s + rng.integers(1, 3000, SUB_NA_LS)
    return _freeze({"contig": np.zeros(SUB_NA_LS, np.int32), "start": s.astype(np.int64),
                    "end": e.astype(np.int64), "lens": [L]})


def sub_window_max(a, b):
    """k_sub_window restated for one-contig sets: the longest window of B
    over the fused tiles of A's sorted rows.  A tile's window runs from the
    first row of B starting at or past (tile's first start - B's max width)
    to the first starting at or past (tile's last start + A's max width),
    that row included; LS needs the longest <= SUB_FWIN"""
    ags, bgs = np.sort(a["start"]), np.sort(b["start"])
    maxw = int((b["end"] - b["start"]).max())
    maxwa = int((a["end"] - a["start"]).max())
    t = np.arange((len(ags) + SUB_FROWS - 1) // SUB_FROWS)
    first = ags[t * SUB_FROWS]
    last = ags[np.minimum((t + 1) * SUB_FROWS, len(ags)) - 1]
    r = np.searchsorted(bgs, first - maxw, "left")
    h = np.searchsorted(bgs, last + maxwa, "left")
    return int((h + 1 - r).max())


# ------------------------------------------------------ D. prefix max
PMAX_N = (2 * T + W + 5, 257 * PT + 9)
# (rows, long rows): the two sets of D.1, and both sizes without long rows
PMAX_CASES = tuple((n, long_rows) for long_rows in (True, False) for n in PMAX_N)


@functools.lru_cache(maxsize=None)
def prefix_case(n, long_rows=True):
    """D.1: random_dense on one contig, plus (long_rows) 1 % long rows of up
    to 200k bases.  With long rows the prefix max is a staircase of a few
    hundred steps; without them it moves on every other row, which pins the
    array row by row.  The set of 257 tiles (of PT rows) also gets two
    planted running maxima: a row inside tile 3 reaching 300k bases past the
    start of sorted row 256 PT + 2000 -- the tile maxima's scan must carry it
    from its first 256-tile iteration into the second -- and a row after that
    one reaching the contig's end.  "planted": their sorted indices."""
    rng = np.random.default_rng(1000 + n % 1000 + int(long_rows))
    L = 4 * n + 600_000
    s = rng.integers(0, 4 * n, n).astype(np.int64)
    ln = rng.integers(0, 8, n).astype(np.int64)
    ln[rng.random(n) < 0.1] = 0
    if long_rows:
        k = rng.random(n) < 0.01
        ln[k] = rng.integers(1, 200_001, int(k.sum()))
    e = s + ln
    planted = []
    if n > 256 * PT + 4000:
        order = device_order_plain(np.zeros(n, np.int64), s, e)
        t1 = 256 * PT + 2000
        # (no long row of tile 256's own before the second maximum: up to
        # there the tile's rows lie under the carried maximum alone)
        own = order[256 * PT:t1 + 1000]
        own = own[e[own] - s[own] > 8]
        e[own] = s[own] + 1 + (e[own] - s[own]) % 7
        for q, reach in ((3 * PT + 100, s[order[t1]] + 300_000), (t1 + 1000, L)):
            while e[order[q]] == s[order[q]]:  # (a zero-width row would change places)
                q += 1
            e[order[q]] = reach
            planted.append(q)
    return _freeze({"contig": np.zeros(n, np.int32), "start": s, "end": e, "lens": [L],
                    "planted": np.array(planted, np.int64)})


@functools.lru_cache(maxsize=None)
def prefix_probe_rows(n, long_rows=True):
    """Left rows for a subtract against prefix_case(n, long_rows) as B: the
    spanning-hit test reads B's prefix max at the row before each left row's
    start, which first_reachings' binary searches never do where the array
    is too low on the right of their answer (a lost carry).  Widths
    U[1, 3000); 3000 rows over the contig and 1000 starting among B's last
    2 PT sorted rows -- under the planted maxima 200 and 300 (with long rows
    30 and 30) starting among sorted rows 256 PT - 200 .. 256 PT + 2900 (the
    oracle's sweep keeps every row under a spanning one cached: its cost
    there goes with the left rows)."""
    b = prefix_case(n, long_rows)
    rng = np.random.default_rng(1100 + n % 1000 + int(long_rows))
    bs = np.sort(b["start"])
    if len(b["planted"]):
        k, m, lo, hi = 200, 300, 256 * PT - 200, 256 * PT + 2900
        if long_rows:  # (hundreds of long rows cached besides: fewer still)
            k, m = 30, 30
    else:
        k, m, lo, hi = 3000, 1000, n - 2 * PT, n - 1
    s = np.concatenate([rng.integers(0, 4 * n, k), rng.integers(bs[lo], bs[hi], m)])
    e = s + rng.integers(1, 3000, len(s))
    return _freeze({"contig": np.zeros(len(s), np.int32), "start": s.astype(np.int64),
                    "end": e.astype(np.int64), "lens": b["lens"]})


def reaching_keys(pm, limit=20000):
    """D.2: the keys that pin a prefix max through upper_bound: every value
    of pm and that value - 1, 0 and 2^32 - 1; past `limit` keys thinned
    evenly, keeping the values at the sorted indices k PT - 1, k PT, k T - 1
    and k T (the rows either side of every tile edge)"""
    pm = np.asarray(pm, np.int64)
    u = np.unique(pm)
    ends = np.array([0, 2**32 - 1], np.int64)
    keys = np.unique(np.concatenate([u, u[u > 0] - 1, ends]))
    if len(keys) > limit:
        idx = np.concatenate([np.arange(PT, len(pm), PT), np.arange(T, len(pm), T)])
        idx = np.unique(np.concatenate([idx, idx - 1]))
        must = pm[idx]
        must = np.unique(np.concatenate([must, must[must > 0] - 1, ends]))
        thin = keys[np.linspace(0, len(keys) - 1, limit - len(must)).astype(np.int64)]
        keys = np.unique(np.concatenate([thin, must]))
    return keys


# ------------------------------------------------------- the case lists
# (id, builder, arguments): what both test modules parametrise over
PLAIN_CASES = (
    [("base", plain_base, ())] +
    [(f"{k}{d:+d}", plain_planted, (k, d)) for k in PLAIN_KINDS for d in PLAIN_DELTAS] +
    [(f"{sh}-{n}", plain_shape, (sh, n)) for sh in PLAIN_SHAPES for n in PLAIN_SHAPE_N] +
    [("contig_edges", plain_contig_edges, ())])
STRANDED_CASES = (
    [(f"{st}-{n}", stranded_random, (n, st)) for st in ("uniform", "stretches")
     for n in STRANDED_N] +
    [(f"width-{w}", stranded_random, (3 * ST + 5, "uniform", w)) for w in STRANDED_WIDTHS] +
    [("equal", stranded_random, (3 * ST + 5, "equal"))] +
    [(f"single-{p}", stranded_planted, ("single", p)) for p in STRANDED_SINGLE_AT] +
    [(k, stranded_planted, (k,)) for k in ("umbrella_cut", "umbrella", "alternate")] +
    [("umbrella_cut-mid", stranded_planted, ("umbrella_cut", 2 * ST + 50))])


def case_by_id(cases, cid):
    for i, fn, args in cases:
        if i == cid:
            return fn(*args)
    raise KeyError(cid)
