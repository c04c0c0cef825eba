"""Reference and planted inputs of lime_annotate, shared by
test_annotate_cases.py (CPU) and test_gpu_annotate.py (GPU).

`annotate_ref` works from the DEFINITION, independent of the kernel's closed
forms: for every row a of A, under the strict half-open predicate
b.start < a.end and b.end > a.start on the same contig,

    n_hits(a)        = the rows b of B that hit a
    covered(a)       = the bases of a inside the union of B
    overlap_bases(a) = the sum over the hits of min(ends) - max(starts)

n_hits and overlap_bases come from a chunked boolean mask of A's rows against
all of B; where the mask would pass MASK_CELLS cells, from the oracle's
intersect pairs reduced by a_row (A taken in chunks, so the pair records stay
small).  covered comes from a per-base paint of the union of B on every
contig (small genomes only).

`closed_forms` is a numpy transcription of what the kernel computes (sorted
starts and ends, their prefix sums, the merge runs and the prefix of their
widths, in global coordinates); the CPU test holds it against annotate_ref.

The planted cases place rows against the kernel's tiling: k_annotate takes T
rows of A (in sorted order) per workgroup and stages the windows of B's sorted
starts, sorted ends and run starts that the tile's starts can fall into -- from
the position of the tile's first start to that of the next tile's first start
(the last tile: of A's last start) -- in LDS when a window holds at most W
entries, and searches it in global memory otherwise.
"""
import os
import re

import numpy as np

from tests.coverage_cases import random_case

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lime_amd",
                    "csrc", "annotate.hip")


def kernel_constants():
    """AN_TILE (rows of A per tile) and AN_W (entries of a staged window) as
    lime_amd/csrc/annotate.hip defines them"""
    src = open(_SRC).read()
    val = {}
    for name in ("ANB", "AN_ITEMS", "AN_W"):
        m = re.search(r"constexpr int %s = (\d+);" % name, src)
        val[name] = int(m.group(1))
    assert re.search(r"constexpr int AN_TILE = ANB \* AN_ITEMS;", src)
    return val["ANB"] * val["AN_ITEMS"], val["AN_W"]


T, W = kernel_constants()
MASK_CELLS = 50_000_000


# ------------------------------------------------------------------ reference
def _cols(rows):
    c, s, e = rows
    return (np.asarray(c, dtype=np.int64), np.asarray(s, dtype=np.int64),
            np.asarray(e, dtype=np.int64))


def _hits_by_mask(A, B):
    ac, as_, ae = A
    bc, bs, be = B
    na, nb = len(ac), len(bc)
    hits = np.zeros(na, dtype=np.int64)
    ov = np.zeros(na, dtype=np.int64)
    step = max(1, 4_000_000 // max(nb, 1))
    for i in range(0, na, step):
        j = min(na, i + step)
        c, s, e = ac[i:j, None], as_[i:j, None], ae[i:j, None]
        m = (bc[None, :] == c) & (bs[None, :] < e) & (be[None, :] > s)
        by = np.minimum(e, be[None, :]) - np.maximum(s, bs[None, :])
        hits[i:j] = m.sum(1)
        ov[i:j] = np.where(m, by, 0).sum(1)
    return hits, ov


def _hits_by_oracle(A, B, lens):
    from oracle import oracle
    ac, as_, ae = A
    na = len(ac)
    hits = np.zeros(na, dtype=np.int64)
    ov = np.zeros(na, dtype=np.int64)
    step = 20_000
    for i in range(0, na, step):
        j = min(na, i + step)
        r = oracle.intersect_mt(len(lens), (ac[i:j], as_[i:j], ae[i:j]), B, records=True)
        row = r["a_row"].astype(np.int64)
        hits[i:j] = np.bincount(row, minlength=j - i)
        ov[i:j] = np.bincount(row, weights=(r["end"] - r["start"]).astype(np.float64),
                              minlength=j - i).astype(np.int64)
    return hits, ov


def annotate_ref(A, B, lens):
    """-> (n_hits, covered, overlap_bases), int64, one entry per row of A in
    A's INPUT order.  A, B: (contig, start, end); lens: the contig lengths."""
    A, B = _cols(A), _cols(B)
    lens = np.asarray(lens, dtype=np.int64)
    ac, as_, ae = A
    bc, bs, be = B
    if len(ac) * len(bc) <= MASK_CELLS:
        hits, ov = _hits_by_mask(A, B)
    else:
        hits, ov = _hits_by_oracle(A, B, lens)
    cov = np.zeros(len(ac), dtype=np.int64)
    for c in range(len(lens)):
        ma = ac == c
        if not ma.any():
            continue
        mb = bc == c
        diff = np.zeros(int(lens[c]) + 2, dtype=np.int64)
        np.add.at(diff, bs[mb], 1)
        np.add.at(diff, be[mb], -1)
        painted = np.cumsum(diff)[:int(lens[c])] > 0  # base p is inside some b
        below = np.concatenate([[0], np.cumsum(painted)])  # painted bases in [0, x)
        cov[ma] = below[ae[ma]] - below[as_[ma]]
    return hits, cov, ov


# -------------------------------------------------- the kernel's closed forms
def offsets(lens):
    lens = np.asarray(lens, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(lens + 1)])


def merge_runs(gs, ge):
    """the engine's merge runs of rows sorted by (gs, ge): a new run at row i
    iff max(ge[:i]) <= gs[i] (book-ended rows do not join)"""
    if len(gs) == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z.copy()
    m = np.maximum.accumulate(ge)
    head = np.concatenate([[True], m[:-1] <= gs[1:]])
    first = np.nonzero(head)[0]
    last = np.concatenate([first[1:] - 1, [len(gs) - 1]])
    return gs[first], m[last]


def closed_forms(A, B, lens):
    """(n_hits, covered, overlap_bases) by the identities of annotate.hip"""
    A, B = _cols(A), _cols(B)
    off = offsets(lens)
    s, e = off[A[0]] + A[1], off[A[0]] + A[2]
    bgs, bge = off[B[0]] + B[1], off[B[0]] + B[2]
    order = np.lexsort((bge, bgs))
    bgs, bge = bgs[order], bge[order]
    S, E = bgs, np.sort(bge)
    PS = np.concatenate([[0], np.cumsum(S)])
    PE = np.concatenate([[0], np.cumsum(E)])
    RS, RE = merge_runs(bgs, bge)
    PW = np.concatenate([[0], np.cumsum(RE - RS)])[:-1] if len(RS) else RS

    def D(x):
        lb, ub = np.searchsorted(S, x, "left"), np.searchsorted(E, x, "right")
        return PE[ub] + x * (lb - ub) - PS[lb]

    def Cc(x):
        k = np.searchsorted(RS, x, "right")
        if len(RS) == 0:
            return np.zeros(len(x), dtype=np.int64)
        j = np.maximum(k - 1, 0)
        return np.where(k > 0, PW[j] + np.minimum(RE[j], x) - RS[j], 0)

    zero = np.sort(bgs[bgs == bge])  # the points of B's zero-width rows
    at = np.searchsorted(zero, s, "right") - np.searchsorted(zero, s, "left")
    hits = (np.searchsorted(S, e, "left") - np.searchsorted(E, s, "right") +
            np.where(s == e, at, 0))
    return hits, Cc(e) - Cc(s), D(e) - D(s)


def tile_windows(A, B, lens):
    """per tile of A (sorted by global (start, end)): the entries of B's
    sorted starts, sorted ends and run starts in the tile's window, (nt, 3)"""
    A, B = _cols(A), _cols(B)
    off = offsets(lens)
    s = np.sort(off[A[0]] + A[1])
    bgs, bge = off[B[0]] + B[1], off[B[0]] + B[2]
    order = np.lexsort((bge, bgs))
    RS, _ = merge_runs(bgs[order], bge[order])
    S, E = np.sort(bgs), np.sort(bge)
    nt = (len(s) + T - 1) // T
    edge = s[np.minimum(np.arange(nt + 1) * T, len(s) - 1)]
    pos = np.stack([np.searchsorted(S, edge, "left"), np.searchsorted(E, edge, "right"),
                    np.searchsorted(RS, edge, "right")], 1)
    return pos[1:] - pos[:-1]


def format_annot(names, A, ref, fields=None, order=None):
    """chrom, start, end, n_hits, covered, overlap_bases lines of A's rows in
    `order` (default: RegionOrdering, stable) + the row's name field where it
    has one"""
    A = _cols(A)
    out = []
    for i in (_region_order(A) if order is None else order):
        line = (f"{names[A[0][i]]}\t{A[1][i]}\t{A[2][i]}\t{ref[0][i]}\t{ref[1][i]}"
                f"\t{ref[2][i]}")
        if fields is not None and fields[i]:
            line += "\t" + fields[i]
        out.append(line + "\n")
    return "".join(out).encode()


def _region_order(A):
    # contig ids are those of the space, whose names are in Java String
    # order: ids sort as the names do; stable in the input row
    return np.lexsort((np.arange(len(A[0])), A[2], A[1], A[0]))


# -------------------------------------------------------------- planted cases
def _case(name, lens, A, B):
    def rows(r):
        r = np.asarray(r, dtype=np.int64).reshape(-1, 3)
        return r[:, 0].astype(np.int32), r[:, 1].copy(), r[:, 2].copy()
    return {"name": name, "lens": np.asarray(lens, dtype=np.int64), "A": rows(A), "B": rows(B)}


def _one(name, length, A, B):
    def rows(r):
        r = np.asarray(r, dtype=np.int64).reshape(-1, 2)
        return np.concatenate([np.zeros((len(r), 1), np.int64), r], 1)
    return _case(name, [length], rows(A), rows(B))


def degenerate_cases():
    return [
        _one("empty_a", 30, [], [[3, 9], [5, 12]]),
        _one("empty_b", 30, [[3, 9], [5, 12], [7, 7]], []),
        _one("both_empty", 30, [], []),
        _one("one_each", 30, [[3, 9]], [[5, 12]]),
    ]


# name -> (case, expected (n_hits, covered, overlap_bases) per row of A)
def edge_cases():
    return [
        (_one("book_ended", 30, [[5, 9]], [[0, 5], [9, 12]]), ([0], [0], [0])),
        (_one("zw_a_inside_b", 30, [[5, 5]], [[2, 8]]), ([1], [0], [0])),
        (_one("zw_b_inside_a", 30, [[2, 8]], [[5, 5]]), ([1], [0], [0])),
        # the zero-width b's at a's point do not hit; [2, 8) around it does;
        # [5, 9) begins and [1, 5) ends at the point: no hits
        (_one("zw_same_point", 30, [[5, 5]],
              [[5, 5], [5, 5], [5, 5], [2, 8], [5, 9], [1, 5], [4, 4], [6, 6]]),
         ([1], [0], [0])),
        (_one("zw_a_at_b_edges", 30, [[5, 5], [9, 9]], [[5, 9]]), ([0, 0], [0, 0], [0, 0])),
        # (a zero-width b at a's start or end: no hit either)
        (_one("zw_b_at_a_edges", 30, [[5, 9]], [[5, 5], [9, 9], [7, 7]]), ([1], [0], [0])),
    ]


def wide():
    """one a over 70,000 identical b rows of width 70,000: n_hits passes 2^16,
    overlap_bases = 4.9e9 passes 2^32, covered = 70,000"""
    return _one("wide", 80_000, [[0, 80_000]], [[5, 70_005]] * 70_000)


def long_b_over_tiles():
    """one b [5, m + 10) over the m = 3T + 5 unit rows [3 + i, 4 + i) of A:
    every one of four tiles finds it, though its start is in the window of
    the first only (a unit b in the last tile's window beside it)"""
    m = 3 * T + 5
    i = np.arange(m)
    return _one("long_b_over_tiles", m + 20, np.stack([3 + i, 4 + i], 1),
                [[5, m + 10], [2, 3], [m, m + 1]])


def long_first_row():
    """the first row of tile 1 is very long: it ends past the windows staged
    for its tile, over B rows all along it and beyond"""
    i = np.arange(T)
    big = 12 * T
    A = np.concatenate([np.stack([i, i + 1], 1), [[T, big]],
                        np.stack([T + 1 + i[:T // 2 + 5], T + 3 + i[:T // 2 + 5]], 1)])
    j = np.arange(5 * T)
    B = np.stack([3 * j, 3 * j + 2], 1)
    return _one("long_first_row", 15 * T + 2, A, B)


TILE_ROWS = [T - 1, T, T + 1, 2 * T + 1, 3 * T - 1]


def tile_sized(n, seed):
    """n rows of A over a heavy-tie B of 300 rows, coordinates from 40 values"""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 40, n)
    e = s + rng.integers(0, 12, n)
    bs = rng.integers(0, 40, 300)
    be = bs + rng.integers(0, 12, 300)
    return _one(f"tile_sized_{n}", 60, np.stack([s, e], 1), np.stack([bs, be], 1))


def window_of(m):
    """tile 0 of A starts at x0 and tile 1 at x1; B has m disjoint unit rows
    (x0 + 1 + 2i, +1) between them, so tile 0's window holds exactly m sorted
    starts, m sorted ends and m run starts; tile 1 has a small window"""
    x0 = 7
    x1 = x0 + 2 * m + 2
    i = np.arange(T)
    s0 = x0 + (i * (x1 - x0)) // T
    A0 = np.stack([s0, s0 + i % 7], 1)
    k = np.arange(50)
    A1 = np.stack([x1 + 3 * k, x1 + 3 * k + 4], 1)
    b = np.arange(m)
    B0 = np.stack([x0 + 1 + 2 * b, x0 + 2 + 2 * b], 1)
    j = np.arange(40)
    B1 = np.stack([x1 + 1 + 5 * j, x1 + 4 + 5 * j], 1)
    return _one(f"window_{m}", x1 + 400, np.concatenate([A0, A1]), np.concatenate([B0, B1]))


WINDOW_ROWS = [W - 1, W, W + 1]


def empty_windows():
    i = np.arange(T + 10)
    A = np.stack([100 + i % 50, 100 + i % 50 + i % 9], 1)
    gapA = np.concatenate([np.stack([i[:T] % 500, i[:T] % 500 + 3], 1),
                           np.stack([2000 + i[:T] % 500, 2000 + i[:T] % 500 + 3], 1),
                           np.stack([20_000 + i[:T] % 500, 20_000 + i[:T] % 500 + 3], 1)])
    gapB = np.stack([10_000 + np.arange(100), 10_002 + np.arange(100)], 1)
    return [
        _one("b_before_a", 400, A, [[0, 5], [3, 100], [50, 60]]),
        _one("b_after_a", 400, A, [[200, 205], [203, 300], [159, 170]]),
        # tiles 0 and 1 before the gap, tile 2 after it: tile 0's and tile
        # 2's windows are empty, tile 1's holds all of B
        _one("b_in_gap", 21_000, gapA, gapB),
    ]


def contig_cases():
    return [
        # a ends at its contig's length, b begins at 0 of the next contig
        (_case("contig_touch", [10, 7], [[0, 3, 10]], [[1, 0, 4]]), ([0], [0], [0])),
        # contig 0 of A has no B rows, contig 2 of B no A rows
        (_case("contig_disjoint", [10, 7, 12], [[0, 1, 4], [1, 0, 5], [1, 6, 7]],
               [[1, 2, 6], [2, 3, 9], [2, 0, 12]]), ([0, 1, 0], [0, 3, 0], [0, 3, 0])),
    ]


# sixteen short contigs (the second without rows), about 2,200 coordinates in
# all: the oracle reference shards by contig
RANDOM_LENS = tuple([140, 0] + [130 + 3 * i for i in range(14)])


def random_pair(seed, n, max_width, lens=RANDOM_LENS, long_rows=20):
    """both sides from coverage_cases.random_case: coordinates from about
    2,000 values, 15 % zero-width rows.  random_case pushes 5 % of the ends to
    the contig's end; of those long rows each side keeps `long_rows` and the
    others get a width within max_width again -- every long row of A hits a
    good part of B, and the pair count is what the reference has to reduce"""
    a = random_case(seed, n, lens, max_width)
    b = random_case(seed + 1, n, lens, max_width)
    for side in (a, b):
        w = side["end"] - side["start"]
        trim = np.nonzero(w > max_width)[0][long_rows:]
        side["end"][trim] = side["start"][trim] + w[trim] % (max_width + 1)
    return {"name": f"random_{n}", "lens": a["lens"],
            "A": (a["contig"], a["start"], a["end"]), "B": (b["contig"], b["start"], b["end"])}


def planted_cases():
    out = degenerate_cases()
    out += [c for c, _ in edge_cases()]
    out += [wide(), long_b_over_tiles(), long_first_row()]
    out += [tile_sized(n, 300 + n) for n in TILE_ROWS]
    out += [window_of(m) for m in WINDOW_ROWS]
    out += empty_windows()
    out += [c for c, _ in contig_cases()]
    return out
