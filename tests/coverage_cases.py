"""Depth-of-coverage reference and planted inputs, shared by
test_coverage_cases.py (CPU) and test_gpu_coverage.py (GPU).

`depth_runs` restates the semantics of lime_coverage in numpy, independent of
the kernel's merge-path walk: per contig, the distinct coordinates of starts
and ends, `searchsorted` left / right for the depth below and from each, the
heads where they differ, and the runs between heads.

The planted cases place coordinate groups at chosen positions of the kernel's
merged event order (starts and ends of one set merged by coordinate, starts
first among equals): the kernel cuts that order into tiles of T events.
"""
import numpy as np

# events per tile of k_cov: CV_TILE = CVB * CV_ITEMS in lime_amd/csrc/coverage.hip
T = 2048


def depth_runs(contig, start, end, lens):
    """-> (contig, start, end, depth) of the maximal constant-depth (>= 1)
    runs, contigs ascending, ascending inside a contig.  `lens`: the contig
    lengths (every end must lie inside its contig)."""
    contig = np.asarray(contig, dtype=np.int64)
    start = np.asarray(start, dtype=np.int64)
    end = np.asarray(end, dtype=np.int64)
    oc, os_, oe, od = [], [], [], []
    for c in range(len(lens)):
        m = contig == c
        if not m.any():
            continue
        S = np.sort(start[m])
        E = np.sort(end[m])
        assert S[0] >= 0 and E[-1] <= lens[c]
        x = np.unique(np.concatenate([S, E]))
        after = np.searchsorted(S, x, "right") - np.searchsorted(E, x, "right")
        before = np.searchsorted(S, x, "left") - np.searchsorted(E, x, "left")
        head = after != before
        opens = head & (after > 0)
        closes = head & (before > 0)
        assert opens.sum() == closes.sum()
        oc.append(np.full(int(opens.sum()), c, dtype=np.int64))
        os_.append(x[opens])
        oe.append(x[closes])
        od.append(after[opens])
    if not oc:
        z = np.zeros(0, dtype=np.int64)
        return z, z.copy(), z.copy(), z.copy()
    return tuple(np.concatenate(v).astype(np.int64) for v in (oc, os_, oe, od))


def brute_runs(contig, start, end, lens):
    """the same from the definition: a difference array and a cumsum over
    every base of every contig (small genomes only)"""
    contig = np.asarray(contig, dtype=np.int64)
    start = np.asarray(start, dtype=np.int64)
    end = np.asarray(end, dtype=np.int64)
    oc, os_, oe, od = [], [], [], []
    for c in range(len(lens)):
        m = contig == c
        diff = np.zeros(int(lens[c]) + 2, dtype=np.int64)
        np.add.at(diff, start[m], 1)
        np.add.at(diff, end[m], -1)
        depth = np.cumsum(diff)[:int(lens[c]) + 1]  # depth[len] == 0: closes the last run
        prev = np.concatenate([[0], depth[:-1]])
        chg = np.nonzero(depth != prev)[0]
        for k, p in enumerate(chg):
            if depth[p] > 0:
                oc.append(c)
                os_.append(p)
                oe.append(chg[k + 1])
                od.append(depth[p])
    return tuple(np.array(v, dtype=np.int64) for v in (oc, os_, oe, od))


def format_bedgraph(names, runs):
    """chrom<TAB>start<TAB>end<TAB>depth lines of depth_runs' output"""
    c, s, e, d = runs
    return "".join(f"{names[ci]}\t{si}\t{ei}\t{di}\n"
                   for ci, si, ei, di in zip(c.tolist(), s.tolist(), e.tolist(), d.tolist())
                   ).encode()


def event_groups(start, end):
    """the merged event order of one contig's rows: for every distinct
    coordinate x (ascending) -> (x, first, last) merged positions of its group
    (all starts and ends at x are contiguous)"""
    S = np.sort(np.asarray(start, dtype=np.int64))
    E = np.sort(np.asarray(end, dtype=np.int64))
    x = np.unique(np.concatenate([S, E]))
    first = np.searchsorted(S, x, "left") + np.searchsorted(E, x, "left")
    last = np.searchsorted(S, x, "right") + np.searchsorted(E, x, "right") - 1
    return x, first, last


def _case(name, lens, contig, start, end):
    return {"name": name, "lens": np.asarray(lens, dtype=np.int64),
            "contig": np.asarray(contig, dtype=np.int32),
            "start": np.asarray(start, dtype=np.int64), "end": np.asarray(end, dtype=np.int64)}


def _one(name, length, rows):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 2)
    return _case(name, [length], np.zeros(len(rows), np.int32), rows[:, 0], rows[:, 1])


def identical(k):
    """k copies of one row: the groups at its start and at its end hold k
    events each (k = 70,000: each spans dozens of tiles, and the depth passes
    2^16)"""
    return _one(f"identical_{k}", 100, [[10, 20]] * k)


def chain(m):
    """m book-ended unit rows [i, i + 1): the group at every interior
    coordinate i is (start, end) at merged positions 2i - 1, 2i -- for i = T/2
    the start is the last event of tile 0 and the end the first of tile 1 --
    with net change 0: ONE run [0, m) of depth 1"""
    i = np.arange(m)
    return _one(f"chain_{m}", m + 1, np.stack([i, i + 1], 1))


def straddle_change():
    """the group at x: 3 ends and 6 starts on merged positions T - 3 .. T + 5
    (net change 3 -> 6), behind (T - 6) / 2 rows [0, 1) and 3 rows [2, x)"""
    x = 50
    rows = [[0, 1]] * ((T - 6) // 2) + [[2, x]] * 3 + [[x, x + 10]] * 6
    return _one("straddle_change", 100, rows)


def edge_is_last():
    """T/2 rows [0, 1): the group at 1 ends on merged position T - 1, the
    tile's last event, and tile 1 begins another coordinate"""
    return _one("edge_is_last", 100, [[0, 1]] * (T // 2) + [[5, 6]])


def edge_not_last():
    """T/2 + 3 rows [0, 1): the group at 1 runs over the tile edge (positions
    T/2 + 3 .. T + 5), so the tile's last event is not the last at 1"""
    return _one("edge_not_last", 100, [[0, 1]] * (T // 2 + 3) + [[5, 6]])


def long_over_chain():
    """one row [0, m + 10) over m = T + 5 book-ended rows [5 + i, 6 + i):
    [0, 5) depth 1, [5, 5 + m) depth 2 -- its opening and closing heads more
    than two tiles of events apart -- and [5 + m, m + 10) depth 1"""
    m = T + 5
    i = np.arange(m)
    rows = np.concatenate([[[0, m + 10]], np.stack([5 + i, 6 + i], 1)])
    return _one("long_over_chain", m + 10, rows)


def staircase(m, w):
    """rows [2i, 2i + w), i < m, w odd: starts on even and ends on odd
    coordinates, so every coordinate is a head and there are 2m - 1 runs; the
    depth ramps up to min(m, (w + 1) / 2) and down again"""
    assert w % 2 == 1
    i = 2 * np.arange(m)
    return _one(f"staircase_{m}_{w}", 2 * m + w, np.stack([i, i + w], 1))


def tile_sized(n, seed):
    """n random rows over a few coordinates (heavy ties) on one contig"""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 40, n)
    e = s + rng.integers(0, 12, n)
    return _one(f"tile_sized_{n}", 60, np.stack([s, e], 1))


# rows whose 2n events come to T - 2, T, T + 2, 2T, 2T + 2 and 3T - 2 (2n is
# even: the odd counts T - 1, T + 1, 2T + 1, 3T - 1 cannot occur, so the even
# counts on either side of each stand in), and the odd row counts themselves
TILE_ROWS = sorted({T // 2 - 1, T // 2, T // 2 + 1, T, T + 1, 3 * T // 2 - 1,
                    T - 1, 2 * T + 1, 3 * T - 1})


def contig_cases():
    return [
        # a row ending at a contig's length, the next row at 0 of the next contig
        _case("contig_touch", [10, 7], [0, 1], [3, 0], [10, 4]),
        # a contig without rows between two with rows
        _case("contig_gap", [10, 7, 12], [0, 2, 2], [1, 0, 3], [4, 5, 9]),
        # a row at the very end of the last contig
        _case("contig_last_end", [10, 7, 12], [0, 2], [2, 8], [10, 12]),
    ]


def small_cases():
    return [
        _case("empty", [10], [], [], []),
        _one("one_row", 30, [[3, 9]]),
        _one("zero_width_only", 30, [[4, 4], [4, 4], [9, 9]]),
        _one("book_ended", 30, [[0, 5], [5, 9]]),
        _one("zero_width_inside", 30, [[2, 8], [5, 5], [8, 8], [2, 2]]),
    ]


def planted_cases():
    out = small_cases()
    out += [identical(k) for k in (1, 2, 65, 70000)]
    out += [tile_sized(n, 100 + n) for n in TILE_ROWS]
    out += [chain(T // 2 + 3), straddle_change(), edge_is_last(), edge_not_last(),
            long_over_chain()]
    out += [staircase(1500, 7), staircase(1500, 3001)]  # w < m, and every row over every other
    out += contig_cases()
    return out


def random_case(seed, n, lens, max_width, zero_frac=0.15):
    """seeded rows over `lens` (contigs with length 0 stay empty): starts and
    widths from small ranges so ties are heavy, some zero-width rows, some
    rows pushed to their contig's end"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    live = np.nonzero(lens > 0)[0]
    c = live[rng.integers(0, len(live), n)]
    ln = lens[c]
    s = (rng.random(n) * (ln + 1)).astype(np.int64)
    w = rng.integers(0, max_width + 1, n)
    w[rng.random(n) < zero_frac] = 0
    e = np.minimum(s + w, ln)
    at_end = rng.random(n) < 0.05
    e[at_end] = ln[at_end]
    s = np.minimum(s, e)
    return _case(f"random_{seed}", lens, c, s, e)
