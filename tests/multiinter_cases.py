"""Reference and planted cases for multiinter (membership runs and m-of-k
consensus over k sets), shared by the CPU and the GPU tests.

A case is {"name", "sets": [(contig, start, end) int64 arrays], "lens"}.
multiinter_ref is formulated independently of the kernel's XOR scan: per contig
and set the union by np.maximum.accumulate, then the distinct coordinates and
one searchsorted per set for inside / outside.  brute paints every base.
Results: (contig, start, end, mask) in membership mode (min_sets == 0),
(contig, start, end) in consensus mode."""
import numpy as np

T = 2048  # events per tile of k_mi (multiinter.hip MI_TILE)
I64 = np.int64


def _rows(c, s, e):
    return (np.asarray(c, I64), np.asarray(s, I64), np.asarray(e, I64))


def _union(s, e):
    """maximal covered intervals of the rows (zero-width rows add nothing,
    book-ended rows join)"""
    keep = e > s
    s, e = s[keep], e[keep]
    if len(s) == 0:
        return s, e
    o = np.argsort(s, kind="stable")
    s, e = s[o], e[o]
    reach = np.maximum.accumulate(e)
    head = np.ones(len(s), bool)
    head[1:] = s[1:] > reach[:-1]
    h = np.flatnonzero(head)
    return s[h], reach[np.append(h[1:] - 1, len(s) - 1)]


def popcount(m):
    m = np.ascontiguousarray(np.asarray(m).astype(np.uint64))
    return np.unpackbits(m.view(np.uint8).reshape(-1, 8), axis=1).sum(1).astype(I64)


def _emit(x, mask, min_sets):
    """runs of the pieces [x[j], x[j + 1]) with masks mask[j] (one contig)"""
    cls = mask if min_sets == 0 else (popcount(mask) >= min_sets).astype(np.uint64)
    on = cls != 0
    head = on.copy()
    head[1:] &= cls[1:] != cls[:-1]
    tail = on.copy()
    tail[:-1] &= cls[1:] != cls[:-1]
    h, t = np.flatnonzero(head), np.flatnonzero(tail)
    return x[h], x[t + 1], mask[h]


def multiinter_ref(sets, lens, min_sets):
    k = len(sets)
    out = [[], [], [], []]
    for c in range(len(lens)):
        un = []
        for cs, s, e in sets:
            sel = cs == c
            un.append(_union(s[sel], e[sel]))
        x = np.unique(np.concatenate([np.concatenate(u) for u in un]))
        if len(x) < 2:
            continue
        left = x[:-1]
        mask = np.zeros(len(left), np.uint64)
        for i, (us, ue) in enumerate(un):
            if len(us) == 0:
                continue
            r = np.searchsorted(us, left, "right") - 1
            inside = (r >= 0) & (left < ue[np.maximum(r, 0)])
            mask |= inside.astype(np.uint64) << np.uint64(i)
        s, e, m = _emit(x, mask, min_sets)
        out[0].append(np.full(len(s), c, I64))
        out[1].append(s)
        out[2].append(e)
        out[3].append(m)
    assert 1 <= k <= 32 and 0 <= min_sets <= k
    res = [np.concatenate(v) if v else np.zeros(0, I64) for v in out[:3]]
    m = np.concatenate(out[3]).astype(I64) if out[3] else np.zeros(0, I64)
    return (res[0], res[1], res[2], m) if min_sets == 0 else tuple(res)


def brute(sets, lens, min_sets):
    """the per-base paint (small genomes)"""
    out = [[], [], [], []]
    for c in range(len(lens)):
        n = int(lens[c])
        mask = np.zeros(n + 1, np.uint64)  # (one base of 0 past the contig)
        for i, (cs, s, e) in enumerate(sets):
            for a, b in zip(s[cs == c].tolist(), e[cs == c].tolist()):
                mask[a:b] |= np.uint64(1) << np.uint64(i)
        assert mask[n] == 0
        cls = mask if min_sets == 0 else (popcount(mask) >= min_sets).astype(np.uint64)
        prev = np.concatenate([[0], cls[:-1]]).astype(np.uint64)
        nxt = np.concatenate([cls[1:], [0]]).astype(np.uint64)
        h = np.flatnonzero((cls != 0) & (cls != prev))
        t = np.flatnonzero((cls != 0) & (cls != nxt))
        out[0].append(np.full(len(h), c, I64))
        out[1].append(h.astype(I64))
        out[2].append(t.astype(I64) + 1)
        out[3].append(mask[h].astype(I64))
    res = [np.concatenate(v) if v else np.zeros(0, I64) for v in out]
    return tuple(res) if min_sets == 0 else tuple(res[:3])


def format_multiinter(names, runs):
    """the device writer's text: five columns in membership mode (n_sets and
    the mask in decimal), three in consensus mode"""
    if len(runs) == 4:
        ns = popcount(runs[3])
        return "".join(f"{names[c]}\t{s}\t{e}\t{n}\t{m}\n" for c, s, e, m, n in
                       zip(*(v.tolist() for v in runs), ns.tolist())).encode()
    return "".join(f"{names[c]}\t{s}\t{e}\n" for c, s, e in
                   zip(*(v.tolist() for v in runs))).encode()


def modes(k):
    """membership, union, a middle value, the k-way AND"""
    return sorted({0, 1, (k + 1) // 2, k})


# ------------------------------------------------------- the kernel's events
def offsets(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, I64) + 1)])


def merge_like_runs(gs, ge):
    """the runs merge_runs gives a plain set: a new run iff next.start >=
    running max end (book-ended rows do not join, zero-width rows stay)"""
    if len(gs) == 0:
        return gs, ge
    o = np.lexsort((ge, gs))
    gs, ge = gs[o], ge[o]
    reach = np.maximum.accumulate(ge)
    head = np.ones(len(gs), bool)
    head[1:] = gs[1:] >= reach[:-1]
    h = np.flatnonzero(head)
    return gs[h], reach[np.append(h[1:] - 1, len(gs) - 1)]


def events(case):
    """(coordinate, set) of the kernel's events in sorted order (the order
    inside a coordinate group is the sort's and not pinned: sets are listed
    ascending there)"""
    off = offsets(case["lens"])
    key, idx = [], []
    for i, (c, s, e) in enumerate(case["sets"]):
        rs, re_ = merge_like_runs(off[c] + s, off[c] + e)
        key += [rs, re_]
        idx += [np.full(2 * len(rs), i, I64)]
    key = np.concatenate(key) if key else np.zeros(0, I64)
    idx = np.concatenate(idx) if idx else np.zeros(0, I64)
    # (key holds starts then ends per set: reorder the set column alike)
    o = np.lexsort((idx, key))
    return key[o], idx[o]


def group_span(case, gcoord):
    """first and last sorted position of the events at global coordinate gcoord"""
    key, _ = events(case)
    p = np.flatnonzero(key == gcoord)
    return int(p[0]), int(p[-1])


# ------------------------------------------------------------- planted cases
def _case(name, sets, lens):
    return {"name": name, "sets": [_rows(*r) for r in sets], "lens": np.asarray(lens, I64)}


def _one(s, e, c=0):
    s = np.asarray(s, I64)
    return (np.full(len(s), c, I64), s, np.asarray(e, I64))


EMPTY = ([], [], [])
TILE_EVENTS = (T - 2, T, T + 2, 2 * T, 2 * T + 2)


def round_robin(n_runs, k=3, step=10, width=5, base=0):
    """n_runs disjoint runs [base + step j, + width) dealt round-robin to k sets"""
    j = np.arange(n_runs, dtype=I64)
    return [_one(base + step * j[j % k == i], base + step * j[j % k == i] + width)
            for i in range(k)]


def _fillers(f, base=0):
    """f runs [base + 2i, base + 2i + 1): 2f events at distinct coordinates"""
    i = np.arange(f, dtype=I64)
    return base + 2 * i, base + 2 * i + 1


def _straddle(change):
    # 2F filler events (set 0), 32 starts at A, then the group at X: every set
    # ends a run and starts the next there (64 events, first at T - 30)
    F = (T - 62) // 2
    A, X, B = 2 * F + 10, 2 * F + 20, 2 * F + 30
    fs, fe = _fillers(F)
    sets = []
    for i in range(32):
        s, e = [A, X], [X, B]
        if change and i == 30:
            s, e = [A], [X]  # ends there and stays off
        if change and i == 31:
            s, e = [A, X], [X, X]  # ends there, and a zero-width row at X
        if i == 0:
            s, e = np.concatenate([fs, s]), np.concatenate([fe, e])
        sets.append(_one(s, e))
    return _case("straddle_change" if change else "straddle_same", sets, [B + 5]), X


def _edge(last):
    # T - 2 filler events (set 3); edge_is_last: sets 0, 1 start at A (events
    # T - 2, T - 1) and set 2 at A + 1 (event T); edge_not_last: set 2 starts
    # at A - 1 (event T - 2), sets 0, 1 at A (events T - 1, T)
    F = (T - 2) // 2
    fs, fe = _fillers(F)
    A = 2 * F + 10
    c = A + 1 if last else A - 1
    sets = [_one([A], [A + 20]), _one([A], [A + 30]), _one([c], [A + 40]), _one(fs, fe)]
    return _case("edge_is_last" if last else "edge_not_last", sets, [A + 50]), A


def _heads_at():
    # sets 0 and 3 lie over everything (events 0, 1); set 1's fillers [20i + 10,
    # 20i + 20) give events 2 + j at 10 (j + 1); set 2's two one-base runs are
    # planted inside fillers so that their events are 63, 64 and 511, 512 of the
    # tile: with min_sets = 4 those are the only heads
    pos = [63, 64, 511, 512]
    n_fill = 300
    L = 20 * n_fill + 100
    i = np.arange(n_fill, dtype=I64)
    s2, e2 = [], []
    for a, shift in ((pos[0], 0), (pos[2], 2)):
        j = a - 2 - shift - 1  # the filler event before it (a start: j even)
        assert j % 2 == 0
        s2.append(10 * (j + 1) + 1)
        e2.append(10 * (j + 1) + 2)
    sets = [_one([0], [L]), _one(20 * i + 10, 20 * i + 20), _one(s2, e2), _one([5], [L - 1])]
    return _case("heads_at_wave_and_thread_edges", sets, [L]), pos


def planted_cases():
    out = []
    out.append(_case("k1", [_one([3, 20, 25], [9, 25, 31])], [40]))
    out.append(_case("all_empty", [EMPTY, EMPTY, EMPTY], [40]))
    out.append(_case("one_empty", [_one([3], [9]), EMPTY, _one([5], [12])], [40]))
    out.append(_case("zero_width_only", [_one([4, 4, 9], [4, 4, 9]), _one([4], [4])], [40]))
    out.append(_case("zero_width_inside", [_one([2], [8]), _one([5, 5], [5, 5])], [40]))
    out.append(_case("book_end_inside", [_one([0, 5], [5, 9])], [40]))
    out.append(_case("book_end_across", [_one([0], [5]), _one([5], [9])], [40]))
    out.append(_case("k32_identical", [_one([10, 30], [20, 31])] * 32, [40]))
    out.append(_case("bit31_alone", [EMPTY] * 31 + [_one([7], [11])], [40]))
    for n_ev in TILE_EVENTS:
        out.append(_case(f"tile_{n_ev}", round_robin(n_ev // 2), [10 * n_ev]))
    out.append(_straddle(False)[0])
    out.append(_straddle(True)[0])
    out.append(_edge(True)[0])
    out.append(_edge(False)[0])
    # set 31 lies over more than 3 tiles of the other sets' events
    n = (7 * T) // 4
    out.append(_case("long_over", [EMPTY] * 28 + round_robin(n, base=10) +
                     [_one([3], [10 * n + 20])], [10 * n + 40]))
    # 5000 zero-width rows of set 0 where set 1 opens a run, under set 2
    out.append(_case("zero_width_5000", [_one([700] * 5000, [700] * 5000),
                                         _one([700], [900]), _one([100], [800])], [1000]))
    out.append(_heads_at()[0])
    # contigs: a run ending at the contig's length, then one at 0 of the next
    # contig (of the same set and of another); a contig with no rows; data on
    # the last contig only
    out.append(_case("contig_touch", [(np.array([0, 1]), [3, 0], [10, 4]),
                                      (np.array([0, 1, 2]), [8, 0, 0], [10, 2, 6])],
                     [10, 8, 6]))
    out.append(_case("contig_empty", [(np.array([0, 2]), [1, 0], [4, 3]),
                                      (np.array([0, 2, 2]), [2, 2, 5], [6, 5, 9])], [9, 7, 9]))
    out.append(_case("contig_last_only", [(np.array([3, 3]), [2, 8], [10, 12]),
                                          (np.array([3]), [9], [12])], [5, 0, 7, 12]))
    return out


def random_case(seed, k, n, lens, max_len, values=None, exact=False):
    """k sets of up to n rows (exact: of n rows) with widths up to max_len; a
    tenth zero-width, a tenth ending at the contig's length, a fifth book-ended
    to another row (of any set).  `values`: heavy ties -- per contig the
    coordinates come from a grid of that many values, a set's starts from a
    random 40 % of them, widths of one or two grid steps (max_len unused)"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, I64)
    live = np.flatnonzero(lens > 0)
    sets, ends = [], []
    for i in range(k):
        m = n if exact or values is not None else int(rng.integers(0, n + 1))
        c = live[rng.integers(0, len(live), m)]
        ln = lens[c]
        if values is None:
            s = (rng.random(m) * ln).astype(I64)
            w = rng.integers(1, max_len + 1, m)
        else:
            grid = np.maximum(ln // values, 1)
            allowed = np.flatnonzero(rng.random(values) < 0.4)
            s = np.minimum(allowed[rng.integers(0, len(allowed), m)] * grid, ln)
            w = grid * (1 + (rng.random(m) < 0.2))
        kind = rng.random(m)
        w[kind < 0.1] = 0
        at_end = kind > 0.9
        s = np.where(at_end, np.maximum(ln - w, 0), s)
        e = np.minimum(s + w, ln)
        if ends and m:
            pool_c = np.concatenate([x[0] for x in ends])
            pool_e = np.concatenate([x[1] for x in ends])
            if len(pool_e):
                pick = rng.integers(0, len(pool_e), m)
                be = (kind > 0.5) & (kind < 0.7)
                c = np.where(be, pool_c[pick], c)
                s = np.where(be, pool_e[pick], s)
                e = np.where(be, np.minimum(s + w, lens[c]), e)
        sets.append(_rows(c, s, e))
        ends.append((c, e))
    return {"name": f"random_{seed}", "sets": sets, "lens": lens}
