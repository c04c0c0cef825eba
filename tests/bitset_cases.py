"""Inputs planted on the bin, tile and slot edges of the bit-per-base path
(lime_amd/csrc/bitset.hip), an independent reference of its five ops, and a
restatement in numpy of the decomposition the kernels' branches depend on --
shared by tests/test_bitset_cases.py (CPU: the reference against a per-base
paint and the oracle, every case on the arm it claims, the constants still
the kernel file's) and tests/test_gpu_bitset_edges.py (the engine against the
reference, run for run in output order, on every path a case can take).

The space.  Contig c covers global bits [off[c], off[c] + len[c]); the bit
after it, off[c + 1] - 1, is its pad and is never set, so no run crosses a
contig.  A bitset covers the window [lo, hi) of the global bits (the whole
space, or a shard's range with lo % 64 == 0).

A case is a dict: key, lens, sets (row sets: contig rows (c, s, e) or global
rows (gs, ge), int64), window, ops [(op, operand indices)], and `claims`: the
arms it was planted on, as numbers the counters below must return.

Ops: 0 a, 1 ~a within the contigs and the window, 2 a & b, 3 a & ~b,
4 the AND of k.

Every builder is cached and returns read-only arrays.
"""
import functools
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------- the constants
# (name in lime_amd/csrc/bitset.hip -> value; SOURCE_LINES quotes the lines)
BSH = 23                      # bin = 2^23 bases
PSH = 19                      # paint tile = 2^19 bases
BIN, TILE = 1 << BSH, 1 << PSH
PSUB = 1 << (BSH - PSH)       # 16 paint tiles per bin
TWORDS = 1 << (PSH - 6)       # 8192 words per paint tile
LENB = 32 - BSH
LMAX = (1 << LENB) - 1        # 511: longest bin piece
SROWS, BINB, WRB = 12, 1024, 1024
STEP = SROWS * BINB           # 12288 rows per count step
WSTEP = SROWS * WRB           # 12288 rows per write step
SPB, PV = 512, 16
SPLIT_CH = SPB * PV           # 8192 rows per split chunk
APV, PAINTB = 16, 512
PAINT_BATCH = APV * PAINTB    # 8192 rows per paint batch
SPLIT_BLOCKS = 3072
EV_NT, EV_W = 256, 8
EV_TW = EV_NT * EV_W          # 2048 words per one-pass extraction tile
EVCAP = 2048                  # events of a one-pass tile
BB, BW = 256, 16
BT = BB * BW                  # 4096 words per two-pass extraction tile
PEW = TWORDS // PAINTB        # 16 consecutive words per thread (k_paint_ev)
EVSLOT_MIN, EVSLOT_MAX = 4096, 2 * TWORDS   # k_paint_ev's slot range
MAXPAD = 64                   # contig pads staged per batch
CMAX = 1024                   # contig table in LDS up to here
MAXK = 16
SLAB_PAD = 0xffffffff
PESSIMISM = 32                # ctx->bin_pessimism after a region overflow

SOURCE_LINES = {
    "BB": r"constexpr int BB = 256;",
    "BW": r"constexpr int BW = 16; ",
    "BT": r"constexpr int BT = BB \* BW;",
    "MAXK": r"constexpr int MAXK = 16;",
    "MAXPAD": r"constexpr int MAXPAD = 64;",
    "BSH": r"#ifndef LIME_BSH\n#define LIME_BSH 23\n",
    "PSH": r"#ifndef LIME_PSH\n#define LIME_PSH 19\n",
    "PAINTB": r"#ifndef LIME_PAINTB\n#define LIME_PAINTB 512\n",
    "PSUB": r"constexpr int PSUB = 1 << \(BSH - PSH\);",
    "LMAX": r"constexpr uint32_t LMAX = \(1u << LENB\) - 1;",
    "LENB": r"constexpr int LENB = 32 - BSH;",
    "BINB": r"constexpr int BINB = 1024;",
    "WRB": r"#ifndef LIME_WRB\n#define LIME_WRB 1024\n",
    "SROWS": r"#ifndef LIME_SROWS\n#define LIME_SROWS 12\n",
    "STEP": r"constexpr int STEP = SROWS \* BINB;",
    "WSTEP": r"constexpr int WSTEP = SROWS \* WRB;",
    "SPB": r"#ifndef LIME_SPB\n#define LIME_SPB 512\n",
    "PV": r"#ifndef LIME_SPLIT_PV\n#define LIME_SPLIT_PV 16\n",
    "SPLIT_CH": r"constexpr uint32_t CH = SPB \* PV;",
    "SPLIT_BLOCKS": r"#ifndef LIME_SPLIT_BLOCKS\n#define LIME_SPLIT_BLOCKS 3072\n",
    "APV": r"constexpr int APV = 16;",
    "PAINT_BATCH": r"constexpr uint32_t B = APV \* PAINTB;",
    "EV_NT": r"#ifndef LIME_EV_NT\n#define LIME_EV_NT 256\n",
    "EV_W": r"#ifndef LIME_EV_W\n#define LIME_EV_W 8\n",
    "EVCAP": r"#ifndef LIME_EVCAP\n#define LIME_EVCAP 2048\n",
    "EVSLOT_MAX": r"constexpr int EVSLOT_MAX = 2 \* TWORDS;",
    "CMAX": r"constexpr int CMAX = 1024;",
    "SLAB_PAD": r"constexpr uint32_t SLAB_PAD = 0xffffffffu;",
    # bin_rows: chunk rows, chunks, chunk groups, optimistic regions
    "R": r"R = std::min<int64_t>\(std::max<int64_t>\(R, STEP\), 16 \* \(int64_t\)STEP\);",
    "nch": r"const uint32_t nch = \(uint32_t\)std::max<int64_t>\(\(n \+ R - 1\) / R, 1\);",
    "ng": r"const int ng = \(int\)std::min<int64_t>\(std::max<int64_t>\(\(LIME_SPLIT_BLOCKS \+ nb - 1\)"
          r" / nb, 1\),\s*\n\s*std::min<int64_t>\(nch, 16\)\);",
    "E": r"const double E = \(double\)R \* \(double\)\(1ll << BSH\) / "
         r"\(double\)std::max<int64_t>\(hi - lo, 1\);",
    "opt_gate": r"if \(allow_opt && opt_on && ctx->bin_pessimism == 0 && nb >= 8 && E >= 128\.0\) \{",
    "rcap": r"const double c = std::ceil\(E \+ 6\.0 \* std::sqrt\(E\)\) \+ 8\.0;\s*\n"
            r"\s*const uint64_t cap = \(\(uint64_t\)c \+ 3\) / 4 \* 4;",
    "pessimism_set": r"ctx->bin_pessimism = 32;",
    "pessimism_spend": r"if \(!rcap && ctx->bin_pessimism > 0\) --ctx->bin_pessimism;",
    # the write pass's bin piece and the split's tile piece
    "bin_piece": r"l = min\(min\(l, LMAX\), \(1u << BSH\) - o\);",
    "write_rem": r"if \(\(valid & \(1u << k\)\) && g1 > g0 \+ l\)",
    "split_clip": r"const uint32_t l2 = o \+ l > qend \? qend - o : l;",
    # cross pieces
    "x_tiles": r"const uint32_t t0 = \(uint32_t\)\(s >> PSH\), t1 = \(uint32_t\)\(\(e - 1\) >> PSH\);",
    "x_full": r"if \(t1 > t0 \+ 1\) \{",
    # the fused extraction's slot
    "slot": r"cap = bound < 0 \? 16384 : 2 \* \(2 \* bound / std::max<int64_t>\(nt, 1\)\) \+ 2048;\s*\n"
            r"\s*cap = std::min<int64_t>\(std::max<int64_t>\(\(cap \+ 255\) / 256 \* 256, 4096\), "
            r"EVSLOT_MAX\);",
    "slot_bound": r"bound = op == 1 \? \(int64_t\)a->n_contigs \+ 1 : 0;",
    "close": r"const bool close = threadIdx\.x == PAINTB - 1 && \(x\[PEW - 1\] >> 63\) != 0;",
    "one_pass_tiles": r"const int64_t ntl = a->n_words / EV_TW \+ 1;",
    "one_pass_oflow": r"if \(tot > \(uint32_t\)EVCAP\) atomicOr\(oflow, 1u\);",
    "two_pass_tiles": r"const int64_t nt = a->n_words == 0 \? 0 : a->n_words / BT \+ 1;",
    "pad_lo": r"const int64_t lo = \(a\.word0 \+ \(w0 > 0 \? w0 - 1 : 0\)\) \* 64;",
}


def source():
    with open(os.path.join(ROOT, "lime_amd", "csrc", "bitset.hip")) as f:
        return f.read()


def _ro(*arrs):
    out = []
    for a in arrs:
        a = np.ascontiguousarray(a, dtype=np.int64)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


# ---------------------------------------------------------------- the space
def offsets(lens):
    """off[c] = global bit of contig c's base 0; off[nc] = the span"""
    return np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64) + 1)]).astype(np.int64)


def window(case):
    off = offsets(case["lens"])
    return case["window"] if case.get("window") else (0, int(off[-1]))


def global_rows(case, i):
    """row set i in global coordinates, as given (not clipped)"""
    rows = case["sets"][i]
    if len(rows) == 2:
        return rows
    off = offsets(case["lens"])
    c, s, e = rows
    return off[c] + s, off[c] + e


# ------------------------------------------------------------ the reference
def merged(gs, ge):
    """sort by start, running maximum of the ends: the maximal runs (rows that
    overlap or touch are one run; zero-width rows hold no base)"""
    keep = ge > gs
    gs, ge = gs[keep], ge[keep]
    if len(gs) == 0:
        return gs, ge
    o = np.argsort(gs, kind="stable")
    gs, ge = gs[o], ge[o]
    top = np.maximum.accumulate(ge)
    first = np.flatnonzero(np.concatenate([[True], gs[1:] > top[:-1]]))
    last = np.concatenate([first[1:] - 1, [len(gs) - 1]])
    return gs[first], top[last]


def _inside(runs, p):
    s, e = runs
    if len(s) == 0:
        return np.zeros(len(p), bool)
    r = np.searchsorted(s, p, "right") - 1
    return (r >= 0) & (e[np.maximum(r, 0)] > p)


@functools.lru_cache(maxsize=None)
def _operand(key, i):
    case = CASES[key]
    lo, hi = window(case)
    gs, ge = global_rows(case, i)
    return merged(np.clip(gs, lo, hi), np.clip(ge, lo, hi))


def reference_global(case, op, idx):
    """the maximal runs of op over operands idx, as global (gs, ge)"""
    off = offsets(case["lens"])
    lo, hi = window(case)
    runs = [_operand(case["key"], i) for i in idx]
    marks = [np.array([lo, hi]), np.clip(off[:-1], lo, hi), np.clip(off[1:] - 1, lo, hi)]
    for s, e in runs:
        marks += [s, e]
    bp = np.unique(np.concatenate(marks))
    p = bp[:-1]  # the elementary segments [bp[j], bp[j + 1]): uniform membership
    if len(p) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    c = np.searchsorted(off, p, "right") - 1
    in_contig = p < off[c + 1] - 1
    ins = [_inside(r, p) for r in runs]
    if op == 0:
        v = ins[0]
    elif op == 1:
        v = ~ins[0] & in_contig
    elif op == 2:
        v = ins[0] & ins[1]
    elif op == 3:
        v = ins[0] & ~ins[1]
    else:
        v = np.logical_and.reduce(ins)
    d = np.diff(np.concatenate([[False], v, [False]]).astype(np.int8))
    return bp[np.flatnonzero(d == 1)], bp[np.flatnonzero(d == -1)]


def to_contig(case, gs, ge):
    off = offsets(case["lens"])
    c = np.searchsorted(off, gs, "right") - 1
    return c.astype(np.int64), gs - off[c], ge - off[c]


@functools.lru_cache(maxsize=None)
def _reference(key, op, idx):
    case = CASES[key]
    gs, ge = reference_global(case, op, idx)
    c, s, e = to_contig(case, gs, ge)
    return _ro(c, s, e) + (int((ge - gs).sum()),)


def reference(case, op, idx):
    """-> (contig, start, end, popcount) of op over operands idx"""
    return _reference(case["key"], op, tuple(idx))


def paint(case, op, idx):
    """the same by one boolean per base (small spaces only): -> global (gs, ge)"""
    off = offsets(case["lens"])
    lo, hi = window(case)
    span = int(off[-1])
    imgs = []
    for i in idx:
        gs, ge = global_rows(case, i)
        d = np.zeros(span + 1, np.int32)
        np.add.at(d, np.clip(gs, lo, hi), 1)
        np.add.at(d, np.clip(np.maximum(ge, gs), lo, hi), -1)
        imgs.append(np.cumsum(d, dtype=np.int32)[:span] > 0)
    ok = np.ones(span, bool)
    ok[off[1:] - 1] = False
    ok[:lo] = False
    ok[hi:] = False
    v = {0: lambda: imgs[0], 1: lambda: ~imgs[0] & ok, 2: lambda: imgs[0] & imgs[1],
         3: lambda: imgs[0] & ~imgs[1], 4: lambda: np.logical_and.reduce(imgs)}[op]()
    d = np.diff(np.concatenate([[False], v, [False]]).astype(np.int8))
    return np.flatnonzero(d == 1), np.flatnonzero(d == -1)


PAINT_MAX = 5 << 20   # per-base check up to here (bits of span)


# ---------------------------------------------------------- the arm counter
def n_bins(width):
    return max((width + BIN - 1) >> BSH, 1)


def chunking(n, width):
    """(nb, R, nch, ng, E, rcap): bin_rows' decomposition of n rows.  R = STEP
    for every n up to (resident write workgroups) x STEP rows -- all the cases
    here on any device with 17 or more of them"""
    assert n <= 17 * STEP
    nb = n_bins(width)
    R = STEP
    nch = max((n + R - 1) // R, 1)
    ng = min(max((SPLIT_BLOCKS + nb - 1) // nb, 1), min(nch, 16))
    E = float(R) * float(BIN) / float(max(width, 1))
    rcap = 0
    if nb >= 8 and E >= 128.0:
        c = math.ceil(E + 6.0 * math.sqrt(E)) + 8.0
        rcap = (int(c) + 3) // 4 * 4
    return nb, R, nch, ng, E, rcap


def group_of_chunk(nch, ng):
    """chunk -> chunk group: group g holds chunks [g nch / ng, (g + 1) nch / ng)"""
    g = np.zeros(nch, np.int64)
    for q in range(ng):
        g[q * nch // ng:(q + 1) * nch // ng] = q
    return g


@functools.lru_cache(maxsize=None)
def _binning(key, i):
    case = CASES[key]
    lo, hi = window(case)
    gs, ge = global_rows(case, i)
    n = len(gs)
    nb, R, nch, ng, E, rcap = chunking(n, hi - lo)
    nt = nb * PSUB
    g0, g1 = np.clip(gs, lo, hi) - lo, np.clip(ge, lo, hi) - lo
    t = np.minimum(g0 >> BSH, nb - 1)
    o = np.minimum(g0 - (t << BSH), BIN - 1)
    length = np.maximum(g1 - g0, 0)
    l = np.minimum(np.minimum(length, LMAX), BIN - o)
    wrem = g1 > g0 + l                                    # k_bin_write -> cross
    q = np.minimum(o >> PSH, PSUB - 1)
    qend = (q + 1) << PSH
    l2 = np.where(o + l > qend, qend - o, l)
    srem = l2 < l                                         # k_bin_split_atomic -> cross
    bin0 = t << BSH
    xs = np.concatenate([(g0 + l)[wrem], (bin0 + o + l2)[srem]])
    xe = np.concatenate([g1[wrem], (bin0 + o + l)[srem]])
    t0, t1 = xs >> PSH, (xe - 1) >> PSH
    diff = np.zeros(nt + 2, np.int64)
    full = t1 > t0 + 1
    np.add.at(diff, t0[full] + 1, 1)
    np.add.at(diff, t1[full], -1)
    chunk = np.arange(n) // R
    grp = group_of_chunk(nch, ng)
    bc = np.zeros((nb, nch), np.int64)
    np.add.at(bc, (t, chunk), 1)
    bg = np.zeros((nb, ng), np.int64)
    np.add.at(bg, (t, grp[chunk] if n else chunk), 1)
    tile = np.bincount(t * PSUB + q, minlength=nt)
    return dict(
        n=n, nb=nb, nt=nt, R=R, nch=nch, ng=ng, E=E, rcap=rcap,
        rows_per_chunk=np.bincount(chunk, minlength=nch),
        chunks_per_group=np.bincount(grp, minlength=ng),
        bin_chunk=bc, bin_group=bg, tile=tile,
        lmax_pieces=int((l == LMAX).sum()), write_rem=int(wrem.sum()), split_rem=int(srem.sum()),
        cross_span=np.bincount(t1 - t0, minlength=6) if len(t0) else np.zeros(6, np.int64),
        cross_on_tile_end=int(((xe & (TILE - 1)) == 0).sum()),
        full_tiles=np.flatnonzero(np.cumsum(diff)[:nt] > 0),
        pad_lookalike=int(((o << LENB | np.minimum(length, LMAX)) == SLAB_PAD).sum()),
        two_word_rows=int((((g0 + np.maximum(l2, 1) - 1) >> 6) - (g0 >> 6) <= 1).sum()),
        three_word_rows=int((((g0 + np.maximum(l2, 1) - 1) >> 6) - (g0 >> 6) == 2).sum()))


def binning(case, i):
    """the counts bin_rows' kernels branch on, for row set i of the case"""
    return _binning(case["key"], i)


def fused_slot(case, op, idx, nt):
    """k_paint_ev's slot (EvPlan::prepare): from the operands' runs bound (a
    row set's rows; the contigs + 1 for NOT)"""
    bound = (len(case["lens"]) + 1 if op == 1 else 0) + sum(len(case["sets"][i][0]) for i in idx)
    cap = 2 * (2 * bound // max(nt, 1)) + 2048
    return min(max((cap + 255) // 256 * 256, EVSLOT_MIN), EVSLOT_MAX)


def pads_per_tile(case, tile_bits, before):
    """contig pads in [tile start - before, tile end) of each tile of the
    window (the word paths stage from the word before the tile: before = 64)"""
    off = offsets(case["lens"])
    lo, hi = window(case)
    pads = off[1:] - 1
    nt = (hi - lo + 63) // 64 * 64 // tile_bits + 1
    t0 = lo + np.arange(nt) * tile_bits
    return np.searchsorted(pads, t0 + tile_bits, "left") - \
        np.searchsorted(pads, np.maximum(t0 - before, lo), "left")


@functools.lru_cache(maxsize=None)
def _events(key, op, idx):
    case = CASES[key]
    lo, hi = window(case)
    gs, ge = reference_global(case, op, idx)
    n_words = (hi - lo + 63) // 64
    ev = np.concatenate([gs, ge]) - lo
    out = {}
    for name, tw in (("ev2048", EV_TW), ("ev4096", BT)):
        out[name] = np.bincount(ev // (tw * 64), minlength=n_words // tw + 1)
    # k_paint_ev: the bit before a tile taken as 0, a run reaching the tile's
    # end closed there: two events per run per tile it has a bit in
    nt = n_bins(hi - lo) * PSUB
    d = np.zeros(nt + 1, np.int64)
    np.add.at(d, (gs - lo) >> PSH, 1)
    np.add.at(d, ((ge - 1 - lo) >> PSH) + 1, -1)
    out["paint"] = 2 * np.cumsum(d)[:nt]
    out["n_words"] = n_words
    return out


def events(case, op, idx):
    """events of op's result per one-pass tile, per two-pass tile and per
    paint tile (as k_paint_ev counts them)"""
    return _events(case["key"], op, tuple(idx))


def path(case, op, idx, binned):
    """the line LIME_TRACE_RUNS prints for this op: binned = every operand
    still holds its binned rows"""
    ev = events(case, op, idx)
    words = "words one-pass" if ev["ev2048"].max() <= EVCAP else "words two-pass"
    if ev["n_words"] == 0:
        words = "empty window"
    if not binned or ev["n_words"] == 0:
        return words
    slot = fused_slot(case, op, idx, len(ev["paint"]))
    return "fused" if ev["paint"].max() <= slot else "fused overflow, " + words


# ----------------------------------------------------------- planted cases
CASES = {}


def _case(key, lens, sets, ops, window=None, **claims):
    assert key not in CASES
    sets = [_ro(*s) for s in sets]
    CASES[key] = dict(key=key, lens=tuple(int(x) for x in lens), sets=sets, ops=ops,
                      window=window, claims=claims)
    return CASES[key]


def _rows0(pairs):
    """(start, end) pairs on contig 0"""
    a = np.array(pairs, np.int64).reshape(-1, 2)
    return np.zeros(len(a), np.int64), a[:, 0], a[:, 1]


ROW_LENGTHS = (0, 1, 63, 64, 65, 128, 129, 510, 511, 512, 513)
WORD_BITS = (0, 63, 64)
EDGE = (-1, 0, 1)


def _piece_rows():
    """group a: every length on every word phase, starts and ends around tile
    and bin bounds, the SLAB_PAD look-alike, cross pieces over 0 .. 4 tiles"""
    r = []
    base = 3 * TILE + 4096
    for i, ln in enumerate(ROW_LENGTHS):            # lengths x word phases, 2048 apart
        for j, b in enumerate(WORD_BITS):
            s = base + (3 * i + j) * 2048 + b
            r.append((s, s + ln))
    for k, bound in enumerate((5 * TILE, 6 * TILE, BIN, 2 * BIN)):
        for d in EDGE:                              # starts at bound - 1, bound, bound + 1
            r.append((bound + d, bound + d + (1, 5, 511, 513)[k]))
    r += [(7 * TILE - 40, 7 * TILE), (8 * TILE - 40, 8 * TILE + 1)]      # ends on / past a tile end
    r += [(BIN + 9 * TILE - 300, BIN + 9 * TILE)]
    r += [(2 * BIN - 700, 2 * BIN - 100), (3 * BIN - 40, 3 * BIN), (3 * BIN - 90, 3 * BIN - 49)]
    r += [(10 * BIN - 40, 10 * BIN + 1)]            # ends one past a bin end
    r += [(9 * TILE - 100, 9 * TILE + 411)]         # a 511-base bin piece the split cuts
    r += [(BIN - 1, BIN), (3 * BIN - 1, 3 * BIN + 510)]   # on a bin's last bit: 1 and 511 bases
    for k in range(5):                              # cross pieces over t1 - t0 = 0 .. 4 tiles
        s = 4 * BIN + 20 * k * TILE + 700
        r.append((s, s + 600 + k * TILE))
    r += [(4 * BIN + 110 * TILE - 511, 4 * BIN + 112 * TILE)]   # its cross piece starts on a tile bound
    r += [(10 * TILE + 50, 10 * TILE + 90)] * 3     # exact duplicates
    r += [(11 * TILE + 100, 11 * TILE + 5000), (11 * TILE + 200, 11 * TILE + 300),
          (11 * TILE + 100, 11 * TILE + 101), (11 * TILE + 4999, 11 * TILE + 5000)]   # nested
    return r


PIECE_LEN = 11 * BIN + 5 * TILE + 12345


def _second_rows():
    """a second operand over the same space: overlaps, covers and misses"""
    r = [(3 * TILE, 3 * TILE + 40000), (5 * TILE - 3, 5 * TILE + 2), (BIN - 10, BIN + 10),
         (7 * TILE - 1, 7 * TILE + 1), (4 * BIN + 600, 4 * BIN + 41 * TILE + 5),
         (11 * TILE + 250, 11 * TILE + 4000), (3 * BIN - 1, 3 * BIN)]
    r += [(12 * TILE + 64 * k, 12 * TILE + 64 * k + 1 + k % 63) for k in range(500)]
    return r


def _shuffled(rows, seed):
    rng = np.random.default_rng(seed)
    c, s, e = rows
    o = rng.permutation(len(s))
    return c[o], s[o], e[o]


def _build_pieces():
    A = _shuffled(_rows0(_piece_rows()), 1)
    B = _shuffled(_rows0(_second_rows()), 2)
    _case("pieces", [PIECE_LEN], [A, B], [(0, (0,)), (1, (0,)), (2, (0, 1)), (3, (0, 1)), (3, (1, 0)),
                                          (4, (0, 1, 0))],
          cross_spans=(0, 1, 2, 3, 4), pad_lookalike=3)
    # one row covering the whole window; a tile wholly covered as a, as the
    # complemented b of a & ~b and as the complemented a of ~a
    L = 2 * BIN + 3 * TILE + 77
    whole = _rows0([(0, L)])
    some = _rows0([(5, 9), (TILE - 1, TILE + 1), (3 * TILE, 4 * TILE), (BIN - 1, BIN + 1),
                   (L - 1, L), (2 * BIN + TILE + 3, 2 * BIN + TILE + 514)])
    _case("whole", [L], [whole, some], [(0, (0,)), (1, (0,)), (2, (1, 0)), (3, (1, 0)), (3, (0, 1)),
                                        (2, (0, 0))], full_tiles=(L >> PSH) - 1)


# group b: row counts, skew, contig tables, global windows
COUNTS = (0, 1, 3, 4, 5, STEP - 1, STEP, STEP + 1, 2 * STEP + 5)
B_LEN = 2 * BIN + 5 * TILE + 999       # 3 bins
IN_TILE = (8191, 8192, 8193)


def _spread(n, seed, length, lo=0, maxlen=300):
    rng = np.random.default_rng(seed)
    s = lo + rng.integers(0, length - maxlen, n)
    return np.zeros(n, np.int64), s, s + rng.integers(0, maxlen, n)


def _build_counts():
    for n in COUNTS:
        _case("count_%d" % n, [B_LEN], [_spread(n, 100 + n, B_LEN), _spread(777, 99, B_LEN, maxlen=5000)],
              [(0, (0,)), (1, (0,)), (3, (1, 0))], n=n)
    # n rows in ONE paint tile (of bin 1), five elsewhere: a chunk wholly in a
    # tile, a (bin, chunk group) and a paint tile of 8191 / 8192 / 8193 rows
    for n in IN_TILE:
        i = np.arange(n)
        # (1500 groups of touching rows: 3000 events, inside the fused slot)
        s = BIN + 2 * TILE + (i % 1500) * 300 + (i // 1500) * 5
        rows = (np.zeros(n + 5, np.int64), np.concatenate([s, [3, TILE, 2 * BIN + 1, BIN - 2, 9]]),
                np.concatenate([s + 5 + i % 7, [9, TILE + 1, 2 * BIN + 3, BIN + 2, 9]]))
        _case("in_tile_%d" % n, [B_LEN], [rows], [(0, (0,)), (1, (0,))], in_tile=n)
    # 17 chunks (16 chunk groups, the last of two chunks): the rows of chunks
    # 15 and 16 -- 16385 of them -- in one paint tile of bin 2, the rest in
    # bin 0; bin 1 and most tiles empty
    n = 15 * STEP + 16385
    i = np.arange(n)
    # (groups of touching rows, so that no tile's events pass the fused slot)
    s = np.where(i < 15 * STEP, (i % 4000) * 2000 + (i // 4000) * 7,
                 2 * BIN + TILE + (i % 1200) * 400 + ((i // 1200) % 14) * 6)
    rows = (np.zeros(n, np.int64), s, s + 7 + i % 11)
    _case("chunks_17", [B_LEN], [rows], [(0, (0,)), (1, (0,))], nch=17, ng=16, big=16385)
    # an operand with no rows inside a k-way AND
    none = (np.zeros(0, np.int64),) * 3
    _case("and_empty", [B_LEN], [_spread(3000, 5, B_LEN, maxlen=9000), none,
                                 _spread(3000, 6, B_LEN, maxlen=9000)],
          [(4, (0, 1, 2)), (4, (0, 2)), (0, (1,)), (1, (1,)), (3, (0, 1))])
    # CMAX and CMAX + 1 contigs: the contig table in LDS / in global memory
    for nc in (CMAX, CMAX + 1):
        rng = np.random.default_rng(nc)
        lens = rng.integers(3000, 9000, nc)
        m = 6000
        c = rng.integers(0, nc, m)
        c[:4] = (0, nc - 1, nc - 1, nc - 2)
        s = (rng.random(m) * (lens[c] - 600)).astype(np.int64)
        e = s + rng.integers(0, 600, m)
        e[1] = lens[nc - 1]                        # reaches the last contig's end
        _case("contigs_%d" % nc, lens, [(c, s, e)], [(0, (0,)), (1, (0,))], nc=nc)
    # global rows through bitset_from_global: windows of one and two bins'
    # width, rows left of, right of and straddling them, clamped at hi
    G_LEN = 4 * BIN
    for nbw in (1, 2):
        lo = BIN - 64 * 1000
        hi = lo + nbw * BIN
        rng = np.random.default_rng(nbw)
        s = rng.integers(0, G_LEN - 3000, 20000)
        e = s + rng.integers(0, 900, 20000)
        s = np.concatenate([s, [lo - 700, lo - 1, lo, hi - 1, hi - 300, hi, hi + 5, 0, lo - 9,
                                hi - 511, G_LEN - 10]])
        e = np.concatenate([e, [lo + 800, lo + 1, lo + 1, hi, hi + 300, hi + 9, hi + 6, lo, lo,
                                hi + 2000, G_LEN]])
        _case("window_%d" % nbw, [G_LEN], [(s, e), (np.minimum(s[::3] + 100, G_LEN), np.minimum(e[::3] + 700, G_LEN))],
              [(0, (0,)), (1, (0,)), (2, (0, 1)), (3, (0, 1))], window=(lo, hi), bins=nbw)


# group c: optimistic binning at its smallest size: 8 bins, one chunk
OPT_LEN = 7 * BIN + 63              # span 7 * 2^23 + 64: just over 7 bins
OPT_BIG = 97 * BIN                  # the space of the 96- and 97-bin windows


def opt_rows(in_bin3, lookalike=False, n=STEP):
    """n rows of which exactly in_bin3 start in bin 3, the others dealt evenly
    over bins 0, 1, 2, 4, 5, 6; in shuffled order"""
    i = np.arange(n)
    rest = n - in_bin3
    b = np.where(i < in_bin3, 3, np.array([0, 1, 2, 4, 5, 6])[i % 6])
    s = b * BIN + (i * 4099) % (BIN - 1000)
    e = s + 1 + i % 40
    if lookalike:                   # the packed word 0xffffffff before its length is clamped
        s[0], e[0] = 4 * BIN - 1, 4 * BIN + 510
    assert rest >= 0
    return _shuffled((np.zeros(n, np.int64), s, e), in_bin3)


def _build_opt():
    nb, R, nch, ng, E, rcap = chunking(STEP, OPT_LEN + 1)
    assert (nb, nch, rcap) == (8, 1, 2016)
    _case("opt_exact", [OPT_LEN], [opt_rows(rcap)], [(0, (0,))], region=rcap, overflow=False)
    _case("opt_over", [OPT_LEN], [opt_rows(rcap + 1)], [(0, (0,))], region=rcap + 1, overflow=True)
    _case("opt_one_bin", [OPT_LEN], [opt_rows(STEP)], [(0, (0,))], region=STEP, overflow=True)
    _case("opt_lookalike", [OPT_LEN], [opt_rows(rcap, True)], [(0, (0,))], region=rcap,
          overflow=False, pad_lookalike=1)
    two = [np.concatenate([x, y + (50 if j else 0)])      # each chunk: rcap rows in bin 3
           for j, (x, y) in enumerate(zip(opt_rows(rcap), opt_rows(rcap)))]
    _case("opt_two_chunks", [OPT_LEN], [two], [(0, (0,))], region=rcap, overflow=False)
    _case("opt_and", [OPT_LEN], [opt_rows(rcap - 7), opt_rows(rcap + 1), opt_rows(rcap - 9)],
          [(4, (0, 1, 2))], overflow=True)
    # windows over one large contig, global rows: 7 bins (counted), 96 bins
    # (E = 128: optimistic), 64 bits wider (E < 128: counted)
    for name, hi in (("opt_7_bins", 7 * BIN), ("opt_96_bins", 96 * BIN), ("opt_97_bins", 96 * BIN + 64)):
        i = np.arange(STEP)
        nbw = hi // BIN
        s = (i % nbw) * BIN + (i * 523) % (BIN - 100)
        _case(name, [OPT_BIG], [(s, s + 1 + i % 50)], [(0, (0,))], window=(0, hi))


# group d: the word paths' extraction
D_WORDS = 3 * BT                     # n_words a multiple of both tile sizes


def _edge_runs():
    """runs on bits 0 and 63, across words, 8-word threads, 512-word waves and
    2048- / 4096-word tiles, ending on a tile end, starting on a tile start"""
    r = [(0, 1), (63, 64), (126, 130), (64 * 3, 64 * 4), (64 * 5 + 63, 64 * 6 + 1)]
    for w in (8, 16, 512, 1024, EV_TW, BT):          # across the boundary at word w
        r.append((64 * w - 1, 64 * w + 1))
    r.append((64 * 3 * EV_TW - 40, 64 * 3 * EV_TW))   # ends on a tile end
    r.append((64 * 2 * BT, 64 * 2 * BT + 3))          # starts on a tile start (of both tilings)
    r.append((64 * 5 * EV_TW, 64 * 5 * EV_TW + 64 * 9))
    r.append((64 * 3000 - 9, 64 * 3000 + 64 * 9))
    return r


def dense(start, nruns):
    """nruns one-base runs two bits apart from `start`"""
    s = start + 2 * np.arange(nruns)
    return list(zip(s.tolist(), (s + 1).tolist()))


def _build_words():
    L = 64 * D_WORDS - 1             # the pad is the window's last bit
    _case("w_edges", [L], [_rows0(_edge_runs()), _rows0([(0, 64 * 9), (64 * 500, 64 * 1030),
                                                         (64 * BT - 1, 64 * BT + 1)])],
          [(0, (0,)), (1, (0,)), (2, (0, 1)), (3, (0, 1)), (4, (0, 1, 0))])
    # a run reaching the window's end: n_words a multiple of 2048, not one, odd
    for nw in (EV_TW, 2 * BT, BT + 77, 2 * EV_TW + 1):
        hi = 64 * nw
        rows = (np.array([5, hi - 130, hi - 64, hi + 9]), np.array([9, hi - 128, hi + 700, hi + 99]))
        _case("w_end_%d" % nw, [64 * 3 * BT], [rows, (np.array([0]), np.array([hi - 1]))],
              [(0, (0,)), (1, (0,)), (3, (0, 1))], window=(0, hi), n_words=nw)
        if nw % 2:      # the same behind an event-dense tile: the two-pass path's odd last word
            d = np.array(dense(640, 1100))
            rows2 = (np.concatenate([rows[0], d[:, 0]]), np.concatenate([rows[1], d[:, 1]]))
            _case("w_end2_%d" % nw, [64 * 3 * BT], [rows2, (np.array([0]), np.array([hi - 1]))],
                  [(0, (0,)), (1, (0,)), (3, (0, 1)), (2, (0, 1))], window=(0, hi), n_words=nw)
    # tile 1 of 2048 words with exactly 2048 (one pass), 2049 and 2050 events
    t1 = 64 * EV_TW
    tail = (t1 + 64 * EV_TW - 20, t1 + 64 * EV_TW + 20)     # starts in tile 1, ends in tile 2
    other = _rows0([(0, t1 + 3000), (t1 + 5001, 64 * D_WORDS - 7)])
    for ev, rows in ((2048, dense(t1 + 10, 1024)), (2049, dense(t1 + 10, 1024) + [tail]),
                     (2050, dense(t1 + 10, 1025))):
        A = _rows0(rows + [(77, 99)])
        _case("w_dense_%d" % ev, [L], [A, other] + [A] * 15,
              [(0, (0,)), (1, (0,)), (2, (0, 1)), (3, (0, 1)), (3, (1, 0)), (4, (0, 1, 0)),
               (4, tuple(range(16))), (4, tuple(range(17)))], events=ev)


# group e: the fused extraction
def _build_fused():
    L = 2 * BIN + 3 * TILE + 64 * 100 + 17     # the last tile cut by the window's end
    r = [(TILE - 9, TILE + 9),                             # across one tile boundary
         (3 * TILE + 5, 7 * TILE - 5),                     # whole tiles 4, 5, 6 inside one run
         (8 * TILE - 30, 8 * TILE), (8 * TILE, 8 * TILE + 1),     # last bit + next first bit: joined
         (10 * TILE - 30, 10 * TILE), (10 * TILE + 1, 10 * TILE + 2),   # next first bit clear
         (12 * TILE + 64 * 16 - 3, 12 * TILE + 64 * 16 + 3),      # on a thread's 16-word boundary
         (12 * TILE + 64 * 32, 12 * TILE + 64 * 48), (12 * TILE + 64 * 64 - 1, 12 * TILE + 64 * 64),
         (L - 40, L), (2 * BIN + 3 * TILE - 2, 2 * BIN + 3 * TILE + 2)]
    B = [(TILE - 100, TILE + 100), (4 * TILE, 5 * TILE), (8 * TILE - 1, 8 * TILE + 1),
         (10 * TILE - 1, 10 * TILE + 2), (L - 70, L - 10)]
    _case("f_edges", [L], [_rows0(r), _rows0(B)],
          [(0, (0,)), (1, (0,)), (2, (0, 1)), (3, (0, 1)), (3, (1, 0)), (4, (0, 1, 0))])
    # a tile with exactly `slot` events, the closing event included, and the
    # next count up.  (Counted k_paint_ev's way a tile's events are even --
    # two per run with a bit in it -- so slot + 2 is the first count past it)
    for runs in (EVSLOT_MIN // 2, EVSLOT_MIN // 2 + 1):
        rows = dense(TILE + 10, runs - 1) + [(2 * TILE - 5, 2 * TILE + 5)]
        _case("f_slot_%d" % (2 * runs), [L], [_rows0(rows)], [(0, (0,))], events=2 * runs)
    # NOT with bits past hi_bit: a window ending inside a word, mid-contig
    lo, hi = 64 * 7, BIN + TILE + 64 * 3 + 5
    rows = (np.array([lo + 3, hi - 200, hi - 3, BIN - 7]), np.array([lo + 9, hi - 100, hi + 50, BIN + 7]))
    _case("f_not_window", [L], [rows], [(0, (0,)), (1, (0,))], window=(lo, hi))


# group f: pads under NOT.  Equal contigs `stride` bits apart; the most pads
# any tile holds (from the word before it on the word paths) is the claim
PAD_WORDS = {63: 2082, 64: 2049, 65: 2018, 130: 1009}      # one-pass tiles (2048 words)
PAD_WORDS2 = {63: 4163, 64: 4098, 65: 4034, 130: 2018}     # two-pass tiles (4096 words)
PAD_PAINT = {64: 8192, 65: 8066, 128: 4096, 129: 4065}     # paint tiles (2^19 bits)
PAD_KINDS = ("empty", "full", "alternate")
DENSE_LEN = 300000                   # a last, long contig for the event-dense tile


def pad_rows(lens, kind, dense_in_last=False):
    nc = len(lens) - (1 if dense_in_last else 0)
    c = np.arange(nc)
    if kind == "empty":
        c = c[:0]
    elif kind == "alternate":
        c = c[::2]
    rows = (c, np.zeros(len(c), np.int64), np.asarray(lens, np.int64)[c])
    if dense_in_last:                # 1100 one-base runs: ~2200 events of a and of ~a
        s = 70000 + 2 * np.arange(1100)
        rows = (np.concatenate([rows[0], np.full(1100, nc)]), np.concatenate([rows[1], s]),
                np.concatenate([rows[2], s + 1]))
    return rows


def _build_pads():
    for table, tile_bits, tag in ((PAD_WORDS, 64 * EV_TW, "p1"), (PAD_WORDS2, 64 * BT, "p2"),
                                  (PAD_PAINT, TILE, "pf")):
        for want, stride in table.items():
            nc = 3 * tile_bits // stride + 40
            two_pass = tag == "p2"
            lens = [stride - 1] * nc + ([DENSE_LEN] if two_pass else [])
            sets = [pad_rows(lens, k, two_pass) for k in PAD_KINDS]
            _case("%s_%d" % (tag, want), lens, sets, [(1, (0,)), (1, (1,)), (1, (2,)), (0, (2,))],
                  pads=want, tile_bits=tile_bits)
    # a pad on bit 63 of the word before a tile, and on a tile's first bit, for
    # both word tilings and the paint tiles; contigs of 1, 63 and 64 bases
    # (the filler contig puts a pad on the same bit of paint tile 1)
    for name, first in (("pad_bit63", BT * 64 - 1), ("pad_bit0", BT * 64)):
        lens = [first, 1, 63, 64, 1, 1, 63]
        lens += [TILE + first - BT * 64 - int(offsets(lens)[-1]), 500, 64, 1]
        sets = [pad_rows(lens, k) for k in PAD_KINDS]
        _case(name, lens, sets, [(1, (0,)), (1, (1,)), (1, (2,)), (0, (2,))], first=first)


for _b in (_build_pieces, _build_counts, _build_opt, _build_words, _build_fused, _build_pads):
    _b()


def contig_rows(case, i):
    """row set i as (contig, start, end), or None for global rows"""
    rows = case["sets"][i]
    return rows if len(rows) == 3 else None


def sortable(case, idx):
    """a sorted set can stand for these operands: contig rows, whole space"""
    return case.get("window") is None and all(len(case["sets"][i]) == 3 for i in idx)


SMALL = [k for k, c in CASES.items() if offsets(c["lens"])[-1] <= PAINT_MAX]
