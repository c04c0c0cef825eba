"""tests/bitset_cases.py on the CPU: its reference against one boolean per base
and against the oracle's merge / complement / subtract, its constants against
the kernel file, and every planted case on the arm it claims -- as numbers of
the arm counter, printed so that a run shows which edges the GPU tests of
tests/test_gpu_bitset_edges.py stand on."""
import re

import numpy as np
import pytest

from oracle import oracle
from tests import bitset_cases as bc

C = bc.CASES


def test_source_lines_still_stand():
    src = bc.source()
    for name, pat in bc.SOURCE_LINES.items():
        assert re.search(pat, src), name
    assert (bc.STEP, bc.WSTEP, bc.SPLIT_CH, bc.PAINT_BATCH) == (12288, 12288, 8192, 8192)
    assert (bc.EV_TW, bc.BT, bc.TWORDS, bc.LMAX, bc.PSUB) == (2048, 4096, 8192, 511, 16)
    assert bc.EVSLOT_MAX == 16384


# ------------------------------------------------------------- the reference
PAINTED = bc.SMALL + ["whole", "f_edges", "f_not_window", "count_5"]


@pytest.mark.parametrize("key", PAINTED)
def test_reference_against_per_base_paint(key):
    case = C[key]
    for op, idx in case["ops"]:
        gs, ge = bc.reference_global(case, op, idx)
        ps, pe = bc.paint(case, op, idx)
        assert np.array_equal(gs, ps) and np.array_equal(ge, pe), (key, op, idx)
        c, s, e, pop = bc.reference(case, op, idx)
        assert pop == int((pe - ps).sum())
        assert (e <= np.asarray(case["lens"])[c]).all() and (s >= 0).all()


def _coalesce(res):
    c, s, e = (np.asarray(res[k]).astype(np.int64) for k in ("contig", "start", "end"))
    keep = e > s
    c, s, e = c[keep], s[keep], e[keep]
    if len(c) == 0:
        return c, s, e
    new = np.concatenate([[True], (c[1:] != c[:-1]) | (s[1:] != e[:-1])])
    first = np.flatnonzero(new)
    last = np.concatenate([first[1:] - 1, [len(c) - 1]])
    return c[first], s[first], e[last]


ORACLE = ["pieces", "whole", "count_5", "count_12289", "in_tile_8193", "contigs_1025", "w_edges",
          "w_dense_2050", "f_edges", "p1_65", "p2_130", "pf_129", "pad_bit0", "pad_bit63"]


@pytest.mark.parametrize("key", ORACLE)
def test_reference_against_oracle(key):
    case = C[key]
    lens = list(case["lens"])
    seen = 0
    for op, idx in case["ops"]:
        rows = [bc.contig_rows(case, i) for i in idx]
        rows = [(r[0].astype(np.int32), r[1], r[2]) for r in rows]
        if op == 0:
            exp = oracle.merge(rows[0])
        elif op == 1:
            exp = oracle.complement(rows[0], lens)
        elif op == 3:
            ma, mb = oracle.merge(rows[0]), oracle.merge(rows[1])
            exp = oracle.subtract((ma["contig"], ma["start"], ma["end"]),
                                  (mb["contig"], mb["start"], mb["end"]), 0, oracle.SUB_SET)
        else:
            continue
        got = bc.reference(case, op, idx)
        for g, w in zip(got[:3], _coalesce(exp)):
            assert np.array_equal(g, w), (key, op)
        seen += 1
    assert seen


def test_no_operand_covers_a_pad():
    # (op 0 of the engine paints rows as given: the reference masks nothing)
    for key, case in C.items():
        off = bc.offsets(case["lens"])
        for i in range(len(case["sets"])):
            gs, ge = bc.global_rows(case, i)
            c = np.searchsorted(off, gs, "right") - 1
            assert (ge <= off[c + 1] - 1).all() and (gs >= 0).all() and (ge >= gs).all(), key


# ------------------------------------------------------------------ the arms
def test_a_row_pieces():
    b = bc.binning(C["pieces"], 0)
    print("pieces", {k: b[k] for k in ("n", "nb", "lmax_pieces", "write_rem", "split_rem",
                                       "cross_span", "cross_on_tile_end", "pad_lookalike",
                                       "three_word_rows", "two_word_rows")})
    for k in C["pieces"]["claims"]["cross_spans"]:
        assert b["cross_span"][k] >= 1, k
    # (511 bases and more from a bin's last bit: at bins 1, 2 and 3)
    assert b["pad_lookalike"] == 3 and b["cross_on_tile_end"] >= 1
    assert b["lmax_pieces"] >= 10 and b["write_rem"] >= 10 and b["split_rem"] >= 3
    assert b["three_word_rows"] >= 3 and b["nb"] == 12
    gs, ge = bc.global_rows(C["pieces"], 0)
    ln = ge - gs
    for want in bc.ROW_LENGTHS:
        for bit in (0, 63):
            assert ((ln == want) & (gs % 64 == bit)).any(), (want, bit)
    for bound in (5 * bc.TILE, bc.BIN, 2 * bc.BIN):
        for d in bc.EDGE:
            assert (gs == bound + d).any()
        assert (ge == 7 * bc.TILE).any() and (ge == 8 * bc.TILE + 1).any()
        assert (ge == 3 * bc.BIN).any() and (ge == 10 * bc.BIN + 1).any()
    # the 511-base row the split cuts, and the rows on a bin's last bit
    assert ((gs == 9 * bc.TILE - 100) & (ln == 511)).any()
    assert ((gs == bc.BIN - 1) & (ln == 1)).any() and ((gs == 3 * bc.BIN - 1) & (ln == 511)).any()
    assert len(np.unique(np.stack([gs, ge]), axis=1)[0]) < len(gs)   # duplicates
    w = bc.binning(C["whole"], 0)
    assert len(w["full_tiles"]) == C["whole"]["claims"]["full_tiles"] == 34
    assert w["cross_span"][5:].sum() == 1 and w["n"] == 1


def test_b_row_counts_and_skew():
    for n in bc.COUNTS:
        b = bc.binning(C["count_%d" % n], 0)
        want = [min(bc.STEP, n - c * bc.STEP) for c in range(b["nch"])] if n else [0]
        assert b["rows_per_chunk"].tolist() == want and b["n"] == n
        print("count", n, "chunks", b["nch"], "groups", b["ng"], b["rows_per_chunk"].tolist())
    for n in bc.IN_TILE:
        b = bc.binning(C["in_tile_%d" % n], 0)
        assert b["tile"][bc.PSUB + 2] == n and b["bin_group"][1, 0] == n and b["nch"] == 1
        assert bc.path(C["in_tile_%d" % n], 0, (0,), True) == "fused"
        assert (b["tile"] == 0).sum() >= 40
    b = bc.binning(C["chunks_17"], 0)
    assert (b["nch"], b["ng"]) == (17, 16)
    assert b["chunks_per_group"].tolist() == [1] * 15 + [2]
    assert b["bin_group"][2, 15] == b["tile"][2 * bc.PSUB + 1] == 16385
    assert b["bin_chunk"][1].sum() == 0                      # an empty bin between full ones
    assert b["rows_per_chunk"][-1] == 16385 - bc.STEP
    assert bc.path(C["chunks_17"], 0, (0,), True) == "fused"
    print("chunks_17", b["chunks_per_group"].tolist(), int(b["bin_group"].max()), int(b["tile"].max()))
    assert len(C["and_empty"]["sets"][1][0]) == 0
    assert [len(C["contigs_%d" % nc]["lens"]) for nc in (bc.CMAX, bc.CMAX + 1)] == [1024, 1025]
    for nbw in (1, 2):
        case = C["window_%d" % nbw]
        lo, hi = case["window"]
        gs, ge = bc.global_rows(case, 0)
        assert bc.binning(case, 0)["nb"] == nbw and lo % 64 == 0 and (hi - lo) == nbw * bc.BIN
        assert (ge <= lo).any() and (gs >= hi).any() and ((gs < lo) & (ge > lo)).any()
        assert ((gs < hi) & (ge > hi)).any() and (gs == hi).any() and (ge == lo).any()


def test_c_optimistic_regions():
    rcap = 2016
    for key in ("opt_exact", "opt_over", "opt_one_bin", "opt_lookalike", "opt_two_chunks"):
        b = bc.binning(C[key], 0)
        cl = C[key]["claims"]
        assert (b["nb"], b["rcap"]) == (8, rcap) and b["E"] >= 128.0
        assert b["bin_chunk"].max() == cl["region"]
        assert (b["bin_chunk"].max() > rcap) == cl["overflow"]
        assert b["pad_lookalike"] == cl.get("pad_lookalike", 0)
        print(key, "E %.2f" % b["E"], "slots", b["rcap"], "fullest region", int(b["bin_chunk"].max()))
    assert bc.binning(C["opt_two_chunks"], 0)["nch"] == 2
    assert (bc.binning(C["opt_two_chunks"], 0)["bin_chunk"][3] == rcap).all()
    over = [int(bc.binning(C["opt_and"], i)["bin_chunk"].max() > rcap) for i in range(3)]
    assert over == [0, 1, 0]
    b7, b96, b97 = (bc.binning(C["opt_%d_bins" % k], 0) for k in (7, 96, 97))
    assert (b7["nb"], b7["rcap"]) == (7, 0)
    assert (b96["nb"], b96["E"], b96["rcap"]) == (96, 128.0, 204) and b96["bin_chunk"].max() == 128
    assert b97["nb"] == 97 and b97["E"] < 128.0 and b97["rcap"] == 0
    # a region overflow sets bin_pessimism to 32; the counted rerun of the same
    # set spends one, so the next 31 builds are counted and the 32nd is
    # optimistic again
    assert bc.PESSIMISM - 1 == 31


def test_d_word_path_events():
    for ev in (2048, 2049, 2050):
        case = C["w_dense_%d" % ev]
        e = bc.events(case, 0, (0,))
        assert e["ev2048"][1] == ev and e["ev2048"].max() == ev
        want = "words one-pass" if ev <= bc.EVCAP else "words two-pass"
        assert bc.path(case, 0, (0,), False) == want
        print("w_dense", ev, e["ev2048"].tolist(), e["ev4096"].tolist())
    case = C["w_dense_2050"]
    two = {op for op, idx in case["ops"] if bc.path(case, op, idx, False) == "words two-pass"}
    assert two == {0, 1, 2, 3, 4}
    assert {len(idx) for op, idx in case["ops"] if op == 4} == {3, 16, 17}
    gs, ge = bc.reference_global(C["w_edges"], 0, (0,))
    for w in (2, 8, 512, bc.EV_TW, bc.BT):
        assert ((gs < 64 * w) & (ge > 64 * w)).any(), w
    assert (ge == 64 * 3 * bc.EV_TW).any() and (gs == 64 * 2 * bc.BT).any()
    assert (gs % 64 == 0).any() and (gs % 64 == 63).any() and (ge % 64 == 0).any()
    for nw in (bc.EV_TW, 2 * bc.BT, bc.BT + 77, 2 * bc.EV_TW + 1):
        case = C["w_end_%d" % nw]
        e = bc.events(case, 0, (0,))
        assert e["n_words"] == nw
        assert bc.reference_global(case, 0, (0,))[1][-1] == 64 * nw     # reaches the window's end
        assert e["ev2048"][nw // bc.EV_TW] >= 1 and e["ev4096"][nw // bc.BT] >= 1
        if nw % 2:      # the pair load's one-word tail, on both word paths
            case = C["w_end2_%d" % nw]
            assert bc.path(case, 0, (0,), False) == "words two-pass"
            assert bc.reference_global(case, 0, (0,))[1][-1] == 64 * nw


def test_e_fused_events():
    case = C["f_edges"]
    e = bc.events(case, 0, (0,))
    assert e["paint"][4:7].tolist() == [2, 2, 2]        # whole tiles inside one run
    assert bc.fused_slot(case, 0, (0,), 48) == bc.EVSLOT_MIN
    gs, ge = bc.reference_global(case, 0, (0,))
    assert ((gs < 8 * bc.TILE) & (ge == 8 * bc.TILE + 1)).any()        # joined
    assert (ge == 10 * bc.TILE).any() and (gs == 10 * bc.TILE + 1).any()   # not joined
    assert ge[-1] == case["lens"][0]
    for ev in (4096, 4098):
        case = C["f_slot_%d" % ev]
        e = bc.events(case, 0, (0,))
        assert e["paint"][1] == ev == e["paint"].max()
        assert bc.fused_slot(case, 0, (0,), len(e["paint"])) == 4096
        assert (e["paint"] % 2 == 0).all()
        print("f_slot", ev, bc.path(case, 0, (0,), True))
    assert bc.path(C["f_slot_4096"], 0, (0,), True) == "fused"
    assert bc.path(C["f_slot_4098"], 0, (0,), True) == "fused overflow, words two-pass"
    lo, hi = C["f_not_window"]["window"]
    assert hi % 64 and lo % 64 == 0


def test_f_pads_per_tile():
    for table, tag, before, tile_bits in ((bc.PAD_WORDS, "p1", 64, 64 * bc.EV_TW),
                                          (bc.PAD_WORDS2, "p2", 64, 64 * bc.BT),
                                          (bc.PAD_PAINT, "pf", 0, bc.TILE)):
        for want in table:
            case = C["%s_%d" % (tag, want)]
            p = bc.pads_per_tile(case, tile_bits, before)
            print(tag, want, "stride", table[want], "pads per tile", p.tolist())
            assert p.max() == want == case["claims"]["pads"]
            for op, idx in case["ops"]:
                assert bc.path(case, op, idx, True) == "fused"
                assert bc.path(case, op, idx, False) == \
                    ("words two-pass" if tag == "p2" else "words one-pass")
    # on the one-pass tiles the two-pass spaces hold more than a batch as well
    assert bc.pads_per_tile(C["p2_130"], 64 * bc.EV_TW, 64).max() == 65
    for key, bit in (("pad_bit63", 63), ("pad_bit0", 0)):
        pads = bc.offsets(C[key]["lens"])[1:] - 1
        first = C[key]["claims"]["first"]
        assert pads[0] == first and first % 64 == bit and (first + (bit == 63)) % (64 * bc.BT) == 0
        assert (pads == bc.TILE + first - 64 * bc.BT).any()
        assert {1, 63, 64} <= set(C[key]["lens"])
