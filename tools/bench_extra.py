"""Supplementary benchmark lines for BASELINE.json configs C3, C4 and C5 and
the 8(f) rows (bench.py measures the headline config C2).  Single GPU; one JSON line each.

  C3  merge of 5e8 ChIP-seq-like pile-ups (2e6 centres, N(0,150) offsets,
      len U[150,600], seeds 0xC / 0xD): sort + merge with run ids.
      unit: intervals/s
  C4  difference + complement against hg38 via the bit-per-base path:
      A, B = 1e7 rows, len U[50,500], seeds 0xD / 0xE: unsorted rows ->
      bitsets (rows binned by 65536-base bin, painted per tile) ->
      complement(merge(A)) runs (NOT) and merge(A) minus merge(B) runs
      (AND-NOT).  unit: bases/s (G/t)
  C5  8-way intersection over 1e9 rows (8 x 1.25e8, len U[10,40], seeds
      0x50..0x57): unsorted rows -> bitsets (binned paint) -> 8-way AND
      runs.  On one GPU
      (the whole genome); unit: intervals/s
  bed BED text parse on the device (lime_bed_parse_device, 8(f) row 1):
      1e7 BED6 lines over hg38 (host text, H2D inside the call); unit:
      lines/s, with the host reader (lime_bed_read, 1 thread) beside it
  subtract DistributedSubtract (lime mode) on C2's inputs: sort + A minus B
  window   DistributedWindow, distance 1000, on C2's inputs (8(f) row 3):
      sort + window join, every record filled through a 32 GiB buffer
  closest  SingleClosest on C2's inputs (8(f) row 4): RegionOrdering sort +
      plan + fill
  closest_single  SingleClosestSingleOverlap (sequential chain per contig) on
      1/100 of C2's rows
  b1_merge  north_star's 1B-interval target, merge side: 1e9 ChIP-seq-like
      pile-up rows (4e6 centres, N(0,150), len U[150,600], seed 0x1B; the
      rows of tests/test_gpu_scale.py): sort + merge (run ids) + complement
  b1_pair   north_star's 1B-interval target, pairwise side: 2 x 5e8 rows
      uniform over hg38, len U[10,40] (seeds 0x1A / 0x1C, as the scale
      tests): sort both + intersect (every pair filled through a 2^31-record
      buffer) + subtract in lime and set mode

  coverage  depth-of-coverage runs (lime_coverage) of a sorted set: --input
      pileup (C3's 5e8 rows) or uniform (1e8 rows as C2's A); the time of
      merge on the same set and of the sort of the ends alone beside it, and
      the depth_stats identity (sum of width x depth == sum of input widths)

  annotate  per-row hits, covered bases and overlap (lime_annotate) of C2's A
      by C2's B (2 x 1e8 rows, seeds 0xA / 0xB, sorted outside the timed
      region), the intersect count pass on the same sets beside it, and the
      identity sum(n_hits) == the plan's pair count

  multiinter  membership runs and m-of-8 consensus (lime_multiinter) of C5's 8
      sets (8 x 1.25e8 rows, len U[10,40], seeds 0x50..0x57; built and sorted
      outside the timed region): membership mode, min_sets = 5 and min_sets =
      8, each timed by device events; beside them the sort of the events alone
      (as many zero-width global rows as the call sorts) and C5's own path
      (bitset_and_from_device + its runs from the unsorted rows), the only
      answer the bit-per-base path has to any of these.  Identities: min_sets
      = 8 against the C5 runs (count and covered bases), and the membership
      depth_bases against the sum of the sets' bitset popcounts

Inputs are generated on the device (counter-based RNG) outside the timed
region; every step starts from unsorted rows in HBM.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 8000.0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--workload", required=True,
                   choices=["c3", "c4", "c5", "bed", "closest", "closest_single", "window",
                            "subtract", "b1_merge", "b1_pair", "coverage", "annotate",
                            "multiinter"])
    p.add_argument("--input", choices=["pileup", "uniform"], default="pileup",
                   help="coverage: C3's pile-up rows or uniform rows as C2's")
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--scale", type=float, default=1.0, help="row-count scale (testing)")
    a = p.parse_args()

    import torch
    import lime_amd
    from lime_amd import synth
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = lime_amd.Context(0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    space = lime_amd.Space(list(synth.HG38.keys()), list(synth.HG38.values()))
    G = int(sum(synth.HG38.values()))

    def ev():
        e = torch.cuda.Event(enable_timing=True)
        e.record(stream)
        return e

    def gen(n, seed, lo, hi, pile=None):
        c = torch.empty(n, dtype=torch.int32, device=dev)
        s = torch.empty(n, dtype=torch.int32, device=dev)
        e = torch.empty(n, dtype=torch.int32, device=dev)
        if pile:
            ctx.synth_pileup(space, n, seed, pile[0], pile[1], lo, hi, c.data_ptr(), s.data_ptr(),
                             e.data_ptr())
        else:
            ctx.synth_uniform(space, n, seed, lo, hi, c.data_ptr(), s.data_ptr(), e.data_ptr())
        return n, c, s, e

    def mkset(x):
        n, c, s, e = x
        return ctx.set_from_device(space, n, c.data_ptr(), s.data_ptr(), e.data_ptr())

    def bits(x):
        n, c, s, e = x
        return ctx.bitset_from_device(space, n, c.data_ptr(), s.data_ptr(), e.data_ptr())

    if a.workload == "bed":
        bed_bench(a, ctx, space)
        return
    step_ms = None  # a workload's own per-step time (device events), else the host clock's
    if a.workload == "c3":
        inp = gen(int(5e8 * a.scale), 0xC, 150, 600, pile=(2_000_000, 150))
        n = inp[0]

        def step(rec):
            t0 = ev()
            S = mkset(inp)
            t1 = ev()
            m = ctx.merge(S)
            t2 = ev()
            rec.append((t0, t1, t2, m.n))
            m.close()
            S.close()
        units, unit = n, "intervals/s"
        desc = f"C3: sort + merge (run ids) of {n} pile-up intervals (2e6 centres, N(0,150), " \
               "len U[150,600])"

        def roof(rec):
            t0, t1, t2, runs = rec[-1]
            ms = t1.elapsed_time(t2)
            b = 12 * n + 8 * runs  # read gs+ge, write run id per row, write runs
            return {"sort_ms": t0.elapsed_time(t1), "merge_ms": ms, "runs": runs}, \
                {"kernel": "k_merge_scan (single pass, decoupled look-back)", "bound": "hbm",
                 "achieved": b / (ms * 1e-3) / 1e9, "alg_bytes": b}
    elif a.workload == "coverage":
        if a.input == "pileup":
            inp = gen(int(5e8 * a.scale), 0xC, 150, 600, pile=(2_000_000, 150))
            what = "C3's pile-up intervals (2e6 centres, N(0,150), len U[150,600])"
        else:
            inp = gen(int(1e8 * a.scale), 0xA, 50, 5000)
            what = "uniform intervals over hg38 (len U[50,5000], as C2's)"
        n = inp[0]
        S = mkset(inp)  # (sorted outside the timed region: coverage takes a set)
        widths = int((inp[3].to(torch.int64) - inp[2].to(torch.int64)).sum().item())

        def step(rec):
            t0 = ev()
            r = ctx.coverage(S)
            t1 = ev()
            m = ctx.merge(S)
            t2 = ev()
            # the sort of the ends alone, as lime_coverage runs it: the set's
            # ends as the starts of zero-width global rows
            gs, ge, row = S.device_arrays()
            E = ctx.set_from_global(space, n, ge, ge, row)
            t3 = ev()
            rec.append((t0, t1, t2, t3, r.n, r.depth_stats()))
            for h in (E, m, r):
                h.close()
        units, unit = n, "intervals/s"
        desc = f"coverage: depth runs of {n} sorted {what}"

        def step_ms(recs):  # the rate is the coverage call's, not the comparisons'
            return sum(r[0].elapsed_time(r[1]) for r in recs) / len(recs)

        def roof(rec):
            t0, t1, t2, t3, runs, (cov, db, mx) = rec[-1]
            ms, sort_ms = t0.elapsed_time(t1), t2.elapsed_time(t3)
            b = 16 * n + 12 * runs  # two walks over gs + sorted ends, the runs written
            walk = max(ms - sort_ms, 1e-6)
            return {"coverage_ms": ms, "merge_ms (same set)": t1.elapsed_time(t2),
                    "sort_of_ends_ms": sort_ms, "sort_share": sort_ms / ms, "runs": runs,
                    "covered_bases": cov, "depth_bases": db, "input_widths": widths,
                    "depth_bases_equals_input_widths": db == widths, "max_depth": mx}, \
                {"kernel": "k_cov count + fill (merge path over starts and sorted ends)",
                 "bound": "hbm", "achieved": b / (walk * 1e-3) / 1e9, "alg_bytes": b}
    elif a.workload == "annotate":
        na = nb_ = int(1e8 * a.scale)
        A_in, B_in = gen(na, 0xA, 50, 5000), gen(nb_, 0xB, 50, 5000)
        A, B = mkset(A_in), mkset(B_in)  # (sorted outside the timed region)
        n = na

        def step(rec):
            t0 = ev()
            an = ctx.annotate(A, B)
            t1 = ev()
            plan = ctx.intersect(A, B)  # the count pass alone: the grand total only
            t2 = ev()
            rec.append((t0, t1, t2, an.totals(), plan.n))
            plan.close()
            an.close()
        units, unit = n, "rows of A/s"
        desc = f"annotate: hits, covered bases and overlap of {na} rows by {nb_} rows (C2's " \
               "sets, uniform over hg38, len U[50,5000])"

        def step_ms(recs):
            return sum(r[0].elapsed_time(r[1]) for r in recs) / len(recs)

        def roof(rec):
            t0, t1, t2, (rows_hit, pairs, cov, ov), n_pairs = rec[-1]
            ms = t0.elapsed_time(t1)
            m = ctx.merge(B)
            nr = m.n
            m.close()
            # per row of B: the sort of the ends (sort.hip's budget for a 12-B
            # row is not counted), S and E widened (4 + 8) and scanned (8 + 8
            # + 8) twice, merge (8), both staged once by k_annotate (8); per
            # run 8 written, widths 8 + 4, scan 12, staged 4; per row of A 8
            # read and 16 written; the gathers (4 x 8 B + up to 6 x 4 B per row
            # of A, mostly cache hits) are not counted
            b = nb_ * (2 * (12 + 24) + 8 + 8) + nr * 36 + na * 24
            return {"annotate_ms": ms, "intersect_count_ms (same sets)": t1.elapsed_time(t2),
                    "rows_hit": rows_hit, "pairs": pairs, "covered_bases": cov,
                    "overlap_bases": ov, "intersect_n_pairs": n_pairs,
                    "pairs_equals_intersect_count": pairs == n_pairs, "runs_of_b": nr}, \
                {"kernel": "lime_annotate (sort of ends, scans, merge, k_ann_split, k_annotate)",
                 "bound": "hbm", "achieved": b / (ms * 1e-3) / 1e9, "alg_bytes": b}
    elif a.workload == "multiinter":
        k = 8
        per = int(1.25e8 * a.scale)
        ins = [gen(per, 0x50 + i, 10, 40) for i in range(k)]
        sets = [mkset(x) for x in ins]  # (sorted outside the timed region)
        pops = []
        for x in sets:  # the bases of every set, one bitset at a time
            b = ctx.bitset(x)
            pops.append(b.popcount())
            b.close()
        n = k * per
        # as many events as the call sorts: both ends of every set's merge runs
        n_ev = 0
        for x in sets:
            m = ctx.merge(x)
            n_ev += 2 * m.n
            m.close()
        ev_keys = torch.empty(max(n_ev, 1), dtype=torch.int32, device=dev)
        tmp = [torch.empty(per, dtype=torch.int32, device=dev) for _ in range(2)]
        at = 0
        for x in sets:  # (any keys of the right count and range: the sets' starts)
            take = min(x.n, n_ev - at)
            x.copy_rows_device(0, take, ev_keys[at:].data_ptr(), tmp[0].data_ptr(),
                               tmp[1].data_ptr())
            at += take
        ctx.synchronize()
        del tmp
        while at < n_ev:  # fewer rows than events: repeat what is there
            take = min(at, n_ev - at)
            ev_keys[at:at + take].copy_(ev_keys[:take])
            at += take
        ev_rows = torch.zeros(n_ev, dtype=torch.int32, device=dev)

        def step(rec):
            t0 = ev()
            r0 = ctx.multiinter(sets, 0)
            t1 = ev()
            r5 = ctx.multiinter(sets, 5)
            t2 = ev()
            r8 = ctx.multiinter(sets, 8)
            t3 = ev()
            E = ctx.set_from_global(space, n_ev, ev_keys.data_ptr(), ev_keys.data_ptr(),
                                    ev_rows.data_ptr())
            t4 = ev()
            fused = ctx.bitset_and_from_device(
                space, [(x[0], x[1].data_ptr(), x[2].data_ptr(), x[3].data_ptr()) for x in ins])
            c5 = ctx.bitset_runs(0, fused)
            t5 = ev()
            h8 = r8.copy_range(0, r8.n) if r8.n else (None, None)
            cov8 = int((h8[1].astype("int64") - h8[0].astype("int64")).sum()) if r8.n else 0
            rec.append((t0, t1, t2, t3, t4, t5, r0.n, r5.n, r8.n, c5.n, r0.depth_stats(), cov8,
                        fused.popcount()))
            for h in (c5, fused, E, r8, r5, r0):
                h.close()
        units, unit = n, "intervals/s"
        desc = f"multiinter: membership runs of {k} x {per} sorted rows (C5's sets, len U[10,40])"

        def step_ms(recs):  # the rate is the membership call's
            return sum(r[0].elapsed_time(r[1]) for r in recs) / len(recs)

        def roof(rec):
            t0, t1, t2, t3, t4, t5, n0, n5, n8, nc5, (cov, db, mx), cov8, pop8 = rec[-1]
            ms, sort_ms = t0.elapsed_time(t1), t3.elapsed_time(t4)
            # the walks: k_mi_tile_xor (4) + k_mi twice (8 + 8) per event, 16 per run
            b = 20 * n_ev + 16 * n0
            walk = max(ms - sort_ms, 1e-6)
            return {"membership_ms": ms, "min_sets_5_ms": t1.elapsed_time(t2),
                    "min_sets_8_ms": t2.elapsed_time(t3), "sort_of_events_ms": sort_ms,
                    "sort_share": sort_ms / ms, "c5_bitset_and_runs_ms": t4.elapsed_time(t5),
                    "events": n_ev, "runs_membership": n0, "runs_min_sets_5": n5,
                    "runs_min_sets_8": n8, "runs_c5": nc5,
                    "depth_stats": {"covered_bases": cov, "depth_bases": db, "max_depth": mx},
                    "min_sets_8_equals_c5": n8 == nc5 and cov8 == pop8,
                    "depth_bases_equals_sum_of_popcounts": db == sum(pops)}, \
                {"kernel": "merges, event writes, k_mi_tile_xor + k_mi count + fill (all but "
                           "the sort of the events)",
                 "bound": "hbm", "achieved": b / (walk * 1e-3) / 1e9, "alg_bytes": b}
    elif a.workload == "b1_merge":
        inp = gen(int(1e9 * a.scale), 0x1B, 150, 600, pile=(4_000_000, 150))
        n = inp[0]

        def step(rec):
            t0 = ev()
            S = mkset(inp)
            t1 = ev()
            m = ctx.merge(S)
            t2 = ev()
            # the complement from the merge's runs (one merge scan per step,
            # as bench.py's C3 line): Complement.scala's gaps of merge(A)
            k = m.n
            rgs = torch.empty(max(k, 1), dtype=torch.int32, device=dev)
            rge = torch.empty(max(k, 1), dtype=torch.int32, device=dev)
            if k:
                m.copy_rows_device(0, k, rgs.data_ptr(), rge.data_ptr())
            c = ctx.complement_runs(space, k, rgs.data_ptr(), rge.data_ptr())
            t3 = ev()
            rec.append((t0, t1, t2, t3, m.n, c.n))
            for h in (c, m, S):
                h.close()
            del rgs, rge
        units, unit = n, "intervals/s"
        desc = f"1B merge side: sort + merge (run ids) + complement of {n} pile-up intervals " \
               "(4e6 centres, N(0,150), len U[150,600])"

        def roof(rec):
            t0, t1, t2, t3, runs, gaps = rec[-1]
            ms = t1.elapsed_time(t2)
            b = 12 * n + 8 * runs
            return {"sort_ms": t0.elapsed_time(t1), "merge_ms": ms,
                    "complement_ms": t2.elapsed_time(t3), "runs": runs, "gaps": gaps,
                    "sort_GBps_24B_per_row": 24 * n / (t0.elapsed_time(t1) * 1e-3) / 1e9}, \
                {"kernel": "k_merge_scan (single pass, decoupled look-back)", "bound": "hbm",
                 "achieved": b / (ms * 1e-3) / 1e9, "alg_bytes": b}
    elif a.workload == "b1_pair":
        ia = gen(int(5e8 * a.scale), 0x1A, 10, 40)
        ib = gen(int(5e8 * a.scale), 0x1C, 10, 40)
        n = ia[0]
        chunk = 1 << 31
        buf = torch.empty((chunk, 4), dtype=torch.int32, device=dev)

        def step(rec):
            t0 = ev()
            SA, SB = mkset(ia), mkset(ib)
            t1 = ev()
            plan = ctx.intersect(SA, SB)
            t2 = ev()
            for f in range(0, plan.n, chunk):
                plan.fill_device(f, min(chunk, plan.n - f), buf.data_ptr())
            t3 = ev()
            r0 = ctx.subtract(SA, SB, 0, 0)
            t4 = ev()
            r1 = ctx.subtract(SA, SB, 0, 1)
            t5 = ev()
            rec.append((t0, t1, t2, t3, t4, t5, plan.n, r0.n, r1.n))
            for h in (r1, r0, plan, SA, SB):
                h.close()
        units, unit = 2 * n, "intervals/s"
        desc = f"1B pairwise side: sort + intersect (every pair filled) + subtract (lime, set) " \
               f"of 2 x {n} intervals, uniform over hg38, len U[10,40]"

        def roof(rec):
            t0, t1, t2, t3, t4, t5, k, s0, s1 = rec[-1]
            ms = t2.elapsed_time(t3)
            b = 16 * k + 20 * 2 * n
            return {"sort_ms": t0.elapsed_time(t1), "count_ms": t1.elapsed_time(t2),
                    "fill_ms": ms, "subtract_lime_ms": t3.elapsed_time(t4),
                    "subtract_set_ms": t4.elapsed_time(t5), "pairs": k,
                    "remnants_lime": s0, "remnants_set": s1,
                    "sort_GBps_24B_per_row": 24 * 2 * n / (t0.elapsed_time(t1) * 1e-3) / 1e9}, \
                {"kernel": "k_fill (all launches)", "bound": "hbm",
                 "achieved": b / (ms * 1e-3) / 1e9, "alg_bytes": b}
    elif a.workload == "c4":
        ia = gen(int(1e7 * a.scale), 0xD, 50, 500)
        ib = gen(int(1e7 * a.scale), 0xE, 50, 500)

        def step(rec):
            t0 = ev()
            t1 = ev()
            # bit-per-base sets straight from the unsorted rows (binned paint)
            ba, bb = bits(ia), bits(ib)
            t2 = ev()
            comp = ctx.bitset_runs(1, ba)
            diff = ctx.bitset_runs(3, ba, bb)
            t3 = ev()
            rec.append((t0, t1, t2, t3, comp.n, diff.n))
            for h in (comp, diff, ba, bb):
                h.close()
        units, unit = G, "bases/s"
        desc = "C4: complement(merge(A)) and merge(A) \\ merge(B) on the hg38 bitset " \
               "(A, B = 1e7 rows, len U[50,500])"

        def roof(rec):
            t0, t1, t2, t3, nc, nd = rec[-1]
            ms = t2.elapsed_time(t3)
            n = int(1e7 * a.scale)
            # the binned rows read once (4 B each, both sets), every event
            # written to its tile slot and read back (4 + 4 B), the runs
            # stored (8 B): no bitset is stored or read on this path
            b = 4 * 2 * n + 8 * 2 * (nc + nd) + 8 * (nc + nd)
            return {"bitset_build_ms (bin, no paint)": t1.elapsed_time(t2),
                    "extract_ms (paint + ops + runs)": ms, "complement_runs": nc,
                    "difference_runs": nd}, \
                {"kernel": "k_paint_ev per op (paint, op, events per tile slot) + "
                           "k_ev_join + k_ev_gather",
                 "bound": "hbm",
                 "achieved": b / (ms * 1e-3) / 1e9, "alg_bytes": b}
    elif a.workload == "subtract":
        # DistributedSubtract (lime mode) on C2's inputs: A minus B, every
        # remnant materialised (contig-local start / end, a_row, b_row)
        ia = gen(int(1e8 * a.scale), 0xA, 50, 5000)
        ib = gen(int(1e8 * a.scale), 0xB, 50, 5000)
        n = ia[0]

        def step(rec):
            t0 = ev()
            SA, SB = mkset(ia), mkset(ib)
            t1 = ev()
            r = ctx.subtract(SA, SB)
            t2 = ev()
            rec.append((t0, t1, t2, r.n))
            r.close()
            SA.close()
            SB.close()
        units, unit = 2 * n, "intervals/s"
        desc = f"subtract (lime mode): sort + A minus B of 2 x {n} intervals, uniform over " \
               "hg38, len U[50,5000] (C2's inputs)"

        def roof(rec):
            t0, t1, t2, k = rec[-1]
            ms = t1.elapsed_time(t2)
            # A rows (gs, ge, row) + B's gs / ge / row / prefix max + 16 B per remnant
            b = 12 * n + 16 * n + 16 * k
            return {"sort_ms": t0.elapsed_time(t1), "subtract_ms": ms, "remnants": k}, \
                {"kernel": "subtract (B's merge runs + k_sub_count_runs + k_subtract write)",
                 "bound": "hbm",
                 "achieved": b / (ms * 1e-3) / 1e9, "alg_bytes": b}
    elif a.workload == "window":
        # DistributedWindow (distance 1000) on C2's inputs: every pair within
        # 1000 bases, 16-B records chunked through a reusable 32 GiB buffer
        ia = gen(int(1e8 * a.scale), 0xA, 50, 5000)
        ib = gen(int(1e8 * a.scale), 0xB, 50, 5000)
        n = ia[0]
        chunk = 1 << 31
        buf = torch.empty((chunk, 4), dtype=torch.int32, device=dev)

        def step(rec):
            t0 = ev()
            SA, SB = mkset(ia), mkset(ib)
            t1 = ev()
            plan = ctx.window(SA, SB, 1000)
            t2 = ev()
            for f in range(0, plan.n, chunk):
                plan.fill_device(f, min(chunk, plan.n - f), buf.data_ptr())
            t3 = ev()
            rec.append((t0, t1, t2, t3, plan.n))
            plan.close()
            SA.close()
            SB.close()
        units, unit = 2 * n, "intervals/s"
        desc = f"window (distance 1000): sort + window join of 2 x {n} intervals, uniform " \
               "over hg38, len U[50,5000] (C2's inputs)"

        def roof(rec):
            t0, t1, t2, t3, k = rec[-1]
            ms = t2.elapsed_time(t3)
            b = 16 * k  # the fill's records
            return {"sort_ms": t0.elapsed_time(t1), "plan_ms": t1.elapsed_time(t2),
                    "fill_ms": ms, "pairs": k}, \
                {"kernel": "k_fill (window records, all launches)", "bound": "hbm",
                 "achieved": b / (ms * 1e-3) / 1e9, "alg_bytes": b}
    elif a.workload in ("closest", "closest_single"):
        # SingleClosest on C2's inputs: sets sorted in full RegionOrdering.
        # closest_single: SingleClosestSingleOverlap, whose (j, p) chain runs
        # in order (one wave per contig): C2's density on 1/100 of the rows
        mode = 1 if a.workload == "closest_single" else 0
        sc = a.scale * (0.01 if mode else 1.0)
        ia = gen(int(1e8 * sc), 0xA, 50, 5000)
        ib = gen(int(1e8 * sc), 0xB, 50, 5000)
        n = ia[0]

        def sset(x):
            m, c, s, e = x
            return ctx.set_from_device_stranded(space, m, c.data_ptr(), s.data_ptr(),
                                                e.data_ptr())

        def step(rec):
            t0 = ev()
            SA, SB = sset(ia), sset(ib)
            t1 = ev()
            plan = ctx.closest(SA, SB, mode)
            out = torch.empty((max(plan.n, 1), 4), dtype=torch.int32, device=dev)
            t2 = ev()
            plan.fill_device(0, plan.n, out.data_ptr())
            t3 = ev()
            rec.append((t0, t1, t2, t3, plan.n))
            plan.close()
            SA.close()
            SB.close()
        units, unit = 2 * n, "intervals/s"
        desc = f"closest ({'SingleClosestSingleOverlap' if mode else 'SingleClosest'}): sort " \
               f"(RegionOrdering) + closest of 2 x {n} intervals, uniform over hg38, " \
               "len U[50,5000]" + (" (1/100 of C2's rows)" if mode else " (C2's inputs)")

        def roof(rec):
            t0, t1, t2, t3, k = rec[-1]
            ms = t1.elapsed_time(t3)
            b = 12 * 2 * n + 16 * k  # read both sets once, write the records
            return {"sort_ms": t0.elapsed_time(t1), "plan_ms": t1.elapsed_time(t2),
                    "fill_ms": t2.elapsed_time(t3), "pairs": k}, \
                {"kernel": "closest plan + fill (per-left searches)", "bound": "hbm",
                 "achieved": b / (ms * 1e-3) / 1e9, "alg_bytes": b}
    else:
        k = 8
        per = int(1.25e8 * a.scale)
        ins = [gen(per, 0x50 + i, 10, 40) for i in range(k)]

        def step(rec):
            t0 = ev()
            t1 = ev()
            # bit-per-base sets straight from the unsorted rows (binned paint)
            bs = [bits(x) for x in ins]
            t2 = ev()
            r = ctx.bitset_and(bs)
            t3 = ev()
            rec.append((t0, t1, t2, t3, r.n))
            for h in [r] + bs:
                h.close()
        units, unit = k * per, "intervals/s"
        desc = f"C5: {k}-way intersection, {k} x {per} rows (len U[10,40]) on 1 GPU, bitset AND"

        def roof(rec):
            t0, t1, t2, t3, nr = rec[-1]
            ms = t2.elapsed_time(t3)
            W = (space.span + 63) // 64 * 8
            b = k * W + 8 * nr  # every operand read once (single-pass extraction)
            return {"bitset_build_ms (bin + paint)": t1.elapsed_time(t2),
                    "and_extract_ms": ms, "runs": nr}, \
                {"kernel": "8-way AND + extraction (k_ev_local + k_ev_gather)", "bound": "hbm",
                 "achieved": b / (ms * 1e-3) / 1e9, "alg_bytes": b}

    torch.cuda.synchronize(dev)
    rec = []
    for _ in range(a.warmup):
        step(rec)
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    for _ in range(a.steps):
        step(rec)
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t) / a.steps
    if step_ms:
        dt = step_ms(rec[-a.steps:]) * 1e-3
    br, rf = roof(rec)
    rf["peak"], rf["unit"] = HBM, "GB/s"
    rf["frac"] = rf["achieved"] / HBM
    print(json.dumps({"workload": a.workload, "config": desc, "value": units / dt, "unit": unit,
                      "ms_per_step": dt * 1e3, "steps": a.steps, "breakdown_ms": br,
                      "roofline": rf}), flush=True)
    ctx.close()


def bed_bench(a, ctx, space):
    import tempfile

    import numpy as np
    import torch
    from lime_amd.engine import read_bed
    n = int(1e7 * a.scale)
    rng = np.random.default_rng(9)
    names = np.array(space.names)
    c = rng.integers(0, len(names), n)
    s = rng.integers(0, 150_000_000, n)
    e = s + rng.integers(50, 5000, n)
    st = rng.choice(np.array(["+", "-", "."]), n)
    lines = np.char.add(np.char.add(np.char.add(names[c], "\t"), s.astype(str)), "\t")
    lines = np.char.add(np.char.add(lines, e.astype(str)), "\tr\t0\t")
    lines = np.char.add(lines, st)
    text = ("\n".join(lines.tolist()) + "\n").encode()
    del lines
    ts = []
    for r in range(a.warmup + a.steps):
        t = time.perf_counter()
        d = ctx.parse_bed(text)
        ctx.synchronize()
        ts.append(time.perf_counter() - t)
        assert d.n == n
        d.close()
    dt = sorted(ts[a.warmup:])[len(ts[a.warmup:]) // 2]
    # the pageable H2D share, warm, same median rule (the cold first copy
    # includes allocator and page-pinning setup and overstates it)
    buf = torch.frombuffer(bytearray(text), dtype=torch.uint8)
    g = torch.empty_like(buf, device="cuda:0")
    hs = []
    for r in range(a.warmup + a.steps):
        t = time.perf_counter()
        g.copy_(buf)
        torch.cuda.synchronize()
        hs.append(time.perf_counter() - t)
    h2d = sorted(hs[a.warmup:])[len(hs[a.warmup:]) // 2]
    del g
    with tempfile.NamedTemporaryFile(suffix=".bed", dir="/dev/shm" if os.path.isdir("/dev/shm")
                                     else None) as f:
        f.write(text)
        f.flush()
        t = time.perf_counter()
        host = read_bed(f.name)
        th = time.perf_counter() - t
    assert len(host["start"]) == n
    print(json.dumps({"workload": "bed", "config": f"device BED parse of {n} BED6 lines "
                      f"({len(text) / 1e9:.2f} GB text, host memory, H2D inside the call)",
                      "value": n / dt, "unit": "lines/s", "ms_per_step": dt * 1e3,
                      "steps": a.steps, "text_GBps_end_to_end": len(text) / dt / 1e9,
                      "breakdown_ms": {"h2d_pageable_ms": h2d * 1e3,
                                       "device_ms_excl_h2d": (dt - h2d) * 1e3},
                      "host_reader": {"value": n / th, "unit": "lines/s", "cores": 1,
                                      "kind": "lime_bed_read (bed.cpp), incl. file read"}}),
          flush=True)


if __name__ == "__main__":
    main()
