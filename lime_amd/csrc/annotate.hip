// annotate.hip -- per row of A: how many rows of B hit it, how many of its
// bases they cover, and the sum of their overlaps (bedtools coverage -a A -b B,
// intersect -c, annotate), without materialising a pair.
//
// For a = [s, e) and B on the same contig, under the strict half-open
// predicate  b.start < a.end && b.end > a.start  (SURVEY.md Appendix A.2):
//       n_hits(a)   = #{b : b hits a}
//       covered(a)  = |a n union(B)|                       (bases, u32)
//       overlap(a)  = sum over the hits of overlapsBy(a, b)        (u64)
// With S = B's sorted starts, E = B's ends sorted ascending, PS / PE their
// exclusive u64 prefix sums (n + 1 entries), (RS, RE) B's merge runs and PW the
// exclusive prefix sum of the run widths (PW <= span < 2^32), in GLOBAL
// coordinates:
//       D(x) = PE[ub(E,x)] + x (lb(S,x) - ub(E,x)) - PS[lb(S,x)]
//                                                     = sum_b |b n [0, x)|
//       C(x) = k = ub(RS,x);  k ? PW[k-1] + min(RE[k-1], x) - RS[k-1] : 0
//                                                     = |union(B) n [0, x)|
//       n_hits  = lb(S, a.e) - ub(E, a.s) + [a.s == a.e] #{b : b.s == b.e == a.s}
//       overlap = D(a.e) - D(a.s)
//       covered = C(a.e) - C(a.s)
// The bracket is the only zero-width correction: a zero-width b at a
// zero-width a's point is counted by ub(E, a.s) and not by lb(S, a.e), and is
// no hit.  Those rows are the front of B's gs == x group (the canonical order
// puts a start's zero-width rows first), so they are counted by two searches
// inside the group, and only when B has a zero-width row at all.  In D the zero-width rows cancel by
// themselves (the differences are taken in wrapping 64-bit arithmetic: lb(S,x)
// - ub(E,x) is negative by exactly those rows).  Merge runs do not join
// book-ended rows; C does not mind.  Contigs need no flags: off[c + 1] =
// off[c] + len[c] + 1 keeps one base between them, as in merge.hip and
// coverage.hip.  Strand is not looked at.
//
// Passes:
//   sort of the ends     sorted_ends (coverage.hip): E
//   k_ann_widen x 2      S, E widened to u64            4 B read, 8 B written / row of B
//   scan_exclusive_u64   PS, PE in place (two reads, one write)   24 B / row of B, x 2
//   merge_runs           RS, RE (merge.hip's budget)
//   k_ann_widths + scan_exclusive_u32   PW              <= 20 B / run
//   k_ann_split          lb(S,.), ub(E,.), ub(RS,.) of the first start of every
//                        tile of A, one thread per tile edge
//   k_annotate           per tile of AN_TILE rows of A (below)
//                                      8 B read + 16 B written / row of A,
//                                      12 B / row of B staged, the gathers on top
//   k_ann_totals         (lime_annot_totals only) 16 B / row of A
//
// k_annotate: A is sorted by start, so every a.s search of a tile falls
// between the tile's split positions and the next tile's.  Each of the three
// windows (of S, E, RS) that holds at most AN_W entries is staged in LDS, a
// longer one is searched in global memory (per array: a dispatch switch, block
// uniform).  a.e >= a.s, so the a.e searches start at the row's own a.s
// positions: a binary search of the rest of the staged window, and past the
// window (a long row) a gallop forward in global memory.  Every global load of
// the tile -- windows and rows -- is issued before the first LDS store.  The
// prefix sums and run ends are gathered from global memory at the positions
// found (six to ten loads per row, neighbours in a tile close together).
#include "common.hpp"

namespace lime {
namespace {

constexpr int ANB = 256;                 // threads per tile
constexpr int AN_ITEMS = 8;              // rows of A per thread
constexpr int AN_TILE = ANB * AN_ITEMS;  // rows of A per tile (tests: annotate_cases.T)
constexpr int AN_W = 4096;               // entries of a window staged in LDS (tests: annotate_cases.W)
constexpr int AN_WQ = AN_W / ANB;        // staging loads per thread and array

struct AnnArgs {
    const uint32_t *as, *ae;  // A, sorted
    int64_t na;
    const uint32_t *S, *Bge;  // B, sorted: starts, and the ends in that order
    const uint32_t *E;        // B's ends sorted
    int64_t nb;
    const uint64_t *PS, *PE;  // nb + 1 each
    const uint32_t *RS, *RE, *PW;
    int64_t nr;
    const uint32_t *split;  // 3 x (nt + 1): lb(S,.) | ub(E,.) | ub(RS,.) per tile edge
    int64_t nt;
    int zero;  // B has a zero-width row
    uint32_t *n_hits, *covered;
    uint64_t *overlap;
};

template <bool UB>
__device__ __forceinline__ bool below(uint32_t v, uint32_t key) {
    return UB ? v <= key : v < key;
}

// first index in [lo, hi) whose entry is not below key (hi when none)
template <bool UB>
__device__ __forceinline__ int64_t bsearch(const uint32_t *a, int64_t lo, int64_t hi,
                                           uint32_t key) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (below<UB>(a[mid], key))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
template <bool UB>
__device__ __forceinline__ int lds_search(const uint32_t *w, int lo, int hi, uint32_t key) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (below<UB>(w[mid], key))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// the same over [lo, n), every entry before lo being below key: steps of 1,
// 2, 4, ... forward, then a binary search of the last step
template <bool UB>
__device__ __forceinline__ int64_t gallop(const uint32_t *a, int64_t lo, int64_t n, uint32_t key) {
    int64_t step = 1;
    while (lo + step <= n && below<UB>(a[lo + step - 1], key)) {
        lo += step;
        step <<= 1;
    }
    const int64_t hi = lo + step - 1 < n ? lo + step - 1 : n;
    return bsearch<UB>(a, lo, hi, key);
}

// one array's window [w0, w1) of a tile: in LDS (w) when staged
struct Win {
    const uint32_t *g;  // the whole array
    const uint32_t *w;  // LDS image of g[w0, w1)
    int64_t w0, w1, n;
    bool staged;
};
// position of a start a.s of the tile: inside [w0, w1]
template <bool UB>
__device__ __forceinline__ int64_t find_in(const Win &x, uint32_t key) {
    if (x.staged) return x.w0 + lds_search<UB>(x.w, 0, (int)(x.w1 - x.w0), key);
    return bsearch<UB>(x.g, x.w0, x.w1, key);
}
// position of the row's end, at or after that of its start (from)
template <bool UB>
__device__ __forceinline__ int64_t find_from(const Win &x, int64_t from, uint32_t key) {
    int64_t r;
    if (x.staged)
        r = x.w0 + lds_search<UB>(x.w, (int)(from - x.w0), (int)(x.w1 - x.w0), key);
    else
        r = bsearch<UB>(x.g, from, x.w1, key);
    // past the window: the row outlasts every start of its tile
    if (r == x.w1 && r < x.n) r = gallop<UB>(x.g, r, x.n, key);
    return r;
}

// |union(B) n [0, x)| with k = ub(RS, x)
__device__ __forceinline__ uint32_t covered_below(const AnnArgs &a, int64_t k, uint32_t x) {
    if (k == 0) return 0;
    const uint32_t re = a.RE[k - 1];
    return a.PW[k - 1] + (re < x ? re : x) - a.RS[k - 1];
}

__global__ __launch_bounds__(ANB) void k_ann_widen(const uint32_t *__restrict__ in, int64_t n,
                                                   uint64_t *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * ANB;
    for (int64_t i = (int64_t)blockIdx.x * ANB + threadIdx.x; i < n; i += stride) out[i] = in[i];
}

__global__ __launch_bounds__(ANB) void k_ann_widths(const uint32_t *__restrict__ rs,
                                                    const uint32_t *__restrict__ re, int64_t n,
                                                    uint32_t *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * ANB;
    for (int64_t i = (int64_t)blockIdx.x * ANB + threadIdx.x; i < n; i += stride)
        out[i] = re[i] - rs[i];
}

// the three positions of tile edge t (t <= nt), one thread per edge so that
// the dependent loads of every edge's searches overlap (k_cov_split's lesson);
// edge nt is the LAST start of A, at or above every start of the last tile
__global__ __launch_bounds__(ANB) void k_ann_split(AnnArgs a, uint32_t *__restrict__ split) {
    const int64_t t = (int64_t)blockIdx.x * ANB + threadIdx.x;
    if (t > a.nt) return;
    const int64_t i = t * AN_TILE < a.na ? t * AN_TILE : a.na - 1;
    const uint32_t x = a.as[i];
    split[t] = (uint32_t)bsearch<false>(a.S, 0, a.nb, x);
    split[a.nt + 1 + t] = (uint32_t)bsearch<true>(a.E, 0, a.nb, x);
    split[2 * (a.nt + 1) + t] = (uint32_t)bsearch<true>(a.RS, 0, a.nr, x);
}

__global__ __launch_bounds__(ANB) void k_annotate(AnnArgs a) {
    __shared__ uint32_t sS[AN_W], sE[AN_W], sR[AN_W];
    const int64_t t = blockIdx.x, t0 = t * AN_TILE;
    Win wS, wE, wR;
    wS.g = a.S;
    wS.w = sS;
    wS.n = a.nb;
    wS.w0 = a.split[t];
    wS.w1 = a.split[t + 1];
    wE.g = a.E;
    wE.w = sE;
    wE.n = a.nb;
    wE.w0 = a.split[a.nt + 1 + t];
    wE.w1 = a.split[a.nt + 2 + t];
    wR.g = a.RS;
    wR.w = sR;
    wR.n = a.nr;
    wR.w0 = a.split[2 * (a.nt + 1) + t];
    wR.w1 = a.split[2 * (a.nt + 1) + t + 1];
    wS.staged = wS.w1 - wS.w0 <= AN_W;
    wE.staged = wE.w1 - wE.w0 <= AN_W;
    wR.staged = wR.w1 - wR.w0 <= AN_W;
    // the rows and the staged windows: every load before the first LDS store
    uint32_t s[AN_ITEMS], e[AN_ITEMS];
    {
        uint32_t vS[AN_WQ], vE[AN_WQ], vR[AN_WQ];
#pragma unroll
        for (int q = 0; q < AN_WQ; ++q) {
            const int64_t k = q * ANB + threadIdx.x;
            vS[q] = wS.staged && wS.w0 + k < wS.w1 ? a.S[wS.w0 + k] : 0u;
            vE[q] = wE.staged && wE.w0 + k < wE.w1 ? a.E[wE.w0 + k] : 0u;
            vR[q] = wR.staged && wR.w0 + k < wR.w1 ? a.RS[wR.w0 + k] : 0u;
        }
#pragma unroll
        for (int k = 0; k < AN_ITEMS; ++k) {
            const int64_t i = t0 + k * ANB + threadIdx.x;
            s[k] = i < a.na ? a.as[i] : 0u;
            e[k] = i < a.na ? a.ae[i] : 0u;
        }
#pragma unroll
        for (int q = 0; q < AN_WQ; ++q) {
            const int k = q * ANB + threadIdx.x;
            sS[k] = vS[q];
            sE[k] = vE[q];
            sR[k] = vR[q];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < AN_ITEMS; ++k) {
        const int64_t i = t0 + k * ANB + threadIdx.x;
        if (i >= a.na) continue;
        const uint32_t as = s[k], ae = e[k];
        const int64_t ls = find_in<false>(wS, as), us = find_in<true>(wE, as),
                      ks = find_in<true>(wR, as);
        const int64_t le = find_from<false>(wS, ls, ae), ue = find_from<true>(wE, us, ae),
                      ke = find_from<true>(wR, ks, ae);
        uint32_t hits = (uint32_t)(le - us);
        if (a.zero && as == ae) {
            // zero-width rows of B at this point: the front of the gs == as
            // group [ls, gend) (ge <= as holds for them and for no row after)
            const int64_t gend = gallop<true>(a.S, ls, a.nb, as);
            hits += (uint32_t)(bsearch<true>(a.Bge, ls, gend, as) - ls);
        }
        const uint64_t ov = (a.PE[ue] - a.PE[us]) + (uint64_t)ae * (uint64_t)(le - ue) -
                            (uint64_t)as * (uint64_t)(ls - us) - (a.PS[le] - a.PS[ls]);
        a.n_hits[i] = hits;
        a.covered[i] = covered_below(a, ke, ae) - covered_below(a, ks, as);
        a.overlap[i] = ov;
    }
}

// rows with a hit, sum of n_hits, sum of covered, sum of overlap
__global__ __launch_bounds__(256) void k_ann_totals(const uint32_t *__restrict__ n_hits,
                                                    const uint32_t *__restrict__ covered,
                                                    const uint64_t *__restrict__ overlap, int64_t n,
                                                    unsigned long long *__restrict__ out) {
    uint64_t rows = 0, pairs = 0, cov = 0, ov = 0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const uint32_t h = n_hits[i];
        rows += h > 0;
        pairs += h;
        cov += covered[i];
        ov += overlap[i];
    }
    rows = dev::wave_reduce_sum(rows);
    pairs = dev::wave_reduce_sum(pairs);
    cov = dev::wave_reduce_sum(cov);
    ov = dev::wave_reduce_sum(ov);
    if (dev::lane_id() == 0) {
        atomicAdd(&out[0], (unsigned long long)rows);
        atomicAdd(&out[1], (unsigned long long)pairs);
        atomicAdd(&out[2], (unsigned long long)cov);
        atomicAdd(&out[3], (unsigned long long)ov);
    }
}

unsigned grid_for(int64_t n) { return std::min<unsigned>(blocks_for(n, ANB), 8192u); }

}  // namespace

int annotate_run(lime_ctx *ctx, const lime_set *A, const lime_set *B, lime_annot *out) {
    const int64_t na = A->n, nb = B->n;
    out->n = na;
    LIME_TRY(alloc(ctx, &out->n_hits, (size_t)na));
    LIME_TRY(alloc(ctx, &out->covered, (size_t)na));
    LIME_TRY(alloc(ctx, &out->overlap, (size_t)na));
    if (na == 0) return LIME_OK;
    if (nb == 0) {
        LIME_HIP(hipMemsetAsync(out->n_hits, 0, 4 * (size_t)na, S(ctx)));
        LIME_HIP(hipMemsetAsync(out->covered, 0, 4 * (size_t)na, S(ctx)));
        LIME_HIP(hipMemsetAsync(out->overlap, 0, 8 * (size_t)na, S(ctx)));
        return LIME_OK;
    }
    // E; only its keys are read
    lime_set ends;
    LIME_TRY(sorted_ends(ctx, B, &ends));
    release(ctx, ends.ge);
    release(ctx, ends.row);
    // PS, PE: widened, then scanned in place; entry nb is the total
    PoolPtr<uint64_t> PS, PE;
    LIME_TRY(PS.alloc(ctx, (size_t)nb + 1));
    LIME_TRY(PE.alloc(ctx, (size_t)nb + 1));
    hipLaunchKernelGGL(k_ann_widen, dim3(grid_for(nb)), dim3(ANB), 0, S(ctx),
                       (const uint32_t *)B->gs, nb, PS.get());
    hipLaunchKernelGGL(k_ann_widen, dim3(grid_for(nb)), dim3(ANB), 0, S(ctx),
                       (const uint32_t *)ends.gs, nb, PE.get());
    LIME_HIP(hipGetLastError());
    LIME_TRY(scan_exclusive_u64(ctx, PS, PS, nb, PS + nb));
    LIME_TRY(scan_exclusive_u64(ctx, PE, PE, nb, PE + nb));
    // B's merge runs and the prefix of their widths
    lime_result runs;
    runs.ctx = ctx;
    {
        PlainView plain(B);
        LIME_TRY(merge_runs(ctx, &plain.v, &runs, false));
    }
    const int64_t nr = runs.n;
    PoolPtr<uint32_t> PW, split;
    LIME_TRY(PW.alloc(ctx, (size_t)nr));
    hipLaunchKernelGGL(k_ann_widths, dim3(grid_for(nr)), dim3(ANB), 0, S(ctx),
                       (const uint32_t *)runs.gs, (const uint32_t *)runs.ge, nr, PW.get());
    LIME_HIP(hipGetLastError());
    LIME_TRY(scan_exclusive_u32(ctx, PW, PW, nr, nullptr));
    const int64_t nt = (na + AN_TILE - 1) / AN_TILE;
    LIME_TRY(split.alloc(ctx, 3 * ((size_t)nt + 1)));
    AnnArgs a;
    a.as = A->gs;
    a.ae = A->ge;
    a.na = na;
    a.S = B->gs;
    a.Bge = B->ge;
    a.E = ends.gs;
    a.nb = nb;
    a.PS = PS;
    a.PE = PE;
    a.RS = runs.gs;
    a.RE = runs.ge;
    a.PW = PW;
    a.nr = nr;
    a.split = split;
    a.nt = nt;
    a.zero = B->has_zero_width;
    a.n_hits = out->n_hits;
    a.covered = out->covered;
    a.overlap = out->overlap;
    hipLaunchKernelGGL(k_ann_split, dim3(blocks_for(nt + 1, ANB)), dim3(ANB), 0, S(ctx), a,
                       split.get());
    hipLaunchKernelGGL(k_annotate, dim3((unsigned)nt), dim3(ANB), 0, S(ctx), a);
    LIME_HIP(hipGetLastError());
    return LIME_OK;
}

int annot_totals(lime_ctx *ctx, const lime_annot *an, uint64_t h[4]) {
    PoolPtr<unsigned long long> d_out;
    LIME_TRY(d_out.alloc(ctx, 4));
    LIME_HIP(hipMemsetAsync(d_out, 0, 32, S(ctx)));
    if (an->n > 0)
        hipLaunchKernelGGL(k_ann_totals, dim3(std::min<unsigned>(blocks_for(an->n, 256), 4096u)),
                           dim3(256), 0, S(ctx), (const uint32_t *)an->n_hits,
                           (const uint32_t *)an->covered, (const uint64_t *)an->overlap, an->n,
                           d_out.get());
    LIME_HIP(hipGetLastError());
    return read_back(ctx, h, d_out, 32);
}

}  // namespace lime
