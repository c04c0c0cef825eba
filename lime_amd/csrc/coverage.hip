// coverage.hip -- depth of coverage: the maximal runs of constant depth >= 1
// (what bedtools genomecov -bg writes as a bedGraph).
//
// depth(p) = #{rows r : gs_r <= p < ge_r}.  With S = the set's gs (sorted
// already) and E = its ge sorted ascending, for a coordinate x
//       after(x)  = ub(S, x) - ub(E, x)     depth on [x, next coordinate)
//       before(x) = lb(S, x) - lb(E, x)     depth just below x
// and x is a HEAD (the depth changes there) iff after(x) != before(x).  A
// head with after > 0 opens a run [x, .) of depth after(x); a head with
// before > 0 closes the run opened by the head before it.  Zero-width rows add
// one to both bounds of both terms and so cancel; book-ended rows [a, x),
// [x, b) leave after(x) == before(x): no head at x.  Contigs need no segment
// flags, as in merge.hip: off[c + 1] = off[c] + len[c] + 1 leaves one base of
// depth 0 between contigs, so the depth returns to 0 at or before a contig's
// last coordinate and a run never crosses into the next contig.
//
// The 2n events of S and E are merged by merge path, starts first among equal
// coordinates (the order inside a coordinate is irrelevant: only the first and
// the last event of a coordinate group are looked at).  At merged position
// (i, j) -- i starts and j ends consumed -- the depth is i - j, so
//       before(x) = i - j at the first event of x's group,
//       after(x)  = i - j past its last event:
// no prefix scan of deltas.  Tiles of CV_TILE events are cut by a diagonal
// binary search over (S, E) and staged in LDS with one event of look-ahead
// past the tile edge (is the tile's last event the last of its coordinate?)
// and one of look-behind (does the tile's first group continue an earlier
// one?).  Only for a group that straddles into the tile from earlier tiles
// does before(x) take two binary searches over the rows before the tile: it
// may have started many tiles back.
//
// Passes (count -> scan -> fill, as complement.hip):
//   sort of the ends   sort_set_global over (ge, ge, row): E; 3 x 4 B per row
//                      held until the fill is queued, then released
//   k_cov_split        the diagonal search of every tile edge, one thread each
//   k_cov<false>       per tile: heads with after > 0          8 B read / row
//   scan_exclusive_u32 over the tiles (2n / CV_TILE words)
//   k_cov<true>        the same walk, writing gs / depth at an opening head
//                      and ge of the run before at a closing one
//                                                   8 B read / row, 12 B / run
// Byte budget: 16 B per row read by the two walks + 12 B per run written, on
// top of the sort of the ends (sort.hip's budget for a 12-B row).
#include "common.hpp"

namespace lime {
namespace {

constexpr int CVB = 256;               // threads per tile
constexpr int CV_ITEMS = 8;            // merged events per thread
constexpr int CV_TILE = CVB * CV_ITEMS;  // events per tile (tests: coverage_cases.T)
constexpr uint32_t CV_NONE = 0xffffffffu;  // above every coordinate (< span <= 2^32 - 1)

struct CovArgs {
    const uint32_t *S, *E;  // sorted starts, sorted ends
    int64_t n;              // rows (events: 2n)
    const uint32_t *split;  // nt + 1: starts consumed before each tile (k_cov_split)
    const uint32_t *tbase;  // fill: opening heads before each tile
    uint32_t *cnt;          // count: opening heads of each tile
    uint32_t *ogs, *oge, *odepth;
    int64_t cap;            // runs the outputs hold
};

// starts consumed on merged diagonal d (ends: d - that), starts first among
// equal coordinates: the smallest i with S[i] > E[d - 1 - i]
__device__ __forceinline__ int64_t diag_split(const uint32_t *S, const uint32_t *E, int64_t n,
                                              int64_t d) {
    int64_t lo = d > n ? d - n : 0, hi = d < n ? d : n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (S[mid] <= E[d - 1 - mid])
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// split[t] = starts consumed before tile t (t <= nt): one thread per tile
// edge, so the ~log2(n) dependent loads of each search overlap those of every
// other edge (searched by the tile's own first threads they were a serial
// ~30-load prologue of every tile: both walks ran at 0.65 TB/s on C3)
__global__ __launch_bounds__(CVB) void k_cov_split(const uint32_t *__restrict__ S,
                                                   const uint32_t *__restrict__ E, int64_t n,
                                                   int64_t nt, uint32_t *__restrict__ split) {
    const int64_t t = (int64_t)blockIdx.x * CVB + threadIdx.x;
    if (t > nt) return;
    const int64_t d = t * CV_TILE < 2 * n ? t * CV_TILE : 2 * n;
    split[t] = (uint32_t)diag_split(S, E, n, d);
}

template <bool FILL>
__global__ __launch_bounds__(CVB) void k_cov(CovArgs a) {
    // sS[k] = S[i0 + k], k <= ns: the tile's starts and the one after them
    // (CV_NONE past the set); sE likewise
    __shared__ uint32_t sS[CV_TILE + 1], sE[CV_TILE + 1];
    __shared__ uint32_t scratch[CVB / 64 + 1];
    const int64_t n = a.n, total = 2 * n;
    const int64_t d0 = (int64_t)blockIdx.x * CV_TILE;
    const int64_t d1 = d0 + CV_TILE < total ? d0 + CV_TILE : total;
    const int64_t i0 = a.split[blockIdx.x], j0 = d0 - i0;
    const int ns = (int)((int64_t)a.split[blockIdx.x + 1] - i0), cnt = (int)(d1 - d0),
              ne = cnt - ns;
    // the ns + 1 starts and ne + 1 ends (cnt + 2 words) as one sequence, every
    // load issued before the first LDS store (loops over each array waited
    // for memory once per 256 words: 8 round trips per tile)
    {
        uint32_t v[CV_ITEMS + 1];
#pragma unroll
        for (int q = 0; q <= CV_ITEMS; ++q) {
            const int k = q * CVB + threadIdx.x, m = k - ns - 1;
            uint32_t x = CV_NONE;
            if (k <= ns) {
                if (i0 + k < n) x = a.S[i0 + k];
            } else if (m <= ne) {
                if (j0 + m < n) x = a.E[j0 + m];
            }
            v[q] = x;
        }
#pragma unroll
        for (int q = 0; q <= CV_ITEMS; ++q) {
            const int k = q * CVB + threadIdx.x, m = k - ns - 1;
            if (k <= ns)
                sS[k] = v[q];
            else if (m <= ne)
                sE[m] = v[q];
        }
    }
    __syncthreads();

    // the thread's CV_ITEMS events start on the tile's diagonal dl
    const int dl = min((int)threadIdx.x * CV_ITEMS, cnt);
    int sa, sb;
    {
        int lo = dl > ne ? dl - ne : 0, hi = dl < ns ? dl : ns;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sS[mid] <= sE[dl - 1 - mid])
                lo = mid + 1;
            else
                hi = mid;
        }
        sa = lo;
        sb = dl - lo;
    }
    // heads are decided at the LAST event of a coordinate group.  `before` is
    // known once a group's first event was seen by this thread; the group the
    // thread starts inside takes it from lower bounds (below)
    bool have = false;
    uint32_t before = 0;
    if (dl < cnt) {
        const uint32_t x0 = min(sS[sa], sE[sb]);
        // the event before the thread's first: the later of the last start
        // and the last end consumed (the merged order is non-decreasing)
        uint32_t px = 0;
        bool prev = false;
        if (i0 + sa > 0) {
            px = sa > 0 ? sS[sa - 1] : a.S[i0 - 1];
            prev = true;
        }
        if (j0 + sb > 0) {
            const uint32_t pe = sb > 0 ? sE[sb - 1] : a.E[j0 - 1];
            px = prev ? max(px, pe) : pe;
            prev = true;
        }
        if (!prev || px != x0) {
            have = true;
            before = (uint32_t)((i0 + sa) - (j0 + sb));
        }
    }
    // pass 1 over the thread's events: its heads, kept as bit masks
    uint32_t open_m = 0, close_m = 0, depth[CV_ITEMS];
    {
        int pa = sa, pb = sb;
#pragma unroll
        for (int k = 0; k < CV_ITEMS; ++k) {
            depth[k] = 0;
            if (dl + k < cnt) {
                const uint32_t vs = sS[pa], ve = sE[pb];
                const uint32_t x = min(vs, ve);
                if (vs <= ve)
                    ++pa;
                else
                    ++pb;
                if (min(sS[pa], sE[pb]) != x) {  // the last event at x
                    const uint32_t after = (uint32_t)((i0 + pa) - (j0 + pb));
                    if (!have) {
                        // the group began before the thread's events: rows
                        // below x among the staged ones, or -- when the group
                        // reaches back past the tile -- among all before it
                        int64_t ls = i0 + dev::lower_bound(sS, 0, (int64_t)pa, x);
                        int64_t le = j0 + dev::lower_bound(sE, 0, (int64_t)pb, x);
                        if (ls == i0 && i0 > 0 && a.S[i0 - 1] == x)
                            ls = dev::lower_bound(a.S, 0, i0 - 1, x);
                        if (le == j0 && j0 > 0 && a.E[j0 - 1] == x)
                            le = dev::lower_bound(a.E, 0, j0 - 1, x);
                        before = (uint32_t)(ls - le);
                    }
                    if (after != before) {
                        if (after > 0) open_m |= 1u << k;
                        if (before > 0) close_m |= 1u << k;
                        depth[k] = after;
                    }
                    have = true;
                    before = after;
                }
            }
        }
    }
    uint32_t tot;
    const uint32_t ex = dev::block_exclusive_sum<CVB>((uint32_t)__popc(open_m), scratch, &tot);
    if (!FILL) {
        if (threadIdx.x == 0) a.cnt[blockIdx.x] = tot;
        return;
    }
    // pass 2: the coordinates again, written at the heads
    int64_t r = (int64_t)a.tbase[blockIdx.x] + ex;  // opening heads before this event
    int pa = sa, pb = sb;
#pragma unroll
    for (int k = 0; k < CV_ITEMS; ++k) {
        if (dl + k < cnt) {
            const uint32_t vs = sS[pa], ve = sE[pb];
            const uint32_t x = min(vs, ve);
            if (vs <= ve)
                ++pa;
            else
                ++pb;
            if (((close_m >> k) & 1u) && r > 0 && r <= a.cap) a.oge[r - 1] = x;
            if ((open_m >> k) & 1u) {
                if (r < a.cap) {
                    a.ogs[r] = x;
                    a.odepth[r] = depth[k];
                }
                ++r;
            }
        }
    }
}

// sum of widths, sum of width x depth, maximum depth of a coverage result
__global__ __launch_bounds__(256) void k_depth_stats(const uint32_t *__restrict__ gs,
                                                     const uint32_t *__restrict__ ge,
                                                     const uint32_t *__restrict__ depth, int64_t n,
                                                     unsigned long long *__restrict__ out) {
    uint64_t cov = 0, db = 0;
    uint32_t mx = 0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const uint64_t w = ge[i] - gs[i];
        const uint32_t d = depth[i];
        cov += w;
        db += w * d;
        mx = max(mx, d);
    }
    cov = dev::wave_reduce_sum(cov);
    db = dev::wave_reduce_sum(db);
    mx = dev::wave_reduce_max(mx);
    if (dev::lane_id() == 0) {
        atomicAdd(&out[0], (unsigned long long)cov);
        atomicAdd(&out[1], (unsigned long long)db);
        atomicMax(&out[2], (unsigned long long)mx);
    }
}

}  // namespace

// E of a set: its ends sorted ascending, as the starts of a temporary set of
// zero-width rows (ge, ge) (the caller's, empty on entry: its blocks go back
// to the pool when it dies).  Shared with annotate.hip: the keys-only sort of
// the ends lands here.
int sorted_ends(lime_ctx *ctx, const lime_set *set, lime_set *ends) {
    ends->ctx = ctx;
    ends->n = set->n;
    ends->n_contigs = set->n_contigs;
    ends->off = set->off;
    ends->len = set->len;
    ends->d_off = set->d_off;
    return sort_set_global(ctx, ends, set->ge, set->ge, set->row, nullptr);
}

// depth runs of a sorted set; the result owns gs / ge / depth
int coverage_run(lime_ctx *ctx, const lime_set *set, lime_result *res) {
    const int64_t n = set->n;
    res->n = 0;
    if (n == 0) {
        LIME_TRY(alloc(ctx, &res->gs, 1));
        LIME_TRY(alloc(ctx, &res->ge, 1));
        LIME_TRY(alloc(ctx, &res->depth, 1));
        return LIME_OK;
    }
    // E: the ends sorted ascending (sorted_ends); released when `ends` dies,
    // on every path
    lime_set ends;
    LIME_TRY(sorted_ends(ctx, set, &ends));
    const int64_t nt = (2 * n + CV_TILE - 1) / CV_TILE;
    PoolPtr<uint32_t> split, cnt, tbase, total;
    LIME_TRY(split.alloc(ctx, (size_t)nt + 1));
    LIME_TRY(cnt.alloc(ctx, (size_t)nt));
    LIME_TRY(tbase.alloc(ctx, (size_t)nt));
    LIME_TRY(total.alloc(ctx, 1));
    CovArgs a;
    a.S = set->gs;
    a.E = ends.gs;
    a.n = n;
    a.split = split;
    a.tbase = tbase;
    a.cnt = cnt;
    a.ogs = a.oge = a.odepth = nullptr;
    a.cap = 0;
    hipLaunchKernelGGL(k_cov_split, dim3(blocks_for(nt + 1, CVB)), dim3(CVB), 0, S(ctx), a.S, a.E,
                       n, nt, split.get());
    hipLaunchKernelGGL(k_cov<false>, dim3((unsigned)nt), dim3(CVB), 0, S(ctx), a);
    LIME_HIP(hipGetLastError());
    LIME_TRY(scan_exclusive_u32(ctx, cnt, tbase, nt, total));
    uint32_t nr = 0;
    LIME_TRY(read_back(ctx, &nr, total, sizeof(nr)));
    LIME_TRY(alloc(ctx, &res->gs, (size_t)nr));
    LIME_TRY(alloc(ctx, &res->ge, (size_t)nr));
    LIME_TRY(alloc(ctx, &res->depth, (size_t)nr));
    a.ogs = res->gs;
    a.oge = res->ge;
    a.odepth = res->depth;
    a.cap = nr;
    hipLaunchKernelGGL(k_cov<true>, dim3((unsigned)nt), dim3(CVB), 0, S(ctx), a);
    LIME_HIP(hipGetLastError());
    res->n = nr;
    return LIME_OK;
}

int depth_stats(lime_ctx *ctx, const lime_result *res, uint64_t *covered, uint64_t *depth_bases,
                uint32_t *max_depth) {
    PoolPtr<unsigned long long> d_out;
    LIME_TRY(d_out.alloc(ctx, 3));
    LIME_HIP(hipMemsetAsync(d_out, 0, 24, S(ctx)));
    if (res->n > 0)
        hipLaunchKernelGGL(k_depth_stats, dim3(std::min<unsigned>(blocks_for(res->n, 256), 4096u)),
                           dim3(256), 0, S(ctx), (const uint32_t *)res->gs,
                           (const uint32_t *)res->ge, (const uint32_t *)res->depth, res->n,
                           d_out.get());
    LIME_HIP(hipGetLastError());
    uint64_t h[3];
    LIME_TRY(read_back(ctx, h, d_out, 24));
    if (covered) *covered = h[0];
    if (depth_bases) *depth_bases = h[1];
    if (max_depth) *max_depth = (uint32_t)h[2];
    return LIME_OK;
}

}  // namespace lime
