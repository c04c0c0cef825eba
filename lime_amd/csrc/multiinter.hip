// multiinter.hip -- k sets at once: the decomposition of the genome by set
// membership (bedtools multiinter) and the m-of-k consensus regions.
//
// mask(p) has bit i set iff some row of set i has start <= p < end.
//   membership (min_sets == 0)  every maximal interval of one contig on which
//                               mask is constant and non-zero, with its mask
//                               and n_sets = popcount(mask)
//   consensus (1 <= min_sets)   every maximal interval of one contig on which
//                               popcount(mask) >= min_sets
// Per set, the merge runs of its plain view are disjoint and sorted (merge_runs
// starts a run iff next.start >= running max end).  Every run gives two EVENTS,
// (gs, 1 << i) and (ge, 1 << i).  With all events of all sets sorted by
// coordinate, the mask on [x, next coordinate) is the XOR of the tags of every
// event at a coordinate <= x: book-ended runs of one set toggle twice where
// they touch and cancel, zero-width runs cancel, and the order inside a
// coordinate group is irrelevant.  XOR is associative: an ordinary scan.
//       after(x)  = the prefix past the last event at x
//       before(x) = the prefix below its first event
//       class(m)  = m (membership) or [popcount(m) >= min_sets] (consensus)
// x is a HEAD iff class(after) != class(before); a head with class(after) != 0
// opens a run, one with class(before) != 0 closes the run before it.  Contigs
// need no flags: off[c + 1] = off[c] + len[c] + 1 leaves one base of mask 0
// between them, as in merge.hip and coverage.hip.
//
// Passes:
//   merge_runs x k       the runs of every set (merge.hip's budget)
//   k_mi_events x k      (coordinate, set) of both ends of every run
//                                            8 B read, 16 B written / run
//   sort                 sort_set_global over (key, key, set) as a temporary
//                        set of zero-width rows (sort.hip's budget, 12-B row)
//   k_mi_tile_xor        the XOR of every tile's tags       4 B read / event
//   k_mi_scan            one workgroup: exclusive XOR scan over the tiles
//   k_mi<false>          per tile: opening heads            8 B read / event
//   scan_exclusive_u32   over the tiles
//   k_mi<true>           the same walk, writing gs (mask, n_sets) at an opening
//                        head and ge of the run before at a closing one
//                                            8 B read / event, 8 or 16 B / run
// Byte budget of the walks: 20 B per event (40 B per run of an input set) and
// up to 16 B per output run, on top of the merges and the sort of the events.
//
// k_mi: a tile is MI_TILE events.  Keys and sets are loaded coalesced, every
// global load before the first LDS store; a thread then owns MI_ITEMS
// consecutive events: XOR of its tags, wave XOR scan on DPP, block scan through
// LDS seeded with the tile's prefix.  Heads are decided at the LAST event of a
// coordinate group (one event of look-ahead past the tile).  `before` of a
// group that began before the thread's events is the stored prefix of the
// thread that holds its first event plus at most 7 tags; of a group that began
// before the TILE (it may span many tiles) it is tile-uniform: a lower bound in
// the global keys, that tile's prefix and at most one tile of tags, XORed by
// the whole workgroup.
#include "common.hpp"

namespace lime {
namespace {

constexpr int MIB = 256;                 // threads per tile
constexpr int MI_ITEMS = 8;              // events per thread
constexpr int MI_TILE = MIB * MI_ITEMS;  // events per tile (tests: multiinter_cases.T)
constexpr uint32_t MI_NONE = 0xffffffffu;  // above every coordinate (<= span <= 2^32 - 1)

struct MiArgs {
    const uint32_t *key, *set;  // the sorted events: coordinate, set index
    int64_t n;                  // events
    const uint32_t *tpre;       // XOR of the tags before each tile
    const uint32_t *tbase;      // fill: opening heads before each tile
    uint32_t *cnt;              // count: opening heads of each tile
    uint32_t *ogs, *oge, *omask, *odepth;
    int64_t cap;  // runs the outputs hold
    int min_sets;
};

__device__ __forceinline__ uint32_t xor_op(uint32_t a, uint32_t b) { return a ^ b; }

// XOR over the workgroup; s holds MIB / 64 words.  Contains barriers.
__device__ __forceinline__ uint32_t block_xor(uint32_t v, uint32_t *s) {
    v = dev::wave_reduce_xor(v);
    if (dev::lane_id() == 0) s[threadIdx.x / dev::WAVE] = v;
    __syncthreads();
    uint32_t r = 0;
#pragma unroll
    for (int w = 0; w < MIB / dev::WAVE; ++w) r ^= s[w];
    __syncthreads();
    return r;
}

// both ends of every run of set `idx` as events [base, base + 2 nr) (base even)
__global__ __launch_bounds__(MIB) void k_mi_events(const uint32_t *__restrict__ rs,
                                                   const uint32_t *__restrict__ re, int64_t nr,
                                                   uint32_t idx, uint2 *__restrict__ key,
                                                   uint2 *__restrict__ set) {
    const int64_t stride = (int64_t)gridDim.x * MIB;
    for (int64_t j = (int64_t)blockIdx.x * MIB + threadIdx.x; j < nr; j += stride) {
        key[j] = make_uint2(rs[j], re[j]);
        set[j] = make_uint2(idx, idx);
    }
}

__global__ __launch_bounds__(MIB) void k_mi_tile_xor(const uint32_t *__restrict__ set, int64_t n,
                                                     uint32_t *__restrict__ agg) {
    __shared__ uint32_t s[MIB / dev::WAVE];
    const int64_t d0 = (int64_t)blockIdx.x * MI_TILE;
    uint32_t v = 0;
#pragma unroll
    for (int q = 0; q < MI_ITEMS; ++q) {
        const int64_t g = d0 + q * MIB + threadIdx.x;
        if (g < n) v ^= 1u << (set[g] & 31u);
    }
    v = block_xor(v, s);
    if (threadIdx.x == 0) agg[blockIdx.x] = v;
}

// exclusive XOR scan of the nt tile aggregates, in place, by one workgroup
__global__ __launch_bounds__(MIB) void k_mi_scan(uint32_t *__restrict__ a, int64_t nt) {
    __shared__ uint32_t s[MIB / dev::WAVE];
    uint32_t carry = 0;
    const int w = threadIdx.x / dev::WAVE;
    for (int64_t base = 0; base < nt; base += MIB) {
        const int64_t i = base + threadIdx.x;
        const uint32_t v = i < nt ? a[i] : 0u;
        const uint32_t inc = dev::wave_scan_dpp(v, 0u, xor_op);
        if (dev::lane_id() == dev::WAVE - 1) s[w] = inc;
        __syncthreads();
        uint32_t pre = carry, tot = 0;
#pragma unroll
        for (int q = 0; q < MIB / dev::WAVE; ++q) {
            if (q < w) pre ^= s[q];
            tot ^= s[q];
        }
        if (i < nt) a[i] = pre ^ inc ^ v;
        carry ^= tot;
        __syncthreads();
    }
}

template <int MODE>
__device__ __forceinline__ uint32_t mi_class(uint32_t m, int min_sets) {
    return MODE ? (uint32_t)(__popc(m) >= min_sets) : m;
}

// MODE 0: membership, 1: consensus
template <bool FILL, int MODE>
__global__ __launch_bounds__(MIB) void k_mi(MiArgs a) {
    // sK[i] = key of the tile's event i, MI_NONE past the events; sK[MI_TILE]
    // the key after the tile.  sT: the tags.  sP: the prefix before every
    // thread's first event.
    __shared__ __align__(16) uint32_t sK[MI_TILE + 4];
    __shared__ __align__(16) uint32_t sT[MI_TILE];
    __shared__ uint32_t sP[MIB];
    __shared__ uint32_t sW[MIB / dev::WAVE + 1];
    const int64_t n = a.n;
    const int64_t d0 = (int64_t)blockIdx.x * MI_TILE;
    const int cnt = (int)(n - d0 < MI_TILE ? n - d0 : MI_TILE);
    uint32_t vk[MI_ITEMS], vt[MI_ITEMS], vx[MI_ITEMS];
#pragma unroll
    for (int q = 0; q < MI_ITEMS; ++q) {
        const int64_t g = d0 + q * MIB + threadIdx.x;
        vk[q] = g < n ? a.key[g] : MI_NONE;
        vt[q] = g < n ? 1u << (a.set[g] & 31u) : 0u;
    }
    const uint32_t ahead = d0 + MI_TILE < n ? a.key[d0 + MI_TILE] : MI_NONE;
    const uint32_t behind = d0 > 0 ? a.key[d0 - 1] : MI_NONE;
    const uint32_t x0 = a.key[d0];
    // the tile's first group began before the tile (tile-uniform)
    const bool cont = d0 > 0 && behind == x0;
    int64_t g0 = 0, tg = 0;
    if (cont) {
        g0 = dev::lower_bound(a.key, 0, d0, x0);  // the group's first event
        tg = g0 / MI_TILE;
#pragma unroll
        for (int q = 0; q < MI_ITEMS; ++q) {
            const int64_t g = tg * MI_TILE + q * MIB + threadIdx.x;
            vx[q] = g < g0 ? 1u << (a.set[g] & 31u) : 0u;
        }
    }
#pragma unroll
    for (int q = 0; q < MI_ITEMS; ++q) {
        sK[q * MIB + threadIdx.x] = vk[q];
        sT[q * MIB + threadIdx.x] = vt[q];
    }
    if (threadIdx.x == 0) sK[MI_TILE] = ahead;
    uint32_t tile_before = 0;
    if (cont) {
        uint32_t v = 0;
#pragma unroll
        for (int q = 0; q < MI_ITEMS; ++q) v ^= vx[q];
        tile_before = a.tpre[tg] ^ block_xor(v, sW);
    } else {
        __syncthreads();
    }

    // the thread's MI_ITEMS events and the key after them
    const int dl = (int)threadIdx.x * MI_ITEMS;
    uint32_t k[MI_ITEMS + 1], t[MI_ITEMS];
    {
        const uint4 k0 = *reinterpret_cast<const uint4 *>(sK + dl);
        const uint4 k1 = *reinterpret_cast<const uint4 *>(sK + dl + 4);
        const uint4 t0 = *reinterpret_cast<const uint4 *>(sT + dl);
        const uint4 t1 = *reinterpret_cast<const uint4 *>(sT + dl + 4);
        k[0] = k0.x, k[1] = k0.y, k[2] = k0.z, k[3] = k0.w;
        k[4] = k1.x, k[5] = k1.y, k[6] = k1.z, k[7] = k1.w;
        k[8] = sK[dl + MI_ITEMS];
        t[0] = t0.x, t[1] = t0.y, t[2] = t0.z, t[3] = t0.w;
        t[4] = t1.x, t[5] = t1.y, t[6] = t1.z, t[7] = t1.w;
    }
    // exclusive XOR prefix of the thread: its own tags, the wave on DPP, the
    // waves through LDS, seeded with the tile's prefix
    uint32_t own = 0;
#pragma unroll
    for (int q = 0; q < MI_ITEMS; ++q) own ^= t[q];
    const uint32_t inc = dev::wave_scan_dpp(own, 0u, xor_op);
    const int w = threadIdx.x / dev::WAVE;
    if (dev::lane_id() == dev::WAVE - 1) sW[w] = inc;
    __syncthreads();
    uint32_t p = a.tpre[blockIdx.x] ^ inc ^ own;
#pragma unroll
    for (int q = 0; q < MIB / dev::WAVE; ++q)
        if (q < w) p ^= sW[q];
    sP[threadIdx.x] = p;
    __syncthreads();

    // `before` is known once a group's first event was seen by this thread
    bool have = false;
    uint32_t before = 0;
    if (dl < cnt) {
        const uint32_t prev = threadIdx.x > 0 ? sK[dl - 1] : behind;
        if ((threadIdx.x == 0 && d0 == 0) || prev != k[0]) {
            have = true;
            before = p;
        }
    }
    // pass 1 over the thread's events: its heads, kept as bit masks
    uint32_t open_m = 0, close_m = 0;
    {
        uint32_t m = p;
#pragma unroll
        for (int q = 0; q < MI_ITEMS; ++q) {
            if (dl + q < cnt) {
                m ^= t[q];
                if (k[q + 1] != k[q]) {  // the last event at this coordinate
                    if (!have) {
                        // the group began before the thread's events: at tile
                        // event j, or (j == 0 in a continuing tile) before the
                        // tile
                        const int j = (int)dev::lower_bound(sK, 0, (int64_t)dl, k[q]);
                        if (j == 0 && cont) {
                            before = tile_before;
                        } else {
                            before = sP[j >> 3];
                            for (int i = j & ~(MI_ITEMS - 1); i < j; ++i) before ^= sT[i];
                        }
                    }
                    const uint32_t ca = mi_class<MODE>(m, a.min_sets),
                                   cb = mi_class<MODE>(before, a.min_sets);
                    if (ca != cb) {
                        if (ca != 0) open_m |= 1u << q;
                        if (cb != 0) close_m |= 1u << q;
                    }
                    have = true;
                    before = m;
                }
            }
        }
    }
    uint32_t tot;
    const uint32_t ex = dev::block_exclusive_sum<MIB>((uint32_t)__popc(open_m), sW, &tot);
    if (!FILL) {
        if (threadIdx.x == 0) a.cnt[blockIdx.x] = tot;
        return;
    }
    // pass 2: the coordinates again, written at the heads
    int64_t r = (int64_t)a.tbase[blockIdx.x] + ex;  // opening heads before this event
    uint32_t m = p;
#pragma unroll
    for (int q = 0; q < MI_ITEMS; ++q) {
        if (dl + q < cnt) {
            m ^= t[q];
            if (((close_m >> q) & 1u) && r > 0 && r <= a.cap) a.oge[r - 1] = k[q];
            if ((open_m >> q) & 1u) {
                if (r < a.cap) {
                    a.ogs[r] = k[q];
                    if (MODE == 0) {
                        a.omask[r] = m;
                        a.odepth[r] = (uint32_t)__popc(m);
                    }
                }
                ++r;
            }
        }
    }
}

template <int MODE>
void launch_mi(lime_ctx *ctx, bool fill, int64_t nt, const MiArgs &a) {
    if (fill)
        hipLaunchKernelGGL((k_mi<true, MODE>), dim3((unsigned)nt), dim3(MIB), 0, S(ctx), a);
    else
        hipLaunchKernelGGL((k_mi<false, MODE>), dim3((unsigned)nt), dim3(MIB), 0, S(ctx), a);
}

}  // namespace

// membership runs (min_sets == 0: res owns gs / ge / mask / depth, depth =
// n_sets) or consensus runs (res owns gs / ge) of k sorted sets of one space
int multiinter_run(lime_ctx *ctx, int k, const lime_set *const *sets, int min_sets,
                   lime_result *res) {
    const bool member = min_sets == 0;
    res->n = 0;
    // the runs of every set's plain view
    std::vector<std::unique_ptr<lime_result>> runs((size_t)k);
    uint64_t n_ev = 0;
    for (int i = 0; i < k; ++i) {
        runs[i].reset(new lime_result());
        runs[i]->ctx = ctx;
        PlainView plain(sets[i]);
        LIME_TRY(merge_runs(ctx, &plain.v, runs[i].get(), false));
        n_ev += 2 * (uint64_t)runs[i]->n;
    }
    if (n_ev > 0xffffffffull)
        return fail(LIME_ERR_OVERFLOW, "multiinter: the events of the sets' runs do not fit a u32 index");
    if (n_ev == 0) {
        LIME_TRY(alloc(ctx, &res->gs, 1));
        LIME_TRY(alloc(ctx, &res->ge, 1));
        if (member) {
            LIME_TRY(alloc(ctx, &res->mask, 1));
            LIME_TRY(alloc(ctx, &res->depth, 1));
        }
        return LIME_OK;
    }
    const int64_t n = (int64_t)n_ev;
    // the events, sorted by coordinate: a temporary set of zero-width rows
    // (key, key) whose row is the set index; released when `ev` dies
    lime_set ev;
    {
        PoolPtr<uint32_t> key, idx;
        LIME_TRY(key.alloc(ctx, (size_t)n));
        LIME_TRY(idx.alloc(ctx, (size_t)n));
        int64_t base = 0;
        for (int i = 0; i < k; ++i) {
            const int64_t nr = runs[i]->n;
            if (nr > 0)
                hipLaunchKernelGGL(k_mi_events,
                                   dim3(std::min<unsigned>(blocks_for(nr, MIB), 8192u)), dim3(MIB),
                                   0, S(ctx), (const uint32_t *)runs[i]->gs,
                                   (const uint32_t *)runs[i]->ge, nr, (uint32_t)i,
                                   reinterpret_cast<uint2 *>(key.get() + base),
                                   reinterpret_cast<uint2 *>(idx.get() + base));
            base += 2 * nr;
        }
        LIME_HIP(hipGetLastError());
        runs.clear();
        ev.ctx = ctx;
        ev.n = n;
        ev.n_contigs = sets[0]->n_contigs;
        ev.off = sets[0]->off;
        ev.len = sets[0]->len;
        ev.d_off = sets[0]->d_off;
        LIME_TRY(sort_set_global(ctx, &ev, key, key, idx, nullptr));
    }
    release(ctx, ev.ge);
    const int64_t nt = (n + MI_TILE - 1) / MI_TILE;
    PoolPtr<uint32_t> tpre, cnt, tbase, total;
    LIME_TRY(tpre.alloc(ctx, (size_t)nt));
    LIME_TRY(cnt.alloc(ctx, (size_t)nt));
    LIME_TRY(tbase.alloc(ctx, (size_t)nt));
    LIME_TRY(total.alloc(ctx, 1));
    hipLaunchKernelGGL(k_mi_tile_xor, dim3((unsigned)nt), dim3(MIB), 0, S(ctx),
                       (const uint32_t *)ev.row, n, tpre.get());
    hipLaunchKernelGGL(k_mi_scan, dim3(1), dim3(MIB), 0, S(ctx), tpre.get(), nt);
    MiArgs a;
    a.key = ev.gs;
    a.set = ev.row;
    a.n = n;
    a.tpre = tpre;
    a.tbase = tbase;
    a.cnt = cnt;
    a.ogs = a.oge = a.omask = a.odepth = nullptr;
    a.cap = 0;
    a.min_sets = min_sets;
    if (member)
        launch_mi<0>(ctx, false, nt, a);
    else
        launch_mi<1>(ctx, false, nt, a);
    LIME_HIP(hipGetLastError());
    LIME_TRY(scan_exclusive_u32(ctx, cnt, tbase, nt, total));
    uint32_t nr = 0;
    LIME_TRY(read_back(ctx, &nr, total, sizeof(nr)));
    LIME_TRY(alloc(ctx, &res->gs, (size_t)nr));
    LIME_TRY(alloc(ctx, &res->ge, (size_t)nr));
    if (member) {
        LIME_TRY(alloc(ctx, &res->mask, (size_t)nr));
        LIME_TRY(alloc(ctx, &res->depth, (size_t)nr));
    }
    a.ogs = res->gs;
    a.oge = res->ge;
    a.omask = res->mask;
    a.odepth = res->depth;
    a.cap = nr;
    if (member)
        launch_mi<0>(ctx, true, nt, a);
    else
        launch_mi<1>(ctx, true, nt, a);
    LIME_HIP(hipGetLastError());
    res->n = nr;
    return LIME_OK;
}

}  // namespace lime
