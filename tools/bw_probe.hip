// bw_probe.hip -- calibration of the HBM write ceiling the fill kernel is
// judged against: streaming stores of N 16-B records in several shapes
// (k_fill's block shape, persistent grid-stride, dword-per-lane, unrolled,
// non-temporal), the fill's ingredients added to its store shape one at a
// time (k_store_fillgap), plus a copy (read + write) reference.
//   ./bw_probe [records [gap]]     (gap: stop after the fill-gap variants)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <bool NT>
__global__ __launch_bounds__(256) void k_store(u32x4 *out, long n, long per_block) {
    long b0 = (long)blockIdx.x * per_block;
    long b1 = b0 + per_block < n ? b0 + per_block : n;
    for (long i = b0 + threadIdx.x; i < b1; i += 256) {
        u32x4 v = {(unsigned)i, (unsigned)(i >> 7), (unsigned)blockIdx.x, 7u};
        if (NT)
            __builtin_nontemporal_store(v, out + i);
        else
            out[i] = v;
    }
}

// k_fill's shape: 512-thread workgroup, each wave writes its own contiguous
// chunk of the workgroup's range (per_block / 8 records)
__global__ __launch_bounds__(512) void k_store_wavechunk(u32x4 *out, long n, long per_block) {
    long b0 = (long)blockIdx.x * per_block;
    long b1 = b0 + per_block < n ? b0 + per_block : n;
    long per = ((b1 - b0 + 7) / 8 + 63) & ~63L;
    long w0 = b0 + (threadIdx.x / 64) * per;
    long w1 = w0 + per < b1 ? w0 + per : b1;
    for (long i = w0 + (threadIdx.x & 63); i < w1; i += 64) {
        u32x4 v = {(unsigned)i, (unsigned)(i >> 7), (unsigned)blockIdx.x, 7u};
        out[i] = v;
    }
}

// persistent grid-stride, 16 B per lane
template <int TB>
__global__ __launch_bounds__(TB) void k_store_grid(u32x4 *out, long n) {
    for (long i = (long)blockIdx.x * TB + threadIdx.x; i < n; i += (long)gridDim.x * TB) {
        u32x4 v = {(unsigned)i, (unsigned)(i >> 7), 3u, 7u};
        out[i] = v;
    }
}

// 4 B per lane (256 B per wave instruction), per_block*4 dwords per block
__global__ __launch_bounds__(256) void k_store_dword(unsigned *out, long n, long per_block) {
    long b0 = (long)blockIdx.x * per_block;
    long b1 = b0 + per_block < n ? b0 + per_block : n;
    for (long i = b0 + threadIdx.x; i < b1; i += 256) out[i] = (unsigned)i;
}

// 4 independent 16-B stores in flight per iteration, wave-contiguous
__global__ __launch_bounds__(256) void k_store_unroll4(u32x4 *out, long n, long per_block) {
    long b0 = (long)blockIdx.x * per_block;
    long b1 = b0 + per_block < n ? b0 + per_block : n;
    for (long i = b0 + threadIdx.x; i < b1; i += 1024) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            long j = i + 256 * k;
            if (j < b1) out[j] = u32x4{(unsigned)j, (unsigned)(j >> 7), 5u, 7u};
        }
    }
}

// 512-thread workgroup over per_block records; wave w writes granules of G
// records at w*G, w*G + 8G, ... (G = 64: block-striped; G = per_block/8:
// one chunk per wave)
template <int G>
__global__ __launch_bounds__(512) void k_store_gran(u32x4 *out, long n, long per_block) {
    long b0 = (long)blockIdx.x * per_block;
    long b1 = b0 + per_block < n ? b0 + per_block : n;
    const int w = threadIdx.x / 64, lane = threadIdx.x & 63;
    for (long g = b0 + (long)w * G; g < b1; g += 8L * G)
        for (int k = 0; k < G; k += 64) {
            long i = g + k + lane;
            if (i < b1) out[i] = u32x4{(unsigned)i, (unsigned)(i >> 7), 9u, 7u};
        }
}

// k_fill's exact store shape with constant data: persistent workgroups of
// 512 threads, each over a contiguous range of `per` records cut into
// "tiles" of T records; inside a tile the range is dealt to the 8 waves in
// granules of G records (G >= T/8: one equal chunk per wave).
__global__ __launch_bounds__(512) void k_store_fillshape(u32x4 *out, long n, long per, long T,
                                                         long G) {
    const long b0 = (long)blockIdx.x * per;
    const long b1 = b0 + per < n ? b0 + per : n;
    const int w = threadIdx.x / 64, lane = threadIdx.x & 63;
    for (long t0 = b0; t0 < b1; t0 += T) {
        const long t1 = t0 + T < b1 ? t0 + T : b1;
        long rounds = (t1 - t0 + 8 * G - 1) / (8 * G);
        if (rounds < 1) rounds = 1;
        const long gsz = (((t1 - t0 + 8 * rounds - 1) / (8 * rounds)) + 63) & ~63L;
        for (long g = t0 + w * gsz; g < t1; g += 8 * gsz) {
            const long ge = g + gsz < t1 ? g + gsz : t1;
            for (long i = g + lane; i < ge; i += 64) out[i] = u32x4{(unsigned)i, 1u, 2u, 3u};
        }
        __syncthreads();
    }
}

// What k_fill adds to that store shape, one ingredient at a time (level L,
// each level on top of the one before), in workgroups of NT threads of which
// the first NSW waves store (a wave past them idles through the store loop):
//   L = 1  every thread prefetches the next tile's staging words (11264 per
//          tile, ~45 KB: 5 words per owner, 3 per partner row) into registers
//          before the store loop and uses them before the tile's closing
//          barrier (the use waits on the wave's vector-memory counter, which
//          the wave's stores share)
//   L = 2  the registers are written to the LDS image (offsets, owners,
//          partner window) behind that barrier, and a second barrier follows
//   L = 3  the store loop reads the image the way the fill's does: a b64
//          owner walk and two b128 reads per record feed the stored value
// LOADER (with L = 3) is the alternative structure: the wave past the store
// waves fetches the next tile's words itself, with 16-B loads, into a second
// LDS image, and the store waves never load; one barrier per tile.
// PW: the staging words read per tile, the first PW of the tile's P_WORDS
// (the image's planes past them stay zero): the slope of the fill's time in
// its staging bytes, at the structure of level 3.
// The input words are all zero at run time (the compiler cannot know), so
// the image's offsets stay q * 82 and every LDS index stays in range.
constexpr int P_OWN = 1024, P_PAR = 2048, P_WORDS = 5 * P_OWN + 3 * P_PAR, P_PPO = 82;
struct ProbeImage {
    uint2 lo_off[P_OWN + 1];
    u32x4 own[P_OWN];
    u32x4 par[P_PAR];
};

template <int NT, int NSW, int L, bool LOADER, int PW = P_WORDS>
__global__ __launch_bounds__(NT) void k_store_fillgap(u32x4 *out, long n, long per,
                                                      const unsigned *__restrict__ in,
                                                      long in_tiles) {
    constexpr long T = (long)P_OWN * P_PPO + 32;  // 84000
    constexpr int NR = PW / NT;                    // staging words per thread
    static_assert(PW % NT == 0, "staging words divide over the threads");
    // (the offsets' planes, words 0 .. 2 P_OWN, keep the LDS indices in range)
    static_assert(PW >= 2 * P_OWN && PW <= P_WORDS && (!LOADER || PW == P_WORDS),
                  "a shorter staging read keeps the lo / off planes; the loader reads it all");
    __shared__ ProbeImage img[LOADER ? 2 : 1];
    if (PW < P_WORDS) {
        for (int i = threadIdx.x; i < (int)(sizeof(ProbeImage) / 4); i += NT)
            ((unsigned *)&img[0])[i] = 0u;
        __syncthreads();
    }
    const long b0 = (long)blockIdx.x * per;
    const long b1 = b0 + per < n ? b0 + per : n;
    const int w = threadIdx.x / 64, lane = threadIdx.x & 63;
    unsigned r[NR];
    unsigned acc = 0;
    auto prefetch = [&](long t0) {
        const unsigned *src = in + ((t0 / T) % in_tiles) * P_WORDS;
#pragma unroll
        for (int k = 0; k < NR; ++k) r[k] = src[k * NT + threadIdx.x];
    };
    auto image_from_regs = [&]() {
        // word k * NT + tid of the tile: planes lo, off, g, e, row of the
        // owners, then g, e, row of the partner rows
#pragma unroll
        for (int k = 0; k < NR; ++k) {
            const int i = k * NT + threadIdx.x;
            unsigned *dst;
            if (i < 2 * P_OWN) {
                const int q = i % P_OWN;
                dst = i < P_OWN ? &img[0].lo_off[q].x : &img[0].lo_off[q].y;
                if (i >= P_OWN) r[k] += q * P_PPO;
            } else if (i < 5 * P_OWN) {
                dst = (unsigned *)&img[0].own[i % P_OWN] + (i / P_OWN - 2);
            } else {
                const int j = i - 5 * P_OWN;
                dst = (unsigned *)&img[0].par[j % P_PAR] + j / P_PAR;
            }
            *dst = r[k];
        }
        if (threadIdx.x == 0) img[0].lo_off[P_OWN] = make_uint2(0u, (unsigned)T);
    };
    auto load_image = [&](long t0, ProbeImage &im) {  // one wave, 16-B loads
        const u32x4 *src = (const u32x4 *)(in + ((t0 / T) % in_tiles) * P_WORDS);
        for (int c = 0; c < P_OWN / 256; ++c) {
            const int q4 = c * 64 + lane;  // owners 4 q4 .. 4 q4 + 3
            u32x4 v[5];
#pragma unroll
            for (int a = 0; a < 5; ++a) v[a] = src[a * (P_OWN / 4) + q4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int q = 4 * q4 + e;
                im.lo_off[q] = make_uint2(v[0][e], v[1][e] + q * P_PPO);
                im.own[q] = u32x4{v[2][e], v[3][e], v[4][e], 0u};
            }
        }
        for (int c = 0; c < P_PAR / 256; ++c) {
            const int i4 = c * 64 + lane;
            u32x4 v[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) v[a] = src[5 * (P_OWN / 4) + a * (P_PAR / 4) + i4];
#pragma unroll
            for (int e = 0; e < 4; ++e) im.par[4 * i4 + e] = u32x4{v[0][e], v[1][e], v[2][e], 0u};
        }
        if (lane == 0) im.lo_off[P_OWN] = make_uint2(0u, (unsigned)T);
    };
    if (LOADER) {
        if (w == NSW) load_image(b0, img[0]);
        __syncthreads();
    } else if (L >= 1) {
        prefetch(b0);
        if (L >= 2) {
            image_from_regs();
            __syncthreads();
        }
    }
    int cur = 0;
    for (long t0 = b0; t0 < b1; t0 += T) {
        const long t1 = t0 + T < b1 ? t0 + T : b1;
        const bool more = t0 + T < b1;
        if (LOADER) {
            if (w == NSW && more) load_image(t0 + T, img[cur ^ 1]);
        } else if (L >= 1 && more) {
            prefetch(t0 + T);
        }
        if (w < NSW) {
            const ProbeImage &im = img[LOADER ? cur : 0];
            const long gsz = (((t1 - t0 + NSW - 1) / NSW) + 63) & ~63L;
            const long g = t0 + w * gsz;
            const long ge = g + gsz < t1 ? g + gsz : t1;
            int q = (int)((g - t0) / P_PPO);
            if (q > P_OWN - 1) q = P_OWN - 1;
            uint2 lof = make_uint2(0u, 0u), nxt = make_uint2(0u, 0u);
            if (L >= 3 && g < ge) {
                lof = im.lo_off[q];
                nxt = im.lo_off[q + 1];
            }
            for (long i = g + lane; i < ge; i += 64) {
                u32x4 v = u32x4{(unsigned)i, 1u, 2u, acc};
                if (L >= 3) {
                    const unsigned ou = (unsigned)(i - t0);
                    while (nxt.y <= ou) {
                        ++q;
                        lof = nxt;
                        nxt = im.lo_off[q + 1];
                    }
                    const u32x4 ow = im.own[q];
                    const u32x4 pa = im.par[(lof.x + (ou - lof.y)) % P_PAR];
                    v = u32x4{(ow.x > pa.x ? ow.x : pa.x) + (unsigned)i, ow.y < pa.y ? ow.y : pa.y,
                              ow.z, pa.z};
                }
                out[i] = v;
            }
        }
        if (!LOADER && L == 1 && more) {
#pragma unroll
            for (int k = 0; k < NR; ++k) acc ^= r[k];
        }
        __syncthreads();
        if (!LOADER && L >= 2 && more) {
            image_from_regs();
            __syncthreads();
            if (L == 2) acc ^= img[0].lo_off[threadIdx.x].x;  // (keeps the image alive)
        }
        cur ^= 1;
    }
}

__global__ __launch_bounds__(256) void k_copy(const u32x4 *in, u32x4 *out, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        out[i] = in[i];
}

__global__ __launch_bounds__(256) void k_read(const u32x4 *in, long n, unsigned *sink) {
    unsigned acc = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        u32x4 v = in[i];
        acc ^= v.x ^ v.y ^ v.z ^ v.w;
    }
    if (acc == 0x12345678u) sink[0] = acc;
}

#define CK(x)                                                         \
    do {                                                              \
        hipError_t e = (x);                                           \
        if (e != hipSuccess) {                                        \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e));    \
            exit(1);                                                  \
        }                                                             \
    } while (0)

static hipEvent_t ea, eb;

template <class F>
static void timeit(const char *name, long recs, double bytes, F launch) {
    float best = 1e30f;
    for (int r = 0; r < 6; ++r) {
        CK(hipEventRecord(ea));
        launch();
        CK(hipEventRecord(eb));
        CK(hipEventSynchronize(eb));
        float ms;
        CK(hipEventElapsedTime(&ms, ea, eb));
        if (r && ms < best) best = ms;
    }
    CK(hipGetLastError());
    printf("{\"probe\": \"%s\", \"records\": %ld, \"ms\": %.3f, \"GBps\": %.1f}\n", name, recs, best,
           bytes / best / 1e6);
    fflush(stdout);
}

int main(int argc, char **argv) {
    long n = argc > 1 ? atol(argv[1]) : (1L << 31);
    const long per_block = 131072;
    u32x4 *out, *in;
    unsigned *sink;
    CK(hipMalloc(&out, n * 16));
    CK(hipMalloc(&sink, 64));
    CK(hipEventCreate(&ea));
    CK(hipEventCreate(&eb));
    unsigned grid = (unsigned)((n + per_block - 1) / per_block);
    timeit("store16_plain", n, n * 16.0, [&] {
        hipLaunchKernelGGL(k_store<false>, dim3(grid), dim3(256), 0, 0, out, n, per_block);
    });
    timeit("store16_nt", n, n * 16.0, [&] {
        hipLaunchKernelGGL(k_store<true>, dim3(grid), dim3(256), 0, 0, out, n, per_block);
    });
    timeit("store16_wavechunk512", n, n * 16.0, [&] {
        hipLaunchKernelGGL(k_store_wavechunk, dim3(grid), dim3(512), 0, 0, out, n, per_block);
    });
    timeit("store16_unroll4", n, n * 16.0, [&] {
        hipLaunchKernelGGL(k_store_unroll4, dim3(grid), dim3(256), 0, 0, out, n, per_block);
    });
    for (unsigned g : {1024u, 2048u, 4096u, 16384u})
        for (int tb : {256, 1024}) {
            char name[64];
            snprintf(name, sizeof name, "store16_grid%u_tb%d", g, tb);
            timeit(name, n, n * 16.0, [&] {
                if (tb == 256)
                    hipLaunchKernelGGL(k_store_grid<256>, dim3(g), dim3(256), 0, 0, out, n);
                else
                    hipLaunchKernelGGL(k_store_grid<1024>, dim3(g), dim3(1024), 0, 0, out, n);
            });
        }
    timeit("store4_dword", n * 4, n * 16.0, [&] {
        hipLaunchKernelGGL(k_store_dword, dim3(grid), dim3(256), 0, 0, (unsigned *)out, n * 4,
                           per_block * 4);
    });
    for (long pb : {131072L, 524288L}) {
#define GRAN(G)                                                                             \
    {                                                                                       \
        char name[64];                                                                      \
        snprintf(name, sizeof name, "gran%d_wg512_per%ld", G, pb);                          \
        unsigned gg = (unsigned)((n + pb - 1) / pb);                                        \
        timeit(name, n, n * 16.0, [&] {                                                     \
            hipLaunchKernelGGL(k_store_gran<G>, dim3(gg), dim3(512), 0, 0, out, n, pb);     \
        });                                                                                 \
    }
        GRAN(64) GRAN(256) GRAN(512) GRAN(2048) GRAN(8192)
    }
    for (long G : {64L, 2048L, 1L << 40})
        for (int wgs_per_cu : {2, 3}) {
            const unsigned g = 256 * wgs_per_cu;
            const long per = (n + g - 1) / g;
            char name[96];
            snprintf(name, sizeof name, "fillshape_T84000_G%ld_wg%d", G > n ? -1L : G, wgs_per_cu);
            timeit(name, n, n * 16.0, [&] {
                hipLaunchKernelGGL(k_store_fillshape, dim3(g), dim3(512), 0, 0, out, n, per, 84000L, G);
            });
        }
    {
        const long T = (long)P_OWN * P_PPO + 32;
        const long in_tiles = n / T + 1024;
        unsigned *stage;
        CK(hipMalloc(&stage, in_tiles * P_WORDS * sizeof(unsigned)));
        CK(hipMemset(stage, 0, in_tiles * P_WORDS * sizeof(unsigned)));
#define GAP(NAME, NT, NSW, L, LOADER)                                                         \
    {                                                                                         \
        const unsigned g = 256 * (1024 / NT);                                                 \
        const long per = (n + g - 1) / g;                                                     \
        timeit("fillgap_" NAME, n, n * 16.0, [&] {                                            \
            hipLaunchKernelGGL((k_store_fillgap<NT, NSW, L, LOADER>), dim3(g), dim3(NT), 0, 0, \
                               out, n, per, stage, in_tiles);                                 \
        });                                                                                   \
    }
        GAP("0_store_wg512x2", 512, 8, 0, false)
        GAP("a_prefetch", 512, 8, 1, false)
        GAP("ab_image", 512, 8, 2, false)
        GAP("abc_ldsreads", 512, 8, 3, false)
        // (c) again at fewer staging words per tile
#define GAPW(NAME, PW)                                                                        \
    {                                                                                         \
        const unsigned g = 256 * 2;                                                           \
        const long per = (n + g - 1) / g;                                                     \
        timeit("fillgap_" NAME, n, n * 16.0, [&] {                                            \
            hipLaunchKernelGGL((k_store_fillgap<512, 8, 3, false, PW>), dim3(g), dim3(512), 0, \
                               0, out, n, per, stage, in_tiles);                              \
        });                                                                                   \
    }
        GAPW("abc_ldsreads_w8192", 8192)
        GAPW("abc_ldsreads_w6144", 6144)
        GAP("abcd_wg1024", 1024, 16, 3, false)
        GAP("abcde_15of16", 1024, 15, 3, false)
        // the pure store stream in the two candidate layouts, and the
        // loader-wave structure itself in each
        GAP("0_store_wg1024", 1024, 16, 0, false)
        GAP("0_store_wg1024_15of16", 1024, 15, 0, false)
        GAP("0_store_wg512x2_7of8", 512, 7, 0, false)
        GAP("loader_wg1024_15of16", 1024, 15, 3, true)
        CK(hipFree(stage));
    }
    if (argc > 2) return 0;  // ./bw_probe N gap: skip the copy / read references
    long nc = n / 2;
    CK(hipMalloc(&in, nc * 16));
    CK(hipMemset(in, 1, nc * 16));
    timeit("copy16", nc, nc * 32.0, [&] {
        hipLaunchKernelGGL(k_copy, dim3(8192), dim3(256), 0, 0, in, out, nc);
    });
    timeit("read16", n, n * 16.0, [&] {
        hipLaunchKernelGGL(k_read, dim3(8192), dim3(256), 0, 0, out, n, sink);
    });
    return 0;
}
