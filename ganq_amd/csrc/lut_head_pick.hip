// Next token straight from a packed head: the decode kernel of lut_linear.hip (lut_mfma_kernel) with the store of the logits replaced
// by a reduction to the chosen token, its score and the log-sum-exp.  The decode-side counterpart of lut_head_nll.hip.
//   l[r][o] = x[r] . dequant(qweight, lut)[o] (+ bias[o])      fp32, never rounded, never written
//   s[r][o] = l[r][o] * inv_t
//   lse[r]  = log sum_o exp(s[r][o])
//   z[r][o] = s[r][o] + noise[r][o]        (noise absent: z = s)
//   token[r]   = the SMALLEST o with z[r][o] = max_o z[r][o]
//   score[r]   = s[r][token[r]]            (without the noise)
//   logprob[r] = score[r] - lse[r]
// Only valid features (o < m) take part.  Greedy: noise = NULL, inv_t = 1.  Exact sampling from softmax(l / T): inv_t = 1 / T and
// noise = -log(E), E ~ Exp(1) iid (Gumbel-max); the noise is the caller's, nothing is drawn here.
//
// lut_head_pick_tile_kernel: one workgroup of 4 waves = 128 features x up to 64 rows x ALL of in_features (a head is wide: 1002
// workgroups at 128256 features; no split of in_features, no ticket, no counters).  The main loop is lut_mfma_kernel's (repeated here
// rather than shared so that lut_linear.hip compiles exactly as it did): packed indices decoded through an LDS codebook table into
// the B operand of v_mfma_f32_16x16x32_{f16,bf16}, activations the A operand, each wave two 16-feature tiles sharing A, RT row tiles
// sharing one decode, loads issued one chunk of four 32-column groups ahead.  Epilogue: bias in fp32, scale, noise; per row the record
//   (mx, sm, zb, sb, ob) = (max_o s, sum_o exp(s - mx), best z, its s, its feature index)
// over the workgroup's valid features, in a fixed order: across the 16 lanes that share a row (__shfl_xor at distances 1, 2, 4, 8),
// across the wave's two tiles, then across the four waves through LDS in wave order.  Merging two records: M = max(m1, m2),
// S = s1 exp(m1 - M) + s2 exp(m2 - M); a strictly larger z wins, an equal z keeps the smaller index.  One record per (feature block,
// row) goes to the workspace.
// lut_head_pick_merge_kernel: one wave per row (a decode batch has few rows and ~1000 feature blocks: a lane per row would walk them
// one dependent load after the other), its 64 lanes take 64 contiguous ranges of the row's feature blocks: the row's maximum first
// (exact in any order), then every lane walks its range in ascending block order (sum of sm exp(mx - max), best z by the same tie
// rule), eight records in flight at a time, and the 64 lanes merge by exchanges at lane distances 1, 2, ..., 32; lane 0 writes token,
// score, lse and logprob.
// No atomics, no memset, no workspace initialisation, no host synchronisation: the same bytes on every call, capturable in a HIP graph.
//
// The seeded pick (ganq_lut_head_pick_seeded, the DRAW instantiations of the tile kernel) draws the Gumbel noise in the epilogue
// instead of reading it: nothing of size [M, m] is drawn, written or read.  The generator is counter-based, Philox4x32-10 (Salmon,
// Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), one evaluation per lane and 16x16 accumulator tile,
// whose four words are exactly the four values the lane holds (feature = lane & 15, rows 4 * (lane >> 4) + reg):
//   key     = (seed_lo, seed_hi)
//   counter = (o, row >> 2, offset_lo, offset_hi)     o the feature, row the GLOBAL row of x: the noise depends neither on how M
//                                                     is cut into tile launches nor on RT
//   word `row & 3` of the result belongs to (row, o)
//   w -> k = w >> 9 -> u = (2 k + 1) 2^-24            exact in fp32, in [2^-24, 1 - 2^-24]
//   E = -logf(u), g = -logf(E), z = s + g             the accurate logf both times: E for u near 1 is the upper tail of the Gumbel
//                                                     distribution, which decides the rare tokens, and a log that is accurate only
//                                                     absolutely near 1 would distort it
// g lies in [-2.82, 16.64] and is always finite: no clamp.  The mass of a Gumbel variable above 16.64 (6e-8 per draw) falls on the
// top value.  Padding features (o >= m) and rows >= M draw nothing; a lane whose four rows are all >= M skips the evaluation (at
// M = 1 three quarters of the lanes).  Everything after z -- records, tie rule, merge order -- is the code of the noise path.
// The state {seed, offset} is two uint64 in device memory.  Every tile launch reads it; one call consumes ONE unit of offset
// whatever its shape: with `advance` set, one lane of the merge launch (stream-ordered after every tile launch of the call) stores
// offset + 1, so a captured call draws fresh noise on every replay without the host.  ganq_lut_head_pick_noise writes the same
// noise (and the raw words) as a tensor through the same device functions, for the composition path and the tests.
#include "common.h"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>

namespace ganq {

typedef _Float16 p_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 p_bf16x8 __attribute__((ext_vector_type(8)));
typedef float p_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t p_u32x4 __attribute__((ext_vector_type(4)));

// two codebook entries (dword slots holding a 16-bit value) -> one packed register, as in lut_linear.hip
__device__ __forceinline__ uint32_t p_lds_pair(uint32_t addr_lo, uint32_t addr_hi) {
    typedef const uint32_t __attribute__((address_space(3))) * lds_u32;
    return *reinterpret_cast<lds_u32>(addr_lo) | (*reinterpret_cast<lds_u32>(addr_hi) << 16);
}

constexpr int PW = 4;                 // waves per workgroup of the tile kernel
constexpr int PFB = 32 * PW;          // features per workgroup
constexpr int PROWS = 64;             // rows of x per tile launch (4 row tiles of 16)
constexpr float PICK_NEG = -FLT_MAX;  // "no feature yet" of the maximum: finite, so that PICK_NEG - PICK_NEG is 0 and not NaN
constexpr int PICK_NONE = INT_MAX;    // "no feature yet" of the pick (its z is -inf): any valid feature has a smaller index
constexpr int PCW = 4;                // waves (= rows) per workgroup of the merge kernel
constexpr int PMB = 8;                // records a lane of the merge kernel loads at a time

struct PickRec {
    float mx, sm, zb, sb;
    int ob;
};

// b joins a: a strictly larger z wins, an equal z keeps the smaller index
__device__ __forceinline__ void pick_merge(PickRec& a, const PickRec& b) {
    const float mm = fmaxf(a.mx, b.mx);
    a.sm = a.sm * __expf(a.mx - mm) + b.sm * __expf(b.mx - mm);
    a.mx = mm;
    const bool take = b.zb > a.zb || (b.zb == a.zb && b.ob < a.ob);
    a.zb = take ? b.zb : a.zb;
    a.sb = take ? b.sb : a.sb;
    a.ob = take ? b.ob : a.ob;
}

// Philox4x32-10: ten rounds of two 32 x 32 -> 64 bit products, the key bumped by the Weyl constants between rounds
__device__ __forceinline__ p_u32x4 pick_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return p_u32x4{c0, c1, c2, c3};
}

// the four words of feature o and rows 4 rg .. 4 rg + 3 under the state (seed, offset)
__device__ __forceinline__ p_u32x4 pick_draw_words(uint64_t seed, uint64_t offset, int o, int rg) {
    return pick_philox((uint32_t)o, (uint32_t)rg, (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
}

// word -> Gumbel noise: u = (2 (w >> 9) + 1) 2^-24 is exact (an odd 24-bit integer, then a power of two)
__device__ __forceinline__ float pick_gumbel(uint32_t w) {
    const float u = (float)(2u * (w >> 9) + 1u) * 0x1p-24f;
    return -logf(-logf(u));
}

// x, noise and the outputs of rows [r0, r0 + 16 RT) of M; rec4 / reco are [M][feature block].  aux: the noise (fp32 [M][m], or NULL),
// DRAW: the state {seed, offset} the noise is drawn from instead
template <int BITS, int RT, bool BF16, bool DRAW>
__global__ __launch_bounds__(PW * 64) void lut_head_pick_tile_kernel(const uint16_t* __restrict__ x, const uint32_t* __restrict__ qw,
                                                                    const uint16_t* __restrict__ lut, const uint16_t* __restrict__ bias,
                                                                    const void* __restrict__ aux, float inv_t, int r0, int M, int m, int n,
                                                                    float4* __restrict__ rec4, int* __restrict__ reco) {
    const float* __restrict__ noise = DRAW ? nullptr : static_cast<const float*>(aux);
    constexpr int V = 1 << BITS;
    constexpr int KC = RT <= 2 ? 4 : 2;              // groups in flight per wave (loads issued one chunk ahead); fewer with many row tiles,
                                                     // whose activations would otherwise leave one wave per SIMD
    constexpr bool STRADDLE = (8 * BITS) % 16 != 0;  // 3-bit: a lane's 24 bits can span two words
    __shared__ __attribute__((aligned(4096))) uint32_t tbl[PW][2][V][64];  // 4 KB alignment: see the v_perm addressing
    __shared__ float4 red4[PW - 1][16 * RT];
    __shared__ int redo[PW - 1][16 * RT];

    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, q = lane >> 4;
    const int o0 = blockIdx.x * PFB + 32 * wv;
    const int nkb = n >> 5;
    const int off = 8 * BITS * q, wi = off >> 5, sh = off & 31;
    const int wi2 = STRADDLE ? min(wi + 1, BITS - 1) : wi;
    // a padding feature decodes a copy of the last one; the epilogue leaves it out
    const int oc0 = min(o0 + col, m - 1), oc1 = min(o0 + 16 + col, m - 1);

    uint32_t wl[2][KC][2], wh[2][KC][2];
    p_u32x4 xa[2][KC][RT];
    auto issue = [&](int buf, int kb0) {  // (32-bit element offsets: the host rejects what does not fit)
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            const int kb = kb0 + c;
            const bool ok = kb < nkb;
            const int kbc = ok ? kb : 0;
            const int row = (kbc * BITS + wi) * m, row2 = (kbc * BITS + wi2) * m;
            wl[buf][c][0] = qw[row + oc0];
            wl[buf][c][1] = qw[row + oc1];
            if (STRADDLE) {
                wh[buf][c][0] = qw[row2 + oc0];
                wh[buf][c][1] = qw[row2 + oc1];
            }
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                const int xr = r0 + 16 * r + col;
                p_u32x4 v = {0u, 0u, 0u, 0u};
                if (ok && xr < M) v = *reinterpret_cast<const p_u32x4*>(x + xr * n + 32 * kbc + 8 * q);
                xa[buf][c][r] = v;
            }
        }
    };
    p_f32x4 acc[2][RT];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < RT; ++r) acc[t][r] = p_f32x4{0.f, 0.f, 0.f, 0.f};

    issue(0, 0);  // weights and activations are in flight while the table is built
    {             // every lane fetches the V entries of its own feature (rows of lut are 2V bytes, 4-byte aligned)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint32_t* lp = reinterpret_cast<const uint32_t*>(lut + (int64_t)(t ? oc1 : oc0) * V);
            uint32_t h[V / 2];
#pragma unroll
            for (int e = 0; e < V / 2; ++e) h[e] = lp[e];
#pragma unroll
            for (int e = 0; e < V / 2; ++e) {
                tbl[wv][t][2 * e][lane] = h[e] & 0xffffu;
                tbl[wv][t][2 * e + 1][lane] = h[e] >> 16;
            }
        }
    }
    __syncthreads();  // tbl ready (each wave reads only its own part; the barrier orders the LDS writes)

    // LDS byte address of entry e: tb0 + 256*e + 4*lane (+ 256*V for tile 1)
    const uint32_t tb0 = (uint32_t)(uintptr_t)(&tbl[0][0][0][0]) + (uint32_t)wv * (2u * V * 256u);
    const uint32_t lane4 = 4u * lane;
    auto consume = [&](int buf) {
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            p_u32x4 b[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                uint32_t bits = wl[buf][c][t] >> sh;
                if (STRADDLE) bits = (uint32_t)((((uint64_t)wh[buf][c][t] << 32) | wl[buf][c][t]) >> sh);
                const uint32_t tb = tb0 + (uint32_t)t * (V * 256u);
                if (BITS == 4) {
                    // byte k of lo/hi = entry index of element 2k / 2k+1, OR-ed with byte 1 of the (4 KB aligned) tile base:
                    // one v_perm per address ({byte1, byte0} = {index | base, 4*lane})
                    const uint32_t hib = ((tb >> 8) & 0xffu) * 0x01010101u;
                    const uint32_t lo = (bits & 0x0f0f0f0fu) | hib, hi = ((bits >> 4) & 0x0f0f0f0fu) | hib;
#pragma unroll
                    for (int p = 0; p < 4; ++p)
                        b[t][p] = p_lds_pair(__builtin_amdgcn_perm(lo, lane4, 0x0c0c0000u | ((4u + p) << 8)),
                                             __builtin_amdgcn_perm(hi, lane4, 0x0c0c0000u | ((4u + p) << 8)));
                } else {
                    const uint32_t base = tb + lane4;
#pragma unroll
                    for (int p = 0; p < 4; ++p)
                        b[t][p] = p_lds_pair((((bits >> (BITS * (2 * p))) & (V - 1)) << 8) + base,
                                             (((bits >> (BITS * (2 * p + 1))) & (V - 1)) << 8) + base);
                }
            }
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < RT; ++r) {
                    if (BF16)
                        acc[t][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(p_bf16x8, xa[buf][c][r]),
                                                                            __builtin_bit_cast(p_bf16x8, b[t]), acc[t][r], 0, 0, 0);
                    else
                        acc[t][r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(p_f16x8, xa[buf][c][r]),
                                                                           __builtin_bit_cast(p_f16x8, b[t]), acc[t][r], 0, 0, 0);
                }
        }
    };
    // groups past the end carry zero activations, so a ragged last chunk needs no special case
    for (int kb0 = 0; kb0 < nkb; kb0 += 2 * KC) {
        if (kb0 + KC < nkb) issue(1, kb0 + KC);
        consume(0);
        if (kb0 + KC < nkb) {
            if (kb0 + 2 * KC < nkb) issue(0, kb0 + 2 * KC);
            consume(1);
        }
    }

    // ---- epilogue.  C layout of the 16x16 tile: feature = lane & 15, row = 4 * (lane >> 4) + reg
    bool ok[2];
    float bv[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int o = o0 + 16 * t + col;
        ok[t] = o < m;
        bv[t] = 0.f;
        if (bias && ok[t]) bv[t] = BF16 ? __builtin_bit_cast(float, (uint32_t)bias[o] << 16) : (float)__builtin_bit_cast(_Float16, bias[o]);
    }
    uint64_t seed = 0, offset = 0;
    if constexpr (DRAW) {
        seed = static_cast<const uint64_t*>(aux)[0];
        offset = static_cast<const uint64_t*>(aux)[1];
    }
    PickRec mine[RT];  // after the reductions lane (q, col) keeps the record of row 16 r + 4 q + (col & 3)
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        p_f32x4 gn[2] = {p_f32x4{0.f, 0.f, 0.f, 0.f}, p_f32x4{0.f, 0.f, 0.f, 0.f}};
        if constexpr (DRAW) {  // one evaluation per tile: its word i is the lane's row i (r0 is a multiple of 64)
            const int rb = r0 + 16 * r + 4 * q;
#pragma unroll
            for (int t = 0; t < 2; ++t)
                if (ok[t] && rb < M) {
                    const p_u32x4 w = pick_draw_words(seed, offset, o0 + 16 * t + col, rb >> 2);
#pragma unroll
                    for (int i = 0; i < 4; ++i) gn[t][i] = pick_gumbel(w[i]);
                }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = r0 + 16 * r + 4 * q + i;
            PickRec rt[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int o = o0 + 16 * t + col;
                const float s = (acc[t][r][i] + bv[t]) * inv_t;
                float z = s;
                if constexpr (DRAW) {
                    if (ok[t] && row < M) z += gn[t][i];
                } else {
                    if (noise && ok[t] && row < M) z += noise[(int64_t)row * m + o];
                }
                rt[t].mx = ok[t] ? s : PICK_NEG;
                rt[t].sm = ok[t] ? 1.f : 0.f;
                rt[t].zb = ok[t] ? z : -INFINITY;
                rt[t].sb = ok[t] ? s : 0.f;
                rt[t].ob = ok[t] ? o : PICK_NONE;
#pragma unroll
                for (int w = 1; w < 16; w <<= 1) {  // the 16 lanes of a row: lane meets lane ^ w
                    PickRec other;
                    other.mx = __shfl_xor(rt[t].mx, w);
                    other.sm = __shfl_xor(rt[t].sm, w);
                    other.zb = __shfl_xor(rt[t].zb, w);
                    other.sb = __shfl_xor(rt[t].sb, w);
                    other.ob = __shfl_xor(rt[t].ob, w);
                    pick_merge(rt[t], other);
                }
            }
            pick_merge(rt[0], rt[1]);  // the wave's two tiles
            if ((col & 3) == i) mine[r] = rt[0];
        }
    }
    // across the four waves: waves 1..3 leave their records in LDS, wave 0 merges them in wave order and writes
    if (wv > 0 && col < 4) {
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            red4[wv - 1][16 * r + 4 * q + col] = make_float4(mine[r].mx, mine[r].sm, mine[r].zb, mine[r].sb);
            redo[wv - 1][16 * r + 4 * q + col] = mine[r].ob;
        }
    }
    __syncthreads();
    if (wv != 0 || col >= 4) return;
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        const int lr = 16 * r + 4 * q + col, row = r0 + lr;
        PickRec a = mine[r];
#pragma unroll
        for (int w = 0; w < PW - 1; ++w) {
            const float4 f = red4[w][lr];
            PickRec b;
            b.mx = f.x;
            b.sm = f.y;
            b.zb = f.z;
            b.sb = f.w;
            b.ob = redo[w][lr];
            pick_merge(a, b);
        }
        if (row < M) {
            rec4[(int64_t)row * gridDim.x + blockIdx.x] = make_float4(a.mx, a.sm, a.zb, a.sb);
            reco[(int64_t)row * gridDim.x + blockIdx.x] = a.ob;
        }
    }
}

__device__ __forceinline__ void pick_merge_rows(const float4* __restrict__ rec4, const int* __restrict__ reco, int M, int blocks,
                                                int64_t* __restrict__ token, float* __restrict__ score, float* __restrict__ lse,
                                                float* __restrict__ logprob) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * PCW + (threadIdx.x >> 6);  // one wave per row (no barrier below: a wave may leave)
    if (row >= M) return;
    const int per = (blocks + 63) / 64;
    const int t0 = min(blocks, lane * per), t1 = min(blocks, t0 + per);
    const float4* r4 = rec4 + (int64_t)row * blocks;
    const int* ro = reco + (int64_t)row * blocks;
    float mrow = PICK_NEG;
    for (int t = t0; t < t1; t += PMB) {  // PMB independent loads at a time
        float v[PMB];
#pragma unroll
        for (int u = 0; u < PMB; ++u) v[u] = t + u < t1 ? r4[t + u].x : PICK_NEG;
#pragma unroll
        for (int u = 0; u < PMB; ++u) mrow = fmaxf(mrow, v[u]);
    }
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) mrow = fmaxf(mrow, __shfl_xor(mrow, w));
    float s = 0.f, zb = -INFINITY, sb = 0.f;
    int ob = PICK_NONE;
    for (int t = t0; t < t1; t += PMB) {
        float4 p[PMB];
        int o[PMB];
#pragma unroll
        for (int u = 0; u < PMB; ++u) {
            const bool in = t + u < t1;
            p[u] = in ? r4[t + u] : make_float4(PICK_NEG, 0.f, -INFINITY, 0.f);
            o[u] = in ? ro[t + u] : PICK_NONE;
        }
#pragma unroll
        for (int u = 0; u < PMB; ++u) {  // ascending block order
            s += p[u].y * expf(p[u].x - mrow);
            const bool take = p[u].z > zb || (p[u].z == zb && o[u] < ob);
            zb = take ? p[u].z : zb;
            sb = take ? p[u].w : sb;
            ob = take ? o[u] : ob;
        }
    }
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) {  // the 64 ranges: lane meets lane ^ w (both sides of an exchange compute the same bits)
        s += __shfl_xor(s, w);
        const float z2 = __shfl_xor(zb, w), s2 = __shfl_xor(sb, w);
        const int o2 = __shfl_xor(ob, w);
        const bool take = z2 > zb || (z2 == zb && o2 < ob);
        zb = take ? z2 : zb;
        sb = take ? s2 : sb;
        ob = take ? o2 : ob;
    }
    if (lane != 0) return;
    const float l = mrow + logf(s);
    token[row] = ob;
    score[row] = sb;
    lse[row] = l;
    logprob[row] = sb - l;
}

__global__ __launch_bounds__(PCW * 64) void lut_head_pick_merge_kernel(const float4* __restrict__ rec4, const int* __restrict__ reco, int M,
                                                                     int blocks, int64_t* __restrict__ token, float* __restrict__ score,
                                                                     float* __restrict__ lse, float* __restrict__ logprob) {
    pick_merge_rows(rec4, reco, M, blocks, token, score, lse, logprob);
}

// the merge launch of a seeded call that advances its state: every tile launch of the call has read the state by now (stream order),
// so one lane stores offset + 1 (an ordinary 64-bit vector store)
__global__ __launch_bounds__(PCW * 64) void lut_head_pick_merge_advance_kernel(const float4* __restrict__ rec4, const int* __restrict__ reco,
                                                                             int M, int blocks, int64_t* __restrict__ token,
                                                                             float* __restrict__ score, float* __restrict__ lse,
                                                                             float* __restrict__ logprob, uint64_t* rng) {
    if (blockIdx.x == 0 && threadIdx.x == 0) rng[1] = rng[1] + 1;
    pick_merge_rows(rec4, reco, M, blocks, token, score, lse, logprob);
}

// noise [M][m] (and the raw words) of the state, through the device functions of the tile kernel: a thread per (four rows, feature)
__global__ __launch_bounds__(256) void lut_head_pick_noise_kernel(const uint64_t* __restrict__ rng, int M, int m, float* __restrict__ noise,
                                                                 uint32_t* __restrict__ words) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)((M + 3) >> 2) * m) return;
    const int rg = (int)(idx / m), o = (int)(idx - (int64_t)rg * m);
    const p_u32x4 w = pick_draw_words(rng[0], rng[1], o, rg);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = 4 * rg + i;
        if (row < M) {
            noise[(int64_t)row * m + o] = pick_gumbel(w[i]);
            if (words) words[(int64_t)row * m + o] = w[i];
        }
    }
}

static int64_t head_pick_blocks(int64_t m) { return (m + PFB - 1) / PFB; }
static int head_pick_rt(int64_t rows) { return rows <= 16 ? 1 : (rows <= 32 ? 2 : (rows <= 48 ? 3 : 4)); }

// aux: the noise (or NULL), or with DRAW the state
template <int BITS, int RT, bool DRAW>
static void launch_head_pick_rt(const uint16_t* x, const uint32_t* qw, const uint16_t* lut, const uint16_t* bias, const void* aux,
                                float inv_t, int dtype, int r0, int M, int m, int n, float4* rec4, int* reco, hipStream_t stream) {
    const dim3 grid((unsigned)head_pick_blocks(m));
    if (dtype == 1)
        hipLaunchKernelGGL((lut_head_pick_tile_kernel<BITS, RT, true, DRAW>), grid, dim3(PW * 64), 0, stream, x, qw, lut, bias, aux, inv_t, r0, M,
                           m, n, rec4, reco);
    else
        hipLaunchKernelGGL((lut_head_pick_tile_kernel<BITS, RT, false, DRAW>), grid, dim3(PW * 64), 0, stream, x, qw, lut, bias, aux, inv_t, r0, M,
                           m, n, rec4, reco);
}

template <int BITS, bool DRAW>
static void launch_head_pick_bits(int rt, const uint16_t* x, const uint32_t* qw, const uint16_t* lut, const uint16_t* bias, const void* aux,
                                  float inv_t, int dtype, int r0, int M, int m, int n, float4* rec4, int* reco, hipStream_t stream) {
    if (rt == 1) launch_head_pick_rt<BITS, 1, DRAW>(x, qw, lut, bias, aux, inv_t, dtype, r0, M, m, n, rec4, reco, stream);
    else if (rt == 2) launch_head_pick_rt<BITS, 2, DRAW>(x, qw, lut, bias, aux, inv_t, dtype, r0, M, m, n, rec4, reco, stream);
    else if (rt == 3) launch_head_pick_rt<BITS, 3, DRAW>(x, qw, lut, bias, aux, inv_t, dtype, r0, M, m, n, rec4, reco, stream);
    else launch_head_pick_rt<BITS, 4, DRAW>(x, qw, lut, bias, aux, inv_t, dtype, r0, M, m, n, rec4, reco, stream);
}

template <bool DRAW>
static void launch_head_pick(int bits, int rt, const uint16_t* x, const uint32_t* qw, const uint16_t* lut, const uint16_t* bias, const void* aux,
                             float inv_t, int dtype, int r0, int M, int m, int n, float4* rec4, int* reco, hipStream_t stream) {
    if (bits == 2) launch_head_pick_bits<2, DRAW>(rt, x, qw, lut, bias, aux, inv_t, dtype, r0, M, m, n, rec4, reco, stream);
    else if (bits == 3) launch_head_pick_bits<3, DRAW>(rt, x, qw, lut, bias, aux, inv_t, dtype, r0, M, m, n, rec4, reco, stream);
    else launch_head_pick_bits<4, DRAW>(rt, x, qw, lut, bias, aux, inv_t, dtype, r0, M, m, n, rec4, reco, stream);
}

}  // namespace ganq

using namespace ganq;

// rec4[M][ceil(m / 128)] of four fp32 (16 bytes each), then reco[M][ceil(m / 128)] int32
extern "C" size_t ganq_lut_head_pick_workspace_bytes(int64_t M, int64_t m, int64_t n, int bits) {
    (void)n;
    (void)bits;
    if (M <= 0 || m <= 0) return 0;
    return (size_t)M * (size_t)head_pick_blocks(m) * (sizeof(float4) + sizeof(int));
}

extern "C" int ganq_debug_head_pick_plan(int64_t M, int64_t m, int64_t n, int bits, int* out, int out_len) {
    const char* who = "ganq_debug_head_pick_plan";
    if (!out || out_len < 3) return fail(-3, "%s: out must hold at least 3 ints", who);
    if (M <= 0 || m <= 0 || M > INT32_MAX / 2 || m > INT32_MAX / 2) return fail(-1, "%s: bad shape", who);
    if (bits != 2 && bits != 3 && bits != 4) return fail(-2, "%s: bits=%d not supported (2, 3, 4 are)", who, bits);
    if (n < 32 || n % 32 != 0) return fail(-2, "%s: in_features=%lld must be a multiple of 32", who, (long long)n);
    const int64_t launches = (M + PROWS - 1) / PROWS;
    out[0] = (int)launches;
    out[1] = (int)head_pick_blocks(m);
    out[2] = (int)((M + PCW - 1) / PCW);
    for (int64_t i = 0; i < launches && 3 + i < out_len; ++i) out[3 + i] = head_pick_rt(std::min<int64_t>(PROWS, M - PROWS * i));
    return 0;
}

// both entries: noise (or NULL) for ganq_lut_head_pick; rng_state, drawn from in the epilogue, for ganq_lut_head_pick_seeded
static int head_pick_run(const char* who, const void* x, const int32_t* qweight, const void* lut, const void* bias, const float* noise,
                         uint64_t* rng_state, bool seeded, int advance, float inv_t, int dtype, int64_t M, int64_t m, int64_t n, int bits,
                         int64_t* token, float* score, float* lse, float* logprob, void* workspace, size_t workspace_bytes, void* stream_) {
    if (M < 0 || m < 0 || n < 0) return fail(-1, "%s: negative shape", who);
    if (M == 0) return 0;
    if (dtype != 0 && dtype != 1) return fail(-2, "%s: dtype %d (0 = fp16, 1 = bf16)", who, dtype);
    if (bits != 2 && bits != 3 && bits != 4) return fail(-2, "%s: bits=%d not supported (2, 3, 4 are)", who, bits);
    if (m < 1) return fail(-2, "%s: out_features must be at least 1", who);
    if (n < 32 || n % 32 != 0) return fail(-2, "%s: in_features=%lld must be a multiple of 32", who, (long long)n);
    if (!std::isfinite(inv_t) || !(inv_t > 0.f)) return fail(-2, "%s: inv_t=%g must be finite and positive", who, (double)inv_t);
    if (m > INT32_MAX / 2 || n > INT32_MAX / 2 || M > INT32_MAX / 2) return fail(-1, "%s: shape too large", who);
    if (!x || !qweight || !lut || !token || !score || !lse || !logprob) return fail(-3, "%s: null pointer", who);
    if (seeded && !rng_state) return fail(-3, "%s: null rng_state", who);
    if (seeded && (reinterpret_cast<uintptr_t>(rng_state) & 7) != 0) return fail(-2, "%s: rng_state must be 8-byte aligned", who);
    if ((reinterpret_cast<uintptr_t>(x) & 15) != 0) return fail(-2, "%s: x must be 16-byte aligned", who);
    if ((reinterpret_cast<uintptr_t>(lut) & 3) != 0) return fail(-2, "%s: lut must be 4-byte aligned", who);
    const size_t need = ganq_lut_head_pick_workspace_bytes(M, m, n, bits);
    if (!workspace || workspace_bytes < need) return fail(-4, "%s: workspace %zu B < required %zu B", who, workspace_bytes, need);
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return fail(-2, "%s: workspace must be 16-byte aligned", who);
    // both operands are addressed through 32-bit offsets
    if (!(M * n * 2 < (1ll << 31) && (int64_t)(n >> 5) * bits * m * 4 < (1ll << 31)))
        return fail(-1, "%s: x (%lld x %lld) or qweight beyond the 2 GB window of the kernel's 32-bit offsets: split the rows of x over "
                        "several calls", who, (long long)M, (long long)n);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t blocks = head_pick_blocks(m);
    float4* rec4 = static_cast<float4*>(workspace);
    int* reco = reinterpret_cast<int*>(static_cast<char*>(workspace) + (size_t)M * (size_t)blocks * sizeof(float4));
    const uint16_t* xp = static_cast<const uint16_t*>(x);
    const uint32_t* qw = reinterpret_cast<const uint32_t*>(qweight);
    const uint16_t* lp = static_cast<const uint16_t*>(lut);
    const uint16_t* bp = static_cast<const uint16_t*>(bias);
    for (int64_t r0 = 0; r0 < M; r0 += PROWS) {  // one tile launch per 64 rows
        const int rt = head_pick_rt(std::min<int64_t>(PROWS, M - r0));
        if (seeded) launch_head_pick<true>(bits, rt, xp, qw, lp, bp, rng_state, inv_t, dtype, (int)r0, (int)M, (int)m, (int)n, rec4, reco, stream);
        else launch_head_pick<false>(bits, rt, xp, qw, lp, bp, noise, inv_t, dtype, (int)r0, (int)M, (int)m, (int)n, rec4, reco, stream);
        GANQ_LAUNCH_CHECK();
    }
    const dim3 grid((unsigned)((M + PCW - 1) / PCW));
    if (seeded && advance)
        hipLaunchKernelGGL(lut_head_pick_merge_advance_kernel, grid, dim3(PCW * 64), 0, stream, rec4, reco, (int)M, (int)blocks, token, score, lse,
                           logprob, rng_state);
    else
        hipLaunchKernelGGL(lut_head_pick_merge_kernel, grid, dim3(PCW * 64), 0, stream, rec4, reco, (int)M, (int)blocks, token, score, lse,
                           logprob);
    GANQ_LAUNCH_CHECK();
    return 0;
}

extern "C" int ganq_lut_head_pick(const void* x, const int32_t* qweight, const void* lut, const void* bias, const float* noise, float inv_t,
                                  int dtype, int64_t M, int64_t m, int64_t n, int bits, int64_t* token, float* score, float* lse,
                                  float* logprob, void* workspace, size_t workspace_bytes, void* stream_) {
    return head_pick_run("ganq_lut_head_pick", x, qweight, lut, bias, noise, nullptr, false, 0, inv_t, dtype, M, m, n, bits, token, score, lse,
                         logprob, workspace, workspace_bytes, stream_);
}

extern "C" int ganq_lut_head_pick_seeded(const void* x, const int32_t* qweight, const void* lut, const void* bias, uint64_t* rng_state,
                                         int advance, float inv_t, int dtype, int64_t M, int64_t m, int64_t n, int bits, int64_t* token,
                                         float* score, float* lse, float* logprob, void* workspace, size_t workspace_bytes, void* stream_) {
    return head_pick_run("ganq_lut_head_pick_seeded", x, qweight, lut, bias, nullptr, rng_state, true, advance, inv_t, dtype, M, m, n, bits,
                         token, score, lse, logprob, workspace, workspace_bytes, stream_);
}

extern "C" int ganq_lut_head_pick_noise(const uint64_t* rng_state, int64_t M, int64_t m, float* noise, uint32_t* words, void* stream_) {
    const char* who = "ganq_lut_head_pick_noise";
    if (M < 0 || m < 0) return fail(-1, "%s: negative shape", who);
    if (M == 0 || m == 0) return 0;
    if (m > INT32_MAX / 2 || M > INT32_MAX / 2) return fail(-1, "%s: shape too large", who);
    if (!rng_state || !noise) return fail(-3, "%s: null pointer", who);
    if ((reinterpret_cast<uintptr_t>(rng_state) & 7) != 0) return fail(-2, "%s: rng_state must be 8-byte aligned", who);
    const int64_t grid = (((M + 3) >> 2) * m + 255) / 256;
    if (grid > INT32_MAX) return fail(-1, "%s: %lld x %lld beyond one launch: split the rows", who, (long long)M, (long long)m);
    hipLaunchKernelGGL(lut_head_pick_noise_kernel, dim3((unsigned)grid), dim3(256), 0, static_cast<hipStream_t>(stream_), rng_state, (int)M,
                       (int)m, noise, words);
    GANQ_LAUNCH_CHECK();
    return 0;
}
