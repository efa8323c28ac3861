// Per-token negative log-likelihood straight from a packed head: the fused LUT-dequant GEMM of lut_gemm.hip with the store of the
// logits replaced by a log-sum-exp reduction.
//   logits[M,m] = x[M,n] @ dequant(qweight, lut)^T (+ bias)   in fp32, never rounded, never written
//   lse[row] = log sum_o exp(logits[row][o]),  tgt_logit[row] = logits[row][target[row]],  nll[row] = lse - tgt_logit
//
// lut_head_nll_tile_kernel: one workgroup = one 256 x 128 tile of the logits.  The main loop is the whole-K loop of
// lut_gemm_kernel<BITS, BF16, /*SPLIT*/false, RAGGED, /*LORA*/false> (same slab and weight staging, same codebook table, same
// XCD tile remap; it is repeated here rather than shared so that lut_gemm.hip's kernels compile exactly as they did).  The
// epilogue adds the bias in fp32 and reduces every row of the tile over the tile's VALID features (o < m) to the pair
//   (mx, sm) = (max_o logit, sum_o exp(logit - mx))      -> partial[tile_n][row]   (8 bytes per row and feature tile)
// in a fixed order: in a lane over its four 32-feature sub-tiles, then across the 32 lanes of a half-wave by a reduce-scatter of
// five ds_bpermute exchanges (lane distances 16, 8, 4, 2, 1; the lane that keeps a row is a fixed function of the row), merging
// (mx, sm) pairs as  M = max(m1, m2), S = s1 exp(m1 - M) + s2 exp(m2 - M).  The lane that holds feature target[row] also writes
// that one fp32 logit to tgt[row]: exactly one lane of one workgroup per row with a target inside [0, m).
// lut_head_nll_combine_kernel: 64 rows per workgroup (lane = row: the reads of partial[tile][row] are whole lines), its 16 waves
// take 16 contiguous ranges of the feature tiles: the row's maximum first (exact in any order), then every wave sums
// sm exp(mx - max) over its range in ascending tile order and wave 0 adds the 16 sums in wave order.  No atomics, no memset, no
// host synchronisation: the same bytes on every call, capturable in a HIP graph.
#include "common.h"

#include <cfloat>

namespace ganq {

typedef _Float16 n_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 n_bf16x8 __attribute__((ext_vector_type(8)));
typedef float n_f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t n_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t n_lds_pair(uint32_t addr_lo, uint32_t addr_hi) {
    typedef const uint32_t __attribute__((address_space(3))) * lds_u32;
    return *reinterpret_cast<lds_u32>(addr_lo) | (*reinterpret_cast<lds_u32>(addr_hi) << 16);
}

constexpr int NBN = 128;               // features per workgroup
constexpr int NBM = 256;               // rows of x per workgroup: 4 waves x 64 rows
constexpr int NST = 2;                 // groups of 32 in_features per stage
constexpr int NPITCH = 64 * NST + 16;  // bytes per LDS row, as in lut_gemm.hip
constexpr float NLL_NEG = -FLT_MAX;    // "no feature yet": finite, so that NLL_NEG - NLL_NEG is 0 and not NaN
constexpr int NCW = 16;                // waves per workgroup of the combine kernel

// one exchange of the reduce-scatter: a lane keeps W of its 2 W rows and receives its partner's pairs for them
template <int W>
__device__ __forceinline__ void nll_fold(float (&mx)[32], float (&sm)[32], int l31) {
    const bool up = (l31 & W) != 0;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        const float km = up ? mx[i + W] : mx[i], ks = up ? sm[i + W] : sm[i];
        const float om = __shfl_xor(up ? mx[i] : mx[i + W], W), os = __shfl_xor(up ? sm[i] : sm[i + W], W);
        const float mm = fmaxf(km, om);
        mx[i] = mm;
        sm[i] = ks * __expf(km - mm) + os * __expf(om - mm);
    }
}

template <int BITS, bool BF16, bool RAGGED>
__global__ __launch_bounds__(256, 2) void lut_head_nll_tile_kernel(const uint16_t* __restrict__ x, const uint32_t* __restrict__ qw,
                                                                 const uint16_t* __restrict__ lut, const uint16_t* __restrict__ bias,
                                                                 const int64_t* __restrict__ targets, int M, int m, int n, int tiles_m,
                                                                 int tiles_n, float2* __restrict__ partial, float* __restrict__ tgt) {
    constexpr int V = 1 << BITS;
    constexpr bool STRADDLE = (8 * BITS) % 16 != 0;  // 3-bit: an octet's 24 bits can span two words
    constexpr int TPR = 4 * NST;                     // threads per slab row (16 B each)
    constexpr int RPP = 256 / TPR;                   // rows per pass of the 256 threads
    constexpr int NLD = NBM / RPP;                   // 16-byte activation loads per thread and stage
    constexpr int NIT = 2 * NST;                     // (group, octet) items a thread decodes per stage
    __shared__ __attribute__((aligned(4096))) uint32_t tbl[2][V][64];  // [feature half][entry][lane]
    __shared__ __attribute__((aligned(16))) unsigned char As[NBM * NPITCH];
    __shared__ __attribute__((aligned(16))) unsigned char Bs[NBN * NPITCH];

    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hf = lane >> 5;
    // XCD-aware tile order of lut_gemm.hip: each XCD walks whole row blocks of x
    int bid = blockIdx.x;
    {
        const int total = tiles_m * tiles_n;
        const int per = total >> 3;
        if ((total & 7) == 0) bid = (bid & 7) * per + (bid >> 3);
    }
    const int tm = bid / tiles_n, tn = bid % tiles_n;
    const int r0 = tm * NBM, o0 = tn * NBN;
    const int nkb = n >> 5, nst = (nkb + NST - 1) / NST;

    // ---- decode role: this thread's feature and octets
    const int dfeat = tid & 127, dq0 = __builtin_amdgcn_readfirstlane(tid >> 7);
    const int dcol = min(o0 + dfeat, m - 1);  // (a padding feature decodes a copy of the last one; the epilogue leaves it out)
    if (wv < 2) {
        const uint32_t* lp = reinterpret_cast<const uint32_t*>(lut + (int64_t)dcol * V);
        uint32_t h[V / 2];
#pragma unroll
        for (int e = 0; e < V / 2; ++e) h[e] = lp[e];
#pragma unroll
        for (int e = 0; e < V / 2; ++e) {
            tbl[wv][2 * e][lane] = h[e] & 0xffffu;
            tbl[wv][2 * e + 1][lane] = h[e] >> 16;
        }
    }
    int wi[2], sh[2], wi2[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int off = 8 * BITS * (dq0 + 2 * j);
        wi[j] = off >> 5;
        sh[j] = off & 31;
        wi2[j] = STRADDLE ? min(wi[j] + 1, BITS - 1) : wi[j];
    }

    // ---- global -> register staging of one stage (buffer loads with 32-bit offsets: the host rejects what does not fit;
    // activation rows past M lie past the resource's end and read as zeros)
    const int achunk = tid % TPR, arow0 = tid / TPR;
    const __amdgpu_buffer_rsrc_t rsx = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(x), 0, (int)((int64_t)M * n * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsw =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(qw), 0, (int)((int64_t)(n >> 5) * BITS * m * 4), 0x00020000);
    int xoff[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) xoff[i] = ((r0 + arow0 + RPP * i) * n + 8 * achunk) * 2;
    const int woff = dcol * 4;
    n_u32x4 xa[NLD];
    uint32_t wl[NIT], wh[NIT];
    auto gload = [&](int st) {
        const int soff = 64 * NST * st;
#pragma unroll
        for (int i = 0; i < NLD; ++i)
            xa[i] = __builtin_bit_cast(n_u32x4, RAGGED ? __builtin_amdgcn_raw_buffer_load_b128(rsx, xoff[i] + soff, 0, 0)
                                                      : __builtin_amdgcn_raw_buffer_load_b128(rsx, xoff[i], soff, 0));
#pragma unroll
        for (int g = 0; g < NST; ++g) {
            const int kb = RAGGED ? min(NST * st + g, nkb - 1) : NST * st + g;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                wl[2 * g + j] = __builtin_amdgcn_raw_buffer_load_b32(rsw, woff, (kb * BITS + wi[j]) * m * 4, 0);
                if (STRADDLE) wh[2 * g + j] = __builtin_amdgcn_raw_buffer_load_b32(rsw, woff, (kb * BITS + wi2[j]) * m * 4, 0);
            }
        }
    };
    const uint32_t tb = (uint32_t)(uintptr_t)(&tbl[0][0][0]) + (uint32_t)(wv & 1) * (V * 256u);
    const uint32_t lane4 = 4u * lane;
    auto sstore = [&](int st) {  // registers -> LDS: the activation slab as it is, the weights decoded
        const bool col_ok = !RAGGED || 32 * NST * st + 8 * achunk < n;
#pragma unroll
        for (int i = 0; i < NLD; ++i)
            *reinterpret_cast<n_u32x4*>(As + (arow0 + RPP * i) * NPITCH + 16 * achunk) = col_ok ? xa[i] : n_u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int g = 0; g < NST; ++g)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                uint32_t bits = wl[2 * g + j] >> sh[j];
                if (STRADDLE) bits = (uint32_t)((((uint64_t)wh[2 * g + j] << 32) | wl[2 * g + j]) >> sh[j]);
                n_u32x4 b;
                if (BITS == 4) {
                    const uint32_t hib = ((tb >> 8) & 0xffu) * 0x01010101u;
                    const uint32_t lo = (bits & 0x0f0f0f0fu) | hib, hi = ((bits >> 4) & 0x0f0f0f0fu) | hib;
#pragma unroll
                    for (int p = 0; p < 4; ++p)
                        b[p] = n_lds_pair(__builtin_amdgcn_perm(lo, lane4, 0x0c0c0000u | ((4u + p) << 8)),
                                          __builtin_amdgcn_perm(hi, lane4, 0x0c0c0000u | ((4u + p) << 8)));
                } else {
                    const uint32_t base = tb + lane4;
#pragma unroll
                    for (int p = 0; p < 4; ++p)
                        b[p] = n_lds_pair((((bits >> (BITS * (2 * p))) & (V - 1)) << 8) + base,
                                          (((bits >> (BITS * (2 * p + 1))) & (V - 1)) << 8) + base);
                }
                *reinterpret_cast<n_u32x4*>(Bs + dfeat * NPITCH + 64 * g + 16 * (dq0 + 2 * j)) = b;
            }
    };

    n_f32x16 acc[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[r][t][i] = 0.f;

    gload(0);
    __syncthreads();  // codebook table
    sstore(0);
    __syncthreads();  // first slab + weight tile
    if (1 < nst) gload(1);
    const unsigned char* abase = As + (64 * wv + l31) * NPITCH + 16 * hf;
    const unsigned char* bbase = Bs + l31 * NPITCH + 16 * hf;
    for (int st = 0; st < nst; ++st) {
        n_u32x4 a_cur[2], b_cur[4];
#pragma unroll
        for (int r = 0; r < 2; ++r) a_cur[r] = *reinterpret_cast<const n_u32x4*>(abase + 32 * r * NPITCH);
#pragma unroll
        for (int t = 0; t < 4; ++t) b_cur[t] = *reinterpret_cast<const n_u32x4*>(bbase + 32 * t * NPITCH);
#pragma unroll
        for (int u = 0; u < 2 * NST; ++u) {
            n_u32x4 a_nxt[2], b_nxt[4];
            if (u + 1 < 2 * NST) {
#pragma unroll
                for (int r = 0; r < 2; ++r) a_nxt[r] = *reinterpret_cast<const n_u32x4*>(abase + 32 * r * NPITCH + 32 * (u + 1));
#pragma unroll
                for (int t = 0; t < 4; ++t) b_nxt[t] = *reinterpret_cast<const n_u32x4*>(bbase + 32 * t * NPITCH + 32 * (u + 1));
            }
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (BF16)
                        acc[r][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(n_bf16x8, a_cur[r]),
                                                                            __builtin_bit_cast(n_bf16x8, b_cur[t]), acc[r][t], 0, 0, 0);
                    else
                        acc[r][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(n_f16x8, a_cur[r]),
                                                                           __builtin_bit_cast(n_f16x8, b_cur[t]), acc[r][t], 0, 0, 0);
                }
            if (u + 1 < 2 * NST) {
#pragma unroll
                for (int r = 0; r < 2; ++r) a_cur[r] = a_nxt[r];
#pragma unroll
                for (int t = 0; t < 4; ++t) b_cur[t] = b_nxt[t];
            }
        }
        if (st + 1 < nst) {
            __syncthreads();  // every wave has read this stage's tiles
            sstore(st + 1);   // the next stage (its loads were issued a stage ago)
            __syncthreads();
            if (st + 2 < nst) gload(st + 2);
        }
    }

    // ---- epilogue.  C layout of the 32x32 tile: feature = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    bool ok[4];
    float bv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int o = o0 + 32 * t + l31;
        ok[t] = o < m;
        bv[t] = 0.f;
        if (bias && ok[t]) bv[t] = BF16 ? __builtin_bit_cast(float, (uint32_t)bias[o] << 16) : (float)__builtin_bit_cast(_Float16, bias[o]);
    }
    const int wrow0 = r0 + 64 * wv + 4 * hf;
    float mx[32], sm[32];  // index q = 16 r + reg: this lane's share of row wrow0 + 32 r + (reg & 3) + 8 * (reg >> 2)
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            float v[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) v[t] = acc[r][t][reg] + bv[t];
            const int row = wrow0 + 32 * r + (reg & 3) + 8 * (reg >> 2);
            if (row < M) {  // the target's logit: d = 32 t for exactly one (lane, t) of one feature tile
                const int64_t tg = targets[row], d = tg - (o0 + l31);
                if (tg >= 0 && tg < m && d >= 0 && d < NBN && (d & 31) == 0) {
                    const int t = (int)(d >> 5);
                    tgt[row] = t == 0 ? v[0] : (t == 1 ? v[1] : (t == 2 ? v[2] : v[3]));
                }
            }
            float mloc = NLL_NEG;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (ok[t]) mloc = fmaxf(mloc, v[t]);
            float s = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t) s += ok[t] ? __expf(v[t] - mloc) : 0.f;
            mx[16 * r + reg] = mloc;
            sm[16 * r + reg] = s;
        }
    nll_fold<16>(mx, sm, l31);
    nll_fold<8>(mx, sm, l31);
    nll_fold<4>(mx, sm, l31);
    nll_fold<2>(mx, sm, l31);
    nll_fold<1>(mx, sm, l31);
    // the lane now holds the pair of q = l31
    const int row = wrow0 + 32 * (l31 >> 4) + (l31 & 3) + 8 * ((l31 & 15) >> 2);
    if (row < M) partial[(int64_t)tn * M + row] = make_float2(mx[0], sm[0]);
}

__global__ __launch_bounds__(NCW * 64) void lut_head_nll_combine_kernel(const float2* __restrict__ partial, const float* __restrict__ tgt,
                                                                      const int64_t* __restrict__ targets, int M, int m, int tiles_n,
                                                                      float* __restrict__ nll, float* __restrict__ lse,
                                                                      float* __restrict__ tgt_logit) {
    __shared__ float red[NCW][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int row = blockIdx.x * 64 + lane;
    const bool live = row < M;
    const int per = (tiles_n + NCW - 1) / NCW;
    const int t0 = min(tiles_n, wv * per), t1 = min(tiles_n, t0 + per);
    float mloc = NLL_NEG;
    if (live)
        for (int t = t0; t < t1; ++t) mloc = fmaxf(mloc, partial[(int64_t)t * M + row].x);
    red[wv][lane] = mloc;
    __syncthreads();
    float mrow = NLL_NEG;
#pragma unroll
    for (int w = 0; w < NCW; ++w) mrow = fmaxf(mrow, red[w][lane]);
    __syncthreads();
    float s = 0.f;
    if (live)
        for (int t = t0; t < t1; ++t) {  // ascending tile order
            const float2 p = partial[(int64_t)t * M + row];
            s += p.y * expf(p.x - mrow);
        }
    red[wv][lane] = s;
    __syncthreads();
    if (wv != 0 || !live) return;
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < NCW; ++w) tot += red[w][lane];  // wave order = ascending tile ranges
    const float l = mrow + logf(tot);
    const int64_t tg = targets[row];
    const bool hit = tg >= 0 && tg < m;  // anything else (-100 included) is an ignored row: tgt[row] was never written
    const float tl = hit ? tgt[row] : 0.f;
    lse[row] = l;
    tgt_logit[row] = tl;
    nll[row] = hit ? l - tl : 0.f;
}

static size_t head_nll_partial_bytes(int64_t M, int64_t m) { return (size_t)M * (size_t)((m + NBN - 1) / NBN) * sizeof(float2); }

template <int BITS>
static void launch_head_nll_bits(const uint16_t* x, const uint32_t* qw, const uint16_t* lut, const uint16_t* bias, const int64_t* targets,
                                 int dtype, int M, int m, int n, int tiles_m, int tiles_n, float2* partial, float* tgt, hipStream_t stream) {
    const dim3 grid((unsigned)(tiles_m * tiles_n));
#define GANQ_NLL_LAUNCH(BF, RG)                                                                                                        \
    hipLaunchKernelGGL((lut_head_nll_tile_kernel<BITS, BF, RG>), grid, dim3(256), 0, stream, x, qw, lut, bias, targets, M, m, n, tiles_m, \
                       tiles_n, partial, tgt)
    const bool ragged = (n & 63) != 0;
    if (dtype == 1) {
        if (ragged) GANQ_NLL_LAUNCH(true, true);
        else GANQ_NLL_LAUNCH(true, false);
    } else {
        if (ragged) GANQ_NLL_LAUNCH(false, true);
        else GANQ_NLL_LAUNCH(false, false);
    }
#undef GANQ_NLL_LAUNCH
}

}  // namespace ganq

using namespace ganq;

// partial[ceil(m / 128)][M] pairs of fp32 (8 bytes each), then tgt[M] fp32
extern "C" size_t ganq_lut_head_nll_workspace_bytes(int64_t M, int64_t m, int64_t n, int bits) {
    (void)n;
    (void)bits;
    if (M <= 0 || m <= 0) return 0;
    return head_nll_partial_bytes(M, m) + (size_t)M * sizeof(float);
}

extern "C" int ganq_lut_head_nll(const void* x, const int32_t* qweight, const void* lut, const void* bias, const int64_t* targets,
                                 int dtype, int64_t M, int64_t m, int64_t n, int bits, float* nll, float* lse, float* tgt_logit,
                                 void* workspace, size_t workspace_bytes, void* stream_) {
    const char* who = "ganq_lut_head_nll";
    if (M < 0 || m < 0 || n < 0) return fail(-1, "%s: negative shape", who);
    if (M == 0) return 0;
    if (dtype != 0 && dtype != 1) return fail(-2, "%s: dtype %d (0 = fp16, 1 = bf16)", who, dtype);
    if (bits != 2 && bits != 3 && bits != 4) return fail(-2, "%s: bits=%d not supported (2, 3, 4 are)", who, bits);
    if (m < 1) return fail(-2, "%s: out_features must be at least 1", who);
    if (n < 32 || n % 32 != 0) return fail(-2, "%s: in_features=%lld must be a multiple of 32", who, (long long)n);
    if (m > INT32_MAX / 2 || n > INT32_MAX / 2 || M > INT32_MAX / 2) return fail(-1, "%s: shape too large", who);
    if (!x || !qweight || !lut || !targets || !nll || !lse || !tgt_logit) return fail(-3, "%s: null pointer", who);
    if ((reinterpret_cast<uintptr_t>(x) & 15) != 0) return fail(-2, "%s: x must be 16-byte aligned", who);
    if ((reinterpret_cast<uintptr_t>(lut) & 3) != 0) return fail(-2, "%s: lut must be 4-byte aligned", who);
    const size_t need = ganq_lut_head_nll_workspace_bytes(M, m, n, bits);
    if (!workspace || workspace_bytes < need) return fail(-4, "%s: workspace %zu B < required %zu B", who, workspace_bytes, need);
    if ((reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return fail(-2, "%s: workspace must be 8-byte aligned", who);
    // both operands are addressed through 32-bit buffer offsets (incl. one stage of look-ahead), as in lut_gemm.hip
    if (!(((int64_t)M + NBM) * n * 2 < (1ll << 31) && (int64_t)(n >> 5) * bits * m * 4 < (1ll << 31)))
        return fail(-1, "%s: x (%lld x %lld) or qweight beyond the 2 GB window of the kernel's buffer loads: split the rows of x over "
                        "several calls", who, (long long)M, (long long)n);
    const int tiles_m = (int)((M + NBM - 1) / NBM), tiles_n = (int)((m + NBN - 1) / NBN);
    if ((int64_t)tiles_m * tiles_n > INT32_MAX) return fail(-1, "%s: too many tiles", who);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    float2* partial = static_cast<float2*>(workspace);
    float* tgt = reinterpret_cast<float*>(static_cast<char*>(workspace) + head_nll_partial_bytes(M, m));
    const uint16_t* xp = static_cast<const uint16_t*>(x);
    const uint32_t* qw = reinterpret_cast<const uint32_t*>(qweight);
    const uint16_t* lp = static_cast<const uint16_t*>(lut);
    const uint16_t* bp = static_cast<const uint16_t*>(bias);
    if (bits == 2) launch_head_nll_bits<2>(xp, qw, lp, bp, targets, dtype, (int)M, (int)m, (int)n, tiles_m, tiles_n, partial, tgt, stream);
    else if (bits == 3) launch_head_nll_bits<3>(xp, qw, lp, bp, targets, dtype, (int)M, (int)m, (int)n, tiles_m, tiles_n, partial, tgt, stream);
    else launch_head_nll_bits<4>(xp, qw, lp, bp, targets, dtype, (int)M, (int)m, (int)n, tiles_m, tiles_n, partial, tgt, stream);
    GANQ_LAUNCH_CHECK();
    hipLaunchKernelGGL(lut_head_nll_combine_kernel, dim3((unsigned)((M + 63) / 64)), dim3(NCW * 64), 0, stream, partial, tgt, targets, (int)M,
                       (int)m, tiles_n, nll, lse, tgt_logit);
    GANQ_LAUNCH_CHECK();
    return 0;
}
