// Backward of the LUT-dequant linear (the gradients autograd takes through FakeQuantLinear.forward, fake.py:88-89):
//   ganq_lut_linear_bwd_input: dx [M,n] = dy [M,m] @ dequant(qweight, lut) (+ addend fp32)   fp32 accumulation, one rounding
//   ganq_lut_linear_bwd_lut:   dlut [m,V] fp32 = sum_b sum_j [Q[o][j] == v] dy[b][o] x[b][j]
// Layout and conventions as ganq_lut_linear_fwd (lut_linear.hip): qweight [n*bits/32][m] int32 (GPTQ packing along in_features),
// lut [m][V] in the activation dtype.  Every reduction runs in a fixed order: bitwise repeatable, no floating-point atomics.
//
// Input gradient.  M > 64: the transposed dequant writes Wq^T [n][ceil64(m)] into the workspace and the dense GEMM of the
//   forward's prefill path (gemm_h16.hip) multiplies; a ragged m gets a zero-padded copy of dy.  M <= 64: one kernel reads the
//   packed indices directly -- a workgroup owns one group of 32 input features and streams the output features o (qweight's
//   contiguous dimension) through v_mfma_f32_16x16x32 with the decoded weights as the A operand; too few groups to fill the chip
//   split o over workgroups, and a second launch sums the splits in order.
// Codebook gradient.  dy^T [m][Mp] and X^T [n][Mp] (tokens contiguous, Mp = ceil64(M), zero-filled) are staged in the workspace;
//   gemm_h16's main loop forms G = dy^T X over the tokens and its bucket epilogue sums each G[o][j] into the bin of Q[o][j], one
//   fp32 partial per 256-column tile; a second launch sums the tiles in order.  More tokens than one launch addresses are taken in
//   chunks whose sums are added in chunk order.
#include "common.h"
#include "lut_bits.h"

#include <algorithm>

namespace ganq {

namespace {

typedef _Float16 lb_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 lb_bf16x8 __attribute__((ext_vector_type(8)));
typedef float lb_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t lb_u32x4 __attribute__((ext_vector_type(4)));

constexpr int LB_SMALL_M = 64;       // rows of dy the direct kernel takes (four 16-row tiles), as the forward's decode kernels
constexpr int LB_TARGET_WGS = 1024;  // workgroups the direct kernel aims for (four per CU of the MI355X, 16 waves to cover the
                                     // latency of the packed-index loads; a constant, not a query)

__device__ __forceinline__ uint16_t lb_round(float v, bool bf16) {
    return bf16 ? __builtin_bit_cast(uint16_t, (__bf16)v) : __builtin_bit_cast(uint16_t, (_Float16)v);
}

// Wt [n][mp] = dequant(qweight, lut)^T, zero in the pad columns o >= m.  64 output features per workgroup (lane = o), their codebooks
// in LDS as tbl[entry][feature]; a wave decodes one group of 32 input features per step from BITS coalesced word loads and writes
// each of its 32 rows j as one whole 128-byte line (64 lanes x 2 B, consecutive o).
template <int BITS>
__global__ __launch_bounds__(256) void lut_dequant_t_kernel(const uint32_t* __restrict__ qw, const uint16_t* __restrict__ lut, int m, int n,
                                                            int mp, uint16_t* __restrict__ Wt) {
    constexpr int V = 1 << BITS;
    __shared__ uint16_t tbl[V][64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int o0 = blockIdx.x * 64;
    for (int i = tid; i < 64 * V; i += 256) {
        const int f = i / V, e = i % V;
        tbl[e][f] = (o0 + f < m) ? lut[(int64_t)(o0 + f) * V + e] : (uint16_t)0;  // (pad features: an all-zero codebook)
    }
    __syncthreads();
    const int o = o0 + lane, oc = min(o, m - 1);
    const int ngroups = n >> 5;
    for (int g = blockIdx.y * 4 + wv; g < ngroups; g += gridDim.y * 4) {
        uint32_t w[BITS];
#pragma unroll
        for (int b = 0; b < BITS; ++b) w[b] = qw[(int64_t)(g * BITS + b) * m + oc];
        uint16_t* out = Wt + (int64_t)(32 * g) * mp + o;
#pragma unroll
        for (int c = 0; c < 32; ++c) out[(int64_t)c * mp] = tbl[extract<BITS>(w, c)][lane];
    }
}

// dst [rows][mp] = src [rows][m] with zero columns m .. mp - 1 (the GEMM takes K in whole tiles of 64)
__global__ __launch_bounds__(256) void lb_pad_cols_kernel(const uint16_t* __restrict__ src, int64_t rows, int m, int mp,
                                                          uint16_t* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * mp) return;
    const int64_t r = i / mp;
    const int k = (int)(i - r * mp);
    dst[i] = k < m ? src[r * m + k] : (uint16_t)0;
}

// dst [width][mp] = src [rows][width]^T with zero tokens rows .. mp - 1: 64 x 64 tiles through LDS, coalesced on both sides
__global__ __launch_bounds__(256) void lb_stage_t_kernel(const uint16_t* __restrict__ src, int64_t rows, int width, int64_t mp,
                                                         uint16_t* __restrict__ dst) {
    __shared__ uint16_t tile[64][66];
    const int c0 = blockIdx.x * 64;
    const int64_t t0 = (int64_t)blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) {
        const int64_t t = t0 + r;
        const int c = c0 + tx;
        tile[r][tx] = (t < rows && c < width) ? src[t * width + c] : (uint16_t)0;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int c = c0 + r;
        if (c < width) dst[(int64_t)c * mp + t0 + tx] = tile[tx][r];
    }
}

// Direct input gradient for M <= 64.  Workgroup (g, ks): input features 32 g .. 32 g + 31, chunks of 32 output features
// [ks * cpw, (ks + 1) * cpw) dealt to its four waves round-robin.  Per chunk the wave stages the chunk's codebooks in its own LDS
// slice (dword slots, row stride V + 2: the four rows one lookup instruction touches fall in distinct banks) and forms
//   D[j][b] += A[j][o] B[o][b],   A = Wq^T (lane: column j = l & 15 (+ 16), the 8 features o = 8 (l >> 4) ..; decoded from the
//   BITS words of each o and looked up in LDS), B = dy^T (lane: row b = l & 15 of a 16-row tile, the same 8 features: 16 bytes).
// The waves' accumulators are summed in wave order through LDS; KS = 1 rounds (+ addend) and stores dx, otherwise the fp32 partial of
// split ks goes to part [ks][M][n].
template <int BITS, int BT, bool BF16, bool VEC>
__global__ __launch_bounds__(256) void lut_bwd_input_small_kernel(const uint16_t* __restrict__ dy, const uint32_t* __restrict__ qw,
                                                                  const uint16_t* __restrict__ lut, const float* __restrict__ addend, int M,
                                                                  int m, int n, int cpw, int KS, float* __restrict__ part,
                                                                  uint16_t* __restrict__ dx) {
    constexpr int V = 1 << BITS, LS = V + 2, VW = V / 4;  // VW: dwords of codebook a lane stages (half a row)
    __shared__ uint32_t lbuf[4][32 * LS];
    __shared__ lb_f32x4 red[4][2][BT][64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // (scalar: the chunk loop below branches on it)
    const int g = blockIdx.x, ks = blockIdx.y;
    const int q = lane >> 4, jj = lane & 15;
    const int nch = (m + 31) >> 5;
    const int c_end = min(nch, (ks + 1) * cpw);
    uint32_t* mb = lbuf[wv];

    lb_f32x4 acc[2][BT];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int b = 0; b < BT; ++b) acc[t][b] = lb_f32x4{0.f, 0.f, 0.f, 0.f};

    // The global loads of a chunk carry no per-lane condition (indices clamped; see dy below), so the ~40 loads of one chunk are
    // in flight together; and the loads of the wave's NEXT chunk are issued before the current one is decoded and multiplied (one
    // chunk of prefetch in registers).
    const int rr = lane >> 1, hh = lane & 1;
    uint32_t lw[VW], w[8][BITS];
    lb_u32x4 Bf[BT];
    auto load = [&](int c) {
        const int oc0 = c * 32;
        const uint32_t* lrow = reinterpret_cast<const uint32_t*>(lut + (int64_t)min(oc0 + rr, m - 1) * V) + hh * VW;
#pragma unroll
        for (int e = 0; e < VW; ++e) lw[e] = lrow[e];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int o = min(oc0 + 8 * q + t, m - 1);  // (features past m: their codebook rows are staged as zeros)
#pragma unroll
            for (int b = 0; b < BITS; ++b) w[t][b] = qw[(int64_t)(g * BITS + b) * m + o];
        }
        // dy: rows past M are clamped (they only feed output columns that are never stored); features past m are clamped here and
        // zeroed when the chunk is multiplied (the last chunk of the layer only), so that no load sits behind a branch
        const int o8 = oc0 + 8 * q;
#pragma unroll
        for (int bt = 0; bt < BT; ++bt) {
            const uint16_t* src = dy + (int64_t)min(bt * 16 + jj, M - 1) * m;
            if constexpr (VEC) {  // m % 8 == 0: a group of 8 features is wholly inside or outside
                Bf[bt] = *reinterpret_cast<const lb_u32x4*>(src + min(o8, m - 8));
            } else {
                uint32_t h[8];
#pragma unroll
                for (int t = 0; t < 8; ++t) h[t] = src[min(o8 + t, m - 1)];
                Bf[bt] = lb_u32x4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
            }
        }
    };

    int c = ks * cpw + wv;
    if (c < c_end) load(c);
    for (; c < c_end; c += 4) {  // (c is wave-uniform)
        const int oc0 = c * 32;
        // codebooks of the chunk's 32 features into the wave's LDS slice: lane -> row l >> 1, half l & 1 of its V entries
        const bool live = oc0 + rr < m;
#pragma unroll
        for (int e = 0; e < VW; ++e) {
            mb[rr * LS + hh * (V / 2) + 2 * e] = live ? (lw[e] & 0xffffu) : 0u;
            mb[rr * LS + hh * (V / 2) + 2 * e + 1] = live ? (lw[e] >> 16) : 0u;
        }
        uint32_t wc[8][BITS];
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
            for (int b = 0; b < BITS; ++b) wc[t][b] = w[t][b];
        lb_u32x4 Bc[BT];
#pragma unroll
        for (int bt = 0; bt < BT; ++bt) Bc[bt] = Bf[bt];
        load(min(c + 4, c_end - 1));  // (the last iteration re-loads its own chunk: no branch around the prefetch)
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        uint32_t a[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int ol = 8 * q + t;
            uint32_t wt[BITS];
#pragma unroll
            for (int b = 0; b < BITS; ++b) wt[b] = wc[t][b];
            const uint32_t v0 = mb[ol * LS + extract<BITS>(wt, jj)];
            const uint32_t v1 = mb[ol * LS + extract<BITS>(wt, jj + 16)];
            a[0][t >> 1] |= v0 << (16 * (t & 1));
            a[1][t >> 1] |= v1 << (16 * (t & 1));
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const lb_u32x4 A0 = lb_u32x4{a[0][0], a[0][1], a[0][2], a[0][3]};
        const lb_u32x4 A1 = lb_u32x4{a[1][0], a[1][1], a[1][2], a[1][3]};
        if (oc0 + 32 > m) {  // the layer's last chunk: zero dy at the features past m (the decoded weights there are 0 already,
                             // but 0 * inf would not be)
            const int o8 = oc0 + 8 * q;
#pragma unroll
            for (int bt = 0; bt < BT; ++bt)
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    uint32_t v = Bc[bt][d];
                    if (o8 + 2 * d >= m) v &= 0xffff0000u;
                    if (o8 + 2 * d + 1 >= m) v &= 0x0000ffffu;
                    Bc[bt][d] = v;
                }
        }
#pragma unroll
        for (int bt = 0; bt < BT; ++bt) {
            const lb_u32x4 B = Bc[bt];
            if constexpr (BF16) {
                acc[0][bt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(lb_bf16x8, A0), __builtin_bit_cast(lb_bf16x8, B), acc[0][bt], 0, 0, 0);
                acc[1][bt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(lb_bf16x8, A1), __builtin_bit_cast(lb_bf16x8, B), acc[1][bt], 0, 0, 0);
            } else {
                acc[0][bt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(lb_f16x8, A0), __builtin_bit_cast(lb_f16x8, B), acc[0][bt], 0, 0, 0);
                acc[1][bt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(lb_f16x8, A1), __builtin_bit_cast(lb_f16x8, B), acc[1][bt], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int b = 0; b < BT; ++b) red[wv][t][b][lane] = acc[t][b];
    __syncthreads();
    // D[j][b]: lane l holds j = 32 g + 16 t + 4 (l >> 4) + r, b = 16 bt + (l & 15)
    for (int e = tid; e < 2 * BT * 64; e += 256) {
        const int l = e & 63, tb = e >> 6, t = tb / BT, bt = tb - t * BT;
        const int b = bt * 16 + (l & 15);
        if (b >= M) continue;
        const lb_f32x4 s = ((red[0][t][bt][l] + red[1][t][bt][l]) + red[2][t][bt][l]) + red[3][t][bt][l];
        const int j = 32 * g + 16 * t + 4 * (l >> 4);
        if (KS > 1) {
            *reinterpret_cast<lb_f32x4*>(part + ((int64_t)ks * M + b) * n + j) = s;
        } else {
            float v[4] = {s[0], s[1], s[2], s[3]};
            if (addend) {
                const lb_f32x4 ad = *reinterpret_cast<const lb_f32x4*>(addend + (int64_t)b * n + j);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += ad[r];
            }
            uint2 pk;
            pk.x = (uint32_t)lb_round(v[0], BF16) | ((uint32_t)lb_round(v[1], BF16) << 16);
            pk.y = (uint32_t)lb_round(v[2], BF16) | ((uint32_t)lb_round(v[3], BF16) << 16);
            *reinterpret_cast<uint2*>(dx + (int64_t)b * n + j) = pk;
        }
    }
}

// dx [M][n] = round(sum over ks in order of part [ks][M][n] (+ addend))
template <bool BF16>
__global__ __launch_bounds__(256) void lut_bwd_input_sum_kernel(const float* __restrict__ part, const float* __restrict__ addend, int64_t Mn,
                                                                int KS, uint16_t* __restrict__ dx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= Mn) return;
    float s = part[i];
    for (int k = 1; k < KS; ++k) s += part[(int64_t)k * Mn + i];
    if (addend) s += addend[i];
    dx[i] = lb_round(s, BF16);
}

// dlut [m][V] (+)= sum over the 256-column tiles in order of bpart [tiles][m][V]
__global__ __launch_bounds__(256) void lut_bwd_lut_sum_kernel(const float* __restrict__ bpart, int64_t mV, int tiles, int accumulate,
                                                              float* __restrict__ dlut) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= mV) return;
    float s = bpart[i];
    for (int t = 1; t < tiles; ++t) s += bpart[(int64_t)t * mV + i];
    dlut[i] = accumulate ? dlut[i] + s : s;
}

struct BwdInputPlan {
    bool dense;
    int64_t mp, rows;  // dense: padded K, rows of dy per GEMM launch
    bool pad;          // dense: dy goes through a zero-padded copy
    int cpw, KS;       // direct: chunks of 32 features per workgroup, splits of o
    size_t wt_bytes, pad_bytes, part_bytes;
};

// host-only: depends on the arguments alone (no device query, no option), so the size query and the call agree on any device
BwdInputPlan bwd_input_plan(int64_t M, int64_t m, int64_t n) {
    BwdInputPlan p{};
    p.dense = M > LB_SMALL_M;
    if (p.dense) {
        p.mp = (m + 63) / 64 * 64;
        p.rows = std::min<int64_t>(M, std::max<int64_t>(1, (int64_t)(((1ll << 32) - 1) / (2 * p.mp))));
        p.pad = (m & 63) != 0;
        p.wt_bytes = align_up((size_t)n * (size_t)p.mp * 2, 256);
        p.pad_bytes = p.pad ? align_up((size_t)p.rows * (size_t)p.mp * 2, 256) : 0;
        return p;
    }
    const int64_t groups = n / 32, nch = (m + 31) / 32;
    // split o until the launch has ~LB_TARGET_WGS workgroups, keeping at least one chunk per wave (4 per workgroup)
    int64_t ks = std::max<int64_t>(1, std::min<int64_t>((LB_TARGET_WGS + groups - 1) / groups, nch / 4));
    p.cpw = (int)((nch + ks - 1) / ks);
    p.KS = (int)((nch + p.cpw - 1) / p.cpw);
    p.part_bytes = p.KS > 1 ? align_up((size_t)p.KS * (size_t)M * (size_t)n * 4, 256) : 0;
    return p;
}

struct BwdLutPlan {
    int64_t mp, chunk;  // tokens padded to 64; tokens per launch
    int tiles;          // 256-column tiles of the GEMM
    size_t dyt_bytes, xt_bytes, part_bytes;
};

BwdLutPlan bwd_lut_plan(int64_t M, int64_t m, int64_t n, int bits) {
    BwdLutPlan p{};
    p.mp = (M + 63) / 64 * 64;
    const int64_t cap = (int64_t)(((1ll << 32) - 1) / (2 * std::max(m, n))) / 64 * 64;  // 32-bit operand offsets of the GEMM
    p.chunk = std::max<int64_t>(64, std::min(p.mp, cap));
    p.tiles = (int)((n + 255) / 256);
    p.dyt_bytes = align_up((size_t)m * (size_t)p.chunk * 2, 256);
    p.xt_bytes = align_up((size_t)n * (size_t)p.chunk * 2, 256);
    p.part_bytes = align_up((size_t)p.tiles * (size_t)m * ((size_t)1 << bits) * 4, 256);
    return p;
}

int check_bwd_args(const char* who, int dtype, int64_t M, int64_t m, int64_t n, int bits) {
    if (M < 0 || m < 0 || n < 0) return fail(-1, "%s: negative shape", who);
    if (dtype != 0 && dtype != 1) return fail(-2, "%s: dtype %d (0 = fp16, 1 = bf16)", who, dtype);
    if (bits != 2 && bits != 3 && bits != 4) return fail(-2, "%s: bits=%d not supported (2, 3, 4 are)", who, bits);
    if (n % 32 != 0) return fail(-2, "%s: in_features=%lld must be a multiple of 32", who, (long long)n);
    if (m > INT32_MAX / 2 || n > INT32_MAX / 2 || M >= (1ll << 30)) return fail(-1, "%s: shape too large", who);
    return 0;
}

template <int BITS, int BT, bool VEC>
void launch_small_v(const uint16_t* dy, const uint32_t* qw, const uint16_t* lut, const float* addend, int dtype, int M, int m, int n,
                    const BwdInputPlan& p, float* part, uint16_t* dx, hipStream_t stream) {
    const dim3 grid((unsigned)(n / 32), (unsigned)p.KS);
    if (dtype == 1)
        hipLaunchKernelGGL((lut_bwd_input_small_kernel<BITS, BT, true, VEC>), grid, dim3(256), 0, stream, dy, qw, lut, addend, M, m, n, p.cpw,
                           p.KS, part, dx);
    else
        hipLaunchKernelGGL((lut_bwd_input_small_kernel<BITS, BT, false, VEC>), grid, dim3(256), 0, stream, dy, qw, lut, addend, M, m, n, p.cpw,
                           p.KS, part, dx);
}

template <int BITS, int BT>
void launch_small(const uint16_t* dy, const uint32_t* qw, const uint16_t* lut, const float* addend, int dtype, int M, int m, int n,
                  const BwdInputPlan& p, int vec, float* part, uint16_t* dx, hipStream_t stream) {
    if (vec) launch_small_v<BITS, BT, true>(dy, qw, lut, addend, dtype, M, m, n, p, part, dx, stream);
    else launch_small_v<BITS, BT, false>(dy, qw, lut, addend, dtype, M, m, n, p, part, dx, stream);
}

template <int BITS>
void launch_small_bt(const uint16_t* dy, const uint32_t* qw, const uint16_t* lut, const float* addend, int dtype, int M, int m, int n,
                     const BwdInputPlan& p, int vec, float* part, uint16_t* dx, hipStream_t stream) {
    if (M <= 16) launch_small<BITS, 1>(dy, qw, lut, addend, dtype, M, m, n, p, vec, part, dx, stream);
    else if (M <= 32) launch_small<BITS, 2>(dy, qw, lut, addend, dtype, M, m, n, p, vec, part, dx, stream);
    else launch_small<BITS, 4>(dy, qw, lut, addend, dtype, M, m, n, p, vec, part, dx, stream);
}

}  // namespace

}  // namespace ganq

using namespace ganq;

extern "C" size_t ganq_lut_linear_bwd_input_workspace_bytes(int64_t M, int64_t m, int64_t n, int bits) {
    if (M <= 0 || m <= 0 || n < 32 || (bits != 2 && bits != 3 && bits != 4)) return 0;
    const BwdInputPlan p = bwd_input_plan(M, m, n);
    return p.dense ? p.wt_bytes + p.pad_bytes : p.part_bytes;
}

extern "C" int ganq_lut_linear_bwd_input(const void* dy, const int32_t* qweight, const void* lut, const float* addend, int dtype, int64_t M,
                                         int64_t m, int64_t n, int bits, void* dx, void* workspace, size_t workspace_bytes, void* stream_) {
    const char* who = "ganq_lut_linear_bwd_input";
    int rc = check_bwd_args(who, dtype, M, m, n, bits);
    if (rc) return rc;
    if (M == 0 || n == 0) return 0;
    if (!dx) return fail(-3, "%s: null dx", who);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (m == 0) {  // an empty sum: dx = addend (or 0), rounded
        if (!addend) {
            GANQ_HIP_CHECK(hipMemsetAsync(dx, 0, (size_t)M * (size_t)n * 2, stream));
            return 0;
        }
        const int64_t Mn = M * n;
        if (dtype == 1) hipLaunchKernelGGL((lut_bwd_input_sum_kernel<true>), dim3((unsigned)((Mn + 255) / 256)), dim3(256), 0, stream, addend, nullptr, Mn, 1, static_cast<uint16_t*>(dx));
        else hipLaunchKernelGGL((lut_bwd_input_sum_kernel<false>), dim3((unsigned)((Mn + 255) / 256)), dim3(256), 0, stream, addend, nullptr, Mn, 1, static_cast<uint16_t*>(dx));
        GANQ_LAUNCH_CHECK();
        return 0;
    }
    if (!dy || !qweight || !lut) return fail(-3, "%s: null pointer", who);
    if ((reinterpret_cast<uintptr_t>(dx) & 7) != 0) return fail(-2, "%s: dx must be 8-byte aligned", who);
    if ((reinterpret_cast<uintptr_t>(lut) & 3) != 0) return fail(-2, "%s: lut must be 4-byte aligned", who);
    if (addend && (reinterpret_cast<uintptr_t>(addend) & 15) != 0) return fail(-2, "%s: addend must be 16-byte aligned", who);
    const BwdInputPlan p = bwd_input_plan(M, m, n);
    const size_t need = p.dense ? p.wt_bytes + p.pad_bytes : p.part_bytes;
    if (need && (!workspace || workspace_bytes < need)) return fail(-4, "%s: workspace %zu B < required %zu B", who, workspace_bytes, need);
    if (p.dense) {  // (every check before the first launch)
        if (!p.pad && (reinterpret_cast<uintptr_t>(dy) & 15) != 0) return fail(-2, "%s: dy must be 16-byte aligned", who);
        if (!gemm_h16_supported(p.rows, n, p.mp))
            return fail(-1, "%s: shape %lld x %lld x %lld too large", who, (long long)M, (long long)m, (long long)n);
    }
    const uint32_t* qw = reinterpret_cast<const uint32_t*>(qweight);
    const uint16_t* lp = static_cast<const uint16_t*>(lut);
    const uint16_t* dyp = static_cast<const uint16_t*>(dy);
    uint16_t* dxp = static_cast<uint16_t*>(dx);
    ProfScope prof(KID_LUT_BWD_INPUT, stream);
    if (!p.dense) {
        const int vec = ((m & 7) == 0 && (reinterpret_cast<uintptr_t>(dy) & 15) == 0) ? 1 : 0;
        float* part = static_cast<float*>(workspace);
        if (bits == 2) launch_small_bt<2>(dyp, qw, lp, addend, dtype, (int)M, (int)m, (int)n, p, vec, part, dxp, stream);
        else if (bits == 3) launch_small_bt<3>(dyp, qw, lp, addend, dtype, (int)M, (int)m, (int)n, p, vec, part, dxp, stream);
        else launch_small_bt<4>(dyp, qw, lp, addend, dtype, (int)M, (int)m, (int)n, p, vec, part, dxp, stream);
        GANQ_LAUNCH_CHECK();
        if (p.KS > 1) {
            const int64_t Mn = M * n;
            const dim3 grid((unsigned)((Mn + 255) / 256));
            if (dtype == 1) hipLaunchKernelGGL((lut_bwd_input_sum_kernel<true>), grid, dim3(256), 0, stream, part, addend, Mn, p.KS, dxp);
            else hipLaunchKernelGGL((lut_bwd_input_sum_kernel<false>), grid, dim3(256), 0, stream, part, addend, Mn, p.KS, dxp);
            GANQ_LAUNCH_CHECK();
        }
        return 0;
    }
    uint16_t* Wt = static_cast<uint16_t*>(workspace);
    uint16_t* dyp_pad = reinterpret_cast<uint16_t*>(static_cast<char*>(workspace) + p.wt_bytes);
    {
        const int gx = (int)(p.mp / 64), ngroups = (int)(n / 32);
        const int gy = std::max(1, std::min((ngroups + 3) / 4, std::max(1, 2048 / gx)));
        const dim3 grid((unsigned)gx, (unsigned)gy);
        if (bits == 2) hipLaunchKernelGGL(lut_dequant_t_kernel<2>, grid, dim3(256), 0, stream, qw, lp, (int)m, (int)n, (int)p.mp, Wt);
        else if (bits == 3) hipLaunchKernelGGL(lut_dequant_t_kernel<3>, grid, dim3(256), 0, stream, qw, lp, (int)m, (int)n, (int)p.mp, Wt);
        else hipLaunchKernelGGL(lut_dequant_t_kernel<4>, grid, dim3(256), 0, stream, qw, lp, (int)m, (int)n, (int)p.mp, Wt);
        GANQ_LAUNCH_CHECK();
    }
    for (int64_t r0 = 0; r0 < M; r0 += p.rows) {
        const int64_t rows = std::min(p.rows, M - r0);
        const uint16_t* a = dyp + r0 * m;
        if (p.pad) {
            const int64_t tot = rows * p.mp;
            hipLaunchKernelGGL(lb_pad_cols_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, a, rows, (int)m, (int)p.mp, dyp_pad);
            GANQ_LAUNCH_CHECK();
            a = dyp_pad;
        }
        rc = gemm_h16(a, Wt, nullptr, addend ? addend + r0 * n : nullptr, dtype, rows, n, p.mp, dxp + r0 * n, stream);
        if (rc) return rc;
    }
    return 0;
}

extern "C" size_t ganq_lut_linear_bwd_lut_workspace_bytes(int64_t M, int64_t m, int64_t n, int bits) {
    if (M <= 0 || m <= 0 || n < 32 || (bits != 2 && bits != 3 && bits != 4)) return 0;
    const BwdLutPlan p = bwd_lut_plan(M, m, n, bits);
    return p.dyt_bytes + p.xt_bytes + p.part_bytes;
}

extern "C" int ganq_lut_linear_bwd_lut(const void* dy, const void* x, const int32_t* qweight, int dtype, int64_t M, int64_t m, int64_t n,
                                       int bits, float* dlut, void* workspace, size_t workspace_bytes, void* stream_) {
    const char* who = "ganq_lut_linear_bwd_lut";
    int rc = check_bwd_args(who, dtype, M, m, n, bits);
    if (rc) return rc;
    if (m == 0) return 0;
    if (!dlut) return fail(-3, "%s: null dlut", who);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int V = 1 << bits;
    if (M == 0 || n == 0) {  // an empty sum
        GANQ_HIP_CHECK(hipMemsetAsync(dlut, 0, (size_t)m * V * sizeof(float), stream));
        return 0;
    }
    if (!dy || !x || !qweight) return fail(-3, "%s: null pointer", who);
    const BwdLutPlan p = bwd_lut_plan(M, m, n, bits);
    const size_t need = p.dyt_bytes + p.xt_bytes + p.part_bytes;
    if (!workspace || workspace_bytes < need) return fail(-4, "%s: workspace %zu B < required %zu B", who, workspace_bytes, need);
    if (!gemm_h16_supported(m, n, p.chunk)) return fail(-1, "%s: shape %lld x %lld too large", who, (long long)m, (long long)n);
    uint16_t* dyt = static_cast<uint16_t*>(workspace);
    uint16_t* xt = reinterpret_cast<uint16_t*>(static_cast<char*>(workspace) + p.dyt_bytes);
    float* bpart = reinterpret_cast<float*>(static_cast<char*>(workspace) + p.dyt_bytes + p.xt_bytes);
    const uint16_t* dyp = static_cast<const uint16_t*>(dy);
    const uint16_t* xp = static_cast<const uint16_t*>(x);
    const uint32_t* qw = reinterpret_cast<const uint32_t*>(qweight);
    ProfScope prof(KID_LUT_BWD_LUT, stream);
    for (int64_t t0 = 0; t0 < M; t0 += p.chunk) {
        const int64_t rows = std::min(p.chunk, M - t0), kp = (rows + 63) / 64 * 64;
        hipLaunchKernelGGL(lb_stage_t_kernel, dim3((unsigned)((m + 63) / 64), (unsigned)(kp / 64)), dim3(256), 0, stream, dyp + t0 * m, rows, (int)m,
                           kp, dyt);
        hipLaunchKernelGGL(lb_stage_t_kernel, dim3((unsigned)((n + 63) / 64), (unsigned)(kp / 64)), dim3(256), 0, stream, xp + t0 * n, rows, (int)n,
                           kp, xt);
        GANQ_LAUNCH_CHECK();
        rc = gemm_h16_buckets(dyt, xt, qw, bits, dtype, m, n, kp, bpart, stream);
        if (rc) return rc;
        const int64_t mV = m * V;
        hipLaunchKernelGGL(lut_bwd_lut_sum_kernel, dim3((unsigned)((mV + 255) / 256)), dim3(256), 0, stream, bpart, mV, p.tiles, t0 > 0 ? 1 : 0,
                           dlut);
        GANQ_LAUNCH_CHECK();
    }
    return 0;
}
