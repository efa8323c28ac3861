// T-update: closed-form codebook update of GANQ (reference ganq.py:570-591, CPU/gelsd branch)
//     A_i = S_i H S_i^T,  b_i = S_i (W H)_i^T,  T_i = minimum-norm lstsq(A_i, b_i)
// and, from the same quantities, the loss of ganq.py:392-395 / :621-622
//     dist = sum_i (w_i - S_i^T t_i)^T H (w_i - S_i^T t_i) = sum_i ( w_i^T H w_i - 2 t_i^T b_i + t_i^T A_i t_i )
// without ever materialising the one-hot tensor S [m,V,n] (1 GiB at 4096^2, ganq.py:505).
//
// A_i[a][b] = sum_{u,v} [Q_iu == a][Q_iv == b] H[u,v] is a bucket sum of ALL of H per row: m*n^2 additions.
// It runs on the integer matrix cores, exactly:
//   * once per layer H is converted to fixed point, H ~= scale * (I + J / 65536) with scale = max|H| / 2^30: I is a
//     31-bit integer split into 4 balanced base-256 digits (int8 planes 0..3 of Hq[p][v][u]); J is a 16-bit
//     EXTENSION word (2 more digits, planes 4..5) that exists only when the dynamic range of H needs it -- decided on
//     the device, max|H| > 16 mean(diag H): with massive-activation features (H_ii 10^4..10^6 x the typical one) a
//     31-bit word leaves the typical entry 10-17 significant bits, against the 24 of the fp32 entries the reference
//     sums (ganq.py:589-591); 47 bits keep every entry of a matrix spanning 2^23 to full fp32 precision.  The bucket
//     sums of I and J are kept as two exact int64 words and meet in fp64 in the per-row solve (t_prepare);
//   * per iteration the indices become bit masks bits[row][u/64][code] (one ballot per code);
//   * v_mfma_i32_16x16x64_i8 multiplies the one-hot matrix [16 codes x 64 u] (expanded from 16 mask bits per lane
//     with one integer multiply per 4 bytes) with a digit tile [64 u x 16 v]: int32 accumulators hold
//     Y_p[a][v] = sum_{u in a, u > v} digit_p(H[v][u]).  Integer sums are exact and order-independent, so the
//     result is deterministic whatever the scheduling;
//   * the v index is bucketed with 64-bit LDS atomics (digits recombined to one int64 first), again exact;
//   * H symmetric: only u > v is visited, A = M + M^T + diag.
// The per-row 16x16 systems are then solved in fp64 (round-robin Jacobi, gelsd cut-off); with A exact and
// b = S (W H) accumulated in fp64 the closed-form loss has no cancellation problem, so no (W-Wq)@H product is
// needed per iteration.
#include <climits>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "common.h"
#include "mfma_h16.h"
#include "update_t.h"
#include "wh_gemm.h"

namespace ganq {

// tile shape of onehot_accum_kernel (overridable for experiments).  Measured on MI355X, 4096x4096: (waves, u per tile) =
// (8, 256) 2.25 ms, (8, 128) 2.31, (4, 256) 3.44, (4, 128) 3.43 -- two smaller workgroups per CU lose more to the halved
// reuse of each staged digit tile than they gain from overlapping each other's barriers
#ifndef ACC_TW
#define ACC_TW 8
#endif
// ACC_VH = 32-column halves per chunk.  2: every expanded one-hot fragment (the kernel's vector work: 14 instructions per
// fragment) serves 8 MFMAs instead of 4 -- two rows per wave instead of four keep the accumulators at 128 registers, and
// 128-wide u tiles keep the two staged digit tiles of 64 columns inside the LDS.  Measured on MI355X, 4096x4096: 2.58 ms
// against 2.22 ms for the default (half the rows per workgroup stream every digit tile twice as often): the fragment
// expansion is not what bounds the kernel.
#ifndef ACC_VH
#define ACC_VH 1
#endif
#ifndef ACC_UT
#define ACC_UT (ACC_VH == 2 ? 128 : 256)
#endif
// ACC_PIN_B = 1 keeps the LDS reads of the next 32-column half in front of this half's matrix instructions (a scheduling barrier:
// the B fragments are then really double-buffered instead of re-using their registers right before use).  Measured: 2.14 vs 2.08 ms.
#ifndef ACC_PIN_B
#define ACC_PIN_B 0
#endif
constexpr int TW = ACC_TW;      // waves per workgroup
constexpr int VH = ACC_VH;
constexpr int RW = VH == 2 ? 2 : 4;  // rows per wave
constexpr int TR = TW * RW;     // rows of W per workgroup
constexpr int VCH = 32 * VH;    // v columns per chunk (32 per MFMA column tile)
constexpr int UT = ACC_UT;      // u per staged tile (UT / 64 MFMA steps of 64)
constexpr int KS64 = UT / 64;
static_assert(KS64 >= 2, "the code masks are requested KS64 - 1 steps ahead");
constexpr int UC16 = UT / 16;   // 16-byte pieces per tile row
constexpr int NP = 8;           // chunk c belongs to part c % NP; every part writes one partial A
constexpr int BROW = UT + 16;   // LDS row pitch of a digit tile in bytes (pad against bank conflicts)
constexpr int btile_bytes(int npl) { return npl * VCH * BROW; }

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

struct TPrep {              // device-side header written by t_prepare
    double scale;           // H ~= scale * (I + J / 65536)
    unsigned int absmax_bits;
    int ext;                // 1: the 16-bit extension word J is in use (planes 4..5, Jint, the *_lo bucket sums)
    // entries with u > v whose digit 3 / whose digit 2 or 3 is not zero (always exact), and how many of them a list may hold to be
    // used instead of the dense planes (< 0: never; the lists hold the first top_cap entries counted)
    unsigned int c3, c2;
    int top_cap;
    int mu_index;           // the D top_index_kernel built the per-column index for (0: it did not run; 4: nothing to index)
};
// capacity of either exception list (entries of 8 bytes): above it a plane is summed on the matrix cores whatever the cap asks for
constexpr int TOP_LIST_MAX = 131072;
// how many digit planes of the 31-bit word the four-wave kernel sums densely; the entries above them come from a list
__host__ __device__ inline int top_dense_planes(long long c3, long long c2, long long cap) {
    if (cap < 0) return 4;
    if (c2 <= cap) return 2;
    return c3 <= cap ? 3 : 4;
}
// ... and how many m_update_mfma_kernel reads (mu_top = GANQ_MU_TOP): the same ones; 0: all four; 3 (A/B): the same ones but never
// fewer than three.  Where the full sum takes two planes, c3 <= c2 <= cap: the list of the entries above digit 2 is complete as well.
__host__ __device__ inline int mu_dense_planes(long long c3, long long c2, long long cap, int mu_top) {
    if (mu_top == 0) return 4;
    const int d = top_dense_planes(c3, c2, cap);
    return d == 2 && mu_top == 3 ? 3 : d;
}
// the value of the D lowest balanced base-256 digits of a 31-bit word x (hquant_kernel's digits): the residue of x modulo 256^D in
// [-B, 256^D - 1 - B], B = 0x80 in each of the D bytes
__host__ __device__ inline long long low_digits(long long x, int D) {
    if (D >= 4) return x;
    const long long B = D == 3 ? 0x808080ll : 0x8080ll;
    return ((x + B) & ((1ll << (8 * D)) - 1)) - B;
}
constexpr double EXT_UNIT = 1.0 / 65536.0;
// two balanced base-256 digits hold J in [-32896, 32639]: the int16 copy stores J + JBIAS, which is exactly [-32768, 32767]
constexpr int JBIAS = 128;

// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ H, int64_t total, TPrep* __restrict__ prep) {
    __shared__ unsigned int wmax[4];
    unsigned int mx = 0;
    const int64_t n4 = (reinterpret_cast<uintptr_t>(H) & 15) == 0 ? (total >> 2) : 0;  // 16-byte loads when aligned
    const uint4* H4 = reinterpret_cast<const uint4*>(H);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const uint4 v = H4[i];  // |x| bits order like the values
        mx = max(max(mx, v.x & 0x7fffffffu), max(max(v.y & 0x7fffffffu, v.z & 0x7fffffffu), v.w & 0x7fffffffu));
    }
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
        mx = max(mx, __builtin_bit_cast(unsigned int, H[i]) & 0x7fffffffu);
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, (unsigned int)__shfl_xor((int)mx, off));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
    __syncthreads();
    // one atomic per workgroup: thousands of same-address atomics were most of this kernel's time
    if (threadIdx.x == 0) atomicMax(&prep->absmax_bits, max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3])));
}

// scale = max|H| / 2^30; the extension word is switched on when the matrix has more dynamic range than one 31-bit
// word serves: a bucket sum A[a][a] is about (n / V) mean(diag H), its rounding error about (n / V) 0.29 scale, so with
// max|H| <= 16 mean(diag H) one word keeps A to 4e-9 relative -- beyond that the second word takes over.
// ext_mode: -1 decide here, 0 never, 1 always (developer switch GANQ_H_EXT).  top_cap: see TPrep (top_cap_in_force).
__global__ __launch_bounds__(256) void prep_scale_kernel(const float* __restrict__ H, int n, TPrep* prep, int ext_mode, int top_cap) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int u = threadIdx.x; u < n; u += 256) s += (double)H[(int64_t)u * n + u];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float mx = __builtin_bit_cast(float, prep->absmax_bits);
        const bool ok = mx > 0.0f && mx < __builtin_inff();
        prep->scale = ok ? (double)mx / 1073741824.0 : 0.0;
        const double mean_diag = sh[0] / (double)n;
        const bool wide = ok && !((double)mx <= 16.0 * mean_diag);  // also for a non-positive / NaN mean
        prep->ext = ext_mode < 0 ? (wide ? 1 : 0) : (ext_mode ? 1 : 0);
        prep->top_cap = top_cap;
    }
}

// planes[p][v][u] (row pitch nq, zero padded; p = 0..3 digits of I, p = 4..5 digits of J), hdiag_int[u] / hdiag_j[u],
// optionally H64[v][u] = scale * (I + J / 65536), Hint = I (int32), Jint = J (int16).
// The entries with u > v (the bytes the full sum reads) whose top digits are not zero are counted in prep->c3 / c2 and, while a list
// has room (prep->top_cap), appended to it as (u | v << 16, value): top3 holds d3, top2 holds d2 + 256 d3.  A workgroup quantises
// `tiles` runs of 1024 entries and collects its list entries in LDS: one atomic on a counter per HQ_BUF / 2 entries or more, and none
// but a last one once a list is known to overflow (thousands of same-address atomics are what absmax and q_diff had to get rid of).
constexpr int HQ_BUF = 2048;  // entries per list a workgroup holds back; a tile adds at most 1024
__global__ __launch_bounds__(256) void hquant_kernel(const float* __restrict__ H, int n, int nq, TPrep* __restrict__ prep,
                                                    int8_t* __restrict__ planes, int* __restrict__ hdiag_int,
                                                    int* __restrict__ hdiag_j, double* __restrict__ H64,
                                                    int* __restrict__ Hint, short* __restrict__ Jint, uint2* __restrict__ top3,
                                                    uint2* __restrict__ top2, int tiles) {
    __shared__ uint2 buf[2][HQ_BUF];
    __shared__ unsigned int fill[2], base_sh[2], late[2];
    const int tid = threadIdx.x;
    if (tid < 2) fill[tid] = late[tid] = 0;
    __syncthreads();
    const int64_t per_row = nq;
    const int64_t total = (int64_t)n * per_row;
    const double scale = prep->scale;
    const bool ext = prep->ext != 0;
    const int cap = prep->top_cap;
    const double inv = scale > 0.0 ? 1.0 / scale : 0.0;
    bool full[2] = {cap < 0, cap < 0};  // (uniform) nothing more is stored in this list: it overflows, or no list is wanted
    unsigned int mine[2] = {0, 0};      // counted, not stored
    // everybody, behind a barrier: the f entries held back go to their place in the list, as far as it has room
    auto flush = [&](int l, unsigned int f) {
        if (tid == 0) base_sh[l] = atomicAdd(l ? &prep->c2 : &prep->c3, f);
        __syncthreads();
        const unsigned int base = base_sh[l];
        uint2* list = l ? top2 : top3;
        for (unsigned int i = tid; i < f; i += 256)
            if (base + i < (unsigned int)cap) list[base + i] = buf[l][i];
        if (base + f > (unsigned int)cap) full[l] = true;
        __syncthreads();
        if (tid == 0) fill[l] = 0;
        __syncthreads();
    };
    for (int t = 0; t < tiles; ++t) {
        const int64_t tile0 = ((int64_t)blockIdx.x * tiles + t) * 1024;
        if (tile0 >= total) break;
        const int64_t i4 = tile0 + 4 * tid;  // 4 consecutive u of one row v
        uint32_t euv[4] = {0, 0, 0, 0};
        int ev[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        if (i4 < total) {
            const int v = (int)(i4 / per_row), u0 = (int)(i4 % per_row);
            uint32_t pk[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int u = u0 + k;
                int xi = 0, xj = 0;
                if (u < n) {
                    const double x = fmin(fmax((double)H[(int64_t)v * n + u] * inv, -1073741824.0), 1073741824.0);
                    xi = (int)__builtin_rint(x);
                    if (ext) {
                        // remainder in units of 2^-16: two balanced base-256 digits hold [-32896, 32639]
                        xj = (int)__builtin_rint((x - (double)xi) * 65536.0);
                        if (xj > 32639) {
                            xi += 1;
                            xj -= 65536;
                        }
                    }
                    if (H64) H64[(int64_t)v * n + u] = scale * ((double)xi + (double)xj * EXT_UNIT);
                    if (Hint) Hint[(int64_t)v * n + u] = xi;
                    if (Jint) Jint[(int64_t)v * n + u] = (short)(xj + JBIAS);
                    if (u == v) {
                        hdiag_int[u] = xi;
                        hdiag_j[u] = xj;
                    }
                }
                int r = xi;
                int dg[4];
#pragma unroll
                for (int p = 0; p < 4; ++p) {  // balanced base-256 digits: r = d + 256 * r', d in [-128, 127]
                    const int d = ((r + 128) & 255) - 128;
                    r = (r - d) >> 8;
                    pk[p] |= (uint32_t)(d & 255) << (8 * k);
                    dg[p] = d;
                }
                if (u < n && u > v) {
                    euv[k] = (uint32_t)u | ((uint32_t)v << 16);
                    ev[0][k] = dg[3];
                    ev[1][k] = dg[2] + 256 * dg[3];  // zero only when both digits are
                }
                r = xj;
#pragma unroll
                for (int p = 4; p < 6; ++p) {
                    const int d = ((r + 128) & 255) - 128;
                    r = (r - d) >> 8;
                    pk[p] |= (uint32_t)(d & 255) << (8 * k);
                }
            }
#pragma unroll
            for (int p = 0; p < 6; ++p)
                if (p < 4 || ext) *reinterpret_cast<uint32_t*>(planes + ((int64_t)p * n + v) * nq + u0) = pk[p];
        }
#pragma unroll
        for (int l = 0; l < 2; ++l) {
            unsigned int cnt = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) cnt += ev[l][k] != 0;
            if (full[l]) mine[l] += cnt;
            else if (cnt) {
                unsigned int s = atomicAdd(&fill[l], cnt);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (ev[l][k] != 0) buf[l][s++] = make_uint2(euv[k], (uint32_t)ev[l][k]);
            }
        }
        if (full[0] && full[1]) continue;
        __syncthreads();
        const unsigned int f0 = fill[0], f1 = fill[1];
        __syncthreads();  // (nobody adds to this tile's fill counts before everybody has read them)
        if (!full[0] && f0 > HQ_BUF - 1024) flush(0, f0);
        if (!full[1] && f1 > HQ_BUF - 1024) flush(1, f1);
    }
    __syncthreads();
#pragma unroll
    for (int l = 0; l < 2; ++l) {
        const unsigned int f = fill[l];  // (uniform: behind a barrier, and flush ends with one)
        if (!full[l] && f) flush(l, f);
        unsigned int c = mine[l];
        for (int off = 32; off > 0; off >>= 1) c += (unsigned int)__shfl_xor((int)c, off);
        if ((tid & 63) == 0 && c) atomicAdd(&late[l], c);
    }
    __syncthreads();
    if (tid < 2 && late[tid]) atomicAdd(tid ? &prep->c2 : &prep->c3, late[tid]);
}

// per-feature exponents for the W @ H product: e[u] = floor(log2(H_uu) / 2), so that H~[u][v] = H[u][v] 2^(-e_u - e_v) has a
// diagonal in [1, 4) and, H being positive semi-definite, no entry above 4 (wh_gemm.hip)
__global__ __launch_bounds__(256) void dexp_kernel(const int* __restrict__ hdiag_int, const int* __restrict__ hdiag_j,
                                                  const TPrep* __restrict__ prep, int n, int* __restrict__ dexp,
                                                  double* __restrict__ hdiag64) {
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= n) return;
    const double h = prep->scale * ((double)hdiag_int[u] + (double)hdiag_j[u] * EXT_UNIT);
    hdiag64[u] = h;
    int e = 0;
    if (h > 0.0 && h < __builtin_inf()) {
        const int lg = ilogb(h);  // floor(log2 h)
        e = lg >= 0 ? lg / 2 : -((-lg + 1) / 2);  // floor(lg / 2)
    }
    dexp[u] = e;
}

// bits[(row * ng + g) * 16 + a] : bit l set  <=>  Q[row][64 g + l] == a
// `changed` (device, may be null): the full-accumulation kernels run only when *changed > thr
__global__ __launch_bounds__(256) void code_masks_kernel(const uint8_t* __restrict__ Q, int m, int n, int ng,
                                                        unsigned long long* __restrict__ bits,
                                                        const long long* __restrict__ changed, long long thr) {
    if (changed && *changed <= thr) return;
    const int lane = threadIdx.x & 63;
    // grid-stride over (row, 64-column group) items: the grid stays small, so the gated-off launches of the
    // incremental iterations cost a few microseconds instead of 15
    for (int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); item < (int64_t)m * ng; item += (int64_t)gridDim.x * 4) {
        const int row = (int)(item / ng), g = (int)(item % ng);
        const int u = 64 * g + lane;
        const uint32_t q = u < n ? Q[(int64_t)row * n + u] : 255u;
        unsigned long long mine = 0;
#pragma unroll
        for (uint32_t a = 0; a < 16; ++a) {
            const unsigned long long mk = __ballot(q == a);
            if ((uint32_t)lane == a) mine = mk;
        }
        // stored with the two middle 16-bit quarters swapped: dword kb of the word then holds, low half first, the bits of columns
        // 16 kb .. 16 kb + 15 and 32 + 16 kb .. 47 + 16 kb -- exactly what lane half kb of onehot_accum_kernel expands in the two
        // 32-column halves of a step (one 4-byte load per step instead of an 8-byte one)
        mine = (mine & 0xffff00000000ffffull) | ((mine & 0x00000000ffff0000ull) << 16) | ((mine & 0x0000ffff00000000ull) >> 16);
        if (lane < 16) bits[item * 16 + lane] = mine;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// NPL digit planes starting at plane P0: <4, 0> sums the 31-bit word I, <2, 4> the extension word J (into its own
// Mpart; that launch leaves at once when the extension is off)
template <int NPL, int P0>
__device__ __forceinline__ void onehot_accum_body(const int8_t* __restrict__ planes_all, const unsigned long long* __restrict__ bits,
                                                  const uint8_t* __restrict__ Q, int m, int n, int nq, int ng,
                                                  long long* __restrict__ Mpart, long long* __restrict__ stamps,
                                                  const TPrep* __restrict__ prep, const int bid) {
    if (P0 != 0 && prep->ext == 0) return;
    constexpr int BTILE = btile_bytes(NPL);
    const int8_t* planes = planes_all + (int64_t)P0 * n * nq;
    extern __shared__ __align__(16) char smem[];
    long long st_pro = 0, st_loop = 0, st_flush = 0, st_t0 = 0;
    char* Bbuf = smem;                                                        // 2 x BTILE
    long long(*Mrow)[RW][256] = reinterpret_cast<long long(*)[RW][256]>(smem + 2 * BTILE);  // [TW][RW][a*16+b]

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // v_mfma_i32_32x32x32_i8: A rows = (row of the pair, code), 32 u per instruction, B columns = the chunk's 32 v.
    // lane l: A row / B column i32 = l & 31, k bytes 16*(l >> 5) .. +15
    const int i32 = lane & 31, kb = lane >> 5;
    const int r2 = i32 >> 4, a16 = i32 & 15;
    const int nrg = (m + TR - 1) / TR;
    const int rg = bid % nrg, part = bid / nrg;
    const int row0 = rg * TR + wv * RW;
    int rowc[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) rowc[r] = min(row0 + r, m - 1);
    int mrow[RW / 2];  // the row whose masks this lane expands, per row pair
#pragma unroll
    for (int p = 0; p < RW / 2; ++p) mrow[p] = min(row0 + 2 * p + r2, m - 1);

    for (int i = lane; i < RW * 256; i += 64) Mrow[wv][i >> 8][i & 255] = 0;

    // staging of one digit tile: NPL planes x VCH rows x 256 B (4 planes: 2048 x 16 B, 4 per thread)
    constexpr int NE = NPL * VCH * UC16 / (TW * 64);  // 16-byte pieces of a digit tile per thread
    static_assert(NE * TW * 64 == NPL * VCH * UC16, "digit tile must split evenly over the threads");
    uint4 stage[NE];
    auto gload = [&](int v0, int t) {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int idx = e * (TW * 64) + tid;
            const int c16 = idx % UC16, vi = (idx / UC16) & (VCH - 1), p = idx / (UC16 * VCH);
            const int v = v0 + vi, ub = t * UT + 16 * c16;
            uint4 x = make_uint4(0, 0, 0, 0);
            if (v < n && ub + 15 > v && ub < nq) {
                x = *reinterpret_cast<const uint4*>(planes + ((int64_t)p * n + v) * nq + ub);
                if (ub <= v) {  // chunk crosses the diagonal: keep bytes with u > v only
                    uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        const int cnt = min(4, max(0, v - (ub + 4 * d) + 1));  // leading bytes to clear
                        w[d] = cnt >= 4 ? 0u : (w[d] & (0xffffffffu << (8 * cnt)));
                    }
                    x = make_uint4(w[0], w[1], w[2], w[3]);
                }
            }
            stage[e] = x;
        }
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int idx = e * (TW * 64) + tid;
            const int c16 = idx % UC16, vi = (idx / UC16) & (VCH - 1), p = idx / (UC16 * VCH);
            *reinterpret_cast<uint4*>(Bbuf + buf * BTILE + (p * VCH + vi) * BROW + 16 * c16) = stage[e];
        }
    };

    const int nchunk = (n + VCH - 1) / VCH;
    const int ntile = (n + UT - 1) / UT;
    // code masks of this lane's (row, code): one dword per 64-column step (see code_masks_kernel), requested KS64 - 1 steps
    // ahead of their use -- one step ahead (round 2) every step waited for its masks: a step is 16 matrix instructions, half a
    // trip to L2
    uint32_t wb[KS64][RW / 2];
    const uint32_t* bits32 = reinterpret_cast<const uint32_t*>(bits);
    auto load_masks = [&](int gi, uint32_t (&dst)[RW / 2]) {
#pragma unroll
        for (int p = 0; p < RW / 2; ++p) dst[p] = gi < ng ? bits32[(((int64_t)mrow[p] * ng + gi) * 16 + a16) * 2 + kb] : 0u;
    };
    // The first digit tile and the first masks of a chunk are requested during the LAST tile of the chunk before it (round 3:
    // a chunk used to open with a load, a store and two barriers in a row -- 7 % of the kernel by its cycle stamps); only the
    // very first chunk of a workgroup waits for them here.  (t_first grows with the chunk: the first chunk past the last tile
    // ends the loop.)
    if (part < nchunk && (part * VCH + 1) / UT < ntile) {
        gload(part * VCH, (part * VCH + 1) / UT);
#pragma unroll
        for (int i = 0; i < KS64 - 1; ++i) load_masks((part * VCH + 1) / UT * KS64 + i, wb[i]);
    }
    for (int c = part; c < nchunk; c += NP) {
        const int v0 = c * VCH;
        const int t_first = (v0 + 1) / UT;
        if (t_first >= ntile) break;
        const int v0n = (c + NP) * VCH, tfn = (v0n + 1) / UT;  // the workgroup's next chunk
        const bool has_next = c + NP < nchunk && tfn < ntile;
        v16i acc[RW / 2][VH][NPL];
#pragma unroll
        for (int p = 0; p < RW / 2; ++p)
#pragma unroll
            for (int vh = 0; vh < VH; ++vh)
#pragma unroll
                for (int d = 0; d < NPL; ++d)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[p][vh][d][r] = 0;

        st_t0 = __builtin_amdgcn_s_memtime();
        __syncthreads();  // previous chunk's last tile fully consumed
        sstore(0);
        __syncthreads();
        { const long long tt = __builtin_amdgcn_s_memtime(); st_pro += tt - st_t0; st_t0 = tt; }
        // one staged tile of UT columns u.  Only the chunk's FIRST tile can touch the diagonal (t_first = (v0 + 1) / UT, so every later
        // tile starts right of v0): its 32-column halves are tested one by one; the others run without a branch in the loop, so the
        // LDS reads of the next half stay in flight across the matrix instructions of this one
        auto tile_body = [&](auto diag_tag, int t) {
            constexpr bool DIAG = decltype(diag_tag)::value;
            const int buf = (t - t_first) & 1;
            if (t + 1 < ntile) gload(v0, t + 1);
            else if (has_next) gload(v0n, tfn);  // (filed by the next chunk's opening)
            // masks of the steps behind this tile: the next tile's, or the first ones of the next chunk
            const int gnext = t + 1 < ntile ? (t + 1) * KS64 : (has_next ? tfn * KS64 : ng);
            const char* Bt = Bbuf + buf * BTILE + i32 * BROW + 16 * kb;
            auto read_b = [&](int ks, int kh, v4i (&bf)[VH][NPL]) {
#pragma unroll
                for (int vh = 0; vh < VH; ++vh)
#pragma unroll
                    for (int d = 0; d < NPL; ++d)
                        bf[vh][d] = *reinterpret_cast<const v4i*>(Bt + (d * VCH + 32 * vh) * BROW + ks * 64 + kh * 32);
            };
            v4i bf[2][VH][NPL];
            read_b(0, 0, bf[0]);
#pragma unroll
            for (int ks = 0; ks < KS64; ++ks) {
                load_masks(ks == 0 ? t * KS64 + KS64 - 1 : gnext + ks - 1, wb[(ks + KS64 - 1) % KS64]);  // KS64 - 1 steps ahead
#pragma unroll
                for (int kh = 0; kh < 2; ++kh) {
                    const int hh = ks * 2 + kh;
                    if (hh + 1 < 2 * KS64) read_b((hh + 1) >> 1, (hh + 1) & 1, bf[(hh + 1) & 1]);  // next 32-column half
#if ACC_PIN_B
                    if (!DIAG) __builtin_amdgcn_sched_barrier(0);  // keep those reads in front of this half's matrix instructions
#endif
                    if (DIAG && t * UT + ks * 64 + kh * 32 + 31 <= v0) continue;  // entirely on or above the diagonal (uniform)
#pragma unroll
                    for (int p = 0; p < RW / 2; ++p) {
                        const uint32_t b16 = (wb[ks][p] >> (16 * kh)) & 0xffffu;
                        v4i af;
#pragma unroll
                        for (int d = 0; d < 4; ++d) af[d] = (int)((((b16 >> (4 * d)) & 0xfu) * 0x00204081u) & 0x01010101u);
#pragma unroll
                        for (int vh = 0; vh < VH; ++vh)
#pragma unroll
                            for (int d = 0; d < NPL; ++d)
                                acc[p][vh][d] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af, bf[hh & 1][vh][d], acc[p][vh][d], 0, 0, 0);
                    }
                }
            }
            if (t + 1 < ntile) sstore(buf ^ 1);
            __syncthreads();
        };
        tile_body(std::true_type{}, t_first);
        for (int t = t_first + 1; t < ntile; ++t) tile_body(std::false_type{}, t);
        { const long long tt = __builtin_amdgcn_s_memtime(); st_loop += tt - st_t0; st_t0 = tt; }
        // bucket the chunk's columns by their code: Mrow[row][a][b] += sum_d 256^d Y_d[(row, a)][v], b = Q[row][v]
        // C layout of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
        for (int vh = 0; vh < VH; ++vh) {
            const int v = v0 + 32 * vh + i32;
#pragma unroll
            for (int p = 0; p < RW / 2; ++p) {
                uint32_t bq[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) bq[h] = v < n ? Q[(int64_t)rowc[2 * p + h] * n + v] : 255u;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int i = (reg & 3) + 8 * (reg >> 2) + 4 * kb;  // (row of the pair, code)
                    const int h = i >> 4, a = i & 15;
                    long long val = 0;
#pragma unroll
                    for (int d = 0; d < NPL; ++d) val += (long long)acc[p][vh][d][reg] << (8 * d);
                    const uint32_t b = bq[h];
                    if (b < 16u && val != 0)
                        atomicAdd(reinterpret_cast<unsigned long long*>(&Mrow[wv][2 * p + h][a * 16 + b]),
                                  (unsigned long long)val);
                }
            }
        }
        { const long long tt = __builtin_amdgcn_s_memtime(); st_flush += tt - st_t0; st_t0 = tt; }
    }
    if (stamps && bid == 0 && tid == 0) { stamps[0] = st_pro; stamps[1] = st_loop; stamps[2] = st_flush; }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < RW; ++r)
        if (row0 + r < m) {
            long long* out = Mpart + ((int64_t)part * m + row0 + r) * 256;
            for (int i = lane; i < 256; i += 64) out[i] = Mrow[wv][r][i];
        }
}

// One launch for both words: the first `nblk_hi` workgroups sum the four digit planes of the 31-bit word, the others the two planes
// of the extension word into its own partial sums (they leave at once when the extension is off).  As two launches the second
// one cost a dispatch (~5 us on the device) in every iteration of the loop, also when the full accumulation is gated off.
__global__ __launch_bounds__(TW * 64) void onehot_accum_kernel(const int8_t* __restrict__ planes_all,
                                                              const unsigned long long* __restrict__ bits,
                                                              const uint8_t* __restrict__ Q, int m, int n, int nq, int ng,
                                                              long long* __restrict__ Mpart_hi, long long* __restrict__ Mpart_lo,
                                                              long long* __restrict__ stamps, const long long* __restrict__ changed,
                                                              long long thr, const TPrep* __restrict__ prep, int nblk_hi) {
    if (changed && *changed <= thr) return;
    if ((int)blockIdx.x < nblk_hi) onehot_accum_body<4, 0>(planes_all, bits, Q, m, n, nq, ng, Mpart_hi, stamps, prep, (int)blockIdx.x);
    else onehot_accum_body<2, 4>(planes_all, bits, Q, m, n, nq, ng, Mpart_lo, nullptr, prep, (int)blockIdx.x - nblk_hi);
}

// ---------------------------------------------------------------------------------------------------------------
// The full accumulation, second implementation: FOUR waves, one per SIMD, 8 rows per wave (GANQ_ACCUM_W4, accum_plan below).
// The same integers as onehot_accum_kernel from the same planes, masks and partial-sum layout; what differs is the schedule:
//   * a wave owns 4 row pairs x NPL planes = 16 accumulator tiles of 32 x 32 (256 registers with four planes), pinned to the
//     accumulation registers by asm "+a" operands (mfma_h16.h says why); a B fragment read from LDS feeds 4 matrix instructions
//     instead of 2, and the vector registers hold two real sets of B fragments: the next 32-column half is read while this
//     half's 16 matrix instructions run;
//   * the digit tiles go global -> LDS by LDS-DMA in SLICES of 128 columns u (NPL planes x 32 v x 128 B) through a ring of four
//     stages that runs across the chunks of a workgroup: slice f + 3 of the workgroup's flat (chunk, slice) sequence is requested
//     during slice f, so a chunk opens without a store or a barrier of its own.  One counted s_waitcnt vmcnt and one barrier
//     per slice: behind them slice f + 1 has landed for every wave and the stage of slice f - 1 is free;
//   * an LDS-DMA image is lane-linear and cannot be padded: the 16-byte slot of a 128-byte row is XORed with (v >> 1) & 7 on the
//     fetch side (the global source slot) and on the read side, so the 16 lanes of a quarter wave read 16 different bank groups;
//   * the diagonal: only a chunk's first slice holds bytes with u <= v.  With v0 a multiple of 32 its 32-column halves left of
//     v0 and the 32 x 32 block on the diagonal are masked IN THE FRAGMENT REGISTERS (a per-lane constant of four dwords) --
//     cheaper than zeroing the landed block in LDS, which would put a wait for the slice and an LDS write in front of the
//     barrier that releases it.  `planes` is only read.
// n must be a multiple of 256 (whole slices, every chunk has a first slice, nq == n).
constexpr int W4_SU = 128;   // u per slice
constexpr int W4_NST = 4;    // LDS stages
constexpr int W4_RING = W4_NST * 4 * 32 * W4_SU;  // bytes of the ring with four planes (the extension's two planes use half of every stage)
// bucket sums [wave][row][a * W4_NB + b]: 16 buckets b per (row, a) and one more that nobody reads, where a column whose code is
// outside 0 .. 15 adds its sums.  The odd count is also the padding: the 16 lanes of a quarter wave hold the 16 codes a of one row
// and add into the same b, 136 bytes apart -- 16 different pairs of banks
constexpr int W4_NB = 17;
constexpr int W4_MROW = 4 * 8 * 16 * W4_NB * (int)sizeof(long long);
constexpr size_t W4_LDS = (size_t)W4_RING + W4_MROW;

struct W4It {  // (chunk, slice) in the flat slice sequence of a workgroup
    int c, s;
};
__device__ __forceinline__ void w4_next(W4It& it, int ns, int nchunk) {
    if (it.s + 1 < ns) ++it.s;
    else if (it.c + NP < nchunk) {
        it.c += NP;
        it.s = it.c >> 2;  // the slice that holds u = v0 + 1
    }
    // past the end: stays on the last slice -- fetched again into a stage nobody reads, so that the counted waits stay uniform
}
// FIRST: the first matrix instruction behind vector instructions that wrote its operands (hipcc's hazard recogniser does not see a
// matrix instruction inside an asm statement)
template <bool FIRST>
__device__ __forceinline__ void w4_mfma(v16i& acc, const v4i& a, const v4i& b) {
    if constexpr (FIRST) asm volatile("s_nop 1\n\tv_mfma_i32_32x32x32_i8 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
    else asm volatile("v_mfma_i32_32x32x32_i8 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}
// a chunk's first matrix instruction of an accumulator tile: acc = a b, born in an accumulation register (no zeroing instruction)
template <bool FIRST>
__device__ __forceinline__ void w4_mfma_open(v16i& acc, const v4i& a, const v4i& b) {
    if constexpr (FIRST) asm volatile("s_nop 1\n\tv_mfma_i32_32x32x32_i8 %0, %1, %2, 0" : "=a"(acc) : "v"(a), "v"(b));
    else asm volatile("v_mfma_i32_32x32x32_i8 %0, %1, %2, 0" : "=a"(acc) : "v"(a), "v"(b));
}
// Loads and LDS atomics the COMPILER DOES NOT COUNT: with LDS-DMA in flight hipcc waits for vmcnt(0) in front of every use of a
// loaded register and of every LDS atomic (it cannot tell what the DMA may still write), which would drain the ring once per slice.
// The waits are written out instead (accum_w4_body: wait_masks / wait_codes name the registers, so no use moves in front of them;
// request and wait stand in the same pass of the slice loop, so the compiler has no copy of a register in flight to make).
__device__ __forceinline__ uint32_t w4_load_u32(const void* sbase, uint32_t voff) {
    uint32_t r;
    asm volatile("global_load_dword %0, %1, %2" : "=v"(r) : "v"(voff), "s"(sbase) : "memory");
    return r;
}
// row pair p of the wave: 2 p rows behind `addr`, in the instruction's immediate offset (p is a constant once the bucketing loop is
// unrolled: the switch folds away)
__device__ __forceinline__ void w4_lds_add_u64(uint32_t addr, int p, uint32_t lo, uint32_t hi) {
    const unsigned long long v = ((unsigned long long)hi << 32) | lo;
#define W4_ADD_AT(P) \
    case P: asm volatile("ds_add_u64 %0, %1 offset:%2" : : "v"(addr), "v"(v), "n"((P) * 2 * 16 * W4_NB * 8) : "memory"); break;
    switch (p) {
        W4_ADD_AT(0) W4_ADD_AT(1) W4_ADD_AT(2) W4_ADD_AT(3)
        default: __builtin_unreachable();
    }
#undef W4_ADD_AT
}

template <int NPL, int P0>
__device__ __forceinline__ void accum_w4_body(const int8_t* __restrict__ planes_all, const unsigned long long* __restrict__ bits,
                                              const uint8_t* __restrict__ Q, int m, int n, int nq, int ng,
                                              long long* __restrict__ Mpart, long long* __restrict__ stamps,
                                              const TPrep* __restrict__ prep, const int bid) {
    if (P0 != 0 && prep->ext == 0) return;
    constexpr int ST = NPL * 32 * W4_SU;  // bytes per stage
    constexpr int NI = ST / 1024 / 4;     // LDS-DMA instructions (64 lanes x 16 B) per wave and slice
    constexpr int HSTEP = 4 / NI;         // ... one in front of every HSTEP-th half (three planes: of the first three halves)
    static_assert(NPL >= 2 && NPL <= 4 && NI * 4 * 1024 == ST && NI * HSTEP <= 4, "a slice is NI LDS-DMA instructions per wave");
    extern __shared__ __align__(1024) char w4_smem[];
    char* const ring = w4_smem;
    long long(*Mrow)[8][16 * W4_NB] = reinterpret_cast<long long(*)[8][16 * W4_NB]>(w4_smem + W4_RING);  // [wave][row][a * W4_NB + b]
    const int8_t* planes = planes_all + (int64_t)P0 * n * nq;
    long long st_pro = 0, st_loop = 0, st_flush = 0;
    long long st_t0 = __builtin_amdgcn_s_memtime();

    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // (scalar: the LDS-DMA destinations are scalar arithmetic)
    // v_mfma_i32_32x32x32_i8 with the operands of onehot_accum_body SWAPPED: A rows = the chunk's 32 v, B columns = (row of the pair,
    // code).  (Both operands have lane l hold row / column l & 31 and k bytes 16 (l >> 5) .. + 15, so the fragments are the same.)
    // The tile comes out transposed: lane l holds (row r2, code a16) for good and its 16 registers hold 16 columns v.  In the
    // bucketing pass the lanes of an instruction then add into DIFFERENT (row, a) -- with (row, a) across the registers and v
    // across the lanes, the lanes of a quarter wave whose columns share a code added to the same address, and an LDS atomic
    // takes them one after the other (profiles/accum_sched_v1.txt: 92 cycles per ds_add_u64, whatever D)
    const int i32 = lane & 31, kb = lane >> 5;
    const int r2 = i32 >> 4, a16 = i32 & 15;
    const int nrg = (m + 31) / 32;
    const int rg = bid % nrg, part = bid / nrg;
    const int row0 = rg * 32 + wv * 8;
    const int ns = n / W4_SU, nchunk = n / 32;
    int mrow[4];  // the row whose masks this lane expands, per row pair
#pragma unroll
    for (int p = 0; p < 4; ++p) mrow[p] = min(row0 + 2 * p + r2, m - 1);
    for (int i = lane; i < 8 * 16 * W4_NB; i += 64) (&Mrow[wv][0][0])[i] = 0;
    // bucketing: this lane's (row r2 of pair 0, code a16, b = 0)
    const uint32_t mrow_l = (uint32_t)(uintptr_t)&Mrow[wv][r2][a16 * W4_NB];

    // LDS-DMA: one instruction = 8 rows (plane, v) x 128 B; wave wv sends instructions NI wv .. NI wv + NI - 1 of a slice.  Lane l
    // writes slot l & 7 of row l >> 3 and fetches the slot that belongs there under the XOR
    uint32_t doff[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int rl = (wv * NI + i) * 8 + (lane >> 3);  // row of the stage: plane rl >> 5, v rl & 31
        const int g = (lane & 7) ^ ((rl >> 1) & 7);
        doff[i] = (uint32_t)(((size_t)(rl >> 5) * n + (rl & 31)) * nq + 16 * g);
    }
    auto dma = [&](const W4It& it, int stage, int i) {
        const int8_t* src = planes + (size_t)(32 * it.c) * nq + W4_SU * it.s;
        char* dst = ring + stage * ST + (wv * NI + i) * 1024;
        __builtin_amdgcn_global_load_lds((hg_gptr)(src + doff[i]), (hg_lptr)dst, 16, 0, 0);
    };
    // masks of this slice / requested for the next one; the chunk's codes: bq[p][j] = the codes of row 2 p + r2 in columns
    // v0 + 8 j + 4 kb .. + 3, the columns of registers 4 j .. 4 j + 3 of a tile
    uint32_t wc[2][4][2], wn[2][4], bq[4][4];
    // everything but the NI LDS-DMA instructions issued last has landed: the slice before theirs, and the masks / codes requested
    // in front of them
    auto wait_masks = [&]() {
        if constexpr (NI == 4)
            asm volatile("s_waitcnt vmcnt(4)" : "+v"(wn[0][0]), "+v"(wn[0][1]), "+v"(wn[0][2]), "+v"(wn[0][3]), "+v"(wn[1][0]), "+v"(wn[1][1]), "+v"(wn[1][2]), "+v"(wn[1][3]) : : "memory");
        else if constexpr (NI == 3)
            asm volatile("s_waitcnt vmcnt(3)" : "+v"(wn[0][0]), "+v"(wn[0][1]), "+v"(wn[0][2]), "+v"(wn[0][3]), "+v"(wn[1][0]), "+v"(wn[1][1]), "+v"(wn[1][2]), "+v"(wn[1][3]) : : "memory");
        else
            asm volatile("s_waitcnt vmcnt(2)" : "+v"(wn[0][0]), "+v"(wn[0][1]), "+v"(wn[0][2]), "+v"(wn[0][3]), "+v"(wn[1][0]), "+v"(wn[1][1]), "+v"(wn[1][2]), "+v"(wn[1][3]) : : "memory");
    };
    auto take_masks = [&]() {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                // the 4-bit pieces of a mask dword, one per byte: even pieces in [0], odd ones in [1] (a piece is then picked with a
                // byte select inside its multiply: 2 instructions instead of 3).  Opaque, so that hipcc does not narrow the byte
                // selects back to 4-bit field extracts
                wc[ks][p][0] = wn[ks][p] & 0x0f0f0f0fu;
                wc[ks][p][1] = (wn[ks][p] >> 4) & 0x0f0f0f0fu;
                asm volatile("" : "+v"(wc[ks][p][0]), "+v"(wc[ks][p][1]));
            }
    };
#define W4_BQ4(P) "+v"(bq[P][0]), "+v"(bq[P][1]), "+v"(bq[P][2]), "+v"(bq[P][3])
#define W4_BQ16 W4_BQ4(0), W4_BQ4(1), W4_BQ4(2), W4_BQ4(3)
    auto wait_codes = [&]() {
        if constexpr (NI == 4)
            asm volatile("s_waitcnt vmcnt(4)" : W4_BQ16 : : "memory");
        else if constexpr (NI == 3)
            asm volatile("s_waitcnt vmcnt(3)" : W4_BQ16 : : "memory");
        else
            asm volatile("s_waitcnt vmcnt(2)" : W4_BQ16 : : "memory");
    };
    // fragment reads: lane l holds column v = l & 31, bytes 16 (l >> 5) .. + 15 of a 32-column half; half h: address ^ (h << 5)
    const uint32_t rd0 = (uint32_t)(uintptr_t)ring + (uint32_t)(i32 * 128 + ((kb ^ ((i32 >> 1) & 7)) << 4));
    auto read_b = [&](int stage, int h, v4i (&bf)[NPL]) {
        typedef const v4i __attribute__((address_space(3))) * lp;
        const uint32_t a = (rd0 + (uint32_t)(stage * ST)) ^ (uint32_t)(h << 5);
#pragma unroll
        for (int d = 0; d < NPL; ++d) bf[d] = *reinterpret_cast<lp>(a + d * 4096);
    };
    // the block on the diagonal: byte 16 kb + 4 j + b of column i32 stays when it lies right of the diagonal
    v4i dmask;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int cnt = min(4, max(0, i32 - (16 * kb + 4 * j) + 1));  // leading bytes to clear
        dmask[j] = cnt >= 4 ? 0 : (int)(0xffffffffu << (8 * cnt));
    }
    // code masks in the layout of code_masks_kernel: one dword per 64-column step and row pair, requested one slice ahead
    // (scalar base of the step + 32-bit lane offset: m n < 2^31, accum_w4_supported)
    uint32_t moff[4], qoff[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) moff[p] = (uint32_t)((((size_t)mrow[p] * ng * 16 + a16) * 2 + kb) * 4);
#pragma unroll
    for (int p = 0; p < 4; ++p) qoff[p] = (uint32_t)((size_t)mrow[p] * n + 4 * kb);
    auto load_masks = [&](const W4It& it) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const unsigned long long* base = bits + (size_t)(2 * it.s + ks) * 16;
#pragma unroll
            for (int p = 0; p < 4; ++p) wn[ks][p] = w4_load_u32(base, moff[p]);
        }
    };

    v16i acc[4][NPL];  // born in the first half of a chunk's first slice (w4_mfma_open)
    v4i bf[2][NPL];

    // prologue: slices 0 .. 2 in flight, the masks of slice 0; then slice 0 has landed for everybody
    W4It msk{part, part >> 2}, iss = msk;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
        for (int i = 0; i < NI; ++i) dma(iss, b, i);
        w4_next(iss, ns, nchunk);
    }
    load_masks(msk);
    w4_next(msk, ns, nchunk);
#pragma unroll
    for (int i = 0; i < NI; ++i) dma(iss, 2, i);
    w4_next(iss, ns, nchunk);
    wait_masks();
    take_masks();
    __builtin_amdgcn_s_barrier();
    read_b(0, 0, bf[0]);
    { const long long tt = __builtin_amdgcn_s_memtime(); st_pro += tt - st_t0; st_t0 = tt; }

    int f = 0;  // flat slice count: slice f lives in stage f & 3
    for (int c = part; c < nchunk; c += NP) {
        const int v0 = 32 * c;
        const int hd = c & 3;  // the half of the chunk's first slice that holds the diagonal
        auto slice = [&](auto diag_tag) {
            constexpr bool DIAG = decltype(diag_tag)::value;
            const int stage = f & 3;
            // slice f + 1 has landed (this wave's share: the wait that closed slice f - 1); behind the barrier: everybody's, and
            // every wave is through slice f - 1: its stage takes slice f + 3
            __builtin_amdgcn_s_barrier();
            if (DIAG) {
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int j = 0; j < 4; ++j) bq[p][j] = w4_load_u32(Q + v0 + 8 * j, qoff[p]);
            }
            load_masks(msk);
            w4_next(msk, ns, nchunk);
            // A one-hot fragment = 4 dwords, each 3 vector instructions (16 mask bits -> 16 bytes).  The wave is alone on its SIMD:
            // whatever it issues between two matrix instructions hides behind the first one, whatever it issues in a row does
            // not.  So the fragment of the NEXT group of NPL matrix instructions is expanded piece by piece between those of this
            // one (measured: expanded in one piece in front of its group, the tile loop was no faster than the first kernel's),
            // and the LDS reads and the LDS-DMA of a half stand behind its first matrix instruction.
            auto piece = [&](int h, int p, int d) {
                return (int)((((wc[h >> 1][p][d & 1] >> (8 * (2 * (h & 1) + (d >> 1)))) & 0xffu) * 0x00204081u) & 0x01010101u);
            };
            v4i af[2];
#pragma unroll
            for (int d = 0; d < 4; ++d) af[0][d] = piece(0, 0, d);
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                auto feed = [&]() {  // this half's share of the slice's LDS-DMA; the B fragments of the next half / slice
                    if (h % HSTEP == 0 && h / HSTEP < NI) dma(iss, (f + 3) & 3, h / HSTEP);
                    if (h < 3) read_b(stage, h + 1, bf[(h + 1) & 1]);
                    else read_b((f + 1) & 3, 0, bf[0]);
                };
                if (DIAG) {
                    // a chunk's first slice: the halves left of v0 count nothing, the one at v0 what lies right of the diagonal.
                    // Masked, not skipped (at most three halves of matrix work per chunk): with branches around the asm
                    // statements hipcc moves accumulator tiles between the register files again (112 spilled registers)
                    const int keep = h > hd ? -1 : 0, on = h == hd ? -1 : 0;
#pragma unroll
                    for (int d = 0; d < NPL; ++d)
#pragma unroll
                        for (int j = 0; j < 4; ++j) bf[h & 1][d][j] &= keep | (on & dmask[j]);
                    __builtin_amdgcn_sched_barrier(0);
                    asm volatile("s_nop 4" ::: "memory");  // (the masked fragments were written just now)
                }
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int g = 4 * h + p;           // parity of the fragment register set
                    const bool more = 4 * h + p < 15;  // the group behind this one is in this slice
                    const int nh = p < 3 ? h : h + 1, np = (p + 1) & 3;
#pragma unroll
                    for (int d = 0; d < NPL; ++d) {
                        if (DIAG && h == 0) {  // masked, never skipped: every tile of the chunk starts here
                            if (d == 0) w4_mfma_open<true>(acc[p][0], bf[0][0], af[g & 1]);
                            else w4_mfma_open<false>(acc[p][d], bf[0][d], af[g & 1]);
                        } else if (d == 0) w4_mfma<true>(acc[p][0], bf[h & 1][0], af[g & 1]);
                        else w4_mfma<false>(acc[p][d], bf[h & 1][d], af[g & 1]);
                        if (p == 0 && d == 0) feed();
                        if (more && d < NPL - 1) {  // pieces of the next fragment; none behind the group's last instruction
                            constexpr int PER = 4 / (NPL - 1) + (4 % (NPL - 1) != 0);
#pragma unroll
                            for (int k = d * PER; k < min(4, (d + 1) * PER); ++k) af[(g + 1) & 1][k] = piece(nh, np, k);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            w4_next(iss, ns, nchunk);
            ++f;
            // all but the LDS-DMA of this pass has landed: slice f + 1, the masks of slice f (and the chunk's codes)
            if (DIAG) wait_codes();
            wait_masks();
            take_masks();
        };
        slice(std::true_type{});
        for (int s = (c >> 2) + 1; s < ns; ++s) slice(std::false_type{});
        { const long long tt = __builtin_amdgcn_s_memtime(); st_loop += tt - st_t0; st_t0 = tt; }
        // bucket the chunk's columns by their code, as onehot_accum_body does.  The accumulation registers are read behind matrix
        // instructions in asm statements: the wait is written out, tied to the registers so that no read moves in front of it
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if constexpr (NPL == 4)
                asm volatile("s_nop 15\n\ts_nop 3" : "+a"(acc[p][0]), "+a"(acc[p][1]), "+a"(acc[p][2]), "+a"(acc[p][3]));
            else if constexpr (NPL == 3)
                asm volatile("s_nop 15\n\ts_nop 3" : "+a"(acc[p][0]), "+a"(acc[p][1]), "+a"(acc[p][2]));
            else asm volatile("s_nop 15\n\ts_nop 3" : "+a"(acc[p][0]), "+a"(acc[p][1]));
        }
        // Register reg of this lane's tile holds column v0 + (reg & 3) + 8 (reg >> 2) + 4 kb, whose code b is byte reg & 3 of
        // bq[p][reg >> 2].  No branch around the atomic (64 of them per chunk cost more than the additions they saved) and no select
        // either: a code outside 0 .. 15 takes the bucket that nobody reads
#pragma unroll
        for (int p = 0; p < 4; ++p) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                // |digit sum| <= 128 n <= 2^22 (n <= 32768): two digits recombine inside 32 bits, lo = d0 + 256 d1 (and hi = d2 + 256 d3).
                // The sum lo + 65536 hi without 64-bit arithmetic: t = hi + floor(lo / 65536) (|t| < 2^31), the low word is the low
                // halves of t and lo side by side, the high word floor(t / 65536)
                const int lo = acc[p][0][reg] + (acc[p][1][reg] << 8);
                uint32_t vlo, vhi;
                if constexpr (NPL == 2) {
                    vlo = (uint32_t)lo;
                    vhi = (uint32_t)(lo >> 31);
                } else {
                    int t = acc[p][2][reg] + (lo >> 16);
                    if constexpr (NPL == 4) t += acc[p][3][reg] << 8;
                    vlo = __builtin_amdgcn_perm((uint32_t)t, (uint32_t)lo, 0x05040100u);
                    vhi = (uint32_t)(t >> 16);
                }
                const uint32_t b = min((bq[p][reg >> 2] >> (8 * (reg & 3))) & 0xffu, 16u);
                w4_lds_add_u64(mrow_l + (b << 3), p, vlo, vhi);
            }
        }
        { const long long tt = __builtin_amdgcn_s_memtime(); st_flush += tt - st_t0; st_t0 = tt; }
    }
    // no LDS-DMA may be in flight when the workgroup's LDS is handed on; the bucket sums are complete
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    if (stamps && bid == 0 && tid == 0) { stamps[0] = st_pro; stamps[1] = st_loop; stamps[2] = st_flush; }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 8; ++r)
        if (row0 + r < m) {
            long long* out = Mpart + ((int64_t)part * m + row0 + r) * 256;
            for (int i = lane; i < 256; i += 64) out[i] = Mrow[wv][r][(i >> 4) * W4_NB + (i & 15)];
        }
#undef W4_BQ4
#undef W4_BQ16
}

// one launch for both words, as onehot_accum_kernel.  The 31-bit word: as many digit planes as top_dense_planes says, one choice for
// the whole launch (top_fixup_kernel adds what lies above them)
__global__ __launch_bounds__(256, 1) void onehot_accum_w4_kernel(const int8_t* __restrict__ planes_all,
                                                                const unsigned long long* __restrict__ bits,
                                                                const uint8_t* __restrict__ Q, int m, int n, int nq, int ng,
                                                                long long* __restrict__ Mpart_hi, long long* __restrict__ Mpart_lo,
                                                                long long* __restrict__ stamps, const long long* __restrict__ changed,
                                                                long long thr, const TPrep* __restrict__ prep, int nblk_hi) {
    if (changed && *changed <= thr) return;
    if ((int)blockIdx.x < nblk_hi) {
        const int D = top_dense_planes(prep->c3, prep->c2, prep->top_cap);
        if (D == 2) accum_w4_body<2, 0>(planes_all, bits, Q, m, n, nq, ng, Mpart_hi, stamps, prep, (int)blockIdx.x);
        else if (D == 3) accum_w4_body<3, 0>(planes_all, bits, Q, m, n, nq, ng, Mpart_hi, stamps, prep, (int)blockIdx.x);
        else accum_w4_body<4, 0>(planes_all, bits, Q, m, n, nq, ng, Mpart_hi, stamps, prep, (int)blockIdx.x);
    } else accum_w4_body<2, 4>(planes_all, bits, Q, m, n, nq, ng, Mpart_lo, nullptr, prep, (int)blockIdx.x - nblk_hi);
}

// which kernel sums the buckets of an [m, n] layer in full: 0 onehot_accum_kernel, 1 onehot_accum_w4_kernel.
// GANQ_ACCUM_W4: 0 never, 1 wherever the four-wave kernel is supported, -1 by shape.
bool accum_w4_supported(int64_t m, int64_t n) { return m >= 1 && n >= 256 && n % 256 == 0 && n <= 32768 && m * n < (1ll << 31); }
int accum_plan(int64_t m, int64_t n) {
    const long long opt = opt_get(OPT_ACCUM_W4);
    if (opt == 0 || !accum_w4_supported(m, n)) return 0;
    if (opt == 1) return 1;
    // by shape (profiles/accum_w4_v1.txt, MI355X, V = 8): 0.91 x the first kernel's time at every in_features from 2048 to 14336
    // (2048 .. 14336 rows), 0.95 x at 768 x 3072; level with it at 3072 x 768 (0.106 against 0.105 ms), so short rows stay
    return n >= 2048 ? 1 : 0;
}

// the cap on the exception lists of an [m, n] layer: < 0 when no list is wanted (the first kernel sums the layer, or GANQ_T_TOP=0).
// GANQ_T_TOP_CAP overrides the default; TOP_LIST_MAX bounds both.
// The default grows with n^2, as the plane it saves does: a dense plane costs every row n^2 / 2 multiply-adds, a list entry one LDS
// atomic per row, so the break-even count is a fixed share of the pairs whatever m is.
constexpr int TOP_CAP_SHARE = 1024;  // default cap = n^2 / TOP_CAP_SHARE
int top_cap_in_force(int64_t m, int64_t n) {
    if (accum_plan(m, n) != 1 || opt_get(OPT_T_TOP) == 0) return -1;
    const long long c = opt_get(OPT_T_TOP_CAP);
    return (int)std::min<long long>(c < 0 ? n * n / TOP_CAP_SHARE : c, TOP_LIST_MAX);
}

// What onehot_accum_w4_kernel left out when it summed D < 4 planes: sum of `value` over the list's entries (u, v) into bucket
// [Q[row][u]][Q[row][v]], times 2^(8 D), added to part 0 of the row's partial sums.  One workgroup per row: the row's codes and 256
// 64-bit buckets in LDS, the threads stride the list (the same list for every row: it stays in L2).  Integers: exact in any order.
__global__ __launch_bounds__(256) void top_fixup_kernel(const uint2* __restrict__ top3, const uint2* __restrict__ top2,
                                                       const uint8_t* __restrict__ Q, int m, int n, long long* __restrict__ Mpart,
                                                       const long long* __restrict__ changed, long long thr,
                                                       const TPrep* __restrict__ prep) {
    if (changed && *changed <= thr) return;
    const int D = top_dense_planes(prep->c3, prep->c2, prep->top_cap);
    if (D == 4) return;
    const unsigned int cnt = D == 2 ? prep->c2 : prep->c3;  // (<= top_cap <= TOP_LIST_MAX: the whole list was stored)
    if (cnt == 0) return;
    const uint2* __restrict__ list = D == 2 ? top2 : top3;
    extern __shared__ __align__(16) char fx_smem[];
    long long* bucket = reinterpret_cast<long long*>(fx_smem);  // [a * 16 + b]
    uint8_t* codes = reinterpret_cast<uint8_t*>(fx_smem) + 256 * sizeof(long long);
    const int tid = threadIdx.x, row = blockIdx.x;
    const uint8_t* q = Q + (int64_t)row * n;
    bucket[tid] = 0;
    for (int x = tid; x < n; x += 256) codes[x] = q[x];
    __syncthreads();
    for (unsigned int i = tid; i < cnt; i += 256) {
        const uint2 e = list[i];
        const uint32_t a = codes[e.x & 0xffffu], b = codes[e.x >> 16];  // a from u, b from v, as the dense kernel
        if (a < 16u && b < 16u)
            __hip_atomic_fetch_add(&bucket[a * 16 + b], (long long)(int)e.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    const long long add = bucket[tid];
    if (add) Mpart[(int64_t)row * 256 + tid] += add * (1ll << (8 * D));
}

// Per-column index of the exception list that goes with the D = mu_dense_planes(..) planes of the incremental sums, once per layer: a
// changed column c must find the listed pairs it is an end of without scanning the list.  Entry (u, v, value) is filed under u as
// (v, value) and under v as (u, value); col_off[c] .. col_off[c + 1] bound column c's run of col_ent (at most 2 TOP_LIST_MAX entries).
// One workgroup: counts, offsets and cursors live in LDS (n + 1 ints, n <= 32768), so a massive column's thousands of increments
// are LDS atomics on one address and not global ones.  The order inside a run depends on the scheduling; the sums formed from it are
// integers.  Leaves at once when all four planes are dense or the list is empty (the consumer then reads nothing).
__global__ __launch_bounds__(1024) void top_index_kernel(const uint2* __restrict__ top3, const uint2* __restrict__ top2,
                                                        TPrep* __restrict__ prep, int n, int* __restrict__ col_off,
                                                        uint2* __restrict__ col_ent, int mu_top) {
    const int D = mu_dense_planes(prep->c3, prep->c2, prep->top_cap, mu_top);
    if (threadIdx.x == 0) prep->mu_index = D;  // (also when nothing is filed below: the consumer then reads nothing)
    if (D == 4) return;
    const unsigned int cnt = D == 2 ? prep->c2 : prep->c3;  // (<= top_cap <= TOP_LIST_MAX: the whole list was stored)
    if (cnt == 0) return;
    const uint2* __restrict__ list = D == 2 ? top2 : top3;
    extern __shared__ int ti_cur[];  // [n]: counts, then cursors
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int c = tid; c < n; c += 1024) ti_cur[c] = 0;
    __syncthreads();
    for (unsigned int i = tid; i < cnt; i += 1024) {
        const uint32_t uv = list[i].x;
        atomicAdd(&ti_cur[uv & 0xffffu], 1);
        atomicAdd(&ti_cur[uv >> 16], 1);
    }
    __syncthreads();
    // exclusive scan: thread t owns columns t per .. t per + per - 1
    const int per = (n + 1023) / 1024, c0 = min(tid * per, n), c1 = min(c0 + per, n);
    int mine = 0;
    for (int c = c0; c < c1; ++c) mine += ti_cur[c];
    int incl = mine;
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int run = incl - mine;
    for (int k = 0; k < wv; ++k) run += wsum[k];
    for (int c = c0; c < c1; ++c) {
        const int k = ti_cur[c];
        col_off[c] = run;
        ti_cur[c] = run;
        run += k;
    }
    if (tid == 1023) col_off[n] = run;  // (the last thread's run ends the scan: 2 cnt)
    __syncthreads();
    for (unsigned int i = tid; i < cnt; i += 1024) {
        const uint2 e = list[i];
        const uint32_t u = e.x & 0xffffu, v = e.x >> 16;
        col_ent[atomicAdd(&ti_cur[u], 1)] = make_uint2(v, e.y);
        col_ent[atomicAdd(&ti_cur[v], 1)] = make_uint2(u, e.y);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// 16 lanes per row, 4 rows per wave, 1 wave per workgroup.
#ifndef GANQ_JACOBI_SWEEPS
#define GANQ_JACOBI_SWEEPS 30
#endif
constexpr int JS = 17;
  // padded leading dimension of the fp64 16x16 matrices in LDS

__device__ __forceinline__ double row16_sum(double x) {
    x += __shfl_xor(x, 1, 16);
    x += __shfl_xor(x, 2, 16);
    x += __shfl_xor(x, 4, 16);
    x += __shfl_xor(x, 8, 16);
    return x;
}
__device__ __forceinline__ double row16_max(double x) {
    x = fmax(x, __shfl_xor(x, 1, 16));
    x = fmax(x, __shfl_xor(x, 2, 16));
    x = fmax(x, __shfl_xor(x, 4, 16));
    x = fmax(x, __shfl_xor(x, 8, 16));
    return x;
}
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ---------------------------------------------------------------------------------------------------------------
// Incremental bucket sums.  F_i[a][b] = sum_{u != v} [Q_iu = a][Q_iv = b] Hint[u][v] (= M + M^T of the full
// accumulation) is an integer, so moving the entries of the columns whose index changed reproduces exactly what a
// full accumulation over the new indices gives.

// Mstate[row] = F = M + M^T with M = sum_p Mpart[p][row]; Qprev = Q   (after a full accumulation)
// is_lo: the sums of the extension word (own Mpart / Mstate; leaves at once when the extension is off; Qprev is the
// other launch's business)
__global__ __launch_bounds__(256) void m_reduce_kernel(const long long* __restrict__ Mpart_hi, const long long* __restrict__ Mpart_lo, int m,
                                                      long long* __restrict__ Mstate_hi, long long* __restrict__ Mstate_lo,
                                                      const uint8_t* __restrict__ Q, uint8_t* __restrict__ Qprev, int64_t qbytes,
                                                      const long long* __restrict__ changed, long long thr,
                                                      const TPrep* __restrict__ prep, int nblk_hi) {
    if (changed && *changed <= thr) return;
    // one launch for both words (a dispatch costs ~5 us on the device even when it leaves at once, and this one sits in every
    // iteration of the loop): the first nblk_hi workgroups sum the 31-bit word and bring Qprev up to date, the others the extension
    const int is_lo = (int)blockIdx.x >= nblk_hi;
    if (is_lo && prep->ext == 0) return;
    const long long* Mpart = is_lo ? Mpart_lo : Mpart_hi;
    long long* Mstate = is_lo ? Mstate_lo : Mstate_hi;
    const int64_t bid = is_lo ? (int64_t)blockIdx.x - nblk_hi : (int64_t)blockIdx.x;
    const int64_t nblk = is_lo ? (int64_t)gridDim.x - nblk_hi : (int64_t)nblk_hi;
    const int64_t total = (int64_t)m * 256;
    for (int64_t i = bid * 256 + threadIdx.x; i < total; i += nblk * 256) {
        const int64_t it = (i & ~255ll) | ((i & 15) << 4) | ((i >> 4) & 15);  // the transposed cell of the same row
        long long s = 0;
#pragma unroll
        for (int p = 0; p < NP; ++p) s += Mpart[(int64_t)p * total + i] + Mpart[(int64_t)p * total + it];
        Mstate[i] = s;
    }
    if (is_lo) return;
    const int64_t q16 = qbytes / 16;
    for (int64_t i = bid * 256 + threadIdx.x; i < q16; i += nblk * 256)
        reinterpret_cast<uint4*>(Qprev)[i] = reinterpret_cast<const uint4*>(Q)[i];
    for (int64_t i = q16 * 16 + bid * 256 + threadIdx.x; i < qbytes; i += nblk * 256) Qprev[i] = Q[i];
}

// one wave per row: columns whose index differs from the previous iteration -> chg[row][0..cnt), chgcnt[row]; *changed += cnt
constexpr int QD_WAVES = 16;  // rows per workgroup: one add to the global change counter per workgroup -- one per row
                              // made 4096 same-address atomics the longest part of the kernel (55 us)
__global__ __launch_bounds__(QD_WAVES * 64) void q_diff_kernel(const uint8_t* __restrict__ Q, const uint8_t* __restrict__ Qprev, int m, int n,
                                                    uint16_t* __restrict__ chg, int* __restrict__ chgcnt,
                                                    long long* __restrict__ changed) {
    __shared__ int wg_total;
    if (threadIdx.x == 0) wg_total = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int row_raw = blockIdx.x * QD_WAVES + (threadIdx.x >> 6);
    const bool active = row_raw < m;
    const int row = active ? row_raw : m - 1;  // a padding wave repeats the last row and writes nothing
    const uint8_t* q = Q + (int64_t)row * n;
    const uint8_t* qp = Qprev + (int64_t)row * n;
    uint16_t* out = chg + (int64_t)row * n;
    int cnt = 0;
    int xdone = 0;
    if ((n & 15) == 0) {  // rows are 16-byte aligned: 1 KB of each row per step, 4 steps in flight
        const int n16 = n >> 4;
        for (int i0 = 0; i0 < n16; i0 += 64 * 4) {
            uint4 a[4], b[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = i0 + 64 * k + lane;
                a[k] = i < n16 ? reinterpret_cast<const uint4*>(q)[i] : make_uint4(0, 0, 0, 0);
                b[k] = i < n16 ? reinterpret_cast<const uint4*>(qp)[i] : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = i0 + 64 * k + lane;
                const uint32_t dw[4] = {a[k].x ^ b[k].x, a[k].y ^ b[k].y, a[k].z ^ b[k].z, a[k].w ^ b[k].w};
                if (__ballot((dw[0] | dw[1] | dw[2] | dw[3]) != 0) == 0) continue;  // uniform
#pragma unroll
                for (int w = 0; w < 4; ++w)
#pragma unroll
                    for (int by = 0; by < 4; ++by) {
                        const bool d = ((dw[w] >> (8 * by)) & 0xffu) != 0;
                        const unsigned long long mk = __ballot(d);
                        if (d && active) out[cnt + __popcll(mk & ((1ull << lane) - 1ull))] = (uint16_t)(16 * i + 4 * w + by);
                        cnt += __popcll(mk);
                    }
            }
        }
        xdone = n;
    }
    for (int x0 = xdone; x0 < n; x0 += 64) {
        const int x = x0 + lane;
        const bool d = x < n && q[x] != qp[x];
        const unsigned long long mk = __ballot(d);
        if (d && active) out[cnt + __popcll(mk & ((1ull << lane) - 1ull))] = (uint16_t)x;
        cnt += __popcll(mk);
    }
    if (lane == 0 && active) {
        chgcnt[row] = cnt;
        if (cnt) atomicAdd(&wg_total, cnt);
    }
    __syncthreads();
    if (threadIdx.x == 0 && wg_total) atomicAdd(reinterpret_cast<unsigned long long*>(changed), (unsigned long long)wg_total);
}

// One workgroup per row, its waves share out the changed columns.  Column c = list[e] goes a_old -> a_new.  Taking the
// changes in list order, the codes seen by step e are the new ones for list[e' < e] and the old ones elsewhere, so with
//   S_e[b] = sum_{x != c, old[x] = b} Hint[c][x]  +  sum_{e' < e} Hint[c][list[e']] * ([new[e'] = b] - [old[e'] = b])
// the step is   F[a_old][b] -= S_e[b], F[b][a_old] -= S_e[b], F[a_new][b] += S_e[b], F[b][a_new] += S_e[b]  for every b.
// No S_e depends on F or on another S, so the steps run in parallel and add into the row's F with LDS atomics.
// S_e is a 16-bucket histogram of one row of Hint: lane-private buckets in LDS ([bucket][lane]: no conflicts), then
// a transposed read sums each bucket over the lanes; the second sum is just 2 more entries per earlier change.
constexpr int MU_WAVES = 4;  // 4096x4096 benchmark layer: 2 -> 0.224, 4 -> 0.210, 8 -> 0.250 ms per iteration
// HT = int: the 31-bit word (Hint -> Mstate), updates Qprev at the end; HT = short: the extension word (Jint ->
// Mstate_lo), launched BEFORE the other one (it needs the old codes), leaves at once when the extension is off.
template <typename HT>
__global__ __launch_bounds__(MU_WAVES * 64) void m_update_kernel(const HT* __restrict__ Hint, const uint8_t* __restrict__ Q,
                                                                uint8_t* __restrict__ Qprev, int m, int n,
                                                                const uint16_t* __restrict__ chg, const int* __restrict__ chgcnt,
                                                                long long* __restrict__ Mstate,
                                                                const long long* __restrict__ changed, long long thr,
                                                                const TPrep* __restrict__ prep) {
    if (*changed > thr) return;  // the full accumulation runs instead
    constexpr bool IS_LO = sizeof(HT) == 2;
    constexpr int BIAS = IS_LO ? JBIAS : 0;  // the int16 copy of the extension word is stored biased
    if (IS_LO && prep->ext == 0) return;
    extern __shared__ __align__(16) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int row = blockIdx.x;
    const int cnt = chgcnt[row];
    if (cnt == 0) return;
    long long* Frow = reinterpret_cast<long long*>(smem);                                   // [16][16]
    long long* priv = reinterpret_cast<long long*>(smem) + 256 + wv * (16 * 64);            // [16][64] per wave
    uint8_t* codes = reinterpret_cast<uint8_t*>(smem) + (size_t)(256 + MU_WAVES * 16 * 64) * sizeof(long long);  // old
    long long* Fg = Mstate + (int64_t)row * 256;
    uint8_t* qp = Qprev + (int64_t)row * n;
    const uint8_t* qn = Q + (int64_t)row * n;
    for (int i = tid; i < 256; i += MU_WAVES * 64) Frow[i] = Fg[i];
    for (int x = tid; x < n; x += MU_WAVES * 64) codes[x] = min((int)qp[x], 15);
    __syncthreads();
    const uint16_t* list = chg + (int64_t)row * n;
    // The work of a wave is a stream of (its changed column, 4096-column chunk of that Hint row) items.  Every item is
    // a dependent L2 / HBM round trip, so the next item's 16 KB are always in flight (16 x 16 B per lane) while the
    // current one is bucketed.
    constexpr int CH = 16;                       // int4 loads per lane and chunk: 64 * 16 * 4 = 4096 columns
    const bool vec = !IS_LO && (n & 3) == 0;     // rows of Hint are 16-byte aligned (int32 only)
    const int nchunk = (n + 64 * CH * 4 - 1) / (64 * CH * 4);
    const int mycols = (cnt - wv + MU_WAVES - 1) / MU_WAVES;  // e = wv, wv + MU_WAVES, ..
    const int nitems = mycols * nchunk;
    // this lane's earlier-change partner e' = lane (the first 64 changes; later ones take the slow loop below)
    const int pc = lane < cnt ? list[lane] : 0;
    const int p_old = lane < cnt ? codes[pc] : 0, p_new = lane < cnt ? min((int)qn[pc], 15) : 0;
    auto load_item = [&](int it, int4 (&buf)[CH], int& corr) {
        const int e = wv + (it / nchunk) * MU_WAVES, k = it % nchunk;
        const HT* hrow = Hint + (int64_t)list[e] * n;
        corr = (k == 0 && lane < e) ? (int)hrow[pc] - BIAS : 0;
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int x = 4 * (64 * (CH * k + j) + lane);
            int4 v = make_int4(0, 0, 0, 0);
            if (vec) {
                if (x < n) v = *reinterpret_cast<const int4*>(reinterpret_cast<const int*>(hrow) + x);
            } else {
                if (x < n) v.x = (int)hrow[x] - BIAS;
                if (x + 1 < n) v.y = (int)hrow[x + 1] - BIAS;
                if (x + 2 < n) v.z = (int)hrow[x + 2] - BIAS;
                if (x + 3 < n) v.w = (int)hrow[x + 3] - BIAS;
            }
            buf[j] = v;
        }
    };
    auto lds_add = [&](long long* p, long long v) {  // fire-and-forget LDS add
        __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    auto bucket_item = [&](int it, const int4 (&buf)[CH], int corr) {
        const int e = wv + (it / nchunk) * MU_WAVES, k = it % nchunk;
        const int c = list[e];
        if (k == 0) {
#pragma unroll
            for (int b = 0; b < 16; ++b) priv[b * 64 + lane] = 0;
            if (lane < e && lane < 64) {  // partner e' = lane < e already carries its new code
                lds_add(&priv[p_new * 64 + lane], (long long)corr);
                lds_add(&priv[p_old * 64 + lane], -(long long)corr);
            }
            for (int e2 = 64 + lane; e2 < e; e2 += 64) {  // more than 64 changes in the row: rare
                const int c2 = list[e2];
                const long long v = (long long)Hint[(int64_t)c * n + c2] - BIAS;
                lds_add(&priv[min((int)qn[c2], 15) * 64 + lane], v);
                lds_add(&priv[(int)codes[c2] * 64 + lane], -v);
            }
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int x = 4 * (64 * (CH * k + j) + lane);
            const int hv[4] = {buf[j].x, buf[j].y, buf[j].z, buf[j].w};
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (x + t < n && x + t != c) lds_add(&priv[(int)codes[x + t] * 64 + lane], (long long)hv[t]);
        }
        if (k != nchunk - 1) return;
        // column finished: bucket b = lane & 15 summed over lanes 16*(lane>>4) .. +15, then over the four quarters
        wave_sync();
        const int a_old = codes[c], a_new = min((int)qn[c], 15);
        long long sb = 0;
        {
            const long long* pb = priv + (lane & 15) * 64 + 16 * (lane >> 4);
#pragma unroll
            for (int t = 0; t < 16; ++t) sb += pb[t];
        }
        sb += __shfl_xor(sb, 16);
        sb += __shfl_xor(sb, 32);
        if (lane < 16) {  // lane = b
            lds_add(&Frow[a_old * 16 + lane], -sb);
            lds_add(&Frow[lane * 16 + a_old], -sb);
            lds_add(&Frow[a_new * 16 + lane], sb);
            lds_add(&Frow[lane * 16 + a_new], sb);
        }
        wave_sync();
    };
    if (nitems > 0) {
        int4 buf0[CH], buf1[CH];
        int corr0 = 0, corr1 = 0;
        load_item(0, buf0, corr0);
        for (int it = 0; it < nitems; it += 2) {
            if (it + 1 < nitems) load_item(it + 1, buf1, corr1);
            bucket_item(it, buf0, corr0);
            if (it + 1 >= nitems) break;
            if (it + 2 < nitems) load_item(it + 2, buf0, corr0);
            bucket_item(it + 1, buf1, corr1);
        }
    }
    __syncthreads();
    for (int i = tid; i < 256; i += MU_WAVES * 64) Fg[i] = Frow[i];
    if (!IS_LO)
        for (int e = tid; e < cnt; e += MU_WAVES * 64) qp[list[e]] = qn[list[e]];
}

// The same move on the integer matrix cores (rows whose length is a multiple of 16).  The 16-bucket histograms of the
// changed columns of one row are one small GEMM:  S[b][e] = sum_x [old[x] == b] * Hint[c_e][x]  =  onehot(old codes)
// [16 x n]  @  digits of the rows c_e of H [n x changes], with the 4 int8 digit planes t_prepare already holds
// (v_mfma_i32_16x16x64_i8, 16 changes per tile, up to 2 tiles per pass).  It is formed with the OLD codes everywhere;
// what the list-order semantics of m_update_kernel adds -- the changed column itself is left out, earlier changes of
// the row already carry their new code -- are cnt diagonal entries and cnt^2/2 single entries of Hint, applied to F
// directly.  One workgroup per row whose 4 waves split the columns (a row is a chain of dependent memory round
// trips; partial sums simply add into F, they are integers); the A operand (one-hot bytes) is built from 16 code bytes per lane with a zero-byte
// test, the B operand is 16 contiguous digit bytes of a changed column's row.  All sums are integers: the result is
// bit-identical to m_update_kernel and to the full accumulation.
constexpr int MG_TILES = 2;   // 32 changes per pass over the row (p99 of the benchmark layer's first update: 28)
constexpr int MG_WAVES = 4;   // the waves of a row's workgroup split the columns

__device__ __forceinline__ uint32_t bytes_equal(uint32_t x, uint32_t pat) {  // 0x01 in every byte of x equal to pat's
    const uint32_t y = x ^ pat;
    const uint32_t t = ((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y;
    return (~t & 0x80808080u) >> 7;
}

// steps of operands m_update_mfma_kernel keeps in flight per wave, by tiles per pass and operand planes per step.  The planes not
// read free registers, but at 168 (three workgroups per CU) only one deeper ring fits without scratch -- two tiles, two planes, 3
// steps -- and it measured level with 2 steps (profiles/mu_top_v1.txt): the depths are the four-plane kernel's
constexpr int mu_depth(int nt, int npl) {
    if (nt == 2) return npl >= 5 ? 1 : 2;
    return npl == 6 ? 2 : npl == 5 ? 3 : 4;
}

// D dense planes of the 31-bit word (operands 0 .. D - 1 -> acc[t][0 .. D - 1]) and, with EXT, planes 4 and 5 of the extension word
// (-> acc[t][4], acc[t][5]); the accumulators of the planes left out stay zero
template <int NT, int D, bool EXT>
__device__ __forceinline__ void mu_group(const int8_t* __restrict__ planes, int n, int nq, const uint8_t* __restrict__ qp,
                                         const int (&cj)[MG_TILES], int lane, int kb, int ke, v4i (&acc)[MG_TILES][6]) {
    constexpr int NPL = D + (EXT ? 2 : 0);
    auto pl = [](int p) { return p < D ? p : p - D + 4; };  // operand p of a step is this plane / accumulator
    const int i16 = lane & 15, kq = lane >> 4;
    const uint32_t pat = (uint32_t)i16 * 0x01010101u;
    const int64_t plane = (int64_t)n * nq;
    const int8_t* bp[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) bp[t] = planes + (int64_t)cj[t] * nq + 16 * kq;
    if (kb >= ke) return;
    auto load = [&](int k0, uint4& cw, v4i (&bf)[NT][NPL]) {
        cw = *reinterpret_cast<const uint4*>(qp + min(k0 + 16 * kq, n - 16));  // past n the digits are zero
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int p = 0; p < NPL; ++p) bf[t][p] = *reinterpret_cast<const v4i*>(bp[t] + pl(p) * plane + k0);
    };
    // every step is one dependent round trip to L2 / Infinity Cache: FL steps of operands are kept in flight
    // (with the extension's six planes half as many as with four: the kernel then fits 168 registers -- three workgroups per CU instead
    // of two for a kernel that is a chain of round trips per row; the six-plane path is the rare one)
    constexpr int FL = mu_depth(NT, NPL);
    uint4 cw[FL];
    v4i bf[FL][NT][NPL];
    auto step = [&](const uint4& c, const v4i (&b)[NT][NPL]) {
        v4i af;
        af[0] = (int)bytes_equal(c.x, pat);
        af[1] = (int)bytes_equal(c.y, pat);
        af[2] = (int)bytes_equal(c.z, pat);
        af[3] = (int)bytes_equal(c.w, pat);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int p = 0; p < NPL; ++p) acc[t][pl(p)] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, b[t][p], acc[t][pl(p)], 0, 0, 0);
    };
#pragma unroll
    for (int d = 0; d < FL; ++d) load(min(kb + 64 * d, ke - 64), cw[d], bf[d]);
    for (int k0 = kb; k0 < ke; k0 += 64 * FL) {
#pragma unroll
        for (int d = 0; d < FL; ++d) {
            if (k0 + 64 * d < ke) step(cw[d], bf[d]);                    // uniform
            load(min(k0 + 64 * (d + FL), ke - 64), cw[d], bf[d]);       // clamped: the tail re-reads its last step
        }
    }
}

// With the extension word on (prep->ext, uniform) the two extra digit planes ride along in the same pass and move the
// second set of sums Mstate_lo; the pair / diagonal corrections come from Jint / hdiag_j.
// Of the 31-bit word only the D = mu_dense_planes(..) lowest planes are read (uniform; D = 4 wherever no exception lists exist):
// S is linear in H, so what the planes above them hold is moved separately -- for a changed column c every listed pair (c, x) moves
// value << 8 D into the bucket of x's OLD code, found through the per-column index of top_index_kernel; the column's own entry is
// taken out with the low D digits of the diagonal, which is all the planes put in.  The pair corrections take the whole Hint.
constexpr int MU_TOP_SMALL = 32;  // a column with more listed partners than this is shared out among the row's threads
constexpr int MU_TOP_BIG = 64;    // ... as long as the row has no more than this many of them
__global__ __launch_bounds__(MG_WAVES * 64, 3) void m_update_mfma_kernel(const int8_t* __restrict__ planes, const int* __restrict__ Hint,
                                                           const short* __restrict__ Jint,
                                                           const int* __restrict__ hdiag_int, const int* __restrict__ hdiag_j,
                                                           const uint8_t* __restrict__ Q,
                                                           uint8_t* __restrict__ Qprev, int m, int n, int nq,
                                                           const uint16_t* __restrict__ chg, const int* __restrict__ chgcnt,
                                                           long long* __restrict__ Mstate, long long* __restrict__ Mstate_lo,
                                                           const long long* __restrict__ changed, long long thr,
                                                           const TPrep* __restrict__ prep, const int* __restrict__ col_off,
                                                           const uint2* __restrict__ col_ent, int mu_top) {
    if (*changed > thr) return;  // the full accumulation runs instead
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int cnt = chgcnt[row];
    if (cnt == 0) return;
    const bool ext = prep->ext != 0;
    // (uniform) the D the index of this H was built for; without one -- t_prepare ran under GANQ_MU_TOP=0 -- all four planes
    const int D = (mu_top == 0 || prep->mu_index == 0) ? 4 : prep->mu_index;
    const bool listed = D < 4 && (D == 2 ? prep->c2 : prep->c3) != 0;                         // entries above the dense planes exist
    __shared__ long long Frow[256];
    __shared__ long long Flo[256];
    long long* Fg = Mstate + (int64_t)row * 256;
    long long* Fgl = Mstate_lo + (int64_t)row * 256;
    uint8_t* qp = Qprev + (int64_t)row * n;
    const uint8_t* qn = Q + (int64_t)row * n;
    const uint16_t* list = chg + (int64_t)row * n;
    Frow[tid] = Fg[tid];
    if (ext) Flo[tid] = Fgl[tid];
    // the row's changes (column, old code, new code): one parallel round of loads instead of dependent ones per use
    constexpr int CAP = 512;
    __shared__ uint16_t s_col[CAP];
    __shared__ uint8_t s_old[CAP], s_new[CAP];
    __shared__ int s_tb[CAP];        // the column's run of the per-column index: begin, length (read here, beside the codes: the
    __shared__ uint16_t s_tl[CAP];   // list phase below then starts without a round trip of its own)
    __shared__ int s_big[MU_TOP_BIG], s_nbig;
    if (tid == 0) s_nbig = 0;
    for (int e = tid; e < min(cnt, CAP); e += MG_WAVES * 64) {
        const int c = list[e];
        s_col[e] = (uint16_t)c;
        s_old[e] = (uint8_t)min((int)qp[c], 15);
        s_new[e] = (uint8_t)min((int)qn[c], 15);
        if (listed) {
            const int b0 = col_off[c];
            s_tb[e] = b0;
            s_tl[e] = (uint16_t)(col_off[c + 1] - b0);  // (a column has fewer than n <= 32768 partners)
        }
    }
    __syncthreads();
    auto col_of = [&](int e) -> int { return e < CAP ? (int)s_col[e] : (int)list[e]; };
    auto old_of = [&](int e) -> int { return e < CAP ? (int)s_old[e] : min((int)qp[list[e]], 15); };
    auto new_of = [&](int e) -> int { return e < CAP ? (int)s_new[e] : min((int)qn[list[e]], 15); };
    const int ksteps = (n + 63) >> 6, kper = (ksteps + MG_WAVES - 1) / MG_WAVES;
    const int kb = min(wv * kper, ksteps) * 64, ke = min((wv + 1) * kper, ksteps) * 64;  // this wave's columns
    auto lds_add = [&](long long* p, long long v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
    // F[a_old][b] -= s, F[b][a_old] -= s, F[a_new][b] += s, F[b][a_new] += s
    auto move_in = [&](long long* F, int a_old, int a_new, int b, long long s) {
        lds_add(&F[a_old * 16 + b], -s);
        lds_add(&F[b * 16 + a_old], -s);
        lds_add(&F[a_new * 16 + b], s);
        lds_add(&F[b * 16 + a_new], s);
    };
    auto move = [&](int a_old, int a_new, int b, long long s) { move_in(Frow, a_old, a_new, b, s); };
    const int i16 = lane & 15, kq = lane >> 4;
    for (int g0 = 0; g0 < cnt; g0 += 16 * MG_TILES) {
        const int nt = min(MG_TILES, (cnt - g0 + 15) >> 4);
        int cj[MG_TILES];
#pragma unroll
        for (int t = 0; t < MG_TILES; ++t) {
            const int e = g0 + 16 * t + i16;
            cj[t] = col_of(e < cnt ? e : g0);  // padding columns repeat a valid one; their sums are dropped below
        }
        v4i acc[MG_TILES][6];
#pragma unroll
        for (int t = 0; t < MG_TILES; ++t)
#pragma unroll
            for (int p = 0; p < 6; ++p) acc[t][p] = v4i{0, 0, 0, 0};
        auto group = [&](auto d_tag, auto ext_tag) {
            constexpr int DD = decltype(d_tag)::value;
            constexpr bool EE = decltype(ext_tag)::value;
            if (nt == 1) mu_group<1, DD, EE>(planes, n, nq, qp, cj, lane, kb, ke, acc);
            else mu_group<2, DD, EE>(planes, n, nq, qp, cj, lane, kb, ke, acc);
        };
        if (ext) {
            if (D == 2) group(std::integral_constant<int, 2>{}, std::true_type{});
            else if (D == 3) group(std::integral_constant<int, 3>{}, std::true_type{});
            else group(std::integral_constant<int, 4>{}, std::true_type{});
        } else {
            if (D == 2) group(std::integral_constant<int, 2>{}, std::false_type{});
            else if (D == 3) group(std::integral_constant<int, 3>{}, std::false_type{});
            else group(std::integral_constant<int, 4>{}, std::false_type{});
        }
        // D layout: lane (j = lane & 15, kq) holds S[b = 4 kq + r][change j], r = 0..3
#pragma unroll
        for (int t = 0; t < MG_TILES; ++t) {
            const int e = g0 + 16 * t + i16;
            if (t < nt && e < cnt) {
                const int a_old = old_of(e), a_new = new_of(e);
                // (what the D planes hold of the column's own entry; the planes left out have zero accumulators: the sum below is theirs)
                const long long self = wv == 0 ? low_digits((long long)hdiag_int[cj[t]], D) : 0;
                const long long self_lo = (ext && wv == 0) ? (long long)hdiag_j[cj[t]] : 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int b = 4 * kq + r;
                    long long sb = (long long)acc[t][0][r] + ((long long)acc[t][1][r] << 8) + ((long long)acc[t][2][r] << 16) +
                                   ((long long)acc[t][3][r] << 24);
                    if (b == a_old) sb -= self;  // the column itself is not part of its own histogram (taken out once)
                    if (sb != 0) move(a_old, a_new, b, sb);
                    if (ext) {
                        long long sl = (long long)acc[t][4][r] + ((long long)acc[t][5][r] << 8);
                        if (b == a_old) sl -= self_lo;
                        if (sl != 0) move_in(Flo, a_old, a_new, b, sl);
                    }
                }
            }
        }
    }
    // the listed entries of the changed columns: what the digits above the D dense planes hold, with the OLD code of the partner
    if (listed) {
        const int sh = 8 * D;
        auto entry = [&](int a_old, int a_new, const uint2 en) {
            const uint32_t b = qp[en.x];
            if (b < 16u) move(a_old, a_new, (int)b, (long long)(int)en.y * (1ll << sh));  // (the matrix sum, too, has no bucket for codes >= 16)
        };
        for (int e = tid; e < cnt; e += MG_WAVES * 64) {
            int b0, len;
            if (e < CAP) {
                b0 = s_tb[e];
                len = s_tl[e];
            } else {
                const int c = list[e];
                b0 = col_off[c];
                len = col_off[c + 1] - b0;
            }
            if (len == 0) continue;
            // a massive column itself: left to the whole workgroup, if the table has room.  (A row that changes more than MU_TOP_BIG
            // such columns at once walks the others' runs in one thread each, up to n entries in a row: correct, slow, and only met
            // with a long list and hundreds of changes in one row.)
            if (len > MU_TOP_SMALL) {
                const int slot = atomicAdd(&s_nbig, 1);
                if (slot < MU_TOP_BIG) {
                    s_big[slot] = e;
                    continue;
                }
            }
            const int a_old = old_of(e), a_new = new_of(e);
            for (int i = 0; i < len; ++i) entry(a_old, a_new, col_ent[b0 + i]);
        }
        __syncthreads();
        const int nbig = min(s_nbig, MU_TOP_BIG);
        for (int k = 0; k < nbig; ++k) {
            const int e = s_big[k], c = col_of(e);
            const int b0 = col_off[c], len = col_off[c + 1] - b0;
            const int a_old = old_of(e), a_new = new_of(e);
            for (int i = tid; i < len; i += MG_WAVES * 64) entry(a_old, a_new, col_ent[b0 + i]);
        }
    }
    // earlier changes e' < e of the row already carry their new code when change e is applied: all pairs at once
    for (int64_t pidx = tid; pidx < (int64_t)cnt * cnt; pidx += MG_WAVES * 64) {
        const int e = (int)(pidx / cnt), e2 = (int)(pidx - (int64_t)e * cnt);
        if (e2 >= e) continue;
        const long long v = (long long)Hint[(int64_t)col_of(e) * n + col_of(e2)];
        if (v != 0) {
            const int a_old = old_of(e), a_new = new_of(e);
            move(a_old, a_new, new_of(e2), v);
            move(a_old, a_new, old_of(e2), -v);
        }
        if (ext) {
            const long long vl = (long long)Jint[(int64_t)col_of(e) * n + col_of(e2)] - JBIAS;
            if (vl != 0) {
                const int a_old = old_of(e), a_new = new_of(e);
                move_in(Flo, a_old, a_new, new_of(e2), vl);
                move_in(Flo, a_old, a_new, old_of(e2), -vl);
            }
        }
    }
    __syncthreads();
    Fg[tid] = Frow[tid];
    if (ext) Fgl[tid] = Flo[tid];
    for (int e = tid; e < cnt; e += MG_WAVES * 64) qp[list[e]] = qn[list[e]];
}

__device__ __forceinline__ void lds_add(double* p, double v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_add(long long* p, long long v) {
    (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <typename WHT>
__global__ __launch_bounds__(64) void t_solve_kernel(const long long* __restrict__ Mpart, const long long* __restrict__ Mpart_lo,
                                                     const TPrep* __restrict__ prep, const int* __restrict__ hdiag_int,
                                                     const int* __restrict__ hdiag_j, const WHT* __restrict__ WH,
                                                     const double* __restrict__ wHw, const uint8_t* __restrict__ Q, int m,
                                                     int n, int V, double rcond, float* __restrict__ T_out,
                                                     float* __restrict__ A_out, float* __restrict__ b_out,
                                                     double* __restrict__ loss_rows, int nparts,
                                                     long long* __restrict__ changed_reset, int allow_fast,
                                                     const int* __restrict__ rowlist, const int* __restrict__ nrows) {
    // the change counter of this iteration has been consumed by the kernels in front of this one: leave it zero for
    // the next iteration's q_diff_kernel (saves a memset launch per iteration)
    if (changed_reset && blockIdx.x == 0 && threadIdx.x == 0) *changed_reset = 0;
    __shared__ double As[4][16][JS];
    __shared__ double Es[4][16][JS];
    __shared__ double A0[4][16][JS];       // unrounded A (for the loss), also scratch for the bucket sums
    __shared__ long long Di[4][16][JS];    // lane-private integer buckets of diag(H), then scratch for the transpose
    // the same for the extension word: aliases Es, which is first written after the bucket sums have been consumed
    long long(*Dj)[16][JS] = reinterpret_cast<long long(*)[16][JS]>(&Es[0][0][0]);
    __shared__ double CS[4][8][2];
    __shared__ double Coef[4][16];

    const int lane = threadIdx.x & 63;
    const int rs = lane >> 4, l = lane & 15;
    // rowlist (iterations >= 1 of the fused loop): only the rows whose indices changed in this iteration are solved -- an unchanged row has
    // the same bucket sums and the same b, hence the same codebook and loss, which stay where they are (T_out is then the previous
    // codebook array, updated in place).  The row's work is dominated by streaming its 32 KB of W H, so the kernel's time follows
    // the number of listed rows.
    int row = blockIdx.x * 4 + rs;
    if (rowlist) {
        const int cnt = *nrows;
        if ((int)blockIdx.x * 4 >= cnt) return;  // (uniform; behind the counter reset above)
        row = row < cnt ? rowlist[row] : m;      // surplus row slots of the last workgroup: compute a valid row, store nothing
    }
    const int rowc = min(row, m - 1);
    double(*A)[JS] = As[rs];
    double(*E)[JS] = Es[rs];
    double(*B0)[JS] = A0[rs];
    const double scale = prep->scale;
    const bool ext = prep->ext != 0;  // uniform

    // ---- b_i[a] = sum_{u in a} WH[row][u] and D[a] = sum_{u in a} H[u][u]: lane l takes u = 16 t + l into its own
    //      16 buckets (no atomics), then lane a sums bucket a over the lanes in fixed order
#pragma unroll
    for (int a = 0; a < 16; ++a) {
        B0[l][a] = 0.0;
        Di[rs][l][a] = 0;
        Dj[rs][l][a] = 0;
    }
    {
        const uint8_t* q = Q + (int64_t)rowc * n;
        const WHT* wh = WH + (int64_t)rowc * n;
        // whole blocks of KB x 16 columns: unconditional loads, all of a block's requests sent before its first element is
        // used -- the wave is alone on its SIMD, a block is one trip to L2 (blocks of 8 elements per lane: 32 trips in a row at
        // n = 4096, half of this kernel's time; 32 elements: 8)
        auto blocks = [&](auto kb_tag, int u_begin, int count) {
            constexpr int KB = decltype(kb_tag)::value;
            for (int blk = 0; blk < count; ++blk) {
                const int u0 = u_begin + blk * (16 * KB) + l;
                int av[KB], hv[KB];
                double wv8[KB];
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    av[k] = min((int)q[u0 + 16 * k], 15);
                    wv8[k] = (double)wh[u0 + 16 * k];
                    hv[k] = hdiag_int[u0 + 16 * k];
                }
                // LDS atomics without a return value instead of read-modify-write: a `+=` on a bucket is a dependent LDS round
                // trip per element (two buckets may be the same one, so the compiler keeps them in order); ds_add_f64 /
                // ds_add_u64 are sent off in program order -- the LDS executes a wave's operations in order, so every bucket
                // still sums its elements in ascending column order, the same bits as before
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    lds_add(&B0[l][av[k]], wv8[k]);
                    lds_add(&Di[rs][l][av[k]], (long long)hv[k]);
                }
            }
        };
        const int nbig = n / 512, nfull = (n - nbig * 512) / 128;
        blocks(std::integral_constant<int, 32>{}, 0, nbig);
        blocks(std::integral_constant<int, 8>{}, nbig * 512, nfull);
        for (int u = nbig * 512 + nfull * 128 + l; u < n; u += 16) {
            const int a = min((int)q[u], 15);
            lds_add(&B0[l][a], (double)wh[u]);
            lds_add(&Di[rs][l][a], (long long)hdiag_int[u]);
        }
        if (ext)
            for (int u = l; u < n; u += 16) lds_add(&Dj[rs][l][min((int)q[u], 15)], (long long)hdiag_j[u]);
    }
    wave_sync();
    double bsum = 0.0;
    long long dsum = 0, dsum_lo = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        bsum += B0[k][l];
        dsum += Di[rs][k][l];
        dsum_lo += Dj[rs][k][l];
    }
    wave_sync();

    // ---- A = M + M^T + diag  (exact integers), lane l owns column l ----
    long long col[16];
#pragma unroll
    for (int a = 0; a < 16; ++a) col[a] = 0;
    const bool sym_in = nparts == 0;  // Mpart is already F = M + M^T (one part)
    for (int p = 0; p < (sym_in ? 1 : nparts); ++p) {
        const long long* src = Mpart + ((int64_t)p * m + rowc) * 256;
#pragma unroll
        for (int a = 0; a < 16; ++a) col[a] += src[a * 16 + l];
    }
#pragma unroll
    for (int a = 0; a < 16; ++a) Di[rs][a][l] = col[a];
    if (ext) {  // the extension word's sums, same layout
#pragma unroll
        for (int a = 0; a < 16; ++a) col[a] = 0;
        for (int p = 0; p < (sym_in ? 1 : nparts); ++p) {
            const long long* src = Mpart_lo + ((int64_t)p * m + rowc) * 256;
#pragma unroll
            for (int a = 0; a < 16; ++a) col[a] += src[a * 16 + l];
        }
#pragma unroll
        for (int a = 0; a < 16; ++a) Dj[rs][a][l] = col[a];
    }
    wave_sync();
    double colA[16], colA0[16];
#pragma unroll
    for (int a = 0; a < 16; ++a) {
        long long x = sym_in ? Di[rs][a][l] : Di[rs][a][l] + Di[rs][l][a];
        if (a == l) x += dsum;
        double xd = (double)x;
        if (ext) {
            long long xl = sym_in ? Dj[rs][a][l] : Dj[rs][a][l] + Dj[rs][l][a];
            if (a == l) xl += dsum_lo;
            xd += (double)xl * EXT_UNIT;
        }
        colA0[a] = scale * xd;
        colA[a] = (double)(float)colA0[a];  // the reference holds A and b in fp32
    }
    const double bl0 = bsum;
    const double bl = (double)(float)bsum;
    wave_sync();
#pragma unroll
    for (int a = 0; a < 16; ++a) {
        A[a][l] = colA[a];
        B0[a][l] = colA0[a];
        E[a][l] = (a == l) ? 1.0 : 0.0;
    }
    if (row < m) {
        if (A_out && l < V)
            for (int a = 0; a < V; ++a) A_out[((int64_t)row * V + a) * V + l] = (float)colA[a];
        if (b_out && l < V) b_out[(int64_t)row * V + l] = (float)bl;
    }
    wave_sync();

    // ---- fast path.  gelsd keeps every singular value larger than rcond * sigma_max; when the row's A is positive
    //      definite with  sigma_min >= 1 / ||L^-1||_F^2  >  4 rcond trace(A) >= 4 rcond sigma_max  (a guaranteed bound
    //      from its Cholesky factor), nothing is cut off and the minimum-norm solution is simply A^-1 b.  Then
    //      t = L^-T (L^-1 b) needs 16 pivots instead of ~60 Jacobi rounds.  All in registers: lane l owns row l of L and
    //      column l of L^-1, values travel by 16-lane shuffles.  Rows with an unused code (a zero pivot), a tiny
    //      pivot or a large inverse take the Jacobi path below (the other rows of their wave walk through it with them and
    //      keep their own result).
    double x = 0.0;
    bool fast = false;
    if (allow_fast) {
        double r[16];
#pragma unroll
        for (int a = 0; a < 16; ++a) r[a] = (l < V && a < V) ? colA[a] : ((a == l) ? 1.0 : 0.0);  // A[l][a] (symmetric)
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const double dk = __shfl(r[k], k, 16);
            ok = ok && (dk > 0.0);
            const double sk = sqrt(dk);
            const double lk = (l == k) ? sk : r[k] / sk;  // L[l][k] for l >= k
            r[k] = lk;
#pragma unroll
            for (int j = k + 1; j < 16; ++j) r[j] -= lk * __shfl(lk, j, 16);  // A[l][j] -= L[l][k] L[j][k]
        }
        double xc[16], yv[16];  // column l of L^-1; y = L^-1 b (every lane holds all of it)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            double sx = (i == l) ? 1.0 : 0.0;
            double sy = __shfl(bl, i, 16);
#pragma unroll
            for (int j = 0; j < i; ++j) {
                const double lij = __shfl(r[j], i, 16);
                sx -= lij * xc[j];
                sy -= lij * yv[j];
            }
            const double lii = __shfl(r[i], i, 16);
            xc[i] = sx / lii;
            yv[i] = sy / lii;
        }
        double n2 = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            n2 += xc[i] * xc[i];
            x += xc[i] * yv[i];  // t_l = (L^-T y)_l = sum_i L^-1[i][l] y_i
        }
        const double inv_norm2 = row16_sum(l < V ? n2 : 0.0);     // ||L^-1||_F^2 >= 1 / sigma_min(A)
        const double tr = row16_sum(l < V ? colA[l] : 0.0);       // trace(A) >= sigma_max(A)
        fast = ok && (4.0 * rcond * tr * inv_norm2 < 1.0);  // false for NaN; decided per row: a row's result must not
                                                             // depend on which rows share its wave
    }
    const double x_fast = x;
    if (!__all(fast)) {
        // ---- round-robin Jacobi: 15 rounds of 8 disjoint rotations per sweep ----
        const int t = l >> 1;  // pair handled (redundantly) by lanes 2t, 2t+1
        for (int sweep = 0; sweep < GANQ_JACOBI_SWEEPS; ++sweep) {
            double off = 0.0, dg = 0.0;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const double x = A[l][j];
                if (j == l) dg += x * x; else off += x * x;
            }
            off = row16_sum(off);
            dg = row16_sum(dg);
            // squared off-diagonal mass below 1e-22 of the diagonal's: the eigenvalues are then converged to ~1e-22 relative
            // (second order), the eigenvectors to ~1e-11 -- six orders below what the fp32 codebook keeps
            const bool done = (off <= 1e-22 * dg) || (off == 0.0);
            if (__all(done)) break;
            for (int r = 0; r < 15; ++r) {
                int p, q;
                if (t == 0) {
                    p = r;
                    q = 15;
                } else {
                    const int x = (r + t) % 15, y = (r - t + 15) % 15;
                    p = min(x, y);
                    q = max(x, y);
                }
                const double apq = A[p][q], app = A[p][p], aqq = A[q][q];
                double cc = 1.0, ss = 0.0;
                if (apq != 0.0 && !done) {
                    // t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)) with theta = alpha / apq, written without forming theta:
                    // t = sgn(alpha) apq / (|alpha| + hypot(alpha, apq))  -- one division and one square root fewer
                    const double alpha = 0.5 * (aqq - app);
                    const double rr = sqrt(alpha * alpha + apq * apq);
                    const double tt = (alpha >= 0.0 ? apq : -apq) / (fabs(alpha) + rr);
                    cc = 1.0 / sqrt(tt * tt + 1.0);
                    ss = tt * cc;
                }
                if ((l & 1) == 0) {
                    CS[rs][t][0] = cc;
                    CS[rs][t][1] = ss;
                }
                wave_sync();
                // column phase: lane l rotates row l's entries (p_i, q_i) for all 8 pairs
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    int pi, qi;
                    if (i == 0) { pi = r; qi = 15; } else {
                        const int x = (r + i) % 15, y = (r - i + 15) % 15;
                        pi = min(x, y); qi = max(x, y);
                    }
                    const double ci = CS[rs][i][0], si = CS[rs][i][1];
                    const double akp = A[l][pi], akq = A[l][qi];
                    A[l][pi] = ci * akp - si * akq;
                    A[l][qi] = si * akp + ci * akq;
                    const double ekp = E[l][pi], ekq = E[l][qi];
                    E[l][pi] = ci * ekp - si * ekq;
                    E[l][qi] = si * ekp + ci * ekq;
                }
                wave_sync();
                // row phase: lane l rotates column l's entries of rows (p_i, q_i)
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    int pi, qi;
                    if (i == 0) { pi = r; qi = 15; } else {
                        const int x = (r + i) % 15, y = (r - i + 15) % 15;
                        pi = min(x, y); qi = max(x, y);
                    }
                    const double ci = CS[rs][i][0], si = CS[rs][i][1];
                    const double apk = A[pi][l], aqk = A[qi][l];
                    A[pi][l] = ci * apk - si * aqk;
                    A[qi][l] = si * apk + ci * aqk;
                }
                wave_sync();
            }
        }

        // ---- minimum-norm solution: x = sum_k [|lam_k| > rcond * lam_max] (e_k . b / lam_k) e_k ----
        const double lam = A[l][l];
        const double lmax = row16_max(fabs(lam));
        Coef[rs][l] = bl;
        wave_sync();
        double proj = 0.0;
#pragma unroll
        for (int a = 0; a < 16; ++a) proj += E[a][l] * Coef[rs][a];
        wave_sync();
        const bool keep = fabs(lam) > rcond * lmax;
        Coef[rs][l] = keep ? proj / lam : 0.0;
        wave_sync();
        x = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) x += E[l][k] * Coef[rs][k];
    }
    if (fast) x = x_fast;
    const float tl = (float)x;
    if (row < m && l < V) T_out[(int64_t)row * V + l] = tl;

    // ---- loss of this row with the NEW codebook: w^T H w - 2 t^T b + t^T A t (fp64, unrounded A and b) ----
    if (loss_rows) {
        const double td = (l < V) ? (double)tl : 0.0;
        wave_sync();
        Coef[rs][l] = td;
        wave_sync();
        double at = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) at += B0[l][k] * Coef[rs][k];  // (A t)_l, A symmetric
        const double term = row16_sum(td * at - 2.0 * td * bl0);
        if (row < m && l == 0) loss_rows[row] = wHw[row] + term;
    }
}

// w_i^T (W H)_i per row, fixed order
__global__ __launch_bounds__(256) void whw_kernel(const float* __restrict__ W, const double* __restrict__ WH64, int m, int n,
                                                 double* __restrict__ wHw) {
    __shared__ double sh[256];
    const int row = blockIdx.x;
    double s = 0.0;
    for (int u = threadIdx.x; u < n; u += 256) s += (double)W[(int64_t)row * n + u] * WH64[(int64_t)row * n + u];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) wHw[row] = sh[0];
}

__global__ __launch_bounds__(256) void sum_rows_kernel(const double* __restrict__ rows, int m, double* __restrict__ out) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < m; i += 256) s += rows[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sh[0];
}

// ---------------------------------------------------------------------------------------------------------------
// fp64 GEMM C[M,N] = A[M,K] (fp32, widened on load) @ B[K,N] (fp64) on v_mfma_f64_16x16x4_f64; used once per layer
// for W @ H_fixed.  64x64 tile, 4 waves x (2x2 tiles of 16x16), K slabs of 16 through LDS.
// C[M,N] (fp64) = A[M,K] (fp32, widened) @ B[K,N] (fp64) on v_mfma_f64_16x16x4_f64.
// 128x128 tile per workgroup, 4 waves of 64x64 (4x4 MFMA tiles: 8 LDS reads per 16 MFMAs), 16-deep k slabs double
// buffered in LDS, the next slab's global loads in flight during the current slab's MFMAs.
constexpr int DM = 128, DN = 128, DK = 16;
constexpr int DPAD = 4;  // row pitch DM + 4 doubles: the 16 lanes x 4 k-rows of an operand read hit distinct banks

__global__ __launch_bounds__(256) void gemm_f64_kernel(const float* __restrict__ A, const double* __restrict__ B,
                                                      double* __restrict__ C, int M, int N, int K) {
    __shared__ double As[2][DK][DM + DPAD];
    __shared__ double Bs[2][DK][DN + DPAD];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tiles_n = (N + DN - 1) / DN;
    const int bm = (blockIdx.x / tiles_n) * DM, bn = (blockIdx.x % tiles_n) * DN;
    const int wm = (wv >> 1) * 64, wn = (wv & 1) * 64;
    f64x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f64x4){0.0, 0.0, 0.0, 0.0};

    // slab loads: A 128 rows x 16 k (fp32): thread -> row tid/2, 8 consecutive k; B 16 k x 128 cols (fp64): thread ->
    // k tid/16, 8 consecutive columns
    const int a_row = tid >> 1, a_k = (tid & 1) * 8;
    const int b_k = tid >> 4, b_col = (tid & 15) * 8;
    float ra[8];
    double rb[8];
    auto gload = [&](int k0) {
        const int row = bm + a_row;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = k0 + a_k + e;
            ra[e] = (row < M && k < K) ? A[(int64_t)row * K + k] : 0.0f;
        }
        const int kk = k0 + b_k;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int col = bn + b_col + e;
            rb[e] = (kk < K && col < N) ? B[(int64_t)kk * N + col] : 0.0;
        }
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int e = 0; e < 8; ++e) As[buf][a_k + e][a_row] = (double)ra[e];
#pragma unroll
        for (int e = 0; e < 8; ++e) Bs[buf][b_k][b_col + e] = rb[e];
    };
    gload(0);
    sstore(0);
    __syncthreads();
    const int nslab = (K + DK - 1) / DK;
    for (int sidx = 0; sidx < nslab; ++sidx) {
        const int buf = sidx & 1;
        if (sidx + 1 < nslab) gload((sidx + 1) * DK);
#pragma unroll
        for (int kk = 0; kk < DK; kk += 4) {
            const int kq = kk + (lane >> 4);
            double a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = As[buf][kq][wm + 16 * i + (lane & 15)];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = Bs[buf][kq][wn + 16 * j + (lane & 15)];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (sidx + 1 < nslab) sstore(buf ^ 1);
        __syncthreads();
    }
    // f64 C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = bm + wm + 16 * i + (lane >> 4) + 4 * r;
                const int col = bn + wn + 16 * j + (lane & 15);
                if (row < M && col < N) C[(int64_t)row * N + col] = acc[i][j][r];
            }
}

// ---------------------------------------------------------------------------------------------------------------
// option GANQ_WH_F64=1: W @ H_fixed by the fp64 GEMM instead of the split-fp16 product -- the A/B reference
static bool wh_use_f64_gemm() { return opt_get(OPT_WH_F64) == 1; }

TLayout t_layout(int64_t m, int64_t n, bool with_f64) {
    TLayout lo;
    lo.nq = (n + UT - 1) / UT * UT;
    lo.ng = (n + 63) / 64;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    };
    lo.off_prep = take(sizeof(TPrep));
    lo.off_planes = take((size_t)6 * n * lo.nq);  // 4 digit planes of I + 2 of the extension word J
    lo.off_hdiag = take((size_t)n * sizeof(int));
    lo.off_hdiag_j = take((size_t)n * sizeof(int));
    lo.off_bits = take((size_t)m * lo.ng * 16 * sizeof(unsigned long long));
    lo.off_mpart = take((size_t)NP * m * 256 * sizeof(long long));
    lo.off_mpart_lo = take((size_t)NP * m * 256 * sizeof(long long));
    lo.off_top3 = take((size_t)TOP_LIST_MAX * sizeof(uint2));  // exception lists: entries with a non-zero digit 3 / digit 2 or 3
    lo.off_top2 = take((size_t)TOP_LIST_MAX * sizeof(uint2));
    lo.off_mstate_lo = lo.off_jint = lo.off_dexp = lo.off_hdiag64 = 0;
    lo.off_h64 = lo.off_wh64 = lo.off_whw = lo.off_lossrows = 0;
    lo.off_hint = lo.off_qprev = lo.off_mstate = lo.off_chg = lo.off_chgcnt = 0;
    lo.off_wp = lo.off_hp = lo.off_rexp = lo.off_wlo = 0;
    lo.off_active = 0;
    lo.off_topoff = lo.off_topent = 0;
    if (with_f64) {
        lo.off_hint = take((size_t)n * n * sizeof(int));
        lo.off_qprev = take((size_t)m * n);
        lo.off_mstate = take((size_t)m * 256 * sizeof(long long));
        lo.off_mstate_lo = take((size_t)m * 256 * sizeof(long long));
        lo.off_jint = take((size_t)n * n * sizeof(short));
        lo.off_dexp = take((size_t)n * sizeof(int));
        lo.off_hdiag64 = take((size_t)n * sizeof(double));
        lo.off_chg = take((size_t)m * n * sizeof(uint16_t));
        lo.off_chgcnt = take((size_t)m * sizeof(int) + 64);  // counts per row, then the 8-byte total
        lo.off_active = take(((size_t)m + 1) * sizeof(int));  // rows that changed in the last iteration, their number
        lo.off_topoff = take(((size_t)n + 1) * sizeof(int));
        lo.off_topent = take((size_t)2 * TOP_LIST_MAX * sizeof(uint2));
        if (wh_use_f64_gemm()) {
            lo.off_h64 = take((size_t)n * n * sizeof(double));
        } else {
            const WhLayout wl = wh_layout(m, n);
            lo.off_wp = take(wl.wp_bytes);
            lo.off_hp = take(wl.hp_bytes);
            lo.off_rexp = take(wl.rexp_bytes);
            lo.off_wlo = take(wl.wlo_bytes);
        }
        lo.off_wh64 = take((size_t)m * n * sizeof(double));
        lo.off_whw = take((size_t)m * sizeof(double));
        lo.off_lossrows = take((size_t)m * sizeof(double));
    }
    lo.total = off;
    return lo;
}

__global__ __launch_bounds__(256) void hfixed_kernel(const int* __restrict__ Hint, const short* __restrict__ Jint,
                                                    const TPrep* __restrict__ prep, int64_t total, double* __restrict__ out) {
    const bool ext = prep->ext != 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
        out[i] = prep->scale * ((double)Hint[i] + (ext ? (double)((int)Jint[i] - JBIAS) * EXT_UNIT : 0.0));
}

// rows whose indices changed in this iteration (ascending) and their number.  A row without a change has reached a
// fixed point: its bucket sums, hence its codebook, hence its next indices repeat -- the S-solve skips it from now on.
__global__ __launch_bounds__(1024) void active_rows_kernel(const int* __restrict__ chgcnt, int m, int* __restrict__ list,
                                                           int* __restrict__ count) {
    __shared__ int wsum[16];
    __shared__ int carry_sh;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) carry_sh = 0;
    __syncthreads();
    for (int base = 0; base < m; base += 1024) {
        const int i = base + tid;
        const int v = (i < m && chgcnt[i] > 0) ? 1 : 0;
        int incl = v;
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        int before = carry_sh;
        for (int k = 0; k < wv; ++k) before += wsum[k];
        if (v) list[before + incl - 1] = i;
        __syncthreads();
        if (tid == 1023) carry_sh = before + incl;
        __syncthreads();
    }
    if (tid == 0) *count = carry_sh;
}

// once per layer: fixed-point planes of H (+ optionally W @ H_fixed in fp64 and w^T H w per row)
int t_prepare(const float* W, const float* H, int64_t m, int64_t n, const TLayout& lo, char* ws, bool with_f64,
              hipStream_t stream) {
    TPrep* prep = reinterpret_cast<TPrep*>(ws + lo.off_prep);
    int8_t* planes = reinterpret_cast<int8_t*>(ws + lo.off_planes);
    int* hdiag = reinterpret_cast<int*>(ws + lo.off_hdiag);
    int* hdiag_j = reinterpret_cast<int*>(ws + lo.off_hdiag_j);
    double* H64 = (with_f64 && lo.off_h64) ? reinterpret_cast<double*>(ws + lo.off_h64) : nullptr;
    ProfScope prof(KID_T_PREP, stream);
    GANQ_HIP_CHECK(hipMemsetAsync(prep, 0, sizeof(TPrep), stream));
    hipLaunchKernelGGL(absmax_kernel, dim3(512), dim3(256), 0, stream, H, n * n, prep);
    hipLaunchKernelGGL(prep_scale_kernel, dim3(1), dim3(256), 0, stream, H, (int)n, prep, (int)opt_get(OPT_H_EXT), top_cap_in_force(m, n));
    // runs of 1024 entries per workgroup: as many as leave about a thousand workgroups, 16 at the most
    const int64_t htiles = (n * lo.nq + 1023) / 1024;
    const int per_wg = (int)std::min<int64_t>(16, std::max<int64_t>(1, htiles / 1024));
    int* Hint = with_f64 ? reinterpret_cast<int*>(ws + lo.off_hint) : nullptr;
    short* Jint = with_f64 ? reinterpret_cast<short*>(ws + lo.off_jint) : nullptr;
    hipLaunchKernelGGL(hquant_kernel, dim3((unsigned)((htiles + per_wg - 1) / per_wg)), dim3(256), 0, stream, H, (int)n, (int)lo.nq, prep,
                       planes, hdiag, hdiag_j, H64, Hint, Jint, reinterpret_cast<uint2*>(ws + lo.off_top3),
                       reinterpret_cast<uint2*>(ws + lo.off_top2), per_wg);
    GANQ_LAUNCH_CHECK();
    // (not under GANQ_MU_TOP=0: the incremental sums then read all four planes and need no index; TPrep::mu_index stays zero)
    if (with_f64 && lo.off_topent && top_cap_in_force(m, n) >= 0 && opt_get(OPT_MU_TOP) != 0) {
        const size_t ilds = (size_t)n * sizeof(int);
        const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(top_index_kernel), ilds);
        if (rc) return rc;
        hipLaunchKernelGGL(top_index_kernel, dim3(1), dim3(1024), ilds, stream, reinterpret_cast<const uint2*>(ws + lo.off_top3),
                           reinterpret_cast<const uint2*>(ws + lo.off_top2), prep, (int)n, reinterpret_cast<int*>(ws + lo.off_topoff),
                           reinterpret_cast<uint2*>(ws + lo.off_topent), (int)opt_get(OPT_MU_TOP));
        GANQ_LAUNCH_CHECK();
    }
    if (with_f64) {
        // change counter of the incremental bucket sums: zero once, every t_solve leaves it zero again
        GANQ_HIP_CHECK(hipMemsetAsync(ws + lo.off_chgcnt + align_up((size_t)m * sizeof(int), 8), 0, sizeof(long long), stream));
        double* WH64 = reinterpret_cast<double*>(ws + lo.off_wh64);
        double* wHw = reinterpret_cast<double*>(ws + lo.off_whw);
        const int tiles = (int)(((m + DM - 1) / DM) * ((n + DN - 1) / DN));
        if (H64) {
            hipLaunchKernelGGL(gemm_f64_kernel, dim3(tiles), dim3(256), 0, stream, W, H64, WH64, (int)m, (int)n, (int)n);
        } else {
            const WhLayout wl = wh_layout(m, n);
            int* dexp = reinterpret_cast<int*>(ws + lo.off_dexp);
            double* hdiag64 = reinterpret_cast<double*>(ws + lo.off_hdiag64);
            hipLaunchKernelGGL(dexp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, hdiag, hdiag_j, prep, (int)n, dexp,
                               hdiag64);
            int rc = wh_gemm(W, Hint, Jint, &prep->ext, dexp, hdiag64, &prep->scale, m, n, wl, ws + lo.off_wp, ws + lo.off_hp,
                             reinterpret_cast<int*>(ws + lo.off_rexp), reinterpret_cast<int*>(ws + lo.off_wlo), WH64, stream);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(whw_kernel, dim3((unsigned)m), dim3(256), 0, stream, W, WH64, (int)m, (int)n, wHw);
        GANQ_LAUNCH_CHECK();
    }
    return 0;
}

// per iteration: bucket sums (full: masks -> integer accumulation; or incremental) -> per-row solve (+ loss rows)
int t_iterate(const uint8_t* Q, int64_t m, int64_t n, int V, double rcond, const TLayout& lo, char* ws, const float* WH32,
              float* T_out, float* A_out, float* b_out, int loss_mode, double* loss_out, int iter, hipStream_t stream, bool changed_rows_only) {
    TPrep* prep = reinterpret_cast<TPrep*>(ws + lo.off_prep);
    int8_t* planes = reinterpret_cast<int8_t*>(ws + lo.off_planes);
    int* hdiag = reinterpret_cast<int*>(ws + lo.off_hdiag);
    int* hdiag_j = reinterpret_cast<int*>(ws + lo.off_hdiag_j);
    unsigned long long* bits = reinterpret_cast<unsigned long long*>(ws + lo.off_bits);
    long long* mpart = reinterpret_cast<long long*>(ws + lo.off_mpart);
    long long* mpart_lo = reinterpret_cast<long long*>(ws + lo.off_mpart_lo);
    // test switches (runtime.hip): GANQ_T_FULL=1 -> stateless full accumulation every call; GANQ_T_INCR_THR=<count> ->
    // device-side fallback threshold (changed indices per layer) instead of m*n/16
    const long long opt_thr = opt_get(OPT_T_INCR_THR);
    const bool stateful = iter >= 0 && lo.off_hint != 0 && opt_get(OPT_T_FULL) != 1;
    long long* mstate = stateful ? reinterpret_cast<long long*>(ws + lo.off_mstate) : nullptr;
    long long* mstate_lo = stateful ? reinterpret_cast<long long*>(ws + lo.off_mstate_lo) : nullptr;
    uint8_t* qprev = stateful ? reinterpret_cast<uint8_t*>(ws + lo.off_qprev) : nullptr;
    int* chgcnt = stateful ? reinterpret_cast<int*>(ws + lo.off_chgcnt) : nullptr;
    long long* changed = stateful ? reinterpret_cast<long long*>(ws + lo.off_chgcnt + align_up((size_t)m * sizeof(int), 8)) : nullptr;
    // more than 1/16 of all indices changed: the full accumulation is cheaper (decided on the device, no host sync)
    const long long thr = opt_thr >= 0 ? opt_thr : (long long)((m * n) >> 4);
    // From the second incremental iteration on the device-side fallback is not even launched (three launches that find the gate shut:
    // 14 us per iteration): the changes shrink from iteration to iteration (the incremental kernel's time on the benchmark layer:
    // 233, 135, 115, 96, 81, 60 .. us), and if a layer ever did change more than 1/16 of its indices that late, the incremental
    // update is still exact -- just slower than the full pass would have been.  (A forced threshold, GANQ_T_INCR_THR, keeps the gate.)
    const bool gated = !(stateful && iter >= 2 && opt_thr < 0);
    const long long* gate = nullptr;  // null: the full path runs unconditionally
    if (stateful && iter > 0) {
        ProfScope prof(KID_T_INCR, stream);
        uint16_t* chg = reinterpret_cast<uint16_t*>(ws + lo.off_chg);
        hipLaunchKernelGGL(q_diff_kernel, dim3((unsigned)((m + QD_WAVES - 1) / QD_WAVES)), dim3(QD_WAVES * 64), 0, stream, Q, qprev, (int)m, (int)n, chg, chgcnt,
                           changed);
        const size_t usmem = (size_t)(256 + MU_WAVES * 16 * 64) * sizeof(long long) + align_up((size_t)n, 16);
        const bool mu_lds = opt_get(OPT_MUPDATE_LDS) == 1;  // A/B switch
        const int* Hint = reinterpret_cast<const int*>(ws + lo.off_hint);
        const short* Jint = reinterpret_cast<const short*>(ws + lo.off_jint);
        if ((n & 15) == 0 && !mu_lds)
            hipLaunchKernelGGL(m_update_mfma_kernel, dim3((unsigned)m), dim3(MG_WAVES * 64), 0, stream, planes, Hint, Jint, hdiag,
                               hdiag_j, Q, qprev, (int)m, (int)n, (int)lo.nq, chg, chgcnt, mstate, mstate_lo, changed, gated ? thr : LLONG_MAX, prep,
                               reinterpret_cast<const int*>(ws + lo.off_topoff), reinterpret_cast<const uint2*>(ws + lo.off_topent),
                               (int)opt_get(OPT_MU_TOP));
        else {
            int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(m_update_kernel<int>), usmem);
            if (!rc) rc = ensure_dynamic_lds(reinterpret_cast<const void*>(m_update_kernel<short>), usmem);
            if (rc) return rc;
            // the extension word first (it needs the old codes; leaves at once when the extension is off), then the
            // 31-bit word, which also brings Qprev up to date
            hipLaunchKernelGGL(m_update_kernel<short>, dim3((unsigned)m), dim3(MU_WAVES * 64), usmem, stream, Jint, Q, qprev, (int)m,
                               (int)n, chg, chgcnt, mstate_lo, changed, gated ? thr : LLONG_MAX, prep);
            hipLaunchKernelGGL(m_update_kernel<int>, dim3((unsigned)m), dim3(MU_WAVES * 64), usmem, stream, Hint, Q, qprev, (int)m,
                               (int)n, chg, chgcnt, mstate, changed, gated ? thr : LLONG_MAX, prep);
        }
        GANQ_LAUNCH_CHECK();
        gate = changed;
    }
    if (gated) {
        ProfScope prof(KID_SORT_CODES, stream);
        const int64_t items = m * lo.ng;
        hipLaunchKernelGGL(code_masks_kernel, dim3((unsigned)std::min<int64_t>((items + 3) / 4, 4096)), dim3(256), 0, stream, Q, (int)m, (int)n,
                           (int)lo.ng, bits, gate, thr);
    }
    GANQ_LAUNCH_CHECK();
    const size_t smem = 2 * (size_t)btile_bytes(4) + (size_t)TW * RW * 256 * sizeof(long long);  // (the extension's two planes need less)
    const bool w4 = accum_plan(m, n) == 1;
    {
        const int rc = w4 ? ensure_dynamic_lds(reinterpret_cast<const void*>(onehot_accum_w4_kernel), W4_LDS)
                          : ensure_dynamic_lds(reinterpret_cast<const void*>(onehot_accum_kernel), smem);
        if (rc) return rc;
    }
    if (gated) {
        ProfScope prof(KID_SHT_ACCUM, stream);
        const int nrg = (int)((m + TR - 1) / TR);
        const bool dbg = opt_get(OPT_ACCUM_DEBUG) == 1;  // developer timing experiment
        long long* stamps = nullptr;
        if (dbg) (void)hipMalloc(&stamps, 64);
        if (w4) {  // (32 rows per workgroup as well: the same grid)
            hipLaunchKernelGGL(onehot_accum_w4_kernel, dim3((unsigned)(2 * nrg * NP)), dim3(256), W4_LDS, stream, planes, bits, Q, (int)m, (int)n,
                               (int)lo.nq, (int)lo.ng, mpart, mpart_lo, stamps, gate, thr, prep, nrg * NP);
            // the digit planes it left to the lists (leaves at once when it summed all four)
            hipLaunchKernelGGL(top_fixup_kernel, dim3((unsigned)m), dim3(256), 256 * sizeof(long long) + (size_t)n, stream,
                               reinterpret_cast<const uint2*>(ws + lo.off_top3), reinterpret_cast<const uint2*>(ws + lo.off_top2), Q, (int)m,
                               (int)n, mpart, gate, thr, prep);
        } else
            hipLaunchKernelGGL(onehot_accum_kernel, dim3((unsigned)(2 * nrg * NP)), dim3(TW * 64), smem, stream, planes, bits, Q, (int)m, (int)n,
                               (int)lo.nq, (int)lo.ng, mpart, mpart_lo, stamps, gate, thr, prep, nrg * NP);
        if (stamps) {
            long long h[3];
            (void)hipStreamSynchronize(stream);
            (void)hipMemcpy(h, stamps, 24, hipMemcpyDeviceToHost);
            (void)hipFree(stamps);
            fprintf(stderr, "[onehot_accum%s stamps] wg0 wave0: prologue %lld, tile loop %lld, flush %lld cycles\n", w4 ? "_w4" : "", h[0], h[1], h[2]);
        }
        if (stateful) {
            hipLaunchKernelGGL(m_reduce_kernel, dim3(1024 + 256), dim3(256), 0, stream, mpart, mpart_lo, (int)m, mstate, mstate_lo, Q, qprev,
                               m * n, gate, thr, prep, 1024);
        }
    }
    GANQ_LAUNCH_CHECK();
    // changed_rows_only (the fused loop, iterations >= 1, T_out = the previous codebooks): the per-row solve runs on the rows that
    // changed in this iteration only; the list is the one the next S-solve takes as well (t_active_rows hands it out without a
    // second launch)
    const int* rowlist = nullptr;
    const int* rowcount = nullptr;
    if (changed_rows_only && stateful && iter >= 1 && t_rows_listable(lo)) {
        int* l = reinterpret_cast<int*>(ws + lo.off_active);
        hipLaunchKernelGGL(active_rows_kernel, dim3(1), dim3(1024), 0, stream, chgcnt, (int)m, l, l + m);
        rowlist = l;
        rowcount = l + m;
    }
    {
        ProfScope prof(KID_T_SOLVE, stream);
        const dim3 grid((unsigned)((m + 3) / 4));
        const int allow_fast = opt_get(OPT_T_JACOBI) != 1;  // test switch: 1 -> every row by the Jacobi eigen-solve
        const long long* msrc = stateful ? mstate : mpart;
        const long long* msrc_lo = stateful ? mstate_lo : mpart_lo;
        const int nparts = stateful ? 0 : NP;  // 0: one part that is already symmetric
        if (WH32) {
            hipLaunchKernelGGL(t_solve_kernel<float>, grid, dim3(64), 0, stream, msrc, msrc_lo, prep, hdiag, hdiag_j, WH32,
                               static_cast<const double*>(nullptr), Q, (int)m, (int)n, V, rcond, T_out, A_out, b_out,
                               static_cast<double*>(nullptr), nparts, static_cast<long long*>(nullptr), allow_fast,
                               static_cast<const int*>(nullptr), static_cast<const int*>(nullptr));
        } else {
            const double* WH64 = reinterpret_cast<const double*>(ws + lo.off_wh64);
            const double* wHw = reinterpret_cast<const double*>(ws + lo.off_whw);
            double* loss_rows = reinterpret_cast<double*>(ws + lo.off_lossrows);
            hipLaunchKernelGGL(t_solve_kernel<double>, grid, dim3(64), 0, stream, msrc, msrc_lo, prep, hdiag, hdiag_j, WH64, wHw, Q, (int)m,
                               (int)n, V, rcond, T_out, A_out, b_out, loss_mode ? loss_rows : nullptr, nparts, changed, allow_fast, rowlist, rowcount);
            if (loss_mode == 2) hipLaunchKernelGGL(sum_rows_kernel, dim3(1), dim3(256), 0, stream, loss_rows, (int)m, loss_out);
        }
    }
    GANQ_LAUNCH_CHECK();
    return 0;
}

// after t_iterate(iter >= 1): device list / count of the rows that changed in that iteration (null when the bucket sums
// are not kept between iterations, i.e. no change lists exist)
bool t_rows_listable(const TLayout& lo) {
    // GANQ_SOLVE_ALL_ROWS=1 (test switch): never skip a row; GANQ_T_FULL=1: no change lists exist
    return lo.off_hint != 0 && lo.off_active != 0 && opt_get(OPT_T_FULL) != 1 && opt_get(OPT_SOLVE_ALL_ROWS) != 1;
}

int t_active_rows(int64_t m, const TLayout& lo, char* ws, const int** list, const int** count, hipStream_t stream, bool already_built) {
    *list = nullptr;
    *count = nullptr;
    if (!t_rows_listable(lo)) return 0;
    int* l = reinterpret_cast<int*>(ws + lo.off_active);
    int* c = l + m;
    if (!already_built)
        hipLaunchKernelGGL(active_rows_kernel, dim3(1), dim3(1024), 0, stream, reinterpret_cast<const int*>(ws + lo.off_chgcnt), (int)m, l, c);
    GANQ_LAUNCH_CHECK();
    *list = l;
    *count = c;
    return 0;
}

}  // namespace ganq

using namespace ganq;

// tests: which kernel the full accumulation of an [m, n] layer takes under the current options (host only)
extern "C" int ganq_debug_accum_plan(int64_t m, int64_t n, int* out) {
    if (!out) return fail(-3, "ganq_debug_accum_plan: null pointer");
    if (m <= 0 || n <= 0) return fail(-1, "ganq_debug_accum_plan: bad shape");
    out[0] = accum_plan(m, n);
    out[1] = accum_w4_supported(m, n) ? 1 : 0;
    return 0;
}

// tests: how many digit planes the four-wave kernel would sum densely for an [m, n] layer whose H has c3 / c2 exceptions, under the
// current options (host only: top_dense_planes is the function the kernels evaluate).  out: D, the cap in force, TOP_LIST_MAX
extern "C" int ganq_debug_top_rule(int64_t m, int64_t n, long long c3, long long c2, int* out) {
    if (!out) return fail(-3, "ganq_debug_top_rule: null pointer");
    if (m <= 0 || n <= 0 || c3 < 0 || c2 < c3) return fail(-1, "ganq_debug_top_rule: bad shape / counts");
    const int cap = top_cap_in_force(m, n);
    out[0] = top_dense_planes(c3, c2, cap);
    out[1] = cap;
    out[2] = TOP_LIST_MAX;
    return 0;
}

// tests: how many digit planes the incremental bucket sums on the matrix cores read for an [m, n] layer whose H has c3 / c2 exceptions,
// under the current options (host only: mu_dense_planes is the function the kernel evaluates).  out: its D, the full sum's D
extern "C" int ganq_debug_mu_planes(int64_t m, int64_t n, long long c3, long long c2, int* out) {
    if (!out) return fail(-3, "ganq_debug_mu_planes: null pointer");
    if (m <= 0 || n <= 0 || c3 < 0 || c2 < c3) return fail(-1, "ganq_debug_mu_planes: bad shape / counts");
    const int cap = top_cap_in_force(m, n);
    out[0] = mu_dense_planes(c3, c2, cap, (int)opt_get(OPT_MU_TOP));
    out[1] = top_dense_planes(c3, c2, cap);
    return 0;
}

// tests, sweeps: the exception counts of H as t_prepare forms them for an [m, n] layer.  out (host, 5 values): c3, c2, the cap in
// force (< 0: no list is wanted), TOP_LIST_MAX, D
extern "C" int ganq_debug_top_planes(const float* H, int64_t n, int64_t m, long long* out, void* stream_) {
    if (!H || !out) return fail(-3, "ganq_debug_top_planes: null pointer");
    if (m <= 0 || n <= 0 || m > INT32_MAX / 2 || n > INT32_MAX / 2) return fail(-1, "ganq_debug_top_planes: bad shape");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const TLayout lo = t_layout(m, n, false);
    char* ws = nullptr;
    GANQ_HIP_CHECK(hipMalloc(&ws, lo.total));
    int rc = t_prepare(nullptr, H, m, n, lo, ws, false, stream);
    TPrep h;
    if (rc == 0) {
        hipError_t e = hipMemcpyAsync(&h, ws + lo.off_prep, sizeof(TPrep), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) rc = fail(-4, "ganq_debug_top_planes: %s", hipGetErrorString(e));
    }
    if (rc != 0) (void)hipDeviceSynchronize();
    (void)hipFree(ws);
    if (rc) return rc;
    out[0] = h.c3;
    out[1] = h.c2;
    out[2] = h.top_cap;
    out[3] = TOP_LIST_MAX;
    out[4] = top_dense_planes(h.c3, h.c2, h.top_cap);
    return 0;
}

// developer check (tests): the W @ H_fixed product of the fused driver and the fixed-point H it was formed with
extern "C" int ganq_debug_wh_product(const float* W, const float* H, int64_t m, int64_t n, double* WH_out, double* Hfixed_out,
                                     void* stream_) {
    if (m <= 0 || n <= 0 || m > INT32_MAX / 2 || n > INT32_MAX / 2) return fail(-1, "ganq_debug_wh_product: bad shape");
    if (!W || !H || !WH_out) return fail(-3, "ganq_debug_wh_product: null pointer");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const TLayout lo = t_layout(m, n, true);
    char* ws = nullptr;
    GANQ_HIP_CHECK(hipMalloc(&ws, lo.total));
    int rc = t_prepare(W, H, m, n, lo, ws, true, stream);
    if (rc == 0) {
        hipError_t e = hipMemcpyAsync(WH_out, ws + lo.off_wh64, (size_t)m * n * sizeof(double), hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess && Hfixed_out) {
            const int* Hint = reinterpret_cast<const int*>(ws + lo.off_hint);
            const short* Jint = reinterpret_cast<const short*>(ws + lo.off_jint);
            hipLaunchKernelGGL(hfixed_kernel, dim3(1024), dim3(256), 0, stream, Hint, Jint,
                               reinterpret_cast<const TPrep*>(ws + lo.off_prep), n * n, Hfixed_out);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) rc = fail(-4, "ganq_debug_wh_product: %s", hipGetErrorString(e));
    }
    (void)hipFree(ws);
    return rc;
}

namespace ganq {
// No bucket sum reaches this value (|sum| <= n^2 2^30 <= 2^58 at n <= 16384): written into the first partial sum before an
// iteration, it is still there afterwards exactly when the full accumulation did not run.
constexpr long long T_FULL_PROBE = LLONG_MIN;

__global__ __launch_bounds__(256) void jint_unbias_kernel(const short* __restrict__ Jint, int64_t total, int* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) out[i] = (int)Jint[i] - JBIAS;
}
__global__ void t_probe_set_kernel(long long* mpart) { mpart[0] = T_FULL_PROBE; }
__global__ void t_probe_get_kernel(const long long* __restrict__ mpart, int* __restrict__ full_ran) {
    *full_ran = mpart[0] != T_FULL_PROBE ? 1 : 0;
}

// body of ganq_debug_t_sums on its own scratch `ws` (layout lo) and codebook buffers Tc / Tn [m,V]
static int debug_t_sums_run(const float* W, const float* H, const uint8_t* Qseq, int64_t m, int64_t n, int V, int K, double rcond,
                            const TLayout& lo, char* ws, float* Tc, float* Tn, double* scale_out, int* ext_out, int* Hint_out,
                            int* J_out, int* hdiag_int_out, int* hdiag_j_out, long long* F_hi, long long* F_lo, int* chgcnt_out,
                            uint8_t* Qprev_out, float* T_all, double* loss_rows_all, int* active_rows, int* active_count,
                            int* full_ran, hipStream_t stream) {
    const size_t fbytes = (size_t)m * 256 * sizeof(long long);
    long long* mpart = reinterpret_cast<long long*>(ws + lo.off_mpart);
    long long* mpart_lo = reinterpret_cast<long long*>(ws + lo.off_mpart_lo);
    // the sums of the extension word are not written when the extension is off: they read as zero then
    GANQ_HIP_CHECK(hipMemsetAsync(mpart_lo, 0, (size_t)NP * fbytes, stream));
    GANQ_HIP_CHECK(hipMemsetAsync(ws + lo.off_mstate_lo, 0, fbytes, stream));
    GANQ_HIP_CHECK(hipMemsetAsync(Tc, 0, (size_t)m * V * sizeof(float), stream));
    int rc = t_prepare(W, H, m, n, lo, ws, true, stream);
    if (rc) return rc;
    const TPrep* prep = reinterpret_cast<const TPrep*>(ws + lo.off_prep);
    if (scale_out) GANQ_HIP_CHECK(hipMemcpyAsync(scale_out, &prep->scale, sizeof(double), hipMemcpyDeviceToDevice, stream));
    if (ext_out) GANQ_HIP_CHECK(hipMemcpyAsync(ext_out, &prep->ext, sizeof(int), hipMemcpyDeviceToDevice, stream));
    if (Hint_out)
        GANQ_HIP_CHECK(hipMemcpyAsync(Hint_out, ws + lo.off_hint, (size_t)n * n * sizeof(int), hipMemcpyDeviceToDevice, stream));
    if (J_out)
        hipLaunchKernelGGL(jint_unbias_kernel, dim3(1024), dim3(256), 0, stream, reinterpret_cast<const short*>(ws + lo.off_jint), n * n,
                           J_out);
    if (hdiag_int_out)
        GANQ_HIP_CHECK(hipMemcpyAsync(hdiag_int_out, ws + lo.off_hdiag, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, stream));
    if (hdiag_j_out)
        GANQ_HIP_CHECK(hipMemcpyAsync(hdiag_j_out, ws + lo.off_hdiag_j, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, stream));
    GANQ_LAUNCH_CHECK();
    const bool stateful = opt_get(OPT_T_FULL) != 1;
    for (int k = 0; k < K; ++k) {
        const uint8_t* Q = Qseq + (size_t)k * m * n;
        hipLaunchKernelGGL(t_probe_set_kernel, dim3(1), dim3(1), 0, stream, mpart);
        // the driver's sequence (run_layer.hip): from the second iteration on only the changed rows are re-solved, in place
        const bool in_place = k >= 1 && t_rows_listable(lo);
        rc = t_iterate(Q, m, n, V, rcond, lo, ws, nullptr, in_place ? Tc : Tn, nullptr, nullptr, 1, nullptr, k, stream, in_place);
        if (rc) return rc;
        if (!in_place) std::swap(Tc, Tn);
        if (full_ran) hipLaunchKernelGGL(t_probe_get_kernel, dim3(1), dim3(1), 0, stream, mpart, full_ran + k);
        GANQ_LAUNCH_CHECK();
        long long* fh = F_hi ? F_hi + (size_t)k * m * 256 : nullptr;
        long long* fl = F_lo ? F_lo + (size_t)k * m * 256 : nullptr;
        if (stateful) {
            if (fh) GANQ_HIP_CHECK(hipMemcpyAsync(fh, ws + lo.off_mstate, fbytes, hipMemcpyDeviceToDevice, stream));
            if (fl) GANQ_HIP_CHECK(hipMemcpyAsync(fl, ws + lo.off_mstate_lo, fbytes, hipMemcpyDeviceToDevice, stream));
            if (Qprev_out)
                GANQ_HIP_CHECK(hipMemcpyAsync(Qprev_out + (size_t)k * m * n, ws + lo.off_qprev, (size_t)m * n, hipMemcpyDeviceToDevice, stream));
            if (chgcnt_out && k >= 1)
                GANQ_HIP_CHECK(hipMemcpyAsync(chgcnt_out + (size_t)k * m, ws + lo.off_chgcnt, (size_t)m * sizeof(int), hipMemcpyDeviceToDevice, stream));
        } else if (fh || fl) {
            // the NP partial sums, summed and symmetrised by the loop's own reduction into a scratch copy of its outputs
            long long* scratch_hi = reinterpret_cast<long long*>(ws + lo.off_mstate);
            long long* scratch_lo = reinterpret_cast<long long*>(ws + lo.off_mstate_lo);
            hipLaunchKernelGGL(m_reduce_kernel, dim3(1024 + 256), dim3(256), 0, stream, mpart, mpart_lo, (int)m, scratch_hi, scratch_lo,
                               static_cast<const uint8_t*>(nullptr), static_cast<uint8_t*>(nullptr), (int64_t)0,
                               static_cast<const long long*>(nullptr), 0ll, prep, 1024);
            GANQ_LAUNCH_CHECK();
            if (fh) GANQ_HIP_CHECK(hipMemcpyAsync(fh, scratch_hi, fbytes, hipMemcpyDeviceToDevice, stream));
            if (fl) GANQ_HIP_CHECK(hipMemcpyAsync(fl, scratch_lo, fbytes, hipMemcpyDeviceToDevice, stream));
        }
        if (T_all) GANQ_HIP_CHECK(hipMemcpyAsync(T_all + (size_t)k * m * V, Tc, (size_t)m * V * sizeof(float), hipMemcpyDeviceToDevice, stream));
        if (loss_rows_all)
            GANQ_HIP_CHECK(hipMemcpyAsync(loss_rows_all + (size_t)k * m, t_loss_rows(lo, ws), (size_t)m * sizeof(double), hipMemcpyDeviceToDevice, stream));
        if (in_place) {
            const int* list = reinterpret_cast<const int*>(ws + lo.off_active);
            if (active_rows)
                GANQ_HIP_CHECK(hipMemcpyAsync(active_rows + (size_t)k * m, list, (size_t)m * sizeof(int), hipMemcpyDeviceToDevice, stream));
            if (active_count) GANQ_HIP_CHECK(hipMemcpyAsync(active_count + k, list + m, sizeof(int), hipMemcpyDeviceToDevice, stream));
        }
    }
    GANQ_HIP_CHECK(hipStreamSynchronize(stream));
    return 0;
}
}  // namespace ganq

// developer check (tests): the loop's T-update on a given index sequence, with the integers behind it
extern "C" int ganq_debug_t_sums(const float* W, const float* H, const uint8_t* Qseq, int64_t m, int64_t n, int V, int K, double rcond,
                                 double* scale_out, int* ext_out, int* Hint_out, int* J_out, int* hdiag_int_out, int* hdiag_j_out,
                                 long long* F_hi, long long* F_lo, int* chgcnt_out, uint8_t* Qprev_out, float* T_all,
                                 double* loss_rows_all, int* active_rows, int* active_count, int* full_ran, void* stream_) {
    if (m <= 0 || n <= 0 || K <= 0 || m > INT32_MAX / 2) return fail(-1, "ganq_debug_t_sums: bad shape / K");
    if (n > 16384) return fail(-1, "ganq_debug_t_sums: n=%lld > 16384 not supported", (long long)n);
    if (V < 2 || V > 16) return fail(-2, "ganq_debug_t_sums: V=%d not supported (bits 2..4 are implemented)", V);
    if (!W || !H || !Qseq) return fail(-3, "ganq_debug_t_sums: null pointer");
    if (rcond < 0) rcond = 1.1920928955078125e-07 * (double)V;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const TLayout lo = t_layout(m, n, true);
    const size_t tbytes = align_up((size_t)m * V * sizeof(float), 256);
    char* ws = nullptr;
    GANQ_HIP_CHECK(hipMalloc(&ws, lo.total + 2 * tbytes));
    // "no list was built" / "no change counts" read as -1 / 0
    hipError_t e = hipSuccess;
    if (active_rows) e = hipMemsetAsync(active_rows, 0xff, (size_t)K * m * sizeof(int), stream);
    if (e == hipSuccess && active_count) e = hipMemsetAsync(active_count, 0xff, (size_t)K * sizeof(int), stream);
    if (e == hipSuccess && chgcnt_out) e = hipMemsetAsync(chgcnt_out, 0, (size_t)K * m * sizeof(int), stream);
    int rc = e == hipSuccess ? 0 : fail(-100, "ganq_debug_t_sums: %s", hipGetErrorString(e));
    if (rc == 0)
        rc = debug_t_sums_run(W, H, Qseq, m, n, V, K, rcond, lo, ws, reinterpret_cast<float*>(ws + lo.total),
                              reinterpret_cast<float*>(ws + lo.total + tbytes), scale_out, ext_out, Hint_out, J_out, hdiag_int_out,
                              hdiag_j_out, F_hi, F_lo, chgcnt_out, Qprev_out, T_all, loss_rows_all, active_rows, active_count, full_ran,
                              stream);
    else
        (void)hipStreamSynchronize(stream);
    if (rc != 0) (void)hipDeviceSynchronize();  // nothing of a failed run may still use the scratch
    (void)hipFree(ws);
    return rc;
}

extern "C" size_t ganq_update_t_workspace_bytes(int64_t m, int64_t n, int V) {
    (void)V;
    if (m <= 0 || n <= 0) return 0;
    return t_layout(m, n, false).total;
}

extern "C" int ganq_update_t(const float* WH, const float* H, const uint8_t* Q, int64_t m, int64_t n, int V,
                             double rcond, float* T_out, float* A_out, float* b_out, void* workspace,
                             size_t workspace_bytes, void* stream_) {
    if (m < 0 || n < 0) return fail(-1, "ganq_update_t: negative shape");
    if (m == 0 || n == 0) return 0;
    if (V < 2 || V > 16) return fail(-2, "ganq_update_t: V=%d not supported (bits 2..4 are implemented)", V);
    if (m > INT32_MAX / 2 || n > INT32_MAX / 2) return fail(-1, "ganq_update_t: shape too large");
    if (!WH || !H || !Q || !T_out) return fail(-3, "ganq_update_t: null pointer");
    const TLayout lo = t_layout(m, n, false);
    if (!workspace || workspace_bytes < lo.total)
        return fail(-4, "ganq_update_t: workspace %zu B < required %zu B", workspace_bytes, lo.total);
    if (rcond < 0) rcond = 1.1920928955078125e-07 * (double)V;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    char* ws = static_cast<char*>(workspace);
    int rc = t_prepare(nullptr, H, m, n, lo, ws, false, stream);
    if (rc) return rc;
    return t_iterate(Q, m, n, V, rcond, lo, ws, WH, T_out, A_out, b_out, 0, nullptr, -1, stream, false);
}
