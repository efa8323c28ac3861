// A LUT-quantized table whose ROWS are looked up (the input embedding on its own, GanqHipPackedEmbedding): the row-packed layout,
// the nearest-code assignment that writes it and the lookup that reads it.
//
//   qrows [m, n * bits / 32] int32, row-major: row `id` is the little-endian bit stream of its n indices, `bits` each -- the stream
//   column `id` of the GPTQ layout [n * bits / 32, m] holds (32 indices in `bits` words, lut_bits.h), so
//   qrows == pack_indices(Q, bits).t().contiguous().  Because a group of 32 indices fills `bits` whole words, the groups of a row
//   join into ONE stream: index j of a row sits at bit j * bits of it.  A token's row is n * bits / 8 contiguous bytes.
//
// Both kernels give a lane 8 consecutive columns, 64 lanes a slice of 512: the 8 indices are 8 * bits consecutive bits of the stream
// (one word at 4 bits, half a word at 2, three bytes that may straddle two words at 3).
//
// ganq_lut_table_assign: one wave per row.  Each lane reads its 8 weights (two 16-byte loads, the wave 2 KiB contiguous), scans the
//   row's codebook upwards with a strict `<` on fabsf(w - T[v]) (the first minimum wins) and builds its 8 * bits bits in a register;
//   neighbouring lanes exchange them by lane permute so that every word of the row is stored once, whole (no uint8 Q in memory).
//   The squared error is summed in fp64 per lane in column order, then over the wave by a fixed butterfly: no atomics, the same
//   bits on every call.
// ganq_lut_table_lookup: units (token, 512-column slice) dealt to the waves of a capped grid, as ganq_lut_embedding does.  A wave
//   reads 64 * bits contiguous bytes of the row (one dword per lane; at 3 bits a second one where the lane's 24 bits straddle), has the row's codebook in lanes 0 .. V-1, picks
//   the values by lane permute and stores 16 bytes per lane, one contiguous KiB per wave.  No LDS, no barrier, no workspace, no
//   host synchronisation, no allocation: the call can be captured in a HIP graph.
#include <algorithm>

#include "common.h"

namespace ganq {

namespace {

constexpr int TAB_WAVES = 4;                 // waves per workgroup
constexpr int TAB_SLICE = 512;               // columns a wave takes at a time (64 lanes x 8)
constexpr int64_t TAB_MAX_GRID = 1 << 15;    // workgroups; more rows / units than that are looped over

__device__ __forceinline__ int tab_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

template <int BITS>
__global__ __launch_bounds__(TAB_WAVES * 64) void lut_table_assign_kernel(const float* __restrict__ W, const float* __restrict__ T,
                                                                           int64_t m, int n, uint32_t* __restrict__ qrows,
                                                                           double* __restrict__ sqerr) {
    constexpr int V = 1 << BITS;
    const int lane = threadIdx.x & 63;
    const int64_t wpr = (int64_t)n * BITS / 32;  // words per row
    const int64_t stride = (int64_t)gridDim.x * TAB_WAVES;
    for (int64_t row = (int64_t)blockIdx.x * TAB_WAVES + (threadIdx.x >> 6); row < m; row += stride) {
        float t[V];
#pragma unroll
        for (int v = 0; v < V; ++v) t[v] = T[row * V + v];
        const float* w = W + row * (int64_t)n;
        uint32_t* q = qrows + row * wpr;
        double acc = 0.0;
        for (int s0 = 0; s0 < n; s0 += TAB_SLICE) {  // (the same trip count for the whole wave: the permutes below need every lane)
            const int c0 = s0 + lane * 8;
            const bool active = c0 < n;  // (n is a multiple of 32: 4 lanes share a group, all active or none)
            float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (active) {
                const float4 a = *reinterpret_cast<const float4*>(w + c0), b = *reinterpret_cast<const float4*>(w + c0 + 4);
                x[0] = a.x, x[1] = a.y, x[2] = a.z, x[3] = a.w, x[4] = b.x, x[5] = b.y, x[6] = b.z, x[7] = b.w;
            }
            uint32_t code = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float d = x[j] - t[0];
                float best = fabsf(d);
                uint32_t idx = 0;
#pragma unroll
                for (int v = 1; v < V; ++v) {
                    const float dv = x[j] - t[v];
                    const bool better = fabsf(dv) < best;
                    best = better ? fabsf(dv) : best;
                    d = better ? dv : d;
                    idx = better ? (uint32_t)v : idx;
                }
                code |= idx << (BITS * j);
                if (active) acc += (double)d * (double)d;
            }
            if (BITS == 4) {
                if (active) q[c0 >> 3] = code;
            } else if (BITS == 2) {  // two lanes a word
                const uint32_t other = (uint32_t)__shfl_down((int)code, 1, 64);
                if (active && !(lane & 1)) q[c0 >> 4] = code | (other << 16);
            } else {  // 3 bits: lanes 4g .. 4g+3 hold 4 x 24 bits = the 3 words of group g; lane 4g + k stores word k
                const uint32_t next = (uint32_t)__shfl_down((int)code, 1, 64);
                const int k = lane & 3;
                if (active && k < 3) q[(int64_t)(c0 >> 5) * 3 + k] = (code >> (8 * k)) | (next << (24 - 8 * k));
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (sqerr && lane == 0) sqerr[row] = acc;
    }
}

// (the codebook entries are moved as 16-bit patterns: fp16 and bf16 tables share the kernel)
template <int BITS>
__global__ __launch_bounds__(TAB_WAVES * 64) void lut_table_lookup_kernel(const int64_t* __restrict__ ids, int64_t N,
                                                                           const uint32_t* __restrict__ qrows,
                                                                           const uint16_t* __restrict__ lut, int64_t m, int n,
                                                                           uint16_t* __restrict__ out) {
    constexpr int V = 1 << BITS;
    const int lane = threadIdx.x & 63;
    const int slices = (n + TAB_SLICE - 1) / TAB_SLICE;
    const int64_t wpr = (int64_t)n * BITS / 32;
    const int64_t units = N * slices;
    const int64_t stride = (int64_t)gridDim.x * TAB_WAVES;
    for (int64_t u = (int64_t)blockIdx.x * TAB_WAVES + (threadIdx.x >> 6); u < units; u += stride) {
        const int64_t t = u / slices;
        const int c0 = (int)(u - t * slices) * TAB_SLICE + lane * 8;  // this lane's 8 columns
        const bool active = c0 < n;
        const int64_t raw = ids[t];
        const int64_t id = ((int64_t)tab_uniform((int)(raw >> 32)) << 32) | (uint32_t)tab_uniform((int)raw);
        uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (id >= 0 && id < m) {  // the same for the whole wave
            const uint32_t code = lane < V ? (uint32_t)lut[id * V + lane] : 0u;
            const uint32_t* q = qrows + id * wpr;
            uint32_t bits8 = 0;  // the lane's 8 indices: bits [c0 * BITS, (c0 + 8) * BITS) of the row's stream
            if (active) {
                const int64_t bit0 = (int64_t)c0 * BITS;
                const int64_t wi = bit0 >> 5;
                const int sh = (int)(bit0 & 31);
                if (BITS == 3) {  // three bytes at a byte offset of 0, 3, 2 or 1 in word wi: at 3 and 2 they reach into word wi + 1
                    const uint32_t lo = q[wi];  // (that word is inside the row: the lane's 24 bits are)
                    const uint32_t hi = sh > 8 ? q[wi + 1] : 0u;
                    bits8 = (uint32_t)(((uint64_t)lo | ((uint64_t)hi << 32)) >> sh);
                } else {
                    bits8 = q[wi] >> sh;
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) h[j] = (uint32_t)__shfl((int)code, (int)((bits8 >> (BITS * j)) & (V - 1)), 64);
        }
        if (active)
            *reinterpret_cast<uint4*>(out + t * (int64_t)n + c0) =
                make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
    }
}

int table_check_shape(const char* who, int64_t m, int64_t n, int bits) {
    if (m < 0 || n < 0) return fail(-1, "%s: negative shape", who);
    if (bits != 2 && bits != 3 && bits != 4) return fail(-2, "%s: bits=%d not supported (2, 3, 4 are)", who, bits);
    if (n % 32 != 0) return fail(-2, "%s: embedding_dim=%lld must be a multiple of 32", who, (long long)n);
    if (m > INT32_MAX / 2 || n > INT32_MAX / 2) return fail(-1, "%s: shape too large", who);
    return 0;
}

}  // namespace

}  // namespace ganq

using namespace ganq;

extern "C" int ganq_lut_table_assign(const float* W, const float* T, int64_t m, int64_t n, int bits, int32_t* qrows, double* sqerr_rows,
                                     void* stream_) {
    if (int rc = table_check_shape("ganq_lut_table_assign", m, n, bits)) return rc;
    if (m == 0) return 0;
    if (!T || (n > 0 && (!W || !qrows))) return fail(-3, "ganq_lut_table_assign: null pointer");
    if ((reinterpret_cast<uintptr_t>(W) & 15) != 0) return fail(-2, "ganq_lut_table_assign: W must be 16-byte aligned");
    const dim3 grid((unsigned)std::min<int64_t>((m + TAB_WAVES - 1) / TAB_WAVES, TAB_MAX_GRID));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    uint32_t* qp = reinterpret_cast<uint32_t*>(qrows);
    if (bits == 2)
        hipLaunchKernelGGL(lut_table_assign_kernel<2>, grid, dim3(TAB_WAVES * 64), 0, stream, W, T, m, (int)n, qp, sqerr_rows);
    else if (bits == 3)
        hipLaunchKernelGGL(lut_table_assign_kernel<3>, grid, dim3(TAB_WAVES * 64), 0, stream, W, T, m, (int)n, qp, sqerr_rows);
    else
        hipLaunchKernelGGL(lut_table_assign_kernel<4>, grid, dim3(TAB_WAVES * 64), 0, stream, W, T, m, (int)n, qp, sqerr_rows);
    GANQ_LAUNCH_CHECK();
    return 0;
}

extern "C" int ganq_lut_table_lookup(const int64_t* ids, int64_t N, const int32_t* qrows, const void* lut, int dtype, int64_t m, int64_t n,
                                     int bits, void* out, void* stream_) {
    if (N < 0) return fail(-1, "ganq_lut_table_lookup: negative shape");
    if (int rc = table_check_shape("ganq_lut_table_lookup", m, n, bits)) return rc;
    if (dtype != 0 && dtype != 1) return fail(-2, "ganq_lut_table_lookup: dtype %d (0 = fp16, 1 = bf16)", dtype);
    if ((reinterpret_cast<uintptr_t>(out) & 15) != 0) return fail(-2, "ganq_lut_table_lookup: out must be 16-byte aligned");
    if (N == 0 || m == 0 || n == 0) return 0;
    if (!ids || !out || !qrows || !lut) return fail(-3, "ganq_lut_table_lookup: null pointer");
    const int64_t slices = (n + TAB_SLICE - 1) / TAB_SLICE;
    if (N > INT64_MAX / slices) return fail(-1, "ganq_lut_table_lookup: too many ids");
    const int64_t units = N * slices;
    const dim3 grid((unsigned)std::min<int64_t>((units + TAB_WAVES - 1) / TAB_WAVES, TAB_MAX_GRID));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const uint32_t* qp = reinterpret_cast<const uint32_t*>(qrows);
    const uint16_t* lp = static_cast<const uint16_t*>(lut);
    uint16_t* op = static_cast<uint16_t*>(out);
    if (bits == 2)
        hipLaunchKernelGGL(lut_table_lookup_kernel<2>, grid, dim3(TAB_WAVES * 64), 0, stream, ids, N, qp, lp, m, (int)n, op);
    else if (bits == 3)
        hipLaunchKernelGGL(lut_table_lookup_kernel<3>, grid, dim3(TAB_WAVES * 64), 0, stream, ids, N, qp, lp, m, (int)n, op);
    else
        hipLaunchKernelGGL(lut_table_lookup_kernel<4>, grid, dim3(TAB_WAVES * 64), 0, stream, ids, N, qp, lp, m, (int)n, op);
    GANQ_LAUNCH_CHECK();
    return 0;
}
