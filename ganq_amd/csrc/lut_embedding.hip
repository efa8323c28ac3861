// ganq_lut_embedding: rows of the dequantised weight of a LUT layer, gathered by token id straight out of the packed stream --
// the embedding lookup of a model whose input embedding is tied to a quantized output head (GanqHipQuantEmbedding).
//
//   out[t][j] = lut[id][Q[id][j]] (+ W_sparse[id][j], one rounded add in the output dtype)      id = ids[t], 0 <= id < m
//   out[t][:] = 0                                                                               otherwise (nothing is read)
//
// The packed layout is [n * bits / 32, m]: the words of ONE vocabulary row lie 4 m bytes apart, every one in a cache line of its
// own, so the lookup is a latency problem, not a bandwidth one.  A wave takes 512 columns of one token: 4 lanes per group of 32
// columns, each lane loads the BITS words of its group (the 4 lanes share the addresses: BITS x 16 independent lines in flight per
// wave), decodes its 8 indices with lut_bits.h and stores 16 bytes; a wave's store is one contiguous KiB of the output row.  The
// row's codebook (4 to 16 values) sits in lanes 0 .. V-1 and is read by a lane permute, so there is no LDS and no barrier.
// Units (token, 512-column slice) are dealt to the waves of a capped grid: N = 1 at 2048 columns is 4 waves, N = 2048 is 8192.
// Outliers: the row's CSR entries are read 64 at a time (coalesced), broadcast by lane permute and added by the lane that owns the
// column.  With a CSR present EVERY element goes through the add (+0 where the row has no entry), as `Wq + W_sparse` does.
// No workspace, no host synchronisation, no allocation: the call can be captured in a HIP graph.
#include <algorithm>

#include "common.h"
#include "lut_bits.h"

namespace ganq {

namespace {

constexpr int EMB_WAVES = 4;                 // waves per workgroup
constexpr int EMB_SLICE = 512;               // columns of one token a wave takes (64 lanes x 8)
constexpr int64_t EMB_MAX_GRID = 1 << 15;    // workgroups; more units than that are looped over

template <bool BF16>
__device__ __forceinline__ float emb_to_float(uint32_t h) {
    return BF16 ? __builtin_bit_cast(float, h << 16) : (float)__builtin_bit_cast(_Float16, (uint16_t)h);
}
template <bool BF16>
__device__ __forceinline__ uint32_t emb_round(float v) {
    return BF16 ? (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)v) : (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)v);
}
__device__ __forceinline__ int emb_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

template <int BITS, bool BF16>
__global__ __launch_bounds__(EMB_WAVES * 64) void lut_embedding_kernel(const int64_t* __restrict__ ids, int64_t N,
                                                                        const uint32_t* __restrict__ qw, const uint16_t* __restrict__ lut,
                                                                        int64_t m, int n, const int* __restrict__ rowptr,
                                                                        const int* __restrict__ cols, const uint16_t* __restrict__ vals,
                                                                        uint16_t* __restrict__ out) {
    constexpr int V = 1 << BITS;
    const int lane = threadIdx.x & 63;
    const int slices = (n + EMB_SLICE - 1) / EMB_SLICE;
    const int64_t units = N * slices;
    const int64_t stride = (int64_t)gridDim.x * EMB_WAVES;
    for (int64_t u = (int64_t)blockIdx.x * EMB_WAVES + (threadIdx.x >> 6); u < units; u += stride) {
        const int64_t t = u / slices;
        const int c0 = (int)(u - t * slices) * EMB_SLICE + lane * 8;  // this lane's 8 columns
        const bool active = c0 < n;                                    // (n is a multiple of 32: all 8 or none)
        const int64_t raw = ids[t];
        const int64_t id = ((int64_t)emb_uniform((int)(raw >> 32)) << 32) | (uint32_t)emb_uniform((int)raw);
        uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (id >= 0 && id < m) {  // the same for the whole wave
            const uint32_t code = lane < V ? (uint32_t)lut[id * V + lane] : 0u;
            uint32_t w[BITS];
#pragma unroll
            for (int b = 0; b < BITS; ++b) w[b] = 0;
            if (active) {
                const int64_t g = c0 >> 5;
#pragma unroll
                for (int b = 0; b < BITS; ++b) w[b] = qw[(g * BITS + b) * m + id];
            }
            // the lane's quarter of the group as 8 nibbles (the quarter is picked after a decode with constant positions)
            const int quarter = (c0 >> 3) & 3;
            uint32_t nib = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint32_t c = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) c |= extract<BITS>(w, 8 * q + j) << (4 * j);
                nib = quarter == q ? c : nib;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) h[j] = (uint32_t)__shfl((int)code, (int)((nib >> (4 * j)) & 15u), 64);
            if (rowptr) {
                float sp[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                const int e0 = emb_uniform(rowptr[id]), e1 = emb_uniform(rowptr[id + 1]);
                for (int e = e0; e < e1; e += 64) {
                    int col = -1;
                    uint32_t val = 0;
                    if (e + lane < e1) {
                        col = cols[e + lane];
                        val = vals[e + lane];
                    }
                    const int cnt = min(64, e1 - e);
                    for (int k = 0; k < cnt; ++k) {
                        const int d = __shfl(col, k, 64) - c0;
                        const float v = emb_to_float<BF16>((uint32_t)__shfl((int)val, k, 64));
#pragma unroll
                        for (int j = 0; j < 8; ++j) sp[j] = d == j ? v : sp[j];
                    }
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) h[j] = emb_round<BF16>(emb_to_float<BF16>(h[j]) + sp[j]);
            }
        }
        if (active)
            *reinterpret_cast<uint4*>(out + t * (int64_t)n + c0) =
                make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
    }
}

template <int BITS>
void launch_embedding(bool bf16, dim3 grid, hipStream_t stream, const int64_t* ids, int64_t N, const uint32_t* qw, const uint16_t* lut,
                      int64_t m, int n, const int* rowptr, const int* cols, const uint16_t* vals, uint16_t* out) {
    if (bf16)
        hipLaunchKernelGGL((lut_embedding_kernel<BITS, true>), grid, dim3(EMB_WAVES * 64), 0, stream, ids, N, qw, lut, m, n, rowptr, cols,
                           vals, out);
    else
        hipLaunchKernelGGL((lut_embedding_kernel<BITS, false>), grid, dim3(EMB_WAVES * 64), 0, stream, ids, N, qw, lut, m, n, rowptr, cols,
                           vals, out);
}

}  // namespace

}  // namespace ganq

using namespace ganq;

extern "C" int ganq_lut_embedding(const int64_t* ids, int64_t N, const int32_t* qweight, const void* lut, int dtype, int64_t m, int64_t n,
                                  int bits, const int32_t* outlier_rowptr, const int32_t* outlier_cols, const void* outlier_vals,
                                  void* out, void* stream_) {
    if (N < 0 || m < 0 || n < 0) return fail(-1, "ganq_lut_embedding: negative shape");
    if (N == 0 || n == 0) return 0;
    if (dtype != 0 && dtype != 1) return fail(-2, "ganq_lut_embedding: dtype %d (0 = fp16, 1 = bf16)", dtype);
    if (bits != 2 && bits != 3 && bits != 4) return fail(-2, "ganq_lut_embedding: bits=%d not supported (2, 3, 4 are)", bits);
    if (n % 32 != 0) return fail(-2, "ganq_lut_embedding: in_features=%lld must be a multiple of 32", (long long)n);
    if (m > INT32_MAX / 2 || n > INT32_MAX / 2) return fail(-1, "ganq_lut_embedding: shape too large");
    if (!ids || !out || (m > 0 && (!qweight || !lut))) return fail(-3, "ganq_lut_embedding: null pointer");
    if ((reinterpret_cast<uintptr_t>(out) & 15) != 0) return fail(-2, "ganq_lut_embedding: out must be 16-byte aligned");
    const int64_t slices = (n + EMB_SLICE - 1) / EMB_SLICE;
    if (N > INT64_MAX / slices) return fail(-1, "ganq_lut_embedding: too many ids");
    const int64_t units = N * slices;
    const dim3 grid((unsigned)std::min<int64_t>((units + EMB_WAVES - 1) / EMB_WAVES, EMB_MAX_GRID));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const uint32_t* qw = reinterpret_cast<const uint32_t*>(qweight);
    const uint16_t* lp = static_cast<const uint16_t*>(lut);
    const uint16_t* vp = static_cast<const uint16_t*>(outlier_vals);
    uint16_t* op = static_cast<uint16_t*>(out);
    if (bits == 2) launch_embedding<2>(dtype == 1, grid, stream, ids, N, qw, lp, m, (int)n, outlier_rowptr, outlier_cols, vp, op);
    else if (bits == 3) launch_embedding<3>(dtype == 1, grid, stream, ids, N, qw, lp, m, (int)n, outlier_rowptr, outlier_cols, vp, op);
    else launch_embedding<4>(dtype == 1, grid, stream, ids, N, qw, lp, m, (int)n, outlier_rowptr, outlier_cols, vp, op);
    GANQ_LAUNCH_CHECK();
    return 0;
}
