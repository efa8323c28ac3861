// Codebook gradient of an embedding LOOKUP out of a packed LUT table (the backward of ganq_lut_table_lookup / ganq_lut_embedding with
// respect to `lut`; lut_backward.hip's dlut without the GEMM):
//
//   dlut[id][v] = sum over the positions p with ids[p] == id and the columns j with Q[id][j] == v of dy[p][j]
//
// Rows no id selects, codes no index of a row uses, ids outside [0, m) and the id `padding_idx` contribute exactly 0; every element
// of dlut is written.  No floating-point atomics: the summation order is a function of (ids, dy) alone, bitwise repeatable.
//
// The caller hands over `order`, a stable ascending sort permutation of ids (it is not trusted: an entry outside [0, N) is skipped,
// never dereferenced).  Two launches after a memset of dlut, whatever the ids hold:
//
// bins: one wave per SORTED position s, p = order[s].  The wave walks row id = ids[p] in 512-column slices (8 columns and 8 codes per
//   lane, as the lookup kernels); each lane sums its dy values into 2^bits bins in registers, and a fixed reduce-scatter over the 64
//   lanes (halving the bins a lane keeps at xor 32, 16, ..., then a butterfly over the lanes that share a bin) leaves
//   partial[s][v] and key[s] = id (-1: the position contributes nothing) in the workspace.  The two layouts differ only in where word
//   w of a row's bit stream lies: q[id * words + w] in the row-packed table, q[w * m + id] in the GPTQ column layout.
//   Going by sorted position puts the partials of one id next to each other, in ascending position order.
// sum: one wave per sorted position; it is a segment head if key[s] >= 0 and (s == 0 or key[s - 1] != key[s]), everything else
//   exits.  A head adds partial[s], partial[s + 1], ... while the key stays the same: the whole wave takes one chunk of 64 * 4 / V
//   positions first (a segment of one position, the common case with ids spread over a vocabulary, ends there), then SUM_UNROLL
//   chunks per step.  A lane loads 4 bins of one position as 16 bytes and the loads of a step are independent; each lane adds its
//   positions in ascending order, and a fixed butterfly over the lanes that hold the same bins gives dlut[id].
//   A padding or BOS token that fills thousands of positions is one such segment: ~N / 64 steps at 4 bits, not N dependent loads.
// No host synchronisation, no allocation: the launch sequence depends on (N, m, n, bits) alone and can be captured in a HIP graph.
#include <algorithm>

#include "common.h"

namespace ganq {

namespace {

constexpr int TBW_WAVES = 4;               // waves per workgroup
constexpr int TBW_SLICE = 512;             // columns a wave takes at a time (64 lanes x 8)
constexpr int64_t TBW_MAX_GRID = 1 << 15;  // workgroups; more positions than that are looped over
constexpr int SUM_UNROLL = 4;              // chunks of positions a head has in flight per step

__device__ __forceinline__ int64_t tbw_uniform(int64_t v) {
    return ((int64_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

template <bool BF16>
__device__ __forceinline__ float tbw_to_float(uint32_t h) {
    return BF16 ? __builtin_bit_cast(float, h << 16) : (float)__builtin_bit_cast(_Float16, (uint16_t)h);
}

// word w of row id's bit stream is q[id * row_stride + w * word_stride]
template <int BITS, bool BF16>
__global__ __launch_bounds__(TBW_WAVES * 64) void lut_table_bwd_bins_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ order,
                                                                             int64_t N, const uint16_t* __restrict__ dy,
                                                                             const uint32_t* __restrict__ q, int64_t row_stride,
                                                                             int64_t word_stride, int64_t m, int n, int64_t padding_idx,
                                                                             float* __restrict__ partial, int64_t* __restrict__ key) {
    constexpr int V = 1 << BITS;
    constexpr int SHARE = 64 / V;  // lanes that end up with the same bin
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * TBW_WAVES;
    for (int64_t s = (int64_t)blockIdx.x * TBW_WAVES + (threadIdx.x >> 6); s < N; s += stride) {
        const int64_t p = tbw_uniform(order[s]);
        int64_t id = -1;
        if (p >= 0 && p < N) id = tbw_uniform(ids[p]);
        if (id < 0 || id >= m || id == padding_idx) {  // the same for the whole wave
            if (lane == 0) key[s] = -1;
            continue;
        }
        const uint32_t* row = q + id * row_stride;
        const uint16_t* g = dy + p * (int64_t)n;
        float bin[V];
#pragma unroll
        for (int v = 0; v < V; ++v) bin[v] = 0.f;
        for (int s0 = 0; s0 < n; s0 += TBW_SLICE) {
            const int c0 = s0 + lane * 8;  // this lane's 8 columns (n is a multiple of 32: all 8 or none)
            if (c0 >= n) continue;
            const uint4 d = *reinterpret_cast<const uint4*>(g + c0);
            const int64_t bit0 = (int64_t)c0 * BITS;  // the lane's 8 codes: bits [c0 * BITS, (c0 + 8) * BITS) of the row's stream
            const int64_t wi = bit0 >> 5;
            const int sh = (int)(bit0 & 31);
            uint32_t bits8;
            if (BITS == 3) {  // three bytes at a byte offset of 0, 3, 2 or 1 in word wi: at 3 and 2 they reach into word wi + 1
                const uint32_t lo = row[wi * word_stride];  // (that word is inside the row: the lane's 24 bits are)
                const uint32_t hi = sh > 8 ? row[(wi + 1) * word_stride] : 0u;
                bits8 = (uint32_t)(((uint64_t)lo | ((uint64_t)hi << 32)) >> sh);
            } else {
                bits8 = row[wi * word_stride] >> sh;
            }
            const uint32_t h[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float x = tbw_to_float<BF16>((h[j >> 1] >> (16 * (j & 1))) & 0xffffu);
                const uint32_t c = (bits8 >> (BITS * j)) & (V - 1);
#pragma unroll
                for (int v = 0; v < V; ++v) bin[v] += c == (uint32_t)v ? x : 0.f;
            }
        }
        // reduce-scatter: at xor `off` a lane keeps one half of its bins and receives that half from its partner, so that after
        // BITS steps lane l holds bin l / SHARE summed over the lanes l' with l' % SHARE == l % SHARE
        int off = 32;
#pragma unroll
        for (int cnt = V; cnt > 1; cnt >>= 1, off >>= 1) {
            const bool upper = (lane & off) != 0;
            const int half = cnt >> 1;
#pragma unroll
            for (int i = 0; i < half; ++i) {
                const float send = upper ? bin[i] : bin[i + half];
                const float keep = upper ? bin[i + half] : bin[i];
                bin[i] = keep + __shfl_xor(send, off, 64);
            }
        }
        float acc = bin[0];
#pragma unroll
        for (int o = SHARE >> 1; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if ((lane & (SHARE - 1)) == 0) partial[s * V + (lane / SHARE)] = acc;
        if (lane == 0) key[s] = id;
    }
}

// One step of a segment head: U chunks of CHUNK positions from `base` on, all loads independent; every lane adds its positions that
// still belong to the segment, in ascending order.  Returns whether the segment goes on past the step (wave-uniform).
template <int V, int U>
__device__ __forceinline__ bool tbw_sum_step(const float* __restrict__ partial, const int64_t* __restrict__ key, int64_t N, int64_t id,
                                             int64_t base, int lane, int r, int vq, f32x4& acc) {
    constexpr int CHUNK = 64 / (V / 4);
    f32x4 x[U];
    bool same[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t t = base + u * CHUNK + r;
        x[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        same[u] = false;
        if (t < N) {
            same[u] = key[t] == id;
            x[u] = *reinterpret_cast<const f32x4*>(partial + t * V + 4 * vq);  // (garbage where the key differs: not used)
        }
    }
    bool open = true;  // the segment has not ended before this chunk
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint64_t mask = __ballot(same[u]);
        const int first = mask == ~0ull ? 64 : __builtin_ctzll(~mask);  // the first lane past the segment
        if (open && lane < first) acc += x[u];
        open = open && first == 64;
    }
    return open;
}

template <int BITS>
__global__ __launch_bounds__(TBW_WAVES * 64) void lut_table_bwd_sum_kernel(const float* __restrict__ partial, const int64_t* __restrict__ key,
                                                                            int64_t N, float* __restrict__ dlut) {
    constexpr int V = 1 << BITS;
    constexpr int LPP = V / 4;       // lanes per position: each loads 4 bins
    constexpr int CHUNK = 64 / LPP;  // positions the wave covers with one load per lane
    const int lane = threadIdx.x & 63;
    const int r = lane / LPP, vq = lane % LPP;
    const int64_t stride = (int64_t)gridDim.x * TBW_WAVES;
    for (int64_t s = (int64_t)blockIdx.x * TBW_WAVES + (threadIdx.x >> 6); s < N; s += stride) {
        const int64_t id = tbw_uniform(key[s]);
        if (id < 0) continue;
        if (s > 0 && tbw_uniform(key[s - 1]) == id) continue;  // not the head of its segment
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        // one chunk first (with ids spread over a vocabulary most segments end inside it), then SUM_UNROLL chunks per step
        bool open = tbw_sum_step<V, 1>(partial, key, N, id, s, lane, r, vq, acc);
        for (int64_t base = s + CHUNK; open && base < N; base += SUM_UNROLL * CHUNK)
            open = tbw_sum_step<V, SUM_UNROLL>(partial, key, N, id, base, lane, r, vq, acc);
#pragma unroll
        for (int o = 32; o >= LPP; o >>= 1) {
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += __shfl_xor(acc[k], o, 64);
        }
        if (r == 0) *reinterpret_cast<f32x4*>(dlut + id * V + 4 * vq) = acc;
    }
}

struct TableBwdPlan {
    size_t part_bytes, key_bytes;
};

// host-only: depends on the arguments alone
TableBwdPlan table_bwd_plan(int64_t N, int bits) {
    TableBwdPlan p{};
    p.part_bytes = align_up((size_t)N * ((size_t)1 << bits) * sizeof(float), 256);
    p.key_bytes = align_up((size_t)N * sizeof(int64_t), 256);
    return p;
}

int table_bwd_check_shape(const char* who, int64_t N, int64_t m, int64_t n, int bits) {
    if (N < 0 || m < 0 || n < 0) return fail(-1, "%s: negative shape", who);
    if (bits != 2 && bits != 3 && bits != 4) return fail(-2, "%s: bits=%d not supported (2, 3, 4 are)", who, bits);
    if (n % 32 != 0) return fail(-2, "%s: embedding_dim=%lld must be a multiple of 32", who, (long long)n);
    if (m > INT32_MAX / 2 || n > INT32_MAX / 2) return fail(-1, "%s: shape too large", who);
    if (N >= (1ll << 40)) return fail(-1, "%s: too many ids (N must be below 2^40)", who);
    return 0;
}

template <int BITS>
void launch_bins(bool bf16, dim3 grid, hipStream_t stream, const int64_t* ids, const int64_t* order, int64_t N, const uint16_t* dy,
                 const uint32_t* q, int64_t row_stride, int64_t word_stride, int64_t m, int n, int64_t padding_idx, float* partial,
                 int64_t* key) {
    if (bf16)
        hipLaunchKernelGGL((lut_table_bwd_bins_kernel<BITS, true>), grid, dim3(TBW_WAVES * 64), 0, stream, ids, order, N, dy, q, row_stride,
                           word_stride, m, n, padding_idx, partial, key);
    else
        hipLaunchKernelGGL((lut_table_bwd_bins_kernel<BITS, false>), grid, dim3(TBW_WAVES * 64), 0, stream, ids, order, N, dy, q, row_stride,
                           word_stride, m, n, padding_idx, partial, key);
}

// both layouts: word w of row id at q[id * row_stride + w * word_stride]
int table_bwd_lut(const char* who, const int64_t* ids, const int64_t* order, int64_t N, const void* dy, int dtype, const int32_t* q,
                  bool by_rows, int64_t m, int64_t n, int bits, int64_t padding_idx, float* dlut, void* workspace, size_t workspace_bytes,
                  void* stream_) {
    if (int rc = table_bwd_check_shape(who, N, m, n, bits)) return rc;
    if (dtype != 0 && dtype != 1) return fail(-2, "%s: dtype %d (0 = fp16, 1 = bf16)", who, dtype);
    if (m == 0) return 0;
    if (!dlut) return fail(-3, "%s: null dlut", who);
    if ((reinterpret_cast<uintptr_t>(dlut) & 15) != 0) return fail(-2, "%s: dlut must be 16-byte aligned", who);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int V = 1 << bits;
    if (N > 0 && n > 0) {  // (every check before the first stream operation)
        if (!ids || !order || !dy || !q) return fail(-3, "%s: null pointer", who);
        if ((reinterpret_cast<uintptr_t>(dy) & 15) != 0) return fail(-2, "%s: dy must be 16-byte aligned", who);
        const TableBwdPlan p = table_bwd_plan(N, bits);
        const size_t need = p.part_bytes + p.key_bytes;
        if (!workspace || workspace_bytes < need) return fail(-4, "%s: workspace %zu B < required %zu B", who, workspace_bytes, need);
        if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return fail(-2, "%s: workspace must be 16-byte aligned", who);
    }
    GANQ_HIP_CHECK(hipMemsetAsync(dlut, 0, (size_t)m * V * sizeof(float), stream));  // rows no segment head writes
    if (N == 0 || n == 0) return 0;
    const TableBwdPlan p = table_bwd_plan(N, bits);
    float* partial = static_cast<float*>(workspace);
    int64_t* key = reinterpret_cast<int64_t*>(static_cast<char*>(workspace) + p.part_bytes);
    const uint32_t* qp = reinterpret_cast<const uint32_t*>(q);
    const uint16_t* dyp = static_cast<const uint16_t*>(dy);
    const int64_t row_stride = by_rows ? n * bits / 32 : 1, word_stride = by_rows ? 1 : m;
    const dim3 grid((unsigned)std::min<int64_t>((N + TBW_WAVES - 1) / TBW_WAVES, TBW_MAX_GRID));
    if (bits == 2) launch_bins<2>(dtype == 1, grid, stream, ids, order, N, dyp, qp, row_stride, word_stride, m, (int)n, padding_idx, partial, key);
    else if (bits == 3) launch_bins<3>(dtype == 1, grid, stream, ids, order, N, dyp, qp, row_stride, word_stride, m, (int)n, padding_idx, partial, key);
    else launch_bins<4>(dtype == 1, grid, stream, ids, order, N, dyp, qp, row_stride, word_stride, m, (int)n, padding_idx, partial, key);
    GANQ_LAUNCH_CHECK();
    if (bits == 2) hipLaunchKernelGGL(lut_table_bwd_sum_kernel<2>, grid, dim3(TBW_WAVES * 64), 0, stream, partial, key, N, dlut);
    else if (bits == 3) hipLaunchKernelGGL(lut_table_bwd_sum_kernel<3>, grid, dim3(TBW_WAVES * 64), 0, stream, partial, key, N, dlut);
    else hipLaunchKernelGGL(lut_table_bwd_sum_kernel<4>, grid, dim3(TBW_WAVES * 64), 0, stream, partial, key, N, dlut);
    GANQ_LAUNCH_CHECK();
    return 0;
}

size_t table_bwd_workspace_bytes(int64_t N, int64_t m, int64_t n, int bits) {
    if (N <= 0 || m <= 0 || n < 32 || (bits != 2 && bits != 3 && bits != 4) || N >= (1ll << 40)) return 0;
    const TableBwdPlan p = table_bwd_plan(N, bits);
    return p.part_bytes + p.key_bytes;
}

}  // namespace

}  // namespace ganq

using namespace ganq;

extern "C" size_t ganq_lut_table_bwd_lut_workspace_bytes(int64_t N, int64_t m, int64_t n, int bits) {
    return table_bwd_workspace_bytes(N, m, n, bits);
}

extern "C" int ganq_lut_table_bwd_lut(const int64_t* ids, const int64_t* order, int64_t N, const void* dy, int dtype, const int32_t* qrows,
                                      int64_t m, int64_t n, int bits, int64_t padding_idx, float* dlut, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    return table_bwd_lut("ganq_lut_table_bwd_lut", ids, order, N, dy, dtype, qrows, true, m, n, bits, padding_idx, dlut, workspace,
                         workspace_bytes, stream);
}

extern "C" size_t ganq_lut_embedding_bwd_lut_workspace_bytes(int64_t N, int64_t m, int64_t n, int bits) {
    return table_bwd_workspace_bytes(N, m, n, bits);
}

extern "C" int ganq_lut_embedding_bwd_lut(const int64_t* ids, const int64_t* order, int64_t N, const void* dy, int dtype,
                                          const int32_t* qweight, int64_t m, int64_t n, int bits, int64_t padding_idx, float* dlut,
                                          void* workspace, size_t workspace_bytes, void* stream) {
    return table_bwd_lut("ganq_lut_embedding_bwd_lut", ids, order, N, dy, dtype, qweight, false, m, n, bits, padding_idx, dlut, workspace,
                         workspace_bytes, stream);
}
