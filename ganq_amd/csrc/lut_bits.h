// The packed index stream of the LUT layers (lut_linear.hip, lut_backward.hip): `bits`-wide indices as one little-endian bit
// stream per output feature along in_features, 32 indices in BITS words (the GPTQ int32 packing, including its 3-bit scheme).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ganq {

// extract element j (0..31) of a 32-element group from its BITS words
template <int BITS>
__device__ __forceinline__ uint32_t extract(const uint32_t (&w)[BITS], int j) {
    const int bitpos = BITS * j;
    const int wi = bitpos >> 5, sh = bitpos & 31;
    uint32_t v = w[wi] >> sh;
    if (sh + BITS > 32) v |= w[wi + 1 < BITS ? wi + 1 : wi] << (32 - sh);
    return v & ((1u << BITS) - 1u);
}

}  // namespace ganq
