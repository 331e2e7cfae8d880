// The scale of the two-term fp16 split (x = 2^k (hi + lo), corr.hip's header): shared by the correlation build (corr.hip) and the fp32
// 3x3 convolution (conv_f32.hip).
#pragma once
#include "common.hpp"

namespace alo {

// ------------------------------------------------------------------------------------------------------------------
// magnitudes as bit patterns of non-negative floats (they order like unsigned integers).  Inf / NaN entries do not take part in a
// scale: it comes from the finite values, so a non-finite feature spoils exactly its own row / column of the volume (as in the
// reference's fp32 matmul) and every other entry keeps its full accuracy.
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned finite_mag(unsigned bits) {
    const unsigned m = bits & 0x7fffffffu;
    return m >= 0x7f800000u ? 0u : m;
}
// The power of two a pixel's feature vector is divided by before it is split: its largest magnitude lands in [2^14, 2^15) (fp16
// holds up to 65504), so the low terms of all but the very smallest channels stay normal fp16 numbers.  0 for a vector without a
// finite non-zero value.
__device__ __forceinline__ int split_exponent(unsigned absmax_bits) {
    const int e = (int)(absmax_bits >> 23);
    if (e == 0 || e == 255) return 0;
    const int k = e - 127 - 14;
    return k < -110 ? -110 : (k > 110 ? 110 : k);
}

}  // namespace alo
