// fp32 products on the fp16 matrix cores with two-term splits, once: the correlation build (corr.hip: the scale only) and the three fp32
// kernels conv3x3_f32_kernel (conv_f32.hip), linear_f32_kernel (gemm_f32.hip) and ffn_f32_kernel (ffn_f32.hip) share this arithmetic
// (tests/split_f16_ref.py restates it):
//   * the scale: an operand group (an image, a row, a (row, chunk), an output channel's weights) is divided by ONE power of two 2^k, from
//     the group's largest FINITE magnitude (finite_mag), which split_exponent brings into [2^14, 2^15).  Exact.
//   * the split: x 2^-k = hi + lo, hi = fp16(x 2^-k), lo = fp16(x 2^-k - hi), both round to nearest (split2); it happens where a tile is
//     parked in LDS (park4: four channels -> four hi terms, and their four lo terms lo_offset bytes behind), so no split copy of an
//     activation exists in memory.  Weights arrive split by the caller, both terms in alo_pack_mfma_b order (alo_hotpath.h).
//   * the non-finite rule: an Inf / NaN element takes no part in the scale and is parked as hi = 0, lo = the element.  It then meets only
//     the high weight term (lo * lo is not formed), so an infinity keeps its sign and a non-finite element spoils exactly the outputs
//     that contain it.
//   * the term order: per 16 input channels three MFMAs per 32 x 32 tile, small terms first: w_lo x_hi, w_hi x_lo, w_hi x_hi, fp32
//     accumulators (mma_split).
//   * the undo: ldexp(acc, k_activation + k_channel), exact; then bias, activation (stage_scaled_quads).
// The rule of mfma_tile.hpp holds here: a helper is used where tools/isa_diff.py shows the kernel's code unchanged, or changed and
// measured (docs/experiments.md, "One split-f16 helper set"); elsewhere the kernel keeps its copy with a comment.
#pragma once
#include "mfma_tile.hpp"

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
// m = max(m, the finite magnitudes of four values)
__device__ __forceinline__ unsigned finite_mag4(unsigned m, u32x4 v) {
    return max(max(m, max(finite_mag(v.x), finite_mag(v.y))), max(finite_mag(v.z), finite_mag(v.w)));
}
// A row spread over LANES adjacent lanes, each with the largest finite magnitude m of its part: -> the row's k, in every one of them
// (the row is then multiplied by 2^-k = ldexpf(1, -k))
template <int LANES>
__device__ __forceinline__ int row_exponent(unsigned m) {
#pragma unroll
    for (int o = LANES / 2; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    return split_exponent(m);
}

// x 2^-k -> (hi, lo); a non-finite element -> (0, itself)
__device__ __forceinline__ void split2(float x, float down, _Float16& hi, _Float16& lo) {
    const float xs = x * down;
    hi = (_Float16)xs;
    lo = (_Float16)(xs - (float)hi);
    if (!(fabsf(xs) < INFINITY)) {
        hi = (_Float16)0.f;
        lo = (_Float16)xs;
    }
}
__device__ __forceinline__ unsigned two_f16(_Float16 e0, _Float16 e1) {
    return (unsigned)__builtin_bit_cast(uint16_t, e0) | ((unsigned)__builtin_bit_cast(uint16_t, e1) << 16);
}
// four consecutive values of one row (floats, or their raw bits) -> their four hi terms at dst, their four lo terms lo_offset behind
__device__ __forceinline__ void park4(unsigned char* dst, int lo_offset, float v0, float v1, float v2, float v3, float down) {
    _Float16 hi[4], lo[4];
    split2(v0, down, hi[0], lo[0]);
    split2(v1, down, hi[1], lo[1]);
    split2(v2, down, hi[2], lo[2]);
    split2(v3, down, hi[3], lo[3]);
    *reinterpret_cast<u32x2*>(dst) = u32x2{two_f16(hi[0], hi[1]), two_f16(hi[2], hi[3])};
    *reinterpret_cast<u32x2*>(dst + lo_offset) = u32x2{two_f16(lo[0], lo[1]), two_f16(lo[2], lo[3])};
}
__device__ __forceinline__ void park4(unsigned char* dst, int lo_offset, const u32x4& v, float down) {
    park4(dst, lo_offset, __uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w), down);
}

// ---- one k-step (16 input channels) of a wave's [2 row tiles][2 column tiles] ------------------------------------------------------------
struct WFrag { u32x4 v[2][2]; };    // weights: [term: hi, lo][column tile]
struct XFrag { u32x4 v[2][2]; };    // activations: [term: hi, lo][row tile]
// both terms of both column tiles; p = this lane's 16 bytes of the high terms' fragment of column tile 0
__device__ __forceinline__ void load_wfrag(WFrag& f, const f16_t* p, size_t term_stride, size_t ctile_stride) {
#pragma unroll
    for (int term = 0; term < 2; ++term)
#pragma unroll
        for (int b = 0; b < 2; ++b) f.v[term][b] = *reinterpret_cast<const u32x4*>(p + term * term_stride + b * ctile_stride);
}
// small cross terms first; the four tiles rotate, so no MFMA waits on the one before it
__device__ __forceinline__ void mma_split(f32x16 (&acc)[2][2], const WFrag& w, const XFrag& x) {
    auto step = [&](int wt, int xt) {
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int a = 0; a < 2; ++a) acc[a][b] = mfma_32x32x16<f16_t>(w.v[wt][b], x.v[xt][a], acc[a][b]);
    };
    step(1, 0);
    step(0, 1);
    step(0, 0);
}

// ---- the frame conv3x3_f32_kernel and linear_f32_kernel share: 64 rows x 128 columns on two waves ---------------------------------------
constexpr int kOutStride = 64 * 4 + 16;           // LDS bytes per row of a wave's 32 x 64 fp32 output block
constexpr int kOutBytes = 32 * kOutStride;        // one row tile of one wave
constexpr int kRedOffset = kOutBytes;             // K-split: wave 1's partial sums [64 regs][64 lanes] sit behind wave 0's output block

// The workgroup's 128 (K-split: 64) bias values and channel exponents, one per thread; kc = the exponents behind the packed weights
template <bool KSPLIT>
__device__ __forceinline__ void fill_channel_tables(float* bias_s, int* kc_s, const float* bias, const int* kc, int first, int N, int tid) {
    const int c = first + tid;
    const bool live = c < N && (!KSPLIT || tid < 64);
    bias_s[tid] = (bias != nullptr && live) ? bias[c] : 0.f;
    kc_s[tid] = live ? kc[c] : 0;
}

// The undo: row tile a of a wave's accumulators -> 2^(k + k_channel), + bias, ReLU when relu -> the wave's fp32 output block, one 16-byte
// LDS write per quad.  lane = row nl of the row tile, registers 4 q .. 4 q + 3 = channels 32 b + 8 q + 4 kg .. + 3 (mfma_tile.hpp); k = the
// exponent of this lane's row (or image); bias_s / kc_s start at the wave's first channel.
__device__ __forceinline__ void stage_scaled_quads(unsigned char* obuf, const f32x16 (&acc)[2], int k, const float* bias_s, const int* kc_s,
                                                   bool relu, int nl, int kg) {
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = 32 * b + 8 * q + 4 * kg;
            const f32x4 bb = *reinterpret_cast<const f32x4*>(bias_s + c);
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = ldexpf(acc[b][4 * q + e], k + kc_s[c + e]) + bb[e];
                if (relu) v[e] = relu_keep_nan(v[e]);
            }
            *reinterpret_cast<f32x4*>(obuf + nl * kOutStride + c * 4) = v;
        }
}

}  // namespace alo
