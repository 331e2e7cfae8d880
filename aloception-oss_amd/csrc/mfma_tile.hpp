// What the GEMM-shaped kernels do around v_mfma_f32_32x32x16_*, once.  linear_shortk_kernel, ffn256_kernel (gemm.hip),
// linear_packed_kernel (gemm_packed.hip), conv1x1_chain_kernel, encoder_block_kernel, conv3x3_kernel, conv3x3_c64_kernel (conv.hip) and
// stem_conv_pool_kernel (stem.hip) share one frame:
//   * A wave owns a 64 x 64 (or 32 x 64) block of the output and computes it TRANSPOSED (weights = the MFMA's row operand), as
//     [row tile][column tile] of 32 x 32: lane (nl = lane & 31, kg = lane >> 5) holds ONE row per row tile, and registers 4 q .. 4 q + 3 of
//     column tile t are the four consecutive columns 32 t + 8 q + 4 kg .. + 3.
//   * Bias, activation and the conversion to the 16-bit storage type T (bf16_t / f16_t) work on those quads, which leave as 8-byte LDS
//     writes into a [row][column] staging area; the staged rows go to memory as whole 128-byte lines.
// Everything here is inlined and is held to adding no instruction, register, LDS or scratch byte to any caller (tools/isa_diff.py against
// the copies it replaced).  Where a helper did change a kernel's counts, that kernel keeps its own copy of the piece.
#pragma once
#include "common.hpp"

namespace alo {

// A wave reads back LDS it wrote itself (its staging area).  Not ALO_WAVE_LDS_ORDER (common.hpp), which orders the compiler alone.
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int R, int C>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[R][C]) {
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
        for (int t = 0; t < C; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][t][i] = 0.f;
}
template <int C>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[C]) {
#pragma unroll
    for (int t = 0; t < C; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
}

// K-split (two waves take every other k-step of one 64-column block): wave 1 hands its partial sums to wave 0 through LDS, `red` =
// [64 registers][64 lanes] of fp32, a fixed order.  A macro: as a function over f32x16 (&)[2][2], with or without the barrier inside,
// the K-split kernels lose their register allocation (linear_f32_kernel<true> 220 -> 256 VGPRs and 36 to 104 bytes of scratch,
// conv3x3_f32_kernel<2, true> 336 + 80 -> 400 + 144 registers).
#define ALO_KSPLIT_HANDOFF(acc, red, wave, lane)                                                                                    \
    do {                                                                                                                            \
        if ((wave) == 1) {                                                                                                          \
            _Pragma("unroll") for (int a_ = 0; a_ < 2; ++a_)                                                                        \
            _Pragma("unroll") for (int b_ = 0; b_ < 2; ++b_)                                                                        \
            _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) (red)[((a_ * 2 + b_) * 16 + r_) * 64 + (lane)] = (acc)[a_][b_][r_];  \
        }                                                                                                                           \
        __syncthreads();                                                                                                            \
        if ((wave) == 0) {                                                                                                          \
            _Pragma("unroll") for (int a_ = 0; a_ < 2; ++a_)                                                                        \
            _Pragma("unroll") for (int b_ = 0; b_ < 2; ++b_)                                                                        \
            _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) (acc)[a_][b_][r_] += (red)[((a_ * 2 + b_) * 16 + r_) * 64 + (lane)];  \
        }                                                                                                                           \
    } while (0)

// ---- the quad epilogue ------------------------------------------------------------------------------------------------------------------
// Column tile t of a wave's accumulators, f32x16[2] (one row tile) or f32x16[2][2] ([row tile][column tile]): + bias[column] when
// ADD_BIAS, ReLU when `relu` (a constant in most callers, conv3x3_c64_kernel's run-time flag otherwise), -> T (one rounding to nearest
// even) -> LDS [row][column] with row stride `stride` bytes, as 8-byte writes.  `row` is this lane's row of row tile 0 and col0 the
// wave's first column, both as the staging area and `bias` count them.
template <int R>
__device__ __forceinline__ const f32x16& acc_tile(const f32x16 (&acc)[R][2], int a, int t) { return acc[a][t]; }
__device__ __forceinline__ const f32x16& acc_tile(const f32x16 (&acc)[2], int, int t) { return acc[t]; }
template <typename T, bool ADD_BIAS, typename Acc>
__device__ __forceinline__ void stage_quads_tile(unsigned char* lds, int stride, const Acc& acc, const float* bias, bool relu, int row,
                                                 int col0, int kg, int t) {
    constexpr int R = sizeof(Acc) / sizeof(f32x16[2]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = col0 + 32 * t + 8 * q + 4 * kg;  // registers 4 q .. 4 q + 3 = columns c .. c + 3
        f32x4 bb = {0.f, 0.f, 0.f, 0.f};
        if constexpr (ADD_BIAS) bb = *reinterpret_cast<const f32x4*>(bias + c);
#pragma unroll
        for (int a = 0; a < R; ++a) {
            const f32x16& v = acc_tile(acc, a, t);
            float v0 = v[4 * q], v1 = v[4 * q + 1], v2 = v[4 * q + 2], v3 = v[4 * q + 3];
            if constexpr (ADD_BIAS) { v0 += bb[0]; v1 += bb[1]; v2 += bb[2]; v3 += bb[3]; }
            if (relu) { v0 = relu_keep_nan(v0); v1 = relu_keep_nan(v1); v2 = relu_keep_nan(v2); v3 = relu_keep_nan(v3); }
            *reinterpret_cast<u32x2*>(lds + (32 * a + row) * stride + c * 2) = u32x2{pack2<T>(v0, v1), pack2<T>(v2, v3)};
        }
    }
}
template <typename T, bool ADD_BIAS, typename Acc>
__device__ __forceinline__ void stage_quads(unsigned char* lds, int stride, const Acc& acc, const float* bias, bool relu, int row, int col0,
                                            int kg) {
#pragma unroll
    for (int t = 0; t < 2; ++t) stage_quads_tile<T, ADD_BIAS>(lds, stride, acc, bias, relu, row, col0, kg, t);
}

// ---- the whole-line row store -----------------------------------------------------------------------------------------------------------
// The 64 staged rows of a wave (64 columns = 128 B per row) -> Y[(grow0 + row) * N + col0 ..]: 8 lanes x 16 B per row, 8 rows per store
// instruction, rows with grow0 + row >= M dropped; HAS_RES: + R at the same coordinates, then the activation (add_residual_x8).
// (The conv3x3 kernels index pixels with 32-bit integers on a 64-bit image base; this loop changes their branches: they keep their own.)
template <typename T, bool RELU, bool HAS_RES>
__device__ __forceinline__ void store_rows(T* Y, const T* R, const unsigned char* obuf, int stride, long grow0, long M, int N, int col0,
                                           int lane) {
#pragma unroll
    for (int pass = 0; pass < 8; ++pass) {
        const int row = pass * 8 + (lane >> 3);
        const long grow = grow0 + row;
        u32x4 v = *reinterpret_cast<const u32x4*>(obuf + row * stride + (lane & 7) * 16);
        if (grow < M) {
            if constexpr (HAS_RES) v = add_residual_x8<T, RELU>(v, *reinterpret_cast<const u32x4*>(R + grow * N + col0 + (lane & 7) * 8));
            *reinterpret_cast<u32x4*>(Y + grow * N + col0 + (lane & 7) * 8) = v;
        }
    }
}

// The same store with the identity fetched AHEAD of the product (linear_shortk_kernel with HAS_RES at K = 64 and 128): inside
// store_rows the identity loads go out after the tile's MFMAs and the staging fence, one exposed memory round trip per tile and wave.
// fetch_identity issues them in store_rows' lane order (pass p of lane l = row 8 p + l / 8, 16-byte piece l % 8), rows past the end
// read from the last row and never stored; the values ride in registers (8 x u32x4) through the product; store_rows_fetched is
// store_rows' arithmetic on them: add_residual_x8 on the staged, already rounded product, then the activation, one rounding.
// sched_barrier keeps the compiler from sinking the requests next to their use.
template <typename T>
__device__ __forceinline__ void fetch_identity(u32x4 (&idn)[8], const T* R, long grow0, long M, int N, int col0, int lane) {
#pragma unroll
    for (int pass = 0; pass < 8; ++pass) {
        long grow = grow0 + pass * 8 + (lane >> 3);
        grow = grow < M ? grow : M - 1;
        idn[pass] = *reinterpret_cast<const u32x4*>(R + grow * N + col0 + (lane & 7) * 8);
    }
    __builtin_amdgcn_sched_barrier(0);
}
template <typename T, bool RELU>
__device__ __forceinline__ void store_rows_fetched(T* Y, const u32x4 (&idn)[8], const unsigned char* obuf, int stride, long grow0, long M,
                                                   int N, int col0, int lane) {
#pragma unroll
    for (int pass = 0; pass < 8; ++pass) {
        const int row = pass * 8 + (lane >> 3);
        const long grow = grow0 + row;
        const u32x4 v = *reinterpret_cast<const u32x4*>(obuf + row * stride + (lane & 7) * 16);
        if (grow < M) *reinterpret_cast<u32x4*>(Y + grow * N + col0 + (lane & 7) * 8) = add_residual_x8<T, RELU>(v, idn[pass]);
    }
}

// ---- weights streamed in MFMA fragment order against an A tile in LDS -------------------------------------------------------------------
// Weight fragments arrive in batches of KB k-steps (2 column tiles x KB x 16 B per lane) through two register buffers: batch i+1 is
// requested before batch i is consumed (L2 latency ~ the MFMA time of one batch).  frag0 = this lane's 16 bytes of the first fragment
// of column tile 0 (alo_pack_mfma_b order: a fragment is 64 lanes x 16 B contiguous), tile_stride = elements between the two column
// tiles.  sched_barrier keeps the compiler from sinking the requests next to their first use.
template <typename T, int KB>
__device__ __forceinline__ void load_batch(u32x4 (&buf)[2][KB], const T* frag0, size_t tile_stride, int batch) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < KB; ++j)
            buf[t][j] = *reinterpret_cast<const u32x4*>(frag0 + t * tile_stride + (size_t)(KB * batch + j) * 512);
    __builtin_amdgcn_sched_barrier(0);
}
// ---- the tile loader: 256 threads move a tile, PIECES 16-byte pieces per row, LOADS pieces per thread, rows contiguous across lanes; fetched
// into registers (in flight during the previous tile's MFMAs, each kernel's own addressing), then parked in LDS with row stride `stride`
template <int PIECES, int LOADS>
__device__ __forceinline__ void park_tile(unsigned char* lds, int stride, const u32x4 (&v)[LOADS], int tid) {
#pragma unroll
    for (int j = 0; j < LOADS; ++j) {
        const int p = tid + 256 * j;
        *reinterpret_cast<u32x4*>(lds + (p / PIECES) * stride + (p % PIECES) * 16) = v[j];
    }
}

// ---- 64 x 256 row tiles in LDS (ffn256_kernel, encoder_block_kernel) --------------------------------------------------------------------
// A workgroup of 4 waves owns 64 rows; wave w computes 64 output columns of them as [2 row tiles][2 column tiles] of 32 x 32.
constexpr int kTileRows = 64;
constexpr int kTileStride = 256 * 2 + 16;  // LDS row stride: +16 B keeps the 16-byte fragment reads conflict-free
constexpr int kTileKB = 2;                 // k-steps per weight batch
constexpr int kTileBatches = 16 / kTileKB; // batches per 256-deep contraction

// acc[row tile][column tile] += A (the LDS tile, k-steps kTileKB * batch ..) x the batch's weight fragments.  (linear_packed_kernel keeps
// this body as a lambda with its own stride: through a shared template four of its instantiations are scheduled with four more s_nop.)
template <typename T = bf16_t>
__device__ __forceinline__ void mma_batch(f32x16 (&acc)[2][2], const unsigned char* a_lds, const u32x4 (&buf)[2][kTileKB], int batch,
                                          int nl, int kg) {
    u32x4 af[2][kTileKB];  // A fragments of the whole batch first: their LDS latency overlaps instead of preceding each MFMA group
#pragma unroll
    for (int j = 0; j < kTileKB; ++j) {
        const int s = kTileKB * batch + j;
        af[0][j] = *reinterpret_cast<const u32x4*>(a_lds + nl * kTileStride + (16 * s + 8 * kg) * 2);
        af[1][j] = *reinterpret_cast<const u32x4*>(a_lds + (32 + nl) * kTileStride + (16 * s + 8 * kg) * 2);
    }
#pragma unroll
    for (int j = 0; j < kTileKB; ++j) {
        const u32x4 a0 = af[0][j], a1 = af[1][j];
        acc[0][0] = mfma_32x32x16<T>(buf[0][j], a0, acc[0][0]);
        acc[0][1] = mfma_32x32x16<T>(buf[1][j], a0, acc[0][1]);
        acc[1][0] = mfma_32x32x16<T>(buf[0][j], a1, acc[1][0]);
        acc[1][1] = mfma_32x32x16<T>(buf[1][j], a1, acc[1][1]);
    }
    __builtin_amdgcn_sched_barrier(0);
}

// One whole 256-deep contraction of the LDS tile against weights w (fragment pointer of k-step 0), through bufa / bufb.  bufa already
// holds batch 0; on return it holds batch 0 of `next` (same tile stride) when next != nullptr.
template <typename T>
__device__ __forceinline__ void mma_tile256(f32x16 (&acc)[2][2], const unsigned char* a_lds, u32x4 (&bufa)[2][kTileKB],
                                            u32x4 (&bufb)[2][kTileKB], const T* w, size_t tile_stride, const T* next,
                                            size_t next_stride, int nl, int kg) {
#pragma unroll
    for (int bt = 0; bt < kTileBatches; bt += 2) {
        load_batch(bufb, w, tile_stride, bt + 1);
        mma_batch<T>(acc, a_lds, bufa, bt, nl, kg);
        if (bt + 2 < kTileBatches) load_batch(bufa, w, tile_stride, bt + 2);
        else if (next != nullptr) load_batch(bufa, next, next_stride, 0);
        mma_batch<T>(acc, a_lds, bufb, bt + 1, nl, kg);
    }
}
// Rows [row0, row0 + 64) of a (M, 256) matrix; rows past the end are read from the last row (never stored) so that all eight requests
// go out back to back, unpredicated.  park_tile<32> would be park_tile256, but p / PIECES and p >> 5 are not the same code to the
// compiler: with either spelling in both places, ffn256_kernel gains 16 bytes of scratch or linear_shortk_kernel ten instructions.
template <typename T>
__device__ __forceinline__ void fetch_tile256(u32x4 (&v)[8], const T* X, long row0, long M, int tid) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int p = tid + 256 * j;
        long row = row0 + (p >> 5);
        row = row < M ? row : M - 1;
        v[j] = *reinterpret_cast<const u32x4*>(X + row * 256 + (p & 31) * 8);
    }
}
__device__ __forceinline__ void park_tile256(unsigned char* lds, const u32x4 (&v)[8], int tid) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int p = tid + 256 * j;
        *reinterpret_cast<u32x4*>(lds + (p >> 5) * kTileStride + (p & 31) * 16) = v[j];
    }
}
// this wave's accumulators (+ bias[column] when ADD_BIAS) -> T -> columns 64 wave .. of the LDS tile
template <bool ADD_BIAS, bool RELU, typename T = bf16_t>
__device__ __forceinline__ void stage_tile256(unsigned char* lds, const f32x16 (&acc)[2][2], const float* bias, int wave, int nl, int kg) {
    stage_quads<T, ADD_BIAS>(lds, kTileStride, acc, bias, RELU, nl, 64 * wave, kg);
}

}  // namespace alo
