// y (M, 256) = relu(x (M, 256) W1 (F, 256)^T + b1) W2 (256, F)^T + b2, fp32 in and out, in ONE kernel on the fp16 matrix cores at fp32-class
// accuracy: the fp32 flavour of alo_ffn256.  The two-term split arithmetic of split_f16.hpp (scale, split, non-finite rule, term order,
// undo) in ffn256_kernel's frame (gemm.hip): a workgroup keeps 64 rows in LDS and the (M, F) hidden activation never reaches memory.
//
// What is this kernel's own (tests/ffn_f32_ref.py restates it):
//   * weights: w1 and w2 each arrive as ONE buffer in the layout of alo_linear_packed's fp32 flavour (alo_hotpath.h) for the (F, 256)
//     and the (256, F) matrix, one power of two per output channel (hidden unit for w1, output column for w2).
//   * first product: one power of two per ROW of x; the whole row is in the tile, so one sweep over the registers the row arrives in
//     finds it and x is read once.  h = relu_keep_nan(ldexp(acc, k_row + k_unit) + b1).
//   * second product: the hidden activation is consumed 256 units at a time.  Each (row, chunk) gets its OWN power of two, from the
//     largest finite |h| of that row in that chunk (the four waves hold 64 of the 256 units each: one cross-wave maximum through LDS);
//     the chunk is split on its way into LDS; the chunk's three products per 16 units go into a FRESH accumulator, and then
//     y_acc += ldexp(acc_chunk, k_row,chunk + k_column)  in fp32, chunks in ascending order; finally  y = y_acc + b2.
//   * a row's result depends on no other row of the call, and there is no atomic and no order that depends on the launch: two launches
//     give the same bits.  An Inf / NaN in x, or one that arises in a hidden row, spoils exactly that row's outputs.
//
// Frame: 256 threads, wave w owns hidden units / output columns 64 w .. 64 w + 63 of the tile's 64 rows as [2 row tiles][2 column tiles]
// of 32 x 32.  LDS: the split x tile and the split hidden chunk, 64 rows x (256 hi | 256 lo) fp16 each (+16 B per row: conflict-free
// 16-byte reads); the fp32 output staging aliases the hidden chunk; behind them b1, the units' exponents, b2, the columns' exponents,
// the rows' exponents and the cross-wave maxima.  That is one workgroup per CU, one wave per SIMD, and the kernel hides latency in
// software: weight fragments stream through two register buffers of two k-steps each (both terms), a batch ahead of their use and
// across the phase boundaries, and the LDS tile's fragments are read a batch ahead as well; the next tile's raw fp32 rows are requested as soon as this tile is parked and ride in registers
// through its products.  Per batch a wave issues 8 ds_read_b128 for 24 MFMAs.  Persistent over the row tiles.
#include "mfma_tile.hpp"
#include "split_f16.hpp"

namespace alo {
namespace {

constexpr int kRows = 64;                       // rows per tile
constexpr int kThreads = 256;                   // four waves
constexpr int kLoOffset = 256 * 2;              // a parked row: 256 hi terms, then 256 lo terms
constexpr int kRowStride = 256 * 4 + 16;        // also the fp32 output staging's row stride
constexpr int kTile = kRows * kRowStride;
constexpr int kKB = 2;                          // k-steps per weight batch
constexpr int kBatches = 16 / kKB;              // batches per 256-deep contraction
constexpr int kRowLanes = 16;                   // lanes that fetch and park one row: four 16-byte pieces each, 256 B apart
constexpr int kPassRows = kThreads / kRowLanes; // rows per pass of the workgroup
constexpr int kPasses = kRows / kPassRows;
static_assert(kTile % 16 == 0 && kPasses * kPassRows == kRows, "16-byte LDS accesses; whole passes");

struct FfnF32Dims {
    long M;
    int F;      // hidden width, multiple of 256
    int tiles;  // ceil(M / 64)
};

// bytes behind the two tiles: b1 and the units' exponents (F each), b2 and the columns' exponents (256 each), the rows' exponents (64),
// the waves' row maxima of a hidden chunk (4 x 64)
constexpr size_t tail_bytes(int F) { return ((size_t)F + 256) * 8 + kRows * 4 + 4 * kRows * 4; }

struct WBatch { WFrag f[kKB]; };   // the k-steps of a batch, both terms of both column tiles each

// load_batch / mma_batch / mma_tile256 of mfma_tile.hpp with both terms of the weights and of the LDS tile.
// frag0 = this lane's 16 bytes of the high terms' first fragment of column tile 0; the low terms sit term_stride elements behind.
__device__ __forceinline__ void load_wbatch(WBatch& buf, const f16_t* frag0, size_t tile_stride, size_t term_stride, int batch) {
#pragma unroll
    for (int term = 0; term < 2; ++term)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int j = 0; j < kKB; ++j)
                buf.f[j].v[term][t] = *reinterpret_cast<const u32x4*>(frag0 + term * term_stride + t * tile_stride + (size_t)(kKB * batch + j) * 512);
    __builtin_amdgcn_sched_barrier(0);
}
// the LDS tile's fragments of a batch, both terms of both row tiles.  One wave per SIMD: nobody else covers an LDS round trip, so a
// batch's fragments are read a batch AHEAD of their use as well, during the previous batch's MFMAs.
struct ABatch { XFrag f[kKB]; };   // the k-steps of a batch, both terms of both row tiles each
__device__ __forceinline__ void read_abatch(ABatch& af, const unsigned char* a_lds, int batch, int nl, int kg) {
#pragma unroll
    for (int j = 0; j < kKB; ++j) {
        const unsigned char* p = a_lds + nl * kRowStride + (16 * (kKB * batch + j) + 8 * kg) * 2;
#pragma unroll
        for (int term = 0; term < 2; ++term) {
            af.f[j].v[term][0] = *reinterpret_cast<const u32x4*>(p + term * kLoOffset);
            af.f[j].v[term][1] = *reinterpret_cast<const u32x4*>(p + 32 * kRowStride + term * kLoOffset);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void mma_wbatch(f32x16 (&acc)[2][2], const WBatch& buf, const ABatch& a) {
#pragma unroll
    for (int j = 0; j < kKB; ++j) mma_split(acc, buf.f[j], a.f[j]);
    __builtin_amdgcn_sched_barrier(0);
}
// One 256-deep contraction of the split LDS tile against the split weights w.  bufa already holds batch 0; on return it holds batch 0 of
// `next` when next != nullptr.
__device__ __forceinline__ void mma_split256(f32x16 (&acc)[2][2], const unsigned char* a_lds, WBatch& bufa, WBatch& bufb, const f16_t* w,
                                             size_t tile_stride, size_t term_stride, const f16_t* next, size_t next_tile_stride,
                                             size_t next_term_stride, int nl, int kg) {
    ABatch afa, afb;
    read_abatch(afa, a_lds, 0, nl, kg);
#pragma unroll
    for (int bt = 0; bt < kBatches; bt += 2) {
        load_wbatch(bufb, w, tile_stride, term_stride, bt + 1);
        read_abatch(afb, a_lds, bt + 1, nl, kg);
        mma_wbatch(acc, bufa, afa);
        if (bt + 2 < kBatches) {
            load_wbatch(bufa, w, tile_stride, term_stride, bt + 2);
            read_abatch(afa, a_lds, bt + 2, nl, kg);
        } else if (next != nullptr) load_wbatch(bufa, next, next_tile_stride, next_term_stride, 0);
        mma_wbatch(acc, bufb, afb);
    }
}

__global__ void __launch_bounds__(kThreads)
ffn_f32_kernel(const float* __restrict__ X, const f16_t* __restrict__ W1, const float* __restrict__ B1, const f16_t* __restrict__ W2,
               const float* __restrict__ B2, float* __restrict__ Y, const FfnF32Dims dm) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const xs = smem;             // split x tile
    unsigned char* const hs = smem + kTile;     // split hidden chunk, then the fp32 output staging
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nl = lane & 31, kg = lane >> 5;
    const int grp = tid / kRowLanes, l16 = tid % kRowLanes;
    const int F = dm.F;
    const size_t term1 = (size_t)F * 256, term2 = term1;   // elements between a weight's packed hi and lo matrices

    float* const b1s = reinterpret_cast<float*>(smem + 2 * kTile);
    int* const kc1s = reinterpret_cast<int*>(b1s + F);
    float* const b2s = reinterpret_cast<float*>(kc1s + F);
    int* const kc2s = reinterpret_cast<int*>(b2s + 256);
    int* const krow_s = kc2s + 256;
    unsigned* const red = reinterpret_cast<unsigned*>(krow_s + kRows);   // [wave][row]
    for (int i = tid; i < F; i += kThreads) {
        b1s[i] = B1 ? B1[i] : 0.f;
        kc1s[i] = reinterpret_cast<const int*>(W1 + 2 * term1)[i];
    }
    b2s[tid] = B2 ? B2[tid] : 0.f;
    kc2s[tid] = reinterpret_cast<const int*>(W2 + 2 * term2)[tid];

    const int fs = F / 16;  // k-steps per output-column tile of the packed W2
    auto w1_frag = [&](int r0) { return W1 + ((size_t)((r0 + 64 * wave) / 32) * 16 * 64 + lane) * 8; };  // tile stride 16 * 512
    auto w2_frag = [&](int r0) { return W2 + (((size_t)(2 * wave) * fs + r0 / 16) * 64 + lane) * 8; };     // tile stride fs * 512

    // thread -> rows grp + 16 it of a tile, channels 64 j + 4 l16 .. + 3; rows past the end are read from the last row and never stored
    u32x4 stage[kPasses][4];
    auto fetch = [&](int tl) {
#pragma unroll
        for (int it = 0; it < kPasses; ++it) {
            long row = (long)tl * kRows + grp + kPassRows * it;
            row = row < dm.M ? row : dm.M - 1;
#pragma unroll
            for (int j = 0; j < 4; ++j) stage[it][j] = *reinterpret_cast<const u32x4*>(X + row * 256 + 64 * j + 4 * l16);
        }
    };

    int tile = blockIdx.x;
    if (tile >= dm.tiles) return;
    fetch(tile);
    WBatch bufa, bufb;

    for (; tile < dm.tiles; tile += gridDim.x) {
        // ---- the rows' powers of two, then x 2^-k -> (hi, lo) -> LDS -----------------------------------------------------------------
#pragma unroll
        for (int it = 0; it < kPasses; ++it) {
            unsigned m = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) m = finite_mag4(m, stage[it][j]);
            // (row_exponent's body: through the helper one more instruction, decoder ffn 53.2 -> 53.8 us against spreads of 0.2 and 0.3)
#pragma unroll
            for (int o = kRowLanes / 2; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
            const int k = split_exponent(m);
            const float down = ldexpf(1.0f, -k);
            const int row = grp + kPassRows * it;
            if (l16 == 0) krow_s[row] = k;
#pragma unroll
            for (int j = 0; j < 4; ++j) park4(xs + row * kRowStride + (64 * j + 4 * l16) * 2, kLoOffset, stage[it][j], down);
        }
        if (tile + (int)gridDim.x < dm.tiles) fetch(tile + gridDim.x);   // in flight through this tile's products
        load_wbatch(bufa, w1_frag(0), (size_t)16 * 512, term1, 0);
        __syncthreads();

        f32x16 acc2[2][2];  // [row tile][column tile] of this wave's 64 output columns
        zero_acc(acc2);

        for (int r0 = 0; r0 < F; r0 += 256) {
            // ---- phase 1: this wave's 64 hidden units of the chunk ----------------------------------------------------------------------
            f32x16 acc1[2][2];
            zero_acc(acc1);
            const f16_t* w2p = w2_frag(r0);
            mma_split256(acc1, xs, bufa, bufb, w1_frag(r0), (size_t)16 * 512, term1, w2p, (size_t)fs * 512, term2, nl, kg);
            // lane = row 32 a + nl, registers 4 q .. 4 q + 3 = units r0 + 64 wave + 32 b + 8 q + 4 kg .. + 3 (mfma_tile.hpp)
            unsigned m[2] = {0u, 0u};
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int krow = krow_s[32 * a + nl];
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int c = r0 + 64 * wave + 32 * b + 8 * q + 4 * kg;
                        const f32x4 bb = *reinterpret_cast<const f32x4*>(b1s + c);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float v = relu_keep_nan(ldexpf(acc1[a][b][4 * q + e], krow + kc1s[c + e]) + bb[e]);
                            acc1[a][b][4 * q + e] = v;
                            m[a] = max(m[a], finite_mag(__float_as_uint(v)));
                        }
                    }
                m[a] = max(m[a], (unsigned)__shfl_xor((int)m[a], 32, 64));
                if (kg == 0) red[wave * kRows + 32 * a + nl] = m[a];
            }
            __syncthreads();  // the four waves' maxima of every row are in LDS

            // ---- the chunk's power of two per row; h 2^-k -> (hi, lo) -> LDS ---------------------------------------------------------------
            int kh[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int row = 32 * a + nl;
                const unsigned mm = max(max(red[row], red[kRows + row]), max(red[2 * kRows + row], red[3 * kRows + row]));
                kh[a] = split_exponent(mm);
                const float down = ldexpf(1.0f, -kh[a]);
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int c = 64 * wave + 32 * b + 8 * q + 4 * kg;
                        park4(hs + row * kRowStride + c * 2, kLoOffset, acc1[a][b][4 * q], acc1[a][b][4 * q + 1], acc1[a][b][4 * q + 2],
                              acc1[a][b][4 * q + 3], down);
                    }
            }
            __syncthreads();  // the whole split 64 x 256 hidden chunk is in LDS

            // ---- phase 2: a fresh accumulator for the chunk, then y_acc += 2^(k_row,chunk + k_column) acc -----------------------------------
            zero_acc(acc1);
            mma_split256(acc1, hs, bufa, bufb, w2p, (size_t)fs * 512, term2, r0 + 256 < F ? w1_frag(r0 + 256) : nullptr, (size_t)16 * 512,
                         term1, nl, kg);
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int c = 64 * wave + 32 * b + 8 * q + 4 * kg;
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc2[a][b][4 * q + e] += ldexpf(acc1[a][b][4 * q + e], kh[a] + kc2s[c + e]);
                    }
            __syncthreads();  // everyone is done reading the chunk (and the maxima) before they are overwritten
        }

        // ---- epilogue: + b2 -> fp32 staging (the hidden-chunk buffer) -> whole rows ---------------------------------------------------------
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = 64 * wave + 32 * b + 8 * q + 4 * kg;
                    const f32x4 bb = *reinterpret_cast<const f32x4*>(b2s + c);
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc2[a][b][4 * q + e] + bb[e];
                    *reinterpret_cast<f32x4*>(hs + (32 * a + nl) * kRowStride + c * 4) = v;
                }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kRows * 64 / kThreads; ++j) {
            const int p = tid + kThreads * j;
            const long row = (long)tile * kRows + (p >> 6);
            if (row < dm.M)
                *reinterpret_cast<f32x4*>(Y + row * 256 + (p & 63) * 4) = *reinterpret_cast<const f32x4*>(hs + (p >> 6) * kRowStride + (p & 63) * 16);
        }
        __syncthreads();  // staging, x tile and the rows' exponents are rewritten by the next tile
    }
}

}  // namespace

int ffn_f32(const void* x, const void* w1_split, const void* b1, const void* w2_split, const void* b2, void* y, long M, int F,
            hipStream_t stream, const char* what) {
    FfnF32Dims dm;
    dm.M = M; dm.F = F; dm.tiles = (int)((M + kRows - 1) / kRows);
    const size_t lds = 2 * (size_t)kTile + tail_bytes(F);
    if (lds > (size_t)kLdsLimit) return fail(ALO_ERR_UNSUPPORTED, "%s: hidden width %d needs %zu bytes of LDS", what, F, lds);
    const int gx = dm.tiles < 256 ? dm.tiles : 256;   // one workgroup per CU
    void* args[] = {&x, &w1_split, &b1, &w2_split, &b2, &y, &dm};
    return launch<ffn_f32_kernel>(gx, kThreads, lds, stream, what, args);
}

}  // namespace alo
