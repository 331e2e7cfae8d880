// Y (M, N) = act(X (M, K) @ W (N, K)^T + bias [+ R]), fp32 in and out, on the fp16 matrix cores at fp32-class accuracy: the two-term split
// arithmetic of split_f16.hpp (scale, split, non-finite rule, term order, undo) in conv3x3_f32_kernel's frame with ONE tap — the fp32
// flavour of alo_linear_packed and of alo_conv1x1_nhwc (the detector's 1x1 convolutions, input projections and transformer matrices in
// fp32 mode).
//
//   * scale: one power of two per ROW, found by a first sweep over the tile's rows inside the kernel — 16 lanes per row, the very lanes
//     that later park that row, so the scale stays in their registers — and a row's result does not depend on any other row of the
//     call.  The raw fp32 rows travel through registers one chunk ahead and are split where the tile is parked in LDS; a non-finite
//     element spoils exactly its own row.
//   * weights: split once by the caller, one power of two per output channel: the layout of conv3x3_f32_kernel for a (N, K) matrix.
//   * epilogue: the undo by k_row + k_channel, + bias, + residual (fp32, before the activation), ReLU, fp32 stores in whole 256-byte runs
//     through LDS.
//
// Tile: 64 rows x 128 columns on two waves (64 each, 2 x 2 MFMA tiles); 64 input channels (four k-steps) are staged per barrier pair, a
// row's hi terms and lo terms side by side; N == 64: the two waves take every other k-step and wave 0 adds wave 1's sums (a fixed
// order).  Rows are addressed through RowGather (common.hpp), so a strided 1x1 convolution reads the kept pixels itself.  Persistent
// workgroups, one contiguous eighth of the row tiles per XCD; weight fragments through two register buffers.
#include "mfma_tile.hpp"
#include "split_f16.hpp"

namespace alo {
namespace {

constexpr int kRows = 64;                         // rows per tile
constexpr int kThreads = 128;                     // two waves
constexpr int kChunk = 64;                        // input channels staged at once
constexpr int kSteps = kChunk / 16;               // k-steps per chunk
constexpr int kLoOffset = kChunk * 2;             // a staged row: kChunk hi terms, then kChunk lo terms
constexpr int kRowStride = kChunk * 4 + 16;       // (+16: conflict-free 16-byte reads)
constexpr int kRowLanes = kChunk / 4;             // lanes per staged row: one 16-byte piece (four fp32 channels) each
constexpr int kPassRows = kThreads / kRowLanes;   // rows staged per pass of the workgroup
constexpr int kLoads = kRows / kPassRows;         // passes = pieces per thread and chunk
constexpr int kTile = kRows * kRowStride;
constexpr int kStaging = kRedOffset + 64 * 64 * 4;        // the epilogue's staging aliases the tile
constexpr int kLds = kTile > kStaging ? kTile : kStaging;
constexpr int kTail = kThreads * 8 + kRows * 20;  // behind both: bias and channel exponents of the column block; the rows' exponents; their offsets, twice
static_assert(kLds % 16 == 0 && kStaging >= 2 * kOutBytes && kLoads * kThreads == kRows * kRowLanes, "16-byte LDS accesses; both waves' blocks");

struct F32Dims {
    long M;
    int N, K, tiles, relu;
    RowGather g;
};

template <bool KSPLIT>
__global__ void __launch_bounds__(kThreads, 2)
linear_f32_kernel(const float* __restrict__ X, const f16_t* __restrict__ Wp, const float* __restrict__ bias, const float* __restrict__ R,
                  float* __restrict__ Y, const F32Dims dm) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const xs = smem;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nl = lane & 31, kg = lane >> 5;
    const int grp = tid / kRowLanes, l16 = tid % kRowLanes;   // staging: kRowLanes lanes per row
    const int col0 = KSPLIT ? blockIdx.y * 64 : blockIdx.y * 128 + wave * 64;  // this wave's 64 output columns
    const bool has_cols = col0 < dm.N;                                  // N % 64 == 0
    const size_t term_stride = (size_t)dm.N * dm.K;                     // elements between the packed hi and lo matrices
    float* const bias_s = reinterpret_cast<float*>(smem + kLds);
    int* const kc_s = reinterpret_cast<int*>(smem + kLds + kThreads * 4);
    int* const krow_s = reinterpret_cast<int*>(smem + kLds + kThreads * 8);
    long* rows = reinterpret_cast<long*>(smem + kLds + kThreads * 8 + kRows * 4);   // this tile's row offsets, and behind them
    long* rows_next = rows + kRows;                                                   // the next tile's (written while this tile's are read)
    fill_channel_tables<KSPLIT>(bias_s, kc_s, bias, reinterpret_cast<const int*>(Wp + 2 * term_stride), KSPLIT ? blockIdx.y * 64 : blockIdx.y * 128,
                                dm.N, tid);

    // persistent workgroups, one contiguous eighth of the row tiles per XCD (see conv3x3_kernel)
    const TileRange range = xcd_tile_range(dm.tiles);
    const int tile_end = range.end, lanes_per_xcd = range.step;
    int tile = range.first;
    if (tile >= tile_end) return;

    const size_t ctile_stride = (size_t)(dm.K / 16) * 512;             // elements between the packed column tiles
    const f16_t* wfrag = Wp + (size_t)(col0 / 32) * ctile_stride + lane * 8;

    // this wave's k-steps of a chunk: all of them, or every other one when the two waves split K
    const int my_batches = KSPLIT ? kSteps / 2 : kSteps;
    auto batch = [&](int i) { return KSPLIT ? wave + 2 * i : i; };

    // where a tile's rows start in X (elements): found once per tile by the first 64 threads (a strided convolution divides), read from
    // LDS by whoever loads; rows past the end are read from the last row and never stored
    auto tile_rows = [&](int tl, long* to) {
        if (tid < kRows) {
            long row = (long)tl * kRows + tid;
            row = row < dm.M ? row : dm.M - 1;
            to[tid] = gather_row(dm.g, row) * dm.K;
        }
    };
    // thread -> rows grp + kPassRows it, channels 4 l16 .. + 3 of a chunk
    auto piece = [&](int it, int c0) { return reinterpret_cast<const u32x4*>(X + rows[grp + kPassRows * it] + c0 + l16 * 4); };
    // raw fp32 pieces travel through registers and are requested one (tile, chunk) AHEAD of their use
    u32x4 stage[kLoads];
    auto load_chunk = [&](int c0) {
#pragma unroll
        for (int it = 0; it < kLoads; ++it) stage[it] = *piece(it, c0);
    };
    tile_rows(tile, rows);
    __syncthreads();
    load_chunk(0);

    for (; tile < tile_end; tile += lanes_per_xcd) {
        // first sweep: the rows' largest finite magnitudes -> their powers of two; the 16 lanes of a row all end up with it
        float down[kLoads];
        {
            unsigned m[kLoads];
#pragma unroll
            for (int it = 0; it < kLoads; ++it) m[it] = 0u;
#pragma unroll 1
            for (int c0 = 0; c0 < dm.K; c0 += kChunk) {
#pragma unroll
                for (int it = 0; it < kLoads; ++it) m[it] = finite_mag4(m[it], *piece(it, c0));
            }
#pragma unroll
            for (int it = 0; it < kLoads; ++it) {
                const int k = row_exponent<kRowLanes>(m[it]);
                down[it] = ldexpf(1.0f, -k);
                if (l16 == 0) krow_s[grp + kPassRows * it] = k;     // read by the epilogue, behind the chunk loop's barriers
            }
        }

        f32x16 acc[2][2];  // [row tile][column tile]
        zero_acc(acc);

        for (int c0 = 0; c0 < dm.K; c0 += kChunk) {
            // weights of k-step ks of this chunk, both terms
            auto load_w = [&](WFrag& f, int ks) { load_wfrag(f, wfrag + (size_t)(c0 / 16 + ks) * 512, term_stride, ctile_stride); };
            auto compute = [&](const WFrag& f, int ks) {
                const unsigned char* a_base = xs + nl * kRowStride + kg * 16 + ks * 32;
                XFrag x;
#pragma unroll
                for (int term = 0; term < 2; ++term) {
                    x.v[term][0] = *reinterpret_cast<const u32x4*>(a_base + term * kLoOffset);
                    x.v[term][1] = *reinterpret_cast<const u32x4*>(a_base + 32 * kRowStride + term * kLoOffset);
                }
                mma_split(acc, f, x);
            };
            WFrag w0, w1;
            if (has_cols) load_w(w0, batch(0));

            // park the chunk: four channels of one row -> four hi terms and four lo terms
#pragma unroll
            for (int it = 0; it < kLoads; ++it) park4(xs + (grp + kPassRows * it) * kRowStride + l16 * 8, kLoOffset, stage[it], down[it]);
            const bool last = c0 + kChunk >= dm.K, more = tile + lanes_per_xcd < tile_end;
            if (last && more) tile_rows(tile + lanes_per_xcd, rows_next);
            __syncthreads();
            if (!last) load_chunk(c0 + kChunk);
            else if (more) {   // every load of this tile has been issued
                long* const t = rows; rows = rows_next; rows_next = t;
                load_chunk(0);
            }

            if (has_cols) {   // (this loop as a shared function over the three lambdas: <true> 220 -> 234 VGPRs)
#pragma unroll 1
                for (int i = 0; i < my_batches; i += 2) {
                    if (i + 1 < my_batches) load_w(w1, batch(i + 1));
                    compute(w0, batch(i));
                    if (i + 2 < my_batches) load_w(w0, batch(i + 2));
                    if (i + 1 < my_batches) compute(w1, batch(i + 1));
                }
            }
            __syncthreads();  // the tile is overwritten by the next chunk (and by the epilogue's staging)
        }

        if (KSPLIT) {  // wave 1 hands its partial sums to wave 0
            float* red = reinterpret_cast<float*>(smem + kRedOffset);
            ALO_KSPLIT_HANDOFF(acc, red, wave, lane);
        }

        if (has_cols && !(KSPLIT && wave == 1)) {
            unsigned char* const obuf = smem + (KSPLIT ? 0 : wave) * kOutBytes;
            const int cs0 = (KSPLIT ? 0 : wave) * 64;    // this wave's first channel in bias_s / kc_s
            const long row0 = (long)tile * kRows;
            const bool relu_first = dm.relu && R == nullptr;
            // lane = row 32 a + nl, registers 4 q .. 4 q + 3 = channels col0 + 32 b + 8 q + 4 kg .. + 3 (mfma_tile.hpp): one row tile at a
            // time -> 2^(k_row + k_channel), bias (ReLU), one 16-byte LDS write per quad; then 16 lanes x 16 B per row (+ identity, ReLU).
            // (stage_scaled_quads' body: through the helper, encoder linear1 went 690.9 -> 699.6 us against spreads of 8.0 and 2.6)
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int krow = krow_s[32 * a + nl];
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int c = 32 * b + 8 * q + 4 * kg;
                        const f32x4 bb = *reinterpret_cast<const f32x4*>(bias_s + cs0 + c);
                        f32x4 v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            v[e] = ldexpf(acc[a][b][4 * q + e], krow + kc_s[cs0 + c + e]) + bb[e];
                            if (relu_first) v[e] = relu_keep_nan(v[e]);
                        }
                        *reinterpret_cast<f32x4*>(obuf + nl * kOutStride + c * 4) = v;
                    }
                wave_lds_fence();
#pragma unroll
                for (int pass = 0; pass < 8; ++pass) {
                    const int row = pass * 4 + (lane >> 4);
                    const long grow = row0 + 32 * a + row;
                    if (grow < dm.M) {
                        const size_t at = (size_t)grow * dm.N + col0 + (lane & 15) * 4;
                        f32x4 v = *reinterpret_cast<const f32x4*>(obuf + row * kOutStride + (lane & 15) * 16);
                        if (R != nullptr) {
                            const f32x4 idn = *reinterpret_cast<const f32x4*>(R + at);
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                v[e] += idn[e];
                                if (dm.relu) v[e] = relu_keep_nan(v[e]);
                            }
                        }
                        *reinterpret_cast<f32x4*>(Y + at) = v;
                    }
                }
                wave_lds_fence();   // the block is read out before the second row tile lands on it
            }
        }
        __syncthreads();  // the staging and the rows' exponents are read out before the next tile lands on them
    }
}

template <bool KSPLIT>
int launch_f32(const void* x, const void* w, const void* bias, const void* residual, void* y, const F32Dims& dm, hipStream_t stream,
               const char* what) {
    void* args[] = {&x, &w, &bias, &residual, &y, const_cast<F32Dims*>(&dm)};
    const unsigned gy = KSPLIT ? dm.N / 64 : (dm.N + 127) / 128;
    const unsigned gx = xcd_grid(dm.tiles, 128);   // 32 CUs per XCD x up to 4 resident workgroups
    return launch<linear_f32_kernel<KSPLIT>>(dim3(gx, gy), kThreads, kLds + kTail, stream, what, args);
}

}  // namespace

int linear_f32(const void* x, const void* w_split, const void* bias, const void* residual, void* y, long M, int N, int K, int relu,
               const RowGather& gather, hipStream_t stream, const char* what) {
    F32Dims dm;
    dm.M = M; dm.N = N; dm.K = K; dm.relu = relu; dm.g = gather;
    dm.tiles = (int)((M + kRows - 1) / kRows);
    return N == 64 ? launch_f32<true>(x, w_split, bias, residual, y, dm, stream, what)
                   : launch_f32<false>(x, w_split, bias, residual, y, dm, stream, what);
}

}  // namespace alo
