// Y (M, N) = act(X (M, K) @ W (N, K)^T + bias), K in {64, 128, 256}, bf16 or fp16 with fp32 accumulation: the short-K linear layers
// around the attention op — MSDeformAttn's value_proj / sampling_offsets / attention_weights / output_proj and the FFN's
// first layer over the encoder's 177784 rows, the backbone's 1x1 convolutions with few input channels over NHWC rows.
//
// These products are memory bound (23 GFLOP against 182 MB at N = 256) and the library kernel PyTorch reaches streams them
// at 2.8 TB/s.  This kernel is built around the stream instead of around the tile:
// The kernels are templated on the 16-bit storage type T (bf16_t / f16_t): same tiles, same operand layout, v_mfma_f32_32x32x16_bf16
// or _f16, one rounding to nearest even per stored result (the comments below say bf16 for both).
//   * the WEIGHTS never move: each of a workgroup's 4 waves keeps its 64 output columns of W (64 x 256 bf16 = 128 VGPRs) in
//     registers for the whole launch, already in the lane order v_mfma_f32_32x32x16_bf16 wants for its B operand;
//   * X streams through: persistent workgroups walk 64-row tiles; a tile is fetched with fully coalesced 16-byte loads
//     (one 512-byte row per 32 lanes) into registers while the previous tile is being multiplied, parked in LDS and read
//     back as A fragments by all four waves;
//   * Y leaves through LDS as well, so that every store instruction writes whole 128-byte lines (the MFMA accumulator
//     layout has a lane own one column and 16 scattered rows).
#include "mfma_tile.hpp"

namespace alo {
namespace {

constexpr int kRows = 64;               // rows of X per tile
constexpr int kOutStride = 64 * 2 + 16; // LDS row stride of a wave's 32 x 64 output block

struct GemmDims {
    long M;
    int N;
    int tiles;  // ceil(M / kRows)
    int S;      // head-major output only: rows per batch item
    RowGather g;
};

// HM = true (value_proj of MSDeformAttn): y is written HEAD-major, (batch, N / 32 heads, S, 32), and rows whose padding-mask
// byte is set are written as zeros — `value.masked_fill(mask, 0)` and the re-layout the head-major attention kernel wants,
// for free in the epilogue (a wave's 64 columns are two heads; 16 rows of a head are 1 KB contiguous).  R then carries the
// (M,) uint8 mask (or NULL) and dm.S the rows per batch item.
template <typename T, int kK, bool RELU, bool HAS_RES, bool HM>
__global__ void __launch_bounds__(256, 2)
linear_shortk_kernel(const T* __restrict__ X, const T* __restrict__ W, const T* __restrict__ bias,
                     const T* __restrict__ R, T* __restrict__ Y, const GemmDims dm) {
    constexpr int kRowBytes = kK * 2 + 16;  // LDS row stride of the X tile: +16 B keeps the 16-byte fragment reads conflict-free
    constexpr int kSteps = kK / 16;         // MFMA k-steps per tile
    constexpr int kPieces = kK / 8;         // 16-byte pieces per row
    constexpr int kLoads = kRows * kPieces / 256;
    static_assert(kRows * kPieces % 256 == 0, "the tile loader gives every thread the same number of pieces");
    // The identity is requested ahead of the product at K = 64 and 128.  At K = 256 its 8 x u32x4 beside 128 VGPRs of weights spill
    // into the tile loop, and warming the lines with one dword each made the launch slower (docs/experiments.md): store_rows loads it.
    constexpr bool kAhead = HAS_RES && !HM && kK <= 128;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const xbuf = smem;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    unsigned char* obuf = smem + kRows * kRowBytes + wave * (kRows * kOutStride);  // per-wave output staging

    const int col0 = blockIdx.y * 256 + wave * 64;  // this wave's 64 output columns
    const bool has_cols = col0 < dm.N;              // N is a multiple of 64
    const int nl = lane & 31, kg = lane >> 5;       // MFMA lane roles: row/column inside a 32-tile, 8-element k group

    // ---- resident B operand: W[col0 + 32 t + nl][16 s + 8 kg .. + 8) for t < 2, s < kSteps ----------------------------------
    // W is the MFMA's ROW operand (the product is computed transposed, Y^T = W X^T), so that a lane ends up holding 2 x 16
    // output columns of ONE row of the tile, four consecutive columns per accumulator quad: they leave as 8-byte LDS writes.
    u32x4 wreg[2][kSteps];
    // bias in accumulator order, [kg][t][16]: register r of lane (nl, kg) is column 32 t + (r & 3) + 8 (r >> 2) + 4 kg; the
    // accumulators start from it
    float* const bias_tab = reinterpret_cast<float*>(smem + kRows * kRowBytes + 4 * (kRows * kOutStride)) + wave * 64;
    if (has_cols) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const T* wr = W + (size_t)(col0 + 32 * t + nl) * kK + 8 * kg;
#pragma unroll
            for (int s = 0; s < kSteps; ++s) wreg[t][s] = *reinterpret_cast<const u32x4*>(wr + 16 * s);
        }
        const int r = lane & 15, t = (lane >> 4) & 1, k2 = lane >> 5;
        bias_tab[lane] = bias != nullptr ? ld(&bias[col0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * k2]) : 0.f;
    }

    // ---- tile loader: kRows rows x 2K bytes in 16-byte pieces; thread -> (row, piece) keeps rows contiguous.  Rows past the
    // end are read from the last row (and never stored), so the requests of a tile go out back to back, unpredicated -----------
    auto fetch = [&](int tile, u32x4 (&r)[kLoads]) {
#pragma unroll
        for (int j = 0; j < kLoads; ++j) {
            const int p = tid + 256 * j;  // piece index: row = p / kPieces, 16-byte column = p % kPieces
            long row = (long)tile * kRows + p / kPieces;
            row = gather_row(dm.g, row < dm.M ? row : dm.M - 1);
            r[j] = *reinterpret_cast<const u32x4*>(X + row * kK + (p % kPieces) * 8);
        }
    };

    int tile = blockIdx.x;
    if (tile >= dm.tiles) return;
    u32x4 stage[kLoads];
    fetch(tile, stage);

    for (;;) {
        park_tile<kPieces>(xbuf, kRowBytes, stage, tid);
        __syncthreads();  // the tile is in LDS
        const int next = tile + gridDim.x;
        const bool more = next < dm.tiles;
        // the identity of THIS tile, in store order: requested here, wanted after the product (fetch_identity of mfma_tile.hpp)
        u32x4 idn[8];
        if constexpr (kAhead) {
            if (has_cols) fetch_identity(idn, R, (long)tile * kRows, dm.M, dm.N, col0, lane);
        }
        if (more) fetch(next, stage);  // in flight during the MFMAs and the stores below

        if (has_cols) {
#pragma unroll
            for (int half = 0; half < kRows / 32; ++half) {  // 32 rows at a time through the same accumulators
                f32x16 acc[2];
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const f32x4 b4 = *reinterpret_cast<const f32x4*>(bias_tab + (kg * 2 + t) * 16 + 4 * q);
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[t][4 * q + i] = b4[i];
                    }
#pragma unroll
                for (int s = 0; s < kSteps; ++s) {
                    // X fragment: X[tile row 32 half + nl][16 s + 8 kg .. + 8)
                    const u32x4 a = *reinterpret_cast<const u32x4*>(xbuf + (32 * half + nl) * kRowBytes + (16 * s + 8 * kg) * 2);
                    acc[0] = mfma_32x32x16<T>(wreg[0][s], a, acc[0]);
                    acc[1] = mfma_32x32x16<T>(wreg[1][s], a, acc[1]);
                }
                // lane = tile row 32 half + nl -> bf16 -> LDS [row][col]
                stage_quads<T, false>(obuf, kOutStride, acc, nullptr, RELU && !HAS_RES, 32 * half + nl, 0, kg);
            }
            wave_lds_fence();
            if constexpr (HM) {
                // per head (32 columns = 64 B per row): 4 lanes x 16 B per row, 16 consecutive rows = 1 KB per store instruction
                const unsigned char* mask = reinterpret_cast<const unsigned char*>(R);
                const int heads = dm.N / 32;
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
#pragma unroll
                    for (int pass = 0; pass < kRows / 16; ++pass) {
                        const int row = pass * 16 + (lane >> 2);
                        const long grow = (long)tile * kRows + row;
                        if (grow < dm.M) {
                            u32x4 v = *reinterpret_cast<const u32x4*>(obuf + row * kOutStride + hh * 64 + (lane & 3) * 16);
                            if (mask != nullptr && mask[grow]) v = u32x4{0u, 0u, 0u, 0u};
                            const long nb = grow / dm.S, sp = grow - nb * dm.S;
                            const int head = col0 / 32 + hh;
                            *reinterpret_cast<u32x4*>(Y + ((nb * heads + head) * dm.S + sp) * 32 + (lane & 3) * 8) = v;
                        }
                    }
                }
            } else if constexpr (kAhead) {
                store_rows_fetched<T, RELU>(Y, idn, obuf, kOutStride, (long)tile * kRows, dm.M, dm.N, col0, lane);
            } else {
                store_rows<T, RELU, HAS_RES>(Y, R, obuf, kOutStride, (long)tile * kRows, dm.M, dm.N, col0, lane);
            }
        }
        if (!more) break;
        __syncthreads();  // every wave has finished reading the tile: it may be overwritten
        tile = next;
    }
}

}  // namespace
}  // namespace alo

using namespace alo;

namespace {
// storage type and K of a launch as ONE template argument (ALO_RELU_RES takes a single leading argument)
template <typename T, int kK>
struct ShortK {
    using type = T;
    static constexpr int K = kK;
};

template <class Cfg, bool RELU, bool HAS_RES, bool HM = false>
int launch_shortk(const void* x, const void* weight, const void* bias, const void* residual, void* y, long M, int N,
                  hipStream_t stream, int S = 0, const RowGather& gather = row_gather()) {
    GemmDims dm;
    dm.M = M; dm.N = N; dm.tiles = (int)((M + kRows - 1) / kRows); dm.S = S; dm.g = gather;
    constexpr int K = Cfg::K;
    const size_t lds = kRows * (K * 2 + 16) + 4 * kRows * kOutStride + 4 * 64 * sizeof(float);
    const int cols = (N + 255) / 256;
    int gx = 512 / cols;  // persistent: about two workgroups per CU in total
    if (gx > dm.tiles) gx = dm.tiles;
    if (gx < 1) gx = 1;
    void* args[] = {&x, &weight, &bias, &residual, &y, &dm};
    return launch<linear_shortk_kernel<typename Cfg::type, K, RELU, HAS_RES, HM>>(dim3(gx, cols), 256, lds, stream, "alo_linear_shortk", args);
}

// K -> f(ShortK<T, K>{}); the one K dispatch of the file (the entry points have checked K, alo_conv1x1_nhwc relies on this check)
template <typename T, typename F>
int with_shortk(int K, F&& f) {
    if (K == 64) return f(ShortK<T, 64>{});
    if (K == 128) return f(ShortK<T, 128>{});
    if (K == 256) return f(ShortK<T, 256>{});
    return fail(ALO_ERR_UNSUPPORTED, "alo_conv1x1_nhwc: the resident-weight kernel needs Cin in (64, 128, 256), got %d", K);
}

// K x relu x residual -> the launch, for storage type T
template <typename T>
int dispatch_shortk(const void* x, const void* weight, const void* bias, const void* residual, void* y, long M, int N, int K, int relu,
                    const RowGather& gather, hipStream_t stream) {
    return with_shortk<T>(K, [&](auto cfg) {
        using Cfg = decltype(cfg);
        return ALO_RELU_RES(launch_shortk, Cfg, relu, residual, x, weight, bias, residual, y, M, N, stream, 0, gather);
    });
}
}  // namespace

extern "C" int alo_linear_shortk(const void* x, const void* weight, const void* bias, const void* residual, void* y, long M,
                                 int N, int K, int relu, int dtype, void* stream) {
    ALO_REQUIRE(dtype == ALO_BF16 || dtype == ALO_F16, ALO_ERR_UNSUPPORTED, "alo_linear_shortk: bf16 / fp16 only (dtype %d)", dtype);
    ALO_REQUIRE(x && weight && y, ALO_ERR_INVALID_ARGUMENT, "alo_linear_shortk: null pointer argument");
    ALO_REQUIRE(M > 0 && N > 0 && N % 64 == 0, ALO_ERR_INVALID_ARGUMENT,
                "alo_linear_shortk: M must be positive and N a positive multiple of 64 (M=%ld N=%d)", M, N);
    ALO_REQUIRE(K == 64 || K == 128 || K == 256, ALO_ERR_UNSUPPORTED, "alo_linear_shortk: K must be 64, 128 or 256, got %d", K);
    ALO_REQUIRE(aligned16(x, weight, y, residual), ALO_ERR_INVALID_ARGUMENT, "alo_linear_shortk: pointers must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    return with_storage_type(dtype, [&](auto t) { return dispatch_shortk<decltype(t)>(x, weight, bias, residual, y, M, N, K, relu, row_gather(), st); });
}

// 1x1 convolution with a spatial stride over an NHWC map, resident-weight flavour: the kept pixels are addressed by the tile
// loader itself (no gathered copy of the input): alo_linear_shortk with the identity gather, alo_conv1x1_nhwc (gemm_packed.hip)
// for unpacked weights.  bf16 (the backbone's kernels are).
int alo::linear_shortk_gather(const void* x, const void* weight, const void* bias, const void* residual, void* y, long M, int N, int K,
                              int relu, const RowGather& gather, hipStream_t stream) {
    return dispatch_shortk<bf16_t>(x, weight, bias, residual, y, M, N, K, relu, gather, stream);
}

// ------------------------------------------------------------------------------------------------------------------
// The transformer layer's feed-forward block in one kernel:  y = relu(x W1^T + b1) W2^T + b2,  x, y (M, 256), hidden F.
// W1 / W2 arrive PACKED in MFMA fragment order (alo_pack_mfma_b: [row tile of 32][k step of 16][lane = 32 kg + n][8]).
//
// Run as two library GEMMs the (M, F) hidden activation makes a round trip through HBM (2 x 364 MB at M = 177784, F = 1024)
// and the pair takes 316 us.  Here a workgroup owns 64 rows: it keeps them in LDS, produces the hidden activation 256
// units at a time (each wave 64 of them) straight into LDS as bf16, and immediately contracts that chunk into its
// 64 x 256 output accumulators (each wave 64 output columns), so the hidden tensor never exists in memory (it is rounded to the
// storage type, bf16 or fp16, on its way into LDS, as the two-launch path stores it).  The weights
// (2 x 512 KB, L2 resident) stream through registers; x is read once, y written once, in whole lines.
// ------------------------------------------------------------------------------------------------------------------
namespace alo {
namespace {

constexpr int kFfnRows = kTileRows;
constexpr int kFfnStride = kTileStride;  // LDS row stride of the 64 x 256 bf16 tiles (x, hidden chunk, output staging)

struct FfnDims {
    long M;
    int F;      // hidden width, multiple of 256
    int tiles;  // ceil(M / 64)
};

template <typename T>
__global__ void __launch_bounds__(256, 2)
ffn256_kernel(const T* __restrict__ X, const T* __restrict__ W1, const T* __restrict__ B1,
              const T* __restrict__ W2, const T* __restrict__ B2, T* __restrict__ Y, const FfnDims dm) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const xs = smem;                            // x tile        [64][256] bf16
    unsigned char* const hs = smem + kFfnRows * kFfnStride;    // hidden chunk  [64][256] bf16, then the output staging
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nl = lane & 31, kg = lane >> 5;
    const int F = dm.F;

    // biases as fp32 in LDS (b1: F values, b2: 256); the products are computed transposed (weights = the MFMA's row operand),
    // so a lane owns ONE row of the tile and four consecutive columns per accumulator quad: bias, activation and the bf16
    // conversion work on quads and leave as 8-byte LDS writes
    float* const b1s = reinterpret_cast<float*>(smem + 2 * kFfnRows * kFfnStride);
    float* const b2s = b1s + F;
    for (int i = tid; i < F; i += 256) b1s[i] = B1 ? ld(B1 + i) : 0.f;
    b2s[tid] = B2 ? ld(B2 + tid) : 0.f;

    // the weights stream through two register buffers, a batch ahead of their use (load_batch / mma_batch of mfma_tile.hpp)
    const int fs = F / 16;  // k steps per output-column tile of the packed W2
    // packed fragment (row tile, k step) = 64 lanes x 16 B contiguous: a load instruction reads 8 whole lines
    auto w1_frag = [&](int r0) { return W1 + ((size_t)((r0 + 64 * wave) / 32) * 16 * 64 + lane) * 8; };  // tile stride 16 * 512
    auto w2_frag = [&](int r0) { return W2 + (((size_t)(2 * wave) * fs + r0 / 16) * 64 + lane) * 8; };     // tile stride fs * 512

    for (int tile = blockIdx.x; tile < dm.tiles; tile += gridDim.x) {
        // ---- x tile -> LDS ------------------------------------------------------------------------------------------------
        {
            u32x4 xv[8];
            fetch_tile256(xv, X, (long)tile * kFfnRows, dm.M, tid);
            park_tile256(xs, xv, tid);
        }
        u32x4 bufa[2][kTileKB], bufb[2][kTileKB];
        load_batch(bufa, w1_frag(0), (size_t)16 * 512, 0);
        __syncthreads();

        f32x16 acc2[2][2];  // [row tile][column tile] of this wave's 64 output columns
        zero_acc(acc2);

        for (int r0 = 0; r0 < F; r0 += 256) {
            // ---- phase 1: this wave's 64 hidden units of the chunk: h = relu(x W1[r0 + 64 wave + ...]^T + b1) ----------------
            f32x16 acc1[2][2];
            zero_acc(acc1);
            const T* w1p = w1_frag(r0);
            const T* w2p = w2_frag(r0);
            mma_tile256(acc1, xs, bufa, bufb, w1p, (size_t)16 * 512, w2p, (size_t)fs * 512, nl, kg);
            stage_tile256<true, true, T>(hs, acc1, b1s + r0, wave, nl, kg);
            __syncthreads();  // the whole 64 x 256 hidden chunk is in LDS

            // ---- phase 2: out[:, 64 wave ..] += h_chunk (64 x 256) W2[64 wave + ..][r0 .. r0 + 256)^T ------------------------
            mma_tile256(acc2, hs, bufa, bufb, w2p, (size_t)fs * 512, r0 + 256 < F ? w1_frag(r0 + 256) : nullptr, (size_t)16 * 512, nl, kg);
            __syncthreads();  // everyone is done reading the chunk before it is overwritten
        }

        // ---- epilogue: + b2 -> bf16 -> staging (the hidden-chunk buffer) -> whole-line stores ---------------------------------
        stage_tile256<true, false, T>(hs, acc2, b2s, wave, nl, kg);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int p = tid + 256 * j;
            const long row = (long)tile * kFfnRows + (p >> 5);
            if (row < dm.M)
                *reinterpret_cast<u32x4*>(Y + row * 256 + (p & 31) * 8) =
                    *reinterpret_cast<const u32x4*>(hs + (p >> 5) * kFfnStride + (p & 31) * 16);
        }
        __syncthreads();  // staging and x tile are rewritten by the next tile
    }
}

}  // namespace
}  // namespace alo

namespace alo {
namespace {
// (16-bit elements, moved as bits: bf16 and fp16 weights take the same kernel)
// W (N, K) row-major -> fragments [N / 32][K / 16][64 lanes][8]: lane (kg, n) of fragment (t, s) holds W[32 t + n][16 s + 8 kg ..+8)
__global__ void __launch_bounds__(256)
pack_mfma_b_kernel(const bf16_t* __restrict__ W, bf16_t* __restrict__ P, int N, int K) {
    const long total = (long)N * K / 8;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int lane = (int)(i % 64);
        const long frag = i / 64;
        const int s = (int)(frag % (K / 16)), t = (int)(frag / (K / 16));
        const int n = 32 * t + (lane & 31), k = 16 * s + 8 * (lane >> 5);
        *reinterpret_cast<u32x4*>(P + i * 8) = *reinterpret_cast<const u32x4*>(W + (size_t)n * K + k);
    }
}
}  // namespace
}  // namespace alo

extern "C" int alo_pack_mfma_b(const void* w, void* packed, int N, int K, int dtype, void* stream) {
    ALO_REQUIRE(dtype == ALO_BF16 || dtype == ALO_F16, ALO_ERR_UNSUPPORTED, "alo_pack_mfma_b: bf16 / fp16 only (dtype %d)", dtype);
    ALO_REQUIRE(w && packed, ALO_ERR_INVALID_ARGUMENT, "alo_pack_mfma_b: null pointer argument");
    ALO_REQUIRE(N > 0 && K > 0 && N % 32 == 0 && K % 16 == 0, ALO_ERR_INVALID_ARGUMENT,
                "alo_pack_mfma_b: N must be a multiple of 32 and K a multiple of 16 (N=%d K=%d)", N, K);
    long total = (long)N * K / 8;
    unsigned blocks = (unsigned)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    void* args[] = {&w, &packed, &N, &K};
    return launch<pack_mfma_b_kernel>(blocks, 256, 0, static_cast<hipStream_t>(stream), "alo_pack_mfma_b", args);
}

extern "C" int alo_ffn256(const void* x, const void* w1, const void* b1, const void* w2, const void* b2, void* y, long M,
                          int F, int dtype, void* stream) {
    ALO_REQUIRE(dtype == ALO_BF16 || dtype == ALO_F16 || dtype == ALO_F32, ALO_ERR_UNSUPPORTED,
                "alo_ffn256: bf16 / fp16 / fp32 only (dtype %d)", dtype);
    ALO_REQUIRE(x && w1 && w2 && y, ALO_ERR_INVALID_ARGUMENT, "alo_ffn256: null pointer argument");
    ALO_REQUIRE(M > 0 && F > 0 && F % 256 == 0, ALO_ERR_INVALID_ARGUMENT,
                "alo_ffn256: M must be positive and the hidden width a positive multiple of 256 (M=%ld F=%d)", M, F);
    ALO_REQUIRE(aligned16(x, w1, w2, y), ALO_ERR_INVALID_ARGUMENT, "alo_ffn256: pointers must be 16-byte aligned");
    if (dtype == ALO_F32) {   // ffn_f32.hip; the fp32 biases are held to the alignment of the other operands
        ALO_REQUIRE(aligned16(b1, b2), ALO_ERR_INVALID_ARGUMENT, "alo_ffn256: pointers must be 16-byte aligned");
        return ffn_f32(x, w1, b1, w2, b2, y, M, F, static_cast<hipStream_t>(stream), "alo_ffn256");
    }
    FfnDims dm;
    dm.M = M; dm.F = F; dm.tiles = (int)((M + kFfnRows - 1) / kFfnRows);
    const size_t lds = 2 * kFfnRows * kFfnStride + ((size_t)F + 256) * sizeof(float);
    int gx = dm.tiles < 512 ? dm.tiles : 512;
    void* args[] = {&x, &w1, &b1, &w2, &b2, &y, &dm};
    if (lds > (size_t)kLdsLimit) return fail(ALO_ERR_UNSUPPORTED, "alo_ffn256: hidden width %d needs %zu bytes of LDS", F, lds);
    return with_storage_type(dtype, [&](auto t) {
        return launch<ffn256_kernel<decltype(t)>>(gx, 256, lds, static_cast<hipStream_t>(stream), "alo_ffn256", args);
    });
}

extern "C" int alo_value_proj_head_major(const void* x, const void* weight, const void* bias, const void* padding_mask,
                                         void* value_hm, int batch, int S, int heads, int K, int dtype, void* stream) {
    ALO_REQUIRE(dtype == ALO_BF16 || dtype == ALO_F16, ALO_ERR_UNSUPPORTED, "alo_value_proj_head_major: bf16 / fp16 only (dtype %d)", dtype);
    ALO_REQUIRE(x && weight && value_hm, ALO_ERR_INVALID_ARGUMENT, "alo_value_proj_head_major: null pointer argument");
    ALO_REQUIRE(batch > 0 && S > 0 && heads > 0 && heads % 2 == 0, ALO_ERR_INVALID_ARGUMENT,
                "alo_value_proj_head_major: batch, S must be positive and the head count even (batch=%d S=%d heads=%d)", batch, S,
                heads);
    ALO_REQUIRE(K == 64 || K == 128 || K == 256, ALO_ERR_UNSUPPORTED, "alo_value_proj_head_major: K must be 64, 128 or 256, got %d", K);
    ALO_REQUIRE(aligned16(x, weight, value_hm), ALO_ERR_INVALID_ARGUMENT, "alo_value_proj_head_major: pointers must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long M = (long)batch * S;
    const int N = heads * 32;
    return with_storage_type(dtype, [&](auto t) {
        return with_shortk<decltype(t)>(K, [&](auto cfg) {
            return launch_shortk<decltype(cfg), false, false, true>(x, weight, bias, padding_mask, value_hm, M, N, st, S);
        });
    });
}
