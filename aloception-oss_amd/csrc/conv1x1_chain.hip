// The row-local chain around a layer1 bottleneck's last 1x1 convolution, in one launch (bf16, 64 -> 256 channels over NHWC rows):
//
//     y = relu(mid W3^T + b3 + identity)                       identity (M, 256) given                        (RES)
//                                                           or identity = bf16(x0 Wd^T + bd), x0 (M, 64)     (DOWN: the `downsample` branch)
//     z = relu(y W1^T + b1), W1 (N2, 256), N2 = 64 or 128      the NEXT bottleneck's first 1x1 convolution    (NEXT, optional)
//
// Run as separate launches of linear_shortk_kernel (gemm.hip) the (M, 256) identity of DOWN is written by one streaming kernel and read
// straight back by the next, and the (M, 256) block output y is read a second time to make the (M, N2) tensor z: at the 534400 rows of
// the bf16 headline each of those passes is 273.6 MB at the HBM rate.  A 1x1 convolution is row-local, so both can stay on chip.
//
// This is linear_shortk_kernel<bf16_t, 64, true, true>'s frame — persistent 256-thread workgroups, two per CU, over 64-row tiles, the next
// tile fetched during the product, W3 resident in registers (32 per wave), the identity requested ahead of the product, per-wave staging,
// whole-line stores — with
//   DOWN  a second input tile x0 fetched and parked like the first, a second resident weight set Wd and a second accumulator pair.  Both
//         accumulator sets start from their own bias and each is rounded to bf16 ONCE, p = bf16(mid W3^T + b3), d = bf16(x0 Wd^T + bd);
//         then y = bf16(relu(float(p) + float(d))): the rounding points of the two launches it stands in for (add_residual_x8<T, true>
//         applied to d), so y is theirs bit for bit.  No identity is loaded.
//   NEXT  the final y values of a tile sit in the four waves' staging areas, which together ARE the 64 x 256 operand of the next
//         convolution.  After a workgroup barrier every wave multiplies that tile by its resident 32 output channels of W1 (16 fragments,
//         64 VGPRs; N2 = 64: one 32 x 32 block per wave, N2 = 128: two, the two row halves against the same fragments), accumulators from
//         the bias, k ascending, as linear_shortk_kernel<256, true, false> does: z is that kernel's output bit for bit.  z leaves through
//         a staging area of its own as whole lines.  One barrier more per tile than the plain frame (the tile-end barrier moves up).
#include "mfma_tile.hpp"

namespace alo {
namespace {

constexpr int kRows = 64;                // rows per tile
constexpr int kK = 64;                   // input channels of both products into y
constexpr int kN = 256;                  // channels of y: one 64-column block per wave
constexpr int kInStride = kK * 2 + 16;   // LDS row stride of a 64-channel input tile: +16 B keeps the 16-byte fragment reads conflict-free
constexpr int kOutStride = 64 * 2 + 16;  // LDS row stride of a wave's 64 x 64 block of y
constexpr int kSteps = kK / 16;          // MFMA k-steps of the products into y
constexpr int kPieces = kK / 8;          // 16-byte pieces per input row
constexpr int kLoads = kRows * kPieces / 256;
constexpr int kNextSteps = kN / 16;      // MFMA k-steps of the product into z

struct ChainArgs {
    const bf16_t *X, *X0, *R;            // mid (M, 64); DOWN: x0 (M, 64); RES: identity (M, 256)
    const bf16_t *W3, *B3, *Wd, *Bd, *W1, *B1;
    bf16_t *Y, *Z;                       // (M, 256), (M, N2)
    long M;
    int tiles;                           // ceil(M / kRows)
};

constexpr int z_stride(int n2) { return n2 * 2 + 16; }
constexpr size_t chain_lds(bool down, int n2) {
    return (size_t)kRows * kInStride * (down ? 2 : 1) + 4 * kRows * kOutStride + (n2 ? kRows * z_stride(n2) : 0) +
           (4 * 64 * (down ? 2 : 1) + (n2 ? 4 * 32 : 0)) * sizeof(float);
}

template <bool DOWN, int N2>
__global__ void __launch_bounds__(256, 2) conv1x1_chain_kernel(const ChainArgs a) {
    using T = bf16_t;
    static_assert(N2 == 0 || N2 == 64 || N2 == 128, "the next convolution has 64 or 128 output channels");
    static_assert(kRows * kPieces % 256 == 0, "the tile loader gives every thread the same number of pieces");
    constexpr int kZStride = z_stride(N2);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nl = lane & 31, kg = lane >> 5;  // MFMA lane roles: row/column inside a 32-tile, 8-element k group
    unsigned char* const xbuf = smem;                                   // mid tile
    unsigned char* const x0buf = smem + kRows * kInStride;              // DOWN: x0 tile
    unsigned char* const ytile = x0buf + (DOWN ? kRows * kInStride : 0);  // four per-wave blocks [64][64] of y, wave after wave
    unsigned char* const obuf = ytile + wave * (kRows * kOutStride);
    unsigned char* const zbuf = ytile + 4 * kRows * kOutStride;         // NEXT: z tile [64][N2]
    float* const tabs = reinterpret_cast<float*>(zbuf + (N2 ? kRows * kZStride : 0));
    float* const b3_tab = tabs + wave * 64;                             // accumulator order, [kg][t][16] (linear_shortk_kernel)
    float* const bd_tab = tabs + 4 * 64 + wave * 64;                    // DOWN
    float* const b1_tab = tabs + 4 * 64 * (DOWN ? 2 : 1) + wave * 32;   // NEXT: [kg][16] of this wave's 32 channels of z
    const int col0 = wave * 64;                                         // this wave's 64 columns of y

    // ---- resident row operands: W[col0 + 32 t + nl][16 s + 8 kg .. + 8), and the biases the accumulators start from ----------------
    u32x4 w3[2][kSteps];
    [[maybe_unused]] u32x4 wd[DOWN ? 2 : 1][kSteps];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < kSteps; ++s) {
            w3[t][s] = *reinterpret_cast<const u32x4*>(a.W3 + (size_t)(col0 + 32 * t + nl) * kK + 8 * kg + 16 * s);
            if constexpr (DOWN) wd[t][s] = *reinterpret_cast<const u32x4*>(a.Wd + (size_t)(col0 + 32 * t + nl) * kK + 8 * kg + 16 * s);
        }
    {
        // register r of lane (nl, kg) of column tile t is column 32 t + (r & 3) + 8 (r >> 2) + 4 kg
        const int r = lane & 15, t = (lane >> 4) & 1, k2 = lane >> 5;
        const int c = col0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * k2;
        b3_tab[lane] = ld(&a.B3[c]);
        if constexpr (DOWN) bd_tab[lane] = ld(&a.Bd[c]);
    }
    // NEXT: this wave's 32 output channels of z (N2 = 64: of rows 32 (wave / 2) .. + 32; N2 = 128: of all 64 rows)
    constexpr int kHalves = N2 == 128 ? 2 : 1;
    const int zcol0 = N2 == 128 ? 32 * wave : 32 * (wave & 1);
    const int zhalf0 = N2 == 128 ? 0 : wave >> 1;
    [[maybe_unused]] u32x4 w1[N2 ? kNextSteps : 1];
    if constexpr (N2 != 0) {
#pragma unroll
        for (int s = 0; s < kNextSteps; ++s)
            w1[s] = *reinterpret_cast<const u32x4*>(a.W1 + (size_t)(zcol0 + nl) * kN + 8 * kg + 16 * s);
        if (lane < 32) {
            const int r = lane & 15, k2 = lane >> 4;
            b1_tab[lane] = ld(&a.B1[zcol0 + (r & 3) + 8 * (r >> 2) + 4 * k2]);
        }
    }

    // ---- tile loader: rows past the end are read from the last row (and never stored): the requests go out unpredicated -----------
    auto fetch = [&](const T* X, int tile, u32x4 (&r)[kLoads]) {
#pragma unroll
        for (int j = 0; j < kLoads; ++j) {
            const int p = tid + 256 * j;  // piece index: row = p / kPieces, 16-byte column = p % kPieces
            long row = (long)tile * kRows + p / kPieces;
            row = row < a.M ? row : a.M - 1;
            r[j] = *reinterpret_cast<const u32x4*>(X + row * kK + (p % kPieces) * 8);
        }
    };

    int tile = blockIdx.x;
    if (tile >= a.tiles) return;
    u32x4 stage[kLoads];
    [[maybe_unused]] u32x4 stage0[DOWN ? kLoads : 1];
    fetch(a.X, tile, stage);
    if constexpr (DOWN) fetch(a.X0, tile, stage0);

    for (;;) {
        park_tile<kPieces>(xbuf, kInStride, stage, tid);
        if constexpr (DOWN) park_tile<kPieces>(x0buf, kInStride, stage0, tid);
        __syncthreads();  // the tile is in LDS (and the bias tables, the first time)
        const long grow0 = (long)tile * kRows;
        const int next = tile + gridDim.x;
        const bool more = next < a.tiles;
        [[maybe_unused]] u32x4 idn[DOWN ? 1 : 8];  // RES: the identity of THIS tile in store order, requested here, wanted after the product
        if constexpr (!DOWN) fetch_identity(idn, a.R, grow0, a.M, kN, col0, lane);
        if (more) {  // in flight during the MFMAs and the stores below
            fetch(a.X, next, stage);
            if constexpr (DOWN) fetch(a.X0, next, stage0);
        }

#pragma unroll
        for (int half = 0; half < kRows / 32; ++half) {  // 32 rows at a time through the same accumulators
            f32x16 acc[2];
            [[maybe_unused]] f32x16 accd[DOWN ? 2 : 1];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 b4 = *reinterpret_cast<const f32x4*>(b3_tab + (kg * 2 + t) * 16 + 4 * q);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[t][4 * q + i] = b4[i];
                    if constexpr (DOWN) {
                        const f32x4 d4 = *reinterpret_cast<const f32x4*>(bd_tab + (kg * 2 + t) * 16 + 4 * q);
#pragma unroll
                        for (int i = 0; i < 4; ++i) accd[t][4 * q + i] = d4[i];
                    }
                }
#pragma unroll
            for (int s = 0; s < kSteps; ++s) {
                const int off = (32 * half + nl) * kInStride + (16 * s + 8 * kg) * 2;  // fragment [tile row 32 half + nl][16 s + 8 kg .. + 8)
                const u32x4 f = *reinterpret_cast<const u32x4*>(xbuf + off);
                acc[0] = mfma_32x32x16<T>(w3[0][s], f, acc[0]);
                acc[1] = mfma_32x32x16<T>(w3[1][s], f, acc[1]);
                if constexpr (DOWN) {
                    const u32x4 f0 = *reinterpret_cast<const u32x4*>(x0buf + off);
                    accd[0] = mfma_32x32x16<T>(wd[0][s], f0, accd[0]);
                    accd[1] = mfma_32x32x16<T>(wd[1][s], f0, accd[1]);
                }
            }
            // lane = tile row 32 half + nl -> bf16 -> LDS [row][col]
            if constexpr (DOWN) {
                // p and d rounded to bf16 once each, then add_residual_x8<T, true>'s arithmetic on the pair: the staged rows are final
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        unsigned o[2];
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
                            float plo, phi, dlo, dhi;
                            unpack2<T>(pack2<T>(acc[t][4 * q + 2 * i], acc[t][4 * q + 2 * i + 1]), plo, phi);
                            unpack2<T>(pack2<T>(accd[t][4 * q + 2 * i], accd[t][4 * q + 2 * i + 1]), dlo, dhi);
                            o[i] = pack2<T>(relu_keep_nan(plo + dlo), relu_keep_nan(phi + dhi));
                        }
                        *reinterpret_cast<u32x2*>(obuf + (32 * half + nl) * kOutStride + (32 * t + 8 * q + 4 * kg) * 2) = u32x2{o[0], o[1]};
                    }
            } else {
                stage_quads<T, false>(obuf, kOutStride, acc, nullptr, false, 32 * half + nl, 0, kg);
            }
        }
        wave_lds_fence();
        // the wave's 64 staged rows -> y as whole lines: 8 lanes x 16 B per row, 8 rows per store instruction
#pragma unroll
        for (int pass = 0; pass < 8; ++pass) {
            const int row = pass * 8 + (lane >> 3);
            unsigned char* const at = obuf + row * kOutStride + (lane & 7) * 16;
            u32x4 v = *reinterpret_cast<const u32x4*>(at);
            if constexpr (!DOWN) {
                v = add_residual_x8<T, true>(v, idn[pass]);
                if constexpr (N2 != 0) *reinterpret_cast<u32x4*>(at) = v;  // the final y back into its place: the next product's operand
            }
            if (grow0 + row < a.M) *reinterpret_cast<u32x4*>(a.Y + (grow0 + row) * kN + col0 + (lane & 7) * 8) = v;
        }

        if constexpr (N2 != 0) {
            __syncthreads();  // the four blocks of y are final: together the 64 x 256 tile (and every wave is done with the input tiles)
            f32x16 accz[kHalves];
#pragma unroll
            for (int h = 0; h < kHalves; ++h)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 b4 = *reinterpret_cast<const f32x4*>(b1_tab + kg * 16 + 4 * q);
#pragma unroll
                    for (int i = 0; i < 4; ++i) accz[h][4 * q + i] = b4[i];
                }
#pragma unroll
            for (int s = 0; s < kNextSteps; ++s) {
                // y[tile row][16 s + 8 kg .. + 8): block s / 4 (the wave that owns those columns), column 16 (s % 4) + 8 kg of it
                const unsigned char* const blk = ytile + (s >> 2) * (kRows * kOutStride) + (16 * (s & 3) + 8 * kg) * 2;
#pragma unroll
                for (int h = 0; h < kHalves; ++h) {
                    const u32x4 f = *reinterpret_cast<const u32x4*>(blk + (32 * (zhalf0 + h) + nl) * kOutStride);
                    accz[h] = mfma_32x32x16<T>(w1[s], f, accz[h]);
                }
            }
#pragma unroll
            for (int h = 0; h < kHalves; ++h)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float v0 = relu_keep_nan(accz[h][4 * q]), v1 = relu_keep_nan(accz[h][4 * q + 1]);
                    const float v2 = relu_keep_nan(accz[h][4 * q + 2]), v3 = relu_keep_nan(accz[h][4 * q + 3]);
                    *reinterpret_cast<u32x2*>(zbuf + (32 * (zhalf0 + h) + nl) * kZStride + (zcol0 + 8 * q + 4 * kg) * 2) =
                        u32x2{pack2<T>(v0, v1), pack2<T>(v2, v3)};
                }
            __syncthreads();  // the z tile is staged (and every wave is done with the y tile)
            constexpr int kZPieces = N2 / 8;  // 16-byte pieces per row of z
#pragma unroll
            for (int j = 0; j < kRows * kZPieces / 256; ++j) {
                const int p = tid + 256 * j, row = p / kZPieces, piece = p % kZPieces;
                if (grow0 + row < a.M)
                    *reinterpret_cast<u32x4*>(a.Z + (grow0 + row) * N2 + piece * 8) =
                        *reinterpret_cast<const u32x4*>(zbuf + row * kZStride + piece * 16);
            }
            if (!more) break;
            // no barrier here: the input tiles were last read before the first barrier above, the y blocks before the second, and the
            // z tile is next written after two barriers of the next tile
        } else {
            if (!more) break;
            __syncthreads();  // every wave has finished reading the tile: it may be overwritten
        }
        tile = next;
    }
}

template <bool DOWN, int N2>
int launch_chain(const ChainArgs& a, hipStream_t stream) {
    int gx = a.tiles < 512 ? a.tiles : 512;  // persistent: two workgroups per CU
    void* args[] = {const_cast<ChainArgs*>(&a)};
    return launch<conv1x1_chain_kernel<DOWN, N2>>(gx, 256, chain_lds(DOWN, N2), stream, "alo_conv1x1_nhwc", args);
}

}  // namespace
}  // namespace alo

// Arguments checked by alo_conv1x1_nhwc (gemm_packed.hip); w_chain in the layout alo_hotpath.h gives.
int alo::conv1x1_chain(const void* mid, const void* w_chain, const void* res_or_x0, void* y, long M, bool down, int n2, hipStream_t stream) {
    const bf16_t* w = static_cast<const bf16_t*>(w_chain);
    ChainArgs a{};
    a.X = static_cast<const bf16_t*>(mid);
    (down ? a.X0 : a.R) = static_cast<const bf16_t*>(res_or_x0);
    a.W3 = w; w += kN * kK;
    a.B3 = w; w += kN;
    if (down) {
        a.Wd = w; w += kN * kK;
        a.Bd = w; w += kN;
    }
    if (n2) {
        a.W1 = w; w += (size_t)n2 * kN;
        a.B1 = w;
    }
    a.Y = static_cast<bf16_t*>(y);
    a.Z = n2 ? a.Y + M * kN : nullptr;
    a.M = M;
    a.tiles = (int)((M + kRows - 1) / kRows);
    if (down) return n2 == 128 ? launch_chain<true, 128>(a, stream) : n2 == 64 ? launch_chain<true, 64>(a, stream) : launch_chain<true, 0>(a, stream);
    return n2 == 128 ? launch_chain<false, 128>(a, stream) : n2 == 64 ? launch_chain<false, 64>(a, stream) : launch_chain<false, 0>(a, stream);
}
