// conv1x1_chain.hip's row-local chain at the widths of a layer2 bottleneck (bf16, 128 -> 512 channels over NHWC rows), in one launch:
//
//     y = relu(mid W3^T + b3 + identity)                       identity (M, 512) given                                   (RES)
//                                                           or identity = bf16(x0 Wd^T + bd), Wd (512, 256), x0 the pixel
//                                                              (n, s yo, s xo) of an (N, H, W, 256) map, s = 1 or 2        (DOWN)
//     z = relu(y W1^T + b1), W1 (128, 512)                     the NEXT bottleneck's first 1x1 convolution               (NEXT, optional)
//
// The launches it stands in for: alo_conv1x1_nhwc's short-K kernel with the stride in its tile loader (linear_shortk_kernel<256, false,
// false>) for the identity of DOWN, linear_shortk_kernel<128, true, true> for y, linear_packed_kernel<bf16, 2, true, false> for z.  The
// (M, 512) identity of DOWN is never written and y is not read back to make z.
//
// What differs from the layer1 kernel is that the weights (W3 128 KB, Wd 256 KB, W1 128 KB) do not all fit in a CU's registers:
//   * ONE 512-thread workgroup per CU, eight waves, each owning 64 columns of y over 64-row tiles: W3 is resident (64 VGPRs per wave).
//   * Wd and W1 stream from the vector cache, which is what bounds them (64 B/clk per CU), so they arrive in alo_pack_mfma_b order
//     (a fragment = 1 KB contiguous: eight whole lines per request) and each fragment of Wd is used for BOTH 32-row halves (four MFMAs
//     per 2 KB) out of a ring of four k-steps, whose last requests of a tile are the next tile's first fragments.  For z a wave takes
//     one 32-channel column tile and one 32-row half (32 fragments, one MFMA each, in batches of four through two buffers); W1
//     resident (128 VGPRs beside W3) spills.
// Rounding points, accumulator starts and the k order are those of the three kernels:
//   d = bf16(bd + x0 Wd^T), p = bf16(b3 + mid W3^T)            accumulators START from the bias, k ascending (linear_shortk_kernel)
//   y = bf16(relu(float(p) + float(identity or d)))             add_residual_x8<T, true>
//   z = bf16(relu((0 + y W1^T) + b1))                           accumulators start from zero, the bias joins in the epilogue
//                                                               (linear_packed_kernel: zero_acc, stage_quads<T, true>)
#include "mfma_tile.hpp"

namespace alo {
namespace {

constexpr int kRows = 64;                 // rows per tile
constexpr int kK = 128;                   // input channels of conv3
constexpr int kK0 = 256;                  // input channels of the downsample convolution
constexpr int kN = 512;                   // channels of y: one 64-column block per wave
constexpr int kZN = 128;                  // channels of z
constexpr int kThreads = 512;
constexpr int kInStride = kK * 2 + 16;    // LDS row strides: +16 B keeps the 16-byte fragment reads conflict-free
constexpr int kIn0Stride = kK0 * 2 + 16;
constexpr int kOutStride = 64 * 2 + 16;   // a wave's 64 x 64 block of y
constexpr int kZStride = kZN * 2 + 16;
constexpr int kSteps = kK / 16, kSteps0 = kK0 / 16, kNextSteps = kN / 16;   // MFMA k-steps of the three products
constexpr int kPieces = kK / 8, kPieces0 = kK0 / 8, kZPieces = kZN / 8;     // 16-byte pieces per row
constexpr int kLoads = kRows * kPieces / kThreads, kLoads0 = kRows * kPieces0 / kThreads;
constexpr int kKB0 = 1;                   // k-steps per streamed batch of Wd (two column tiles each)
constexpr int kRing = 4;                  // batches of Wd in registers; divides kSteps0, so a slot holds the same k-steps every tile
constexpr int kKB1 = 4;                   // k-steps per streamed batch of W1 (one column tile)

struct Chain2Args {
    const bf16_t *X, *X0, *R;             // mid (M, 128); DOWN: x0 map (N, H, W, 256); RES: identity (M, 512)
    const bf16_t *W3, *B3, *Wd, *Bd, *W1, *B1;
    bf16_t *Y, *Z;                        // (M, 512), (M, 128)
    long M;
    int tiles;                            // ceil(M / kRows)
    RowGather g;                          // DOWN: output row -> pixel of x0's map
};

constexpr size_t chain2_lds(bool down, bool next) {
    return (size_t)kRows * kInStride + (down ? kRows * kIn0Stride : 0) + 8 * kRows * kOutStride + (next ? kRows * kZStride : 0) +
           (8 * 64 * (down ? 2 : 1) + (next ? kZN : 0)) * sizeof(float);
}

template <int PIECES, int LOADS>
__device__ __forceinline__ void park512(unsigned char* lds, int stride, const u32x4 (&v)[LOADS], int tid) {
#pragma unroll
    for (int j = 0; j < LOADS; ++j) {
        const int p = tid + kThreads * j;
        *reinterpret_cast<u32x4*>(lds + (p / PIECES) * stride + (p % PIECES) * 16) = v[j];
    }
}

template <bool DOWN, bool NEXT>
__global__ void __launch_bounds__(kThreads, 2) conv1x1_chain_l2_kernel(const Chain2Args a) {
    using T = bf16_t;
    static_assert(kRows * kPieces % kThreads == 0 && kRows * kPieces0 % kThreads == 0 && kRows * kZPieces % kThreads == 0,
                  "the tile loaders give every thread the same number of pieces");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nl = lane & 31, kg = lane >> 5;  // MFMA lane roles: row/column inside a 32-tile, 8-element k group
    unsigned char* const xbuf = smem;                                      // mid tile
    unsigned char* const x0buf = smem + kRows * kInStride;                 // DOWN: x0 tile
    unsigned char* const ytile = x0buf + (DOWN ? kRows * kIn0Stride : 0);  // eight per-wave blocks [64][64] of y, wave after wave
    unsigned char* const obuf = ytile + wave * (kRows * kOutStride);
    unsigned char* const zbuf = ytile + 8 * kRows * kOutStride;            // NEXT: z tile [64][128]
    float* const tabs = reinterpret_cast<float*>(zbuf + (NEXT ? kRows * kZStride : 0));
    float* const b3_tab = tabs + wave * 64;                                // accumulator order, [kg][t][16] (linear_shortk_kernel)
    float* const bd_tab = tabs + 8 * 64 + wave * 64;                       // DOWN
    float* const b1_tab = tabs + 8 * 64 * (DOWN ? 2 : 1);                  // NEXT: [128], by column of z (linear_packed_kernel)
    const int col0 = wave * 64;                                            // this wave's 64 columns of y

    // ---- resident row operand W3[col0 + 32 t + nl][16 s + 8 kg .. + 8), and the biases ---------------------------------------------
    u32x4 w3[2][kSteps];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < kSteps; ++s)
            w3[t][s] = *reinterpret_cast<const u32x4*>(a.W3 + (size_t)(col0 + 32 * t + nl) * kK + 8 * kg + 16 * s);
    {
        // register r of lane (nl, kg) of column tile t is column 32 t + (r & 3) + 8 (r >> 2) + 4 kg
        const int r = lane & 15, t = (lane >> 4) & 1, k2 = lane >> 5;
        const int c = col0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * k2;
        b3_tab[lane] = ld(&a.B3[c]);
        if constexpr (DOWN) bd_tab[lane] = ld(&a.Bd[c]);
    }
    // DOWN: Wd arrives in alo_pack_mfma_b order, [column tile of 32][k-step][lane][8]: a fragment is 1 KB contiguous, eight whole
    // lines per request (read row-major a request touches 32 lines for 32 bytes each, and the vector cache, which the stream is
    // bound by, serves it at a third of the rate).  This lane's 16 bytes of fragment (column tile t of the wave, k-step s):
    // wdp + (t * kSteps0 + s) * 512
    // The base is uniform (readfirstlane tells the compiler so) and the lane's part a 32-bit offset, redefined every tile (the empty asm
    // at the top of the tile loop): every request is then a scalar base, one shared offset register and an immediate.  Left loop
    // invariant, the 16 / 32 fragment addresses are hoisted out of the tile loop as 64-bit register pairs and spill.
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    unsigned lane_off = lane * 8;
    [[maybe_unused]] const T* const wdp = DOWN ? a.Wd + (size_t)(2 * wave_u) * kSteps0 * 512 : nullptr;
    auto load_wd = [&](u32x4 (&buf)[2][kKB0], int batch) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int j = 0; j < kKB0; ++j) buf[t][j] = *reinterpret_cast<const u32x4*>(wdp + (t * kSteps0 + kKB0 * batch + j) * 512 + lane_off);
        __builtin_amdgcn_sched_barrier(0);
    };
    // NEXT: this wave's 32 output channels of z, of rows 32 zhalf .. + 32
    const int zcol0 = 32 * (wave & 3), zhalf = wave >> 2;
    [[maybe_unused]] const T* const w1p = NEXT ? a.W1 + (size_t)(wave_u & 3) * kNextSteps * 512 : nullptr;   // packed like Wd
    auto load_w1 = [&](u32x4 (&buf)[kKB1], int batch) {
#pragma unroll
        for (int j = 0; j < kKB1; ++j) buf[j] = *reinterpret_cast<const u32x4*>(w1p + (kKB1 * batch + j) * 512 + lane_off);
        __builtin_amdgcn_sched_barrier(0);
    };
    if constexpr (NEXT) {
        if (tid < kZN) b1_tab[tid] = ld(&a.B1[tid]);
    }

    // ---- tile loaders: rows past the end are read from the last row (and never stored): the requests go out unpredicated -----------
    auto fetch = [&](int tile, u32x4 (&r)[kLoads]) {
#pragma unroll
        for (int j = 0; j < kLoads; ++j) {
            const int p = tid + kThreads * j;  // piece index: row = p / kPieces, 16-byte column = p % kPieces
            long row = (long)tile * kRows + p / kPieces;
            row = row < a.M ? row : a.M - 1;
            r[j] = *reinterpret_cast<const u32x4*>(a.X + row * kK + (p % kPieces) * 8);
        }
    };
    auto fetch0 = [&](int tile, u32x4 (&r)[kLoads0]) {  // the kept pixels of x0's map, addressed here: no gathered copy
#pragma unroll
        for (int j = 0; j < kLoads0; ++j) {
            const int p = tid + kThreads * j;
            long row = (long)tile * kRows + p / kPieces0;
            row = gather_row(a.g, row < a.M ? row : a.M - 1);
            r[j] = *reinterpret_cast<const u32x4*>(a.X0 + row * kK0 + (p % kPieces0) * 8);
        }
    };

    int tile = blockIdx.x;
    if (tile >= a.tiles) return;
    u32x4 stage[kLoads];
    [[maybe_unused]] u32x4 stage0[DOWN ? kLoads0 : 1];
    [[maybe_unused]] u32x4 wd[kRing][2][kKB0];
    fetch(tile, stage);
    if constexpr (DOWN) {
        fetch0(tile, stage0);
#pragma unroll
        for (int b = 0; b + 1 < kRing; ++b) load_wd(wd[b], b);
    }

    for (;;) {
        asm volatile("" : "+v"(lane_off));
        park512<kPieces>(xbuf, kInStride, stage, tid);
        if constexpr (DOWN) park512<kPieces0>(x0buf, kIn0Stride, stage0, tid);
        __syncthreads();  // the tile is in LDS (and the bias tables, the first time)
        const long grow0 = (long)tile * kRows;
        const int next = tile + gridDim.x;
        const bool more = next < a.tiles;
        [[maybe_unused]] u32x4 idn[DOWN ? 1 : 8];  // RES: the identity of THIS tile in store order, requested here, wanted after the product
        if constexpr (!DOWN) fetch_identity(idn, a.R, grow0, a.M, kN, col0, lane);
        if (more) {  // in flight during the MFMAs and the stores below
            fetch(next, stage);
        }

        // ---- DOWN: d = bf16(bd + x0 Wd^T) for both 32-row halves, Wd streamed once per tile -------------------------------------------
        [[maybe_unused]] unsigned dpk[DOWN ? 2 : 1][2][8];  // [row half][column tile][pair]: d rounded, two columns per word
        if constexpr (DOWN) {
            f32x16 accd[2][2];  // [row half][column tile]
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 d4 = *reinterpret_cast<const f32x4*>(bd_tab + (kg * 2 + t) * 16 + 4 * q);
#pragma unroll
                    for (int i = 0; i < 4; ++i) accd[0][t][4 * q + i] = accd[1][t][4 * q + i] = d4[i];
                }
            auto mma_wd = [&](const u32x4 (&buf)[2][kKB0], int batch) {
                u32x4 af[2][kKB0];
#pragma unroll
                for (int j = 0; j < kKB0; ++j) {
                    const int s = kKB0 * batch + j;
                    af[0][j] = *reinterpret_cast<const u32x4*>(x0buf + nl * kIn0Stride + (16 * s + 8 * kg) * 2);
                    af[1][j] = *reinterpret_cast<const u32x4*>(x0buf + (32 + nl) * kIn0Stride + (16 * s + 8 * kg) * 2);
                }
#pragma unroll
                for (int j = 0; j < kKB0; ++j)
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int t = 0; t < 2; ++t) accd[h][t] = mfma_32x32x16<T>(buf[t][j], af[h][j], accd[h][t]);
                __builtin_amdgcn_sched_barrier(0);
            };
            // a ring of kRing single k-step batches, requested kRing - 1 k-steps (four MFMAs each) ahead; the last kRing - 1 requests of a
            // tile are the next tile's first batches
#pragma unroll
            for (int bt = 0; bt < kSteps0; ++bt) {
                load_wd(wd[(bt + kRing - 1) % kRing], (bt + kRing - 1) % kSteps0);
                mma_wd(wd[bt % kRing], bt);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int i = 0; i < 8; ++i) dpk[h][t][i] = pack2<T>(accd[h][t][2 * i], accd[h][t][2 * i + 1]);
            // the next x0 tile is requested here, not with the mid tile above: its 16 registers beside the four accumulators of the
            // product above spill; it still has the second product, the stores and the z product to arrive in
            if (more) fetch0(next, stage0);
        }

        // ---- p = bf16(b3 + mid W3^T), then y --------------------------------------------------------------------------------------------
#pragma unroll
        for (int half = 0; half < kRows / 32; ++half) {  // 32 rows at a time through the same accumulators
            f32x16 acc[2];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 b4 = *reinterpret_cast<const f32x4*>(b3_tab + (kg * 2 + t) * 16 + 4 * q);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[t][4 * q + i] = b4[i];
                }
#pragma unroll
            for (int s = 0; s < kSteps; ++s) {
                const u32x4 f = *reinterpret_cast<const u32x4*>(xbuf + (32 * half + nl) * kInStride + (16 * s + 8 * kg) * 2);
                acc[0] = mfma_32x32x16<T>(w3[0][s], f, acc[0]);
                acc[1] = mfma_32x32x16<T>(w3[1][s], f, acc[1]);
            }
            // lane = tile row 32 half + nl -> bf16 -> LDS [row][col]
            if constexpr (DOWN) {
                // p rounded to bf16 once, then add_residual_x8<T, true>'s arithmetic on (p, d): the staged rows are final
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        unsigned o[2];
#pragma unroll
                        for (int i = 0; i < 2; ++i) {
                            float plo, phi, dlo, dhi;
                            unpack2<T>(pack2<T>(acc[t][4 * q + 2 * i], acc[t][4 * q + 2 * i + 1]), plo, phi);
                            unpack2<T>(dpk[half][t][2 * q + i], dlo, dhi);
                            o[i] = pack2<T>(relu_keep_nan(plo + dlo), relu_keep_nan(phi + dhi));
                        }
                        *reinterpret_cast<u32x2*>(obuf + (32 * half + nl) * kOutStride + (32 * t + 8 * q + 4 * kg) * 2) = u32x2{o[0], o[1]};
                    }
            } else {
                stage_quads<T, false>(obuf, kOutStride, acc, nullptr, false, 32 * half + nl, 0, kg);
            }
        }
        [[maybe_unused]] u32x4 w1a[kKB1], w1b[kKB1];
        if constexpr (NEXT) load_w1(w1a, 0);  // wanted after the stores and the barrier below
        wave_lds_fence();
        // the wave's 64 staged rows -> y as whole lines: 8 lanes x 16 B per row, 8 rows per store instruction
#pragma unroll
        for (int pass = 0; pass < 8; ++pass) {
            const int row = pass * 8 + (lane >> 3);
            unsigned char* const at = obuf + row * kOutStride + (lane & 7) * 16;
            u32x4 v = *reinterpret_cast<const u32x4*>(at);
            if constexpr (!DOWN) {
                v = add_residual_x8<T, true>(v, idn[pass]);
                if constexpr (NEXT) *reinterpret_cast<u32x4*>(at) = v;  // the final y back into its place: the next product's operand
            }
            if (grow0 + row < a.M) *reinterpret_cast<u32x4*>(a.Y + (grow0 + row) * kN + col0 + (lane & 7) * 8) = v;
        }

        if constexpr (NEXT) {
            __syncthreads();  // the eight blocks of y are final: together the 64 x 512 tile (and every wave is done with the input tiles)
            f32x16 accz;
#pragma unroll
            for (int i = 0; i < 16; ++i) accz[i] = 0.f;
            // y[tile row 32 zhalf + nl][16 s + 8 kg .. + 8): block s / 4 (the wave that owns those columns), column 16 (s % 4) + 8 kg of it
            const unsigned char* const yrow = ytile + (32 * zhalf + nl) * kOutStride + 8 * kg * 2;
            auto mma_w1 = [&](const u32x4 (&buf)[kKB1], int batch) {
                u32x4 af[kKB1];
#pragma unroll
                for (int j = 0; j < kKB1; ++j) {
                    const int s = kKB1 * batch + j;
                    af[j] = *reinterpret_cast<const u32x4*>(yrow + (s >> 2) * (kRows * kOutStride) + 16 * (s & 3) * 2);
                }
#pragma unroll
                for (int j = 0; j < kKB1; ++j) accz = mfma_32x32x16<T>(buf[j], af[j], accz);
                __builtin_amdgcn_sched_barrier(0);
            };
            constexpr int kBatches = kNextSteps / kKB1;
#pragma unroll
            for (int bt = 0; bt < kBatches; bt += 2) {
                load_w1(w1b, bt + 1);
                mma_w1(w1a, bt);
                if (bt + 2 < kBatches) load_w1(w1a, bt + 2);
                mma_w1(w1b, bt + 1);
            }
            // + b1 -> ReLU -> bf16 (stage_quads<T, true> of linear_packed_kernel's epilogue)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = zcol0 + 8 * q + 4 * kg;
                const f32x4 bb = *reinterpret_cast<const f32x4*>(b1_tab + c);
                float v0 = accz[4 * q], v1 = accz[4 * q + 1], v2 = accz[4 * q + 2], v3 = accz[4 * q + 3];
                v0 += bb[0]; v1 += bb[1]; v2 += bb[2]; v3 += bb[3];
                v0 = relu_keep_nan(v0); v1 = relu_keep_nan(v1); v2 = relu_keep_nan(v2); v3 = relu_keep_nan(v3);
                *reinterpret_cast<u32x2*>(zbuf + (32 * zhalf + nl) * kZStride + c * 2) = u32x2{pack2<T>(v0, v1), pack2<T>(v2, v3)};
            }
            __syncthreads();  // the z tile is staged (and every wave is done with the y tile)
#pragma unroll
            for (int j = 0; j < kRows * kZPieces / kThreads; ++j) {
                const int p = tid + kThreads * j, row = p / kZPieces, piece = p % kZPieces;
                if (grow0 + row < a.M)
                    *reinterpret_cast<u32x4*>(a.Z + (grow0 + row) * kZN + piece * 8) =
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

template <bool DOWN, bool NEXT>
int launch_chain2(const Chain2Args& a, hipStream_t stream) {
    int gx = a.tiles < 256 ? a.tiles : 256;  // persistent: one 8-wave workgroup per CU
    void* args[] = {const_cast<Chain2Args*>(&a)};
    return launch<conv1x1_chain_l2_kernel<DOWN, NEXT>>(gx, kThreads, chain2_lds(DOWN, NEXT), stream, "alo_conv1x1_nhwc", args);
}

}  // namespace
}  // namespace alo

// Arguments checked by alo_conv1x1_nhwc (gemm_packed.hip); w_chain in the layout alo_hotpath.h gives.
int alo::conv1x1_chain_l2(const void* mid, const void* w_chain, const void* res_or_x0, void* y, long M, bool down, int n2,
                          const RowGather& gather, hipStream_t stream) {
    const bf16_t* w = static_cast<const bf16_t*>(w_chain);
    Chain2Args a{};
    a.X = static_cast<const bf16_t*>(mid);
    (down ? a.X0 : a.R) = static_cast<const bf16_t*>(res_or_x0);
    a.W3 = w; w += kN * kK;
    a.B3 = w; w += kN;
    if (down) {
        a.Wd = w; w += kN * kK0;
        a.Bd = w; w += kN;
    }
    if (n2) {
        a.W1 = w; w += (size_t)kZN * kN;
        a.B1 = w;
    }
    a.Y = static_cast<bf16_t*>(y);
    a.Z = n2 ? a.Y + M * kN : nullptr;
    a.M = M;
    a.tiles = (int)((M + kRows - 1) / kRows);
    a.g = gather;
    if (down) return n2 ? launch_chain2<true, true>(a, stream) : launch_chain2<true, false>(a, stream);
    return n2 ? launch_chain2<false, true>(a, stream) : launch_chain2<false, false>(a, stream);
}
