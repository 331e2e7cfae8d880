// 3x3 convolution, padding 1, stride 1 or 2, NHWC bf16 (fp32 accumulation) with bias + ReLU in the epilogue: the middle
// convolution of the ResNet bottlenecks (alonet/detr/backbone.py + torchvision Bottleneck.conv2, FrozenBatchNorm folded in).
//
// An implicit GEMM on v_mfma_f32_32x32x16_bf16: y[p, :] = sum over the 9 taps of x[pixel of tap(p), :] W_tap^T, K = 9 * Cin.
//   * a workgroup (two waves) owns 64 consecutive output pixels of one image (flattened y * Wo + x, so rows of any width
//     tile without waste) and 128 output channels, 64 per wave = 2 x 2 MFMA tiles per wave;
//   * the input pixels the tile touches are copied, CHUNK channels at a time, into LDS with whole-line loads that are issued
//     one chunk ahead of their use (register staged), so their round trip hides behind the previous chunk's MFMAs:
//       stride 1: three runs of 66 consecutive input pixels (rows y-1, y, y+1; flattened index p - 1 .. p + 64), tap (dy, dx)
//                 of tile pixel m reads slot 66 dy + dx + m;
//       stride 2: per tap row dy a run of 65 odd-column and a run of 64 even-column pixels of input row 2 y + dy - 1 — in the
//                 four parity phases of the input a stride-2 tap is again a shift of the flattened OUTPUT index;
//     A fragments are ds_read from there and zeroed per lane where the tap falls outside the image (the zero padding);
//   * the weights arrive pre-packed in MFMA B-fragment order ([Cout / 32][9 Cin / 16][64 lanes][8], k = tap * Cin + c), are
//     read as whole 1 KB lines per instruction and stream through two register buffers, one batch of two k-steps ahead;
//   * Cout == 64 (ResNet layer1) would leave the second wave without columns: there the two waves split K instead (each takes
//     every other weight batch) and the partial sums meet in LDS.
//     Cin == Cout == 64 at stride 1 goes to conv3x3_c64_kernel, the same split on four waves with the weights kept in registers.
//   * stride 1 with Cout >= 128 and no split-K goes to conv3x3_pipe_kernel: this arithmetic on four waves per halo, with the LDS reads
//     and the weight requests issued ahead of the MFMAs that use them.
//   * stride 2 with Cout >= 128 and no split-K goes to conv3x3_pipe_s2_kernel: the same loop over the stride-2 halo, 32 channels per chunk.
//   * ALO_CONV_DILATION_2 in `stride` (dilation 2, padding 2, stride 1: layer4 of a DC5 backbone) goes to conv3x3_d2_kernel, the
//     stride-1 loop over runs of 68 pixels two rows apart with the taps two slots apart.
#include <cstdlib>
#include <cstring>

#include "mfma_tile.hpp"

namespace alo {
namespace {

constexpr int kPix = 64;                     // output pixels per tile
constexpr int kThreads = 128;                // two waves
constexpr int kOutStride = 64 * 2 + 16;      // LDS bytes per pixel of a wave's 64 x 64 output block
constexpr int kRedOffset = kPix * kOutStride;  // K-split: wave 1's fp32 partial sums [64 regs][64 lanes] sit behind wave 0's output block

template <int STRIDE>
struct Geo {
    static constexpr int kChunk = STRIDE == 1 ? 64 : 32;     // input channels staged at once
    static constexpr int kBpt = kChunk / 32;                 // weight batches (two k-steps each) per tap and chunk
    static constexpr int kRun = STRIDE == 1 ? kPix + 2 : 2 * kPix + 1;  // staged pixels per tap row
    static constexpr int kSlots = 3 * kRun;
    static constexpr int kPixStride = kChunk * 2 + 16;       // LDS bytes per staged pixel (+16: conflict-free 16-byte reads)
    static constexpr int kPieces = kSlots * (kChunk / 8);    // 16-byte pieces per chunk
    static constexpr int kIters = (kPieces + kThreads - 1) / kThreads;
    static constexpr int kLds = kSlots * kPixStride;
    static_assert(kLds >= kRedOffset + 64 * 64 * 4, "the epilogue's staging aliases the halo");
};

struct ConvDims {
    int N, H, W, Ho, Wo, Cin, Cout;
    int tiles_per_image;
    int relu;
    int zsplit, cin_per_z;   // split-K over gridDim.z: workgroup z reduces input channels [z * cin_per_z, + cin_per_z)
};

struct WFrag { u32x4 v[2][2]; };    // [k-step of the batch][column tile]

// flattened input pixel (clamped into the image) behind staging slot `slot` of the tile whose first output pixel is p0
template <int STRIDE>
__device__ __forceinline__ int slot_pixel(int slot, int p0, const ConvDims& dm) {
    if (STRIDE == 1) {
        const int run = slot / Geo<1>::kRun, pix = slot - run * Geo<1>::kRun;
        const int q = p0 + (run - 1) * dm.W - 1 + pix;
        const int last = dm.H * dm.W - 1;
        return q < 0 ? 0 : (q > last ? last : q);
    }
    const int dy = slot / Geo<2>::kRun, r = slot - dy * Geo<2>::kRun;
    const int odd = r < kPix + 1 ? 1 : 0;                        // column parity of this run
    int f = p0 + (odd ? r - 1 : r - (kPix + 1)) - (dy == 0 ? dm.Wo : 0);   // output-index space: (yo + oy) * Wo + xo + ox
    const int last = dm.Ho * dm.Wo - 1;
    f = f < 0 ? 0 : (f > last ? last : f);
    const int yp = f / dm.Wo, xp = f - yp * dm.Wo;
    int iy = 2 * yp + (dy == 1 ? 0 : 1), ix = 2 * xp + odd;
    iy = iy > dm.H - 1 ? dm.H - 1 : iy;
    ix = ix > dm.W - 1 ? dm.W - 1 : ix;
    return iy * dm.W + ix;
}

template <int STRIDE, bool KSPLIT>
__global__ void __launch_bounds__(kThreads, 2)
conv3x3_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ Wp, const bf16_t* __restrict__ bias,
               bf16_t* __restrict__ Y, float* __restrict__ partial, const ConvDims dm) {
    using G = Geo<STRIDE>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const halo = smem;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nl = lane & 31, kg = lane >> 5;
    const int HWo = dm.Ho * dm.Wo;
    const int col0 = KSPLIT ? blockIdx.y * 64 : blockIdx.y * 128 + wave * 64;  // this wave's 64 output channels
    const bool has_cols = col0 < dm.Cout;                               // Cout % 64 == 0
    float* const bias_s = reinterpret_cast<float*>(smem + G::kLds);     // the workgroup's 128 (K-split: 64) bias values, fp32
    {
        const int c = (KSPLIT ? blockIdx.y * 64 : blockIdx.y * 128) + tid;
        bias_s[tid] = (bias != nullptr && c < dm.Cout && (!KSPLIT || tid < 64)) ? bf16_to_f32(bias[c].bits) : 0.f;
    }

    // persistent workgroups, one contiguous eighth of the tiles per XCD: neighbouring tiles share two of their three halo rows
    const TileRange range = xcd_tile_range(dm.tiles_per_image * dm.N);
    const int tile_end = range.end, lanes_per_xcd = range.step;
    int tile = range.first;
    if (tile >= tile_end) return;

    const int ksteps_per_tap = dm.Cin / 16;
    const size_t ctile_stride = (size_t)9 * ksteps_per_tap * 512;      // elements between the packed column tiles
    const bf16_t* wfrag = Wp + (size_t)(col0 / 32) * ctile_stride + lane * 8;

    // this wave's weight batches of a chunk: all 9 kBpt of them, or every other one when the two waves split K
    constexpr int kBatches = 9 * G::kBpt;
    const int my_batches = KSPLIT ? (kBatches - wave + 1) / 2 : kBatches;
    auto batch = [&](int i) { return KSPLIT ? wave + 2 * i : i; };

    // halo pieces travel through registers and are requested one (tile, chunk) AHEAD of their use
    u32x4 stage[G::kIters];
    auto load_halo = [&](int tl, int c0) {
        const int im = tl / dm.tiles_per_image, first = (tl - im * dm.tiles_per_image) * kPix;
        const bf16_t* ximg = X + (size_t)im * dm.H * dm.W * dm.Cin + c0;
#pragma unroll
        for (int it = 0; it < G::kIters; ++it) {
            const int i = tid + it * kThreads;
            const int piece = i % (G::kChunk / 8), slot = i / (G::kChunk / 8);
            if (i < G::kPieces)
                stage[it] = *reinterpret_cast<const u32x4*>(ximg + (size_t)slot_pixel<STRIDE>(slot, first, dm) * dm.Cin + piece * 8);
        }
    };
    const int cbeg = blockIdx.z * dm.cin_per_z, cend = cbeg + dm.cin_per_z;
    load_halo(tile, cbeg);

    for (; tile < tile_end; tile += lanes_per_xcd) {
        const int img = tile / dm.tiles_per_image;
        const int p0 = (tile - img * dm.tiles_per_image) * kPix;       // first output pixel of the tile inside the image

        // which of the 9 taps exist for this lane's two pixels (row tiles a = 0, 1: output pixel p0 + 32 a + nl)
        unsigned tapmask[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int q = p0 + 32 * a + nl;
            const int y = q / dm.Wo, x = q - y * dm.Wo;
            unsigned m = 0;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int yy = y * STRIDE + t / 3 - 1, xx = x * STRIDE + t % 3 - 1;
                if (q < HWo && yy >= 0 && yy < dm.H && xx >= 0 && xx < dm.W) m |= 1u << t;
            }
            tapmask[a] = m;
        }

        // zeroing, quad epilogue and row store stay this kernel's own: with zero_acc / stage_quads (mfma_tile.hpp) in their place the
        // <1, false> instantiation (256 registers, 36 bytes of scratch) gains an instruction or 260 bytes of scratch
        f32x16 acc[2][2];  // [row tile][column tile]
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

        for (int c0 = cbeg; c0 < cend; c0 += G::kChunk) {
            // weights of batch kb of this chunk: tap kb / kBpt, k-steps 2 (kb % kBpt) and + 1 of the chunk
            auto load_w = [&](WFrag& f, int kb) {
                const bf16_t* p = wfrag + (size_t)((kb / G::kBpt) * ksteps_per_tap + c0 / 16 + 2 * (kb % G::kBpt)) * 512;
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
                        f.v[j][b] = *reinterpret_cast<const u32x4*>(p + (size_t)j * 512 + b * ctile_stride);
            };
            auto compute = [&](const WFrag& f, int kb) {
                const int t = kb / G::kBpt, dy = t / 3, dx = t - 3 * dy;
                const int slot = STRIDE == 1 ? dy * G::kRun + dx : dy * G::kRun + (dx == 0 ? 0 : (dx == 1 ? kPix + 1 : 1));
                const bool ok0 = (tapmask[0] >> t) & 1u, ok1 = (tapmask[1] >> t) & 1u;
                const unsigned char* a_base = halo + (slot + nl) * G::kPixStride + kg * 16 + (kb % G::kBpt) * 64;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    u32x4 a0 = *reinterpret_cast<const u32x4*>(a_base + j * 32);
                    u32x4 a1 = *reinterpret_cast<const u32x4*>(a_base + 32 * G::kPixStride + j * 32);
                    if (!ok0) a0 = u32x4{0u, 0u, 0u, 0u};
                    if (!ok1) a1 = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        acc[0][b] = mfma_32x32x16<bf16_t>(f.v[j][b], a0, acc[0][b]);
                        acc[1][b] = mfma_32x32x16<bf16_t>(f.v[j][b], a1, acc[1][b]);
                    }
                }
            };
            WFrag w0, w1;
            if (has_cols) load_w(w0, batch(0));

#pragma unroll
            for (int it = 0; it < G::kIters; ++it) {
                const int i = tid + it * kThreads;
                const int piece = i % (G::kChunk / 8), slot = i / (G::kChunk / 8);
                if (i < G::kPieces) *reinterpret_cast<u32x4*>(halo + slot * G::kPixStride + piece * 16) = stage[it];
            }
            __syncthreads();
            if (c0 + G::kChunk < cend) load_halo(tile, c0 + G::kChunk);
            else if (tile + lanes_per_xcd < tile_end) load_halo(tile + lanes_per_xcd, cbeg);

            if (has_cols) {
#pragma unroll 1
                for (int i = 0; i < my_batches; i += 2) {
                    if (i + 1 < my_batches) load_w(w1, batch(i + 1));
                    compute(w0, batch(i));
                    if (i + 2 < my_batches) load_w(w0, batch(i + 2));
                    if (i + 1 < my_batches) compute(w1, batch(i + 1));
                }
            }
            __syncthreads();  // the halo is overwritten by the next channel chunk (and by the epilogue's staging)
        }

        if (KSPLIT) {  // wave 1 hands its partial sums to wave 0
            float* red = reinterpret_cast<float*>(smem + kRedOffset);
            ALO_KSPLIT_HANDOFF(acc, red, wave, lane);
        }

        if (!KSPLIT && dm.zsplit > 1) {
            // split-K: the raw fp32 partial sums of this channel range go to partial[z][pixel][channel]; conv_splitk_finalize_kernel
            // adds the ranges up in a fixed order (deterministic), then bias / ReLU / bf16
            if (has_cols) {
                float* pz = partial + ((size_t)blockIdx.z * dm.N + img) * HWo * dm.Cout + col0;
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const int q = p0 + 32 * a + nl;
                    if (q < HWo) {
#pragma unroll
                        for (int b = 0; b < 2; ++b)
#pragma unroll
                            for (int qd = 0; qd < 4; ++qd)
                                *reinterpret_cast<f32x4*>(pz + (size_t)q * dm.Cout + 32 * b + 8 * qd + 4 * kg) =
                                    f32x4{acc[a][b][4 * qd], acc[a][b][4 * qd + 1], acc[a][b][4 * qd + 2], acc[a][b][4 * qd + 3]};
                    }
                }
            }
        } else if (has_cols && !(KSPLIT && wave == 1)) {
            unsigned char* const obuf = smem + (KSPLIT ? 0 : wave) * (kPix * kOutStride);
            // the product is computed transposed (weights = the MFMA's row operand): lane = output pixel 32 a + nl, registers
            // 4 q .. 4 q + 3 = channels col0 + 32 b + 8 q + 4 kg .. + 3 -> bias, ReLU, bf16, one 8-byte LDS write per quad
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = 32 * b + 8 * q + 4 * kg;
                    const f32x4 bb = *reinterpret_cast<const f32x4*>(bias_s + (KSPLIT ? 0 : wave) * 64 + c);
#pragma unroll
                    for (int a = 0; a < 2; ++a) {
                        float v0 = acc[a][b][4 * q] + bb[0], v1 = acc[a][b][4 * q + 1] + bb[1];
                        float v2 = acc[a][b][4 * q + 2] + bb[2], v3 = acc[a][b][4 * q + 3] + bb[3];
                        if (dm.relu) { v0 = relu_keep_nan(v0); v1 = relu_keep_nan(v1); v2 = relu_keep_nan(v2); v3 = relu_keep_nan(v3); }
                        *reinterpret_cast<u32x2*>(obuf + (32 * a + nl) * kOutStride + c * 2) = u32x2{pack_bf16x2(v0, v1), pack_bf16x2(v2, v3)};
                    }
                }
            wave_lds_fence();
            // 64 pixels x 128 B: 8 lanes x 16 B per pixel, 8 pixels per store instruction
#pragma unroll
            for (int pass = 0; pass < 8; ++pass) {
                const int row = pass * 8 + (lane >> 3);
                const int q = p0 + row;
                if (q < HWo)
                    *reinterpret_cast<u32x4*>(Y + ((size_t)img * HWo + q) * dm.Cout + col0 + (lane & 7) * 8) =
                        *reinterpret_cast<const u32x4*>(obuf + row * kOutStride + (lane & 7) * 16);
            }
        }
        __syncthreads();  // the staging is read out before the next tile's halo lands on it
    }
}

// ---- Cin = Cout = 64, stride 1 (the three conv2 of ResNet layer1): the weights never leave the registers --------------------------
// Same tile, same halo and the same K split as conv3x3_kernel<1, true>, on four waves instead of two: wave 2 h + p takes K-half h
// (that kernel's weight batches h, h + 2, .., h + 16 = channels 32 h .. 32 h + 31 of every tap, in its order) of pixels 32 p .. 32 p + 31
// of the tile.  A wave's share of the packed matrix is 9 taps x 2 k-steps x 2 column tiles x 16 B per lane = 144 registers: loaded
// once per persistent workgroup, so the tile loop has no weight traffic left.  Waves 2 and 3 hand their sums to waves 0 and 1, which
// add them (own half first) and run the epilogue for their 32 pixels each: every output is summed exactly as conv3x3_kernel<1, true>
// sums it, bit for bit.  The halo, the output staging and the partial sums have LDS of their own, which leaves two barriers per tile.
constexpr int kC64Threads = 256;
constexpr int kC64Iters = (Geo<1>::kPieces + kC64Threads - 1) / kC64Threads;   // halo pieces per thread: 7
constexpr int kC64Out = Geo<1>::kLds;                                          // bf16 output block [64 pixels][kOutStride]
constexpr int kC64Red = kC64Out + kPix * kOutStride;                           // fp32 sums of waves 2, 3: [2][32 regs][64 lanes]
constexpr int kC64Bias = kC64Red + 2 * 32 * 64 * 4;                            // 64 bias values, fp32
constexpr int kC64Lds = kC64Bias + 64 * 4;
static_assert(kC64Out % 16 == 0 && kC64Red % 16 == 0 && kC64Bias % 16 == 0, "16-byte LDS accesses");

__global__ void __launch_bounds__(kC64Threads, 2)
conv3x3_c64_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ Wp, const bf16_t* __restrict__ bias,
                   bf16_t* __restrict__ Y, const ConvDims dm) {
    using G = Geo<1>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const halo = smem;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nl = lane & 31, kg = lane >> 5;
    const int half = wave >> 1, ph = wave & 1;     // K-half, pixel half
    const int HW = dm.H * dm.W;
    float* const bias_s = reinterpret_cast<float*>(smem + kC64Bias);
    if (tid < 64) bias_s[tid] = bias != nullptr ? bf16_to_f32(bias[tid].bits) : 0.f;   // read after the tile's barriers

    // persistent workgroups, one contiguous eighth of the tiles per XCD (see conv3x3_kernel)
    const TileRange range = xcd_tile_range(dm.tiles_per_image * dm.N);
    const int tile_end = range.end, lanes_per_xcd = range.step;
    int tile = range.first;
    if (tile >= tile_end) return;

    // batch half + 2 t of conv3x3_kernel's numbering: tap t, k-steps 2 half and 2 half + 1 of the tap's four; column tiles 0 and 1
    u32x4 wreg[9][2][2];
    {
        const size_t ctile_stride = (size_t)9 * 4 * 512;
        const bf16_t* wfrag = Wp + lane * 8;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    wreg[t][j][b] = *reinterpret_cast<const u32x4*>(wfrag + (size_t)(t * 4 + 2 * half + j) * 512 + b * ctile_stride);
    }

    // The halo travels through registers, requested one tile ahead.  Piece i = tid + 256 it is 16 bytes (tid & 7) of staging slot i >> 3,
    // which holds input pixel p0 + hoff[it] of the image (clamped into it; slots past the last one repeat it and are not parked).
    u32x4 stage[kC64Iters];
    int hoff[kC64Iters];
#pragma unroll
    for (int it = 0; it < kC64Iters; ++it) {
        int slot = (tid >> 3) + it * (kC64Threads / 8);
        slot = slot < G::kSlots ? slot : G::kSlots - 1;
        const int run = slot / G::kRun;
        hoff[it] = (run - 1) * dm.W - 1 + (slot - run * G::kRun);
    }
    const unsigned piece_bytes = (tid & 7) * 16;
    auto load_halo = [&](int tl) {
        const int im = tl / dm.tiles_per_image, first = (tl - im * dm.tiles_per_image) * kPix;
        const unsigned char* ximg = reinterpret_cast<const unsigned char*>(X) + (size_t)im * HW * 128;
#pragma unroll
        for (int it = 0; it < kC64Iters; ++it) {
            int q = first + hoff[it];
            q = q < 0 ? 0 : (q > HW - 1 ? HW - 1 : q);
            stage[it] = *reinterpret_cast<const u32x4*>(ximg + ((unsigned)q * 128u + piece_bytes));   // H W < 2^24
        }
    };
    load_halo(tile);

    const unsigned char* const a_lane = halo + (32 * ph + nl) * G::kPixStride + kg * 16 + half * 64;
    float* const red = reinterpret_cast<float*>(smem + kC64Red) + ph * (32 * 64) + lane;
    unsigned char* const obuf = smem + kC64Out;

    for (; tile < tile_end; tile += lanes_per_xcd) {
        const int img = tile / dm.tiles_per_image;
        const int p0 = (tile - img * dm.tiles_per_image) * kPix;

        unsigned tapmask = 0;   // which of the 9 taps exist for this lane's pixel
        {
            const int q = p0 + 32 * ph + nl;
            const int y = q / dm.W, x = q - y * dm.W;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
                if (q < HW && yy >= 0 && yy < dm.H && xx >= 0 && xx < dm.W) tapmask |= 1u << t;
            }
        }

#pragma unroll
        for (int it = 0; it < kC64Iters; ++it) {
            const int i = tid + it * kC64Threads;
            if (it < G::kPieces / kC64Threads || i < G::kPieces)
                *reinterpret_cast<u32x4*>(halo + (i >> 3) * G::kPixStride + (i & 7) * 16) = stage[it];
        }
        __syncthreads();
        if (tile + lanes_per_xcd < tile_end) load_halo(tile + lanes_per_xcd);

        f32x16 acc[2];   // [column tile]
        zero_acc(acc);
        // A fragments of tap t + 1 are read before the MFMAs of tap t: their LDS latency hides behind four MFMAs
        u32x4 a[2][2];
#pragma unroll
        for (int j = 0; j < 2; ++j) a[0][j] = *reinterpret_cast<const u32x4*>(a_lane + j * 32);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            if (t + 1 < 9) {
                const int slot = ((t + 1) / 3) * G::kRun + (t + 1) % 3;
#pragma unroll
                for (int j = 0; j < 2; ++j) a[(t + 1) & 1][j] = *reinterpret_cast<const u32x4*>(a_lane + slot * G::kPixStride + j * 32);
            }
            const bool ok = (tapmask >> t) & 1u;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const u32x4 av = ok ? a[t & 1][j] : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
                for (int b = 0; b < 2; ++b)
                    acc[b] = mfma_32x32x16<bf16_t>(wreg[t][j][b], av, acc[b]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }

        if (half == 1) {
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[(b * 16 + r) * 64] = acc[b][r];
        }
        __syncthreads();   // the sums are in LDS, and every wave is done reading the halo
        if (half == 0) {
            // lane = output pixel 32 ph + nl, registers 4 q .. 4 q + 3 = channels 32 b + 8 q + 4 kg .. + 3 (see conv3x3_kernel).  One column
            // tile at a time (sched_barrier): 16 of the other half's sums in flight, not 32, next to the weights and the staged halo
#pragma unroll
            for (int b = 0; b < 2; ++b) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[b][r] += red[(b * 16 + r) * 64];
                stage_quads_tile<bf16_t, true>(obuf, kOutStride, acc, bias_s, dm.relu, 32 * ph + nl, 0, kg, b);
                __builtin_amdgcn_sched_barrier(0);
            }
            wave_lds_fence();
            // this wave's 32 pixels x 128 B: 8 lanes x 16 B per pixel, 8 pixels per store instruction (not store_rows: see there)
#pragma unroll
            for (int pass = 0; pass < 4; ++pass) {
                const int row = 32 * ph + pass * 8 + (lane >> 3);
                const int q = p0 + row;
                if (q < HW)
                    *reinterpret_cast<u32x4*>(Y + ((size_t)img * HW + q) * 64 + (lane & 7) * 8) =
                        *reinterpret_cast<const u32x4*>(obuf + row * kOutStride + (lane & 7) * 16);
            }
        }
        // No barrier here: the next tile's halo lands on LDS that every wave left before the barrier above; a wave re-writes its rows
        // of the output block only after its own reads of them; and waves 2, 3 re-write the sums only after the next tile's first
        // barrier, which waves 0, 1 reach after reading them.
    }
}

// ---- dilation 2, padding 2, stride 1 (layer4.1 / layer4.2 conv2 of a DC5 backbone): the nine taps sit two pixels apart ----------------
// conv3x3_kernel<1, KSPLIT>'s loop over another halo: three runs of kPix + 4 consecutive input pixels (rows y - 2, y, y + 2; flattened
// index p - 2 .. p + 65), tap (dy, dx) of tile pixel m reads slot kRun dy + 2 dx + m, and the tap mask is built from y + 2 (dy - 1),
// x + 2 (dx - 1).  The weights, their order, the K split, split-K and the epilogue are that kernel's.  It is a kernel of its own: as a
// third template argument of conv3x3_kernel the geometry would rename the existing instantiations, and <1, false> sits at 256 registers.
struct GeoD2 {
    static constexpr int kChunk = Geo<1>::kChunk;
    static constexpr int kBpt = kChunk / 32;                 // weight batches (two k-steps each) per tap and chunk
    static constexpr int kRun = kPix + 4;                    // staged pixels per tap row
    static constexpr int kSlots = 3 * kRun;
    static constexpr int kPixStride = Geo<1>::kPixStride;
    static constexpr int kPieces = kSlots * (kChunk / 8);    // 16-byte pieces per chunk
    static constexpr int kIters = (kPieces + kThreads - 1) / kThreads;
    static constexpr int kLds = kSlots * kPixStride;
    static_assert(kLds >= kRedOffset + 64 * 64 * 4, "the epilogue's staging aliases the halo");
    static_assert(kIters == Geo<1>::kIters, "as many halo registers in flight as conv3x3_kernel<1>");
};

// flattened input pixel (clamped into the image) behind staging slot `slot` of the tile whose first output pixel is p0
__device__ __forceinline__ int slot_pixel_d2(int slot, int p0, const ConvDims& dm) {
    const int run = slot / GeoD2::kRun, pix = slot - run * GeoD2::kRun;
    const int q = p0 + (run - 1) * 2 * dm.W - 2 + pix;
    const int last = dm.H * dm.W - 1;
    return q < 0 ? 0 : (q > last ? last : q);
}

template <bool KSPLIT>
__global__ void __launch_bounds__(kThreads, 2)
conv3x3_d2_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ Wp, const bf16_t* __restrict__ bias,
                  bf16_t* __restrict__ Y, float* __restrict__ partial, const ConvDims dm) {
    using G = GeoD2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const halo = smem;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nl = lane & 31, kg = lane >> 5;
    const int HW = dm.H * dm.W;
    const int col0 = KSPLIT ? blockIdx.y * 64 : blockIdx.y * 128 + wave * 64;  // this wave's 64 output channels
    const bool has_cols = col0 < dm.Cout;                               // Cout % 64 == 0
    float* const bias_s = reinterpret_cast<float*>(smem + G::kLds);     // the workgroup's 128 (K-split: 64) bias values, fp32
    {
        const int c = (KSPLIT ? blockIdx.y * 64 : blockIdx.y * 128) + tid;
        bias_s[tid] = (bias != nullptr && c < dm.Cout && (!KSPLIT || tid < 64)) ? bf16_to_f32(bias[c].bits) : 0.f;
    }

    // persistent workgroups, one contiguous eighth of the tiles per XCD (see conv3x3_kernel)
    const TileRange range = xcd_tile_range(dm.tiles_per_image * dm.N);
    const int tile_end = range.end, lanes_per_xcd = range.step;
    int tile = range.first;
    if (tile >= tile_end) return;

    const int ksteps_per_tap = dm.Cin / 16;
    const size_t ctile_stride = (size_t)9 * ksteps_per_tap * 512;      // elements between the packed column tiles
    const bf16_t* wfrag = Wp + (size_t)(col0 / 32) * ctile_stride + lane * 8;

    // this wave's weight batches of a chunk: all 9 kBpt of them, or every other one when the two waves split K
    constexpr int kBatches = 9 * G::kBpt;
    const int my_batches = KSPLIT ? (kBatches - wave + 1) / 2 : kBatches;
    auto batch = [&](int i) { return KSPLIT ? wave + 2 * i : i; };

    // halo pieces travel through registers and are requested one (tile, chunk) AHEAD of their use
    u32x4 stage[G::kIters];
    auto load_halo = [&](int tl, int c0) {
        const int im = tl / dm.tiles_per_image, first = (tl - im * dm.tiles_per_image) * kPix;
        const bf16_t* ximg = X + (size_t)im * HW * dm.Cin + c0;
#pragma unroll
        for (int it = 0; it < G::kIters; ++it) {
            const int i = tid + it * kThreads;
            const int piece = i % (G::kChunk / 8), slot = i / (G::kChunk / 8);
            if (i < G::kPieces)
                stage[it] = *reinterpret_cast<const u32x4*>(ximg + (size_t)slot_pixel_d2(slot, first, dm) * dm.Cin + piece * 8);
        }
    };
    const int cbeg = blockIdx.z * dm.cin_per_z, cend = cbeg + dm.cin_per_z;
    load_halo(tile, cbeg);

    for (; tile < tile_end; tile += lanes_per_xcd) {
        const int img = tile / dm.tiles_per_image;
        const int p0 = (tile - img * dm.tiles_per_image) * kPix;       // first output pixel of the tile inside the image

        // which of the 9 taps exist for this lane's two pixels (row tiles a = 0, 1: output pixel p0 + 32 a + nl)
        unsigned tapmask[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int q = p0 + 32 * a + nl;
            const int y = q / dm.W, x = q - y * dm.W;
            unsigned m = 0;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int yy = y + 2 * (t / 3 - 1), xx = x + 2 * (t % 3 - 1);
                if (q < HW && yy >= 0 && yy < dm.H && xx >= 0 && xx < dm.W) m |= 1u << t;
            }
            tapmask[a] = m;
        }

        f32x16 acc[2][2];  // [row tile][column tile]
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

        for (int c0 = cbeg; c0 < cend; c0 += G::kChunk) {
            // weights of batch kb of this chunk: tap kb / kBpt, k-steps 2 (kb % kBpt) and + 1 of the chunk
            auto load_w = [&](WFrag& f, int kb) {
                const bf16_t* p = wfrag + (size_t)((kb / G::kBpt) * ksteps_per_tap + c0 / 16 + 2 * (kb % G::kBpt)) * 512;
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
                        f.v[j][b] = *reinterpret_cast<const u32x4*>(p + (size_t)j * 512 + b * ctile_stride);
            };
            auto compute = [&](const WFrag& f, int kb) {
                const int t = kb / G::kBpt, dy = t / 3, dx = t - 3 * dy;
                const int slot = dy * G::kRun + 2 * dx;
                const bool ok0 = (tapmask[0] >> t) & 1u, ok1 = (tapmask[1] >> t) & 1u;
                const unsigned char* a_base = halo + (slot + nl) * G::kPixStride + kg * 16 + (kb % G::kBpt) * 64;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    u32x4 a0 = *reinterpret_cast<const u32x4*>(a_base + j * 32);
                    u32x4 a1 = *reinterpret_cast<const u32x4*>(a_base + 32 * G::kPixStride + j * 32);
                    if (!ok0) a0 = u32x4{0u, 0u, 0u, 0u};
                    if (!ok1) a1 = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        acc[0][b] = mfma_32x32x16<bf16_t>(f.v[j][b], a0, acc[0][b]);
                        acc[1][b] = mfma_32x32x16<bf16_t>(f.v[j][b], a1, acc[1][b]);
                    }
                }
            };
            WFrag w0, w1;
            if (has_cols) load_w(w0, batch(0));

#pragma unroll
            for (int it = 0; it < G::kIters; ++it) {
                const int i = tid + it * kThreads;
                const int piece = i % (G::kChunk / 8), slot = i / (G::kChunk / 8);
                if (i < G::kPieces) *reinterpret_cast<u32x4*>(halo + slot * G::kPixStride + piece * 16) = stage[it];
            }
            __syncthreads();
            if (c0 + G::kChunk < cend) load_halo(tile, c0 + G::kChunk);
            else if (tile + lanes_per_xcd < tile_end) load_halo(tile + lanes_per_xcd, cbeg);

            if (has_cols) {
#pragma unroll 1
                for (int i = 0; i < my_batches; i += 2) {
                    if (i + 1 < my_batches) load_w(w1, batch(i + 1));
                    compute(w0, batch(i));
                    if (i + 2 < my_batches) load_w(w0, batch(i + 2));
                    if (i + 1 < my_batches) compute(w1, batch(i + 1));
                }
            }
            __syncthreads();  // the halo is overwritten by the next channel chunk (and by the epilogue's staging)
        }

        if (KSPLIT) {  // wave 1 hands its partial sums to wave 0
            float* red = reinterpret_cast<float*>(smem + kRedOffset);
            ALO_KSPLIT_HANDOFF(acc, red, wave, lane);
        }

        if (!KSPLIT && dm.zsplit > 1) {
            // split-K: raw fp32 partial sums to partial[z][pixel][channel] for conv_splitk_finalize_kernel (see conv3x3_kernel)
            if (has_cols) {
                float* pz = partial + ((size_t)blockIdx.z * dm.N + img) * HW * dm.Cout + col0;
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const int q = p0 + 32 * a + nl;
                    if (q < HW) {
#pragma unroll
                        for (int b = 0; b < 2; ++b)
#pragma unroll
                            for (int qd = 0; qd < 4; ++qd)
                                *reinterpret_cast<f32x4*>(pz + (size_t)q * dm.Cout + 32 * b + 8 * qd + 4 * kg) =
                                    f32x4{acc[a][b][4 * qd], acc[a][b][4 * qd + 1], acc[a][b][4 * qd + 2], acc[a][b][4 * qd + 3]};
                    }
                }
            }
        } else if (has_cols && !(KSPLIT && wave == 1)) {
            unsigned char* const obuf = smem + (KSPLIT ? 0 : wave) * (kPix * kOutStride);
            // lane = output pixel 32 a + nl, registers 4 q .. 4 q + 3 = channels col0 + 32 b + 8 q + 4 kg .. + 3 (see conv3x3_kernel)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = 32 * b + 8 * q + 4 * kg;
                    const f32x4 bb = *reinterpret_cast<const f32x4*>(bias_s + (KSPLIT ? 0 : wave) * 64 + c);
#pragma unroll
                    for (int a = 0; a < 2; ++a) {
                        float v0 = acc[a][b][4 * q] + bb[0], v1 = acc[a][b][4 * q + 1] + bb[1];
                        float v2 = acc[a][b][4 * q + 2] + bb[2], v3 = acc[a][b][4 * q + 3] + bb[3];
                        if (dm.relu) { v0 = relu_keep_nan(v0); v1 = relu_keep_nan(v1); v2 = relu_keep_nan(v2); v3 = relu_keep_nan(v3); }
                        *reinterpret_cast<u32x2*>(obuf + (32 * a + nl) * kOutStride + c * 2) = u32x2{pack_bf16x2(v0, v1), pack_bf16x2(v2, v3)};
                    }
                }
            wave_lds_fence();
            // 64 pixels x 128 B: 8 lanes x 16 B per pixel, 8 pixels per store instruction
#pragma unroll
            for (int pass = 0; pass < 8; ++pass) {
                const int row = pass * 8 + (lane >> 3);
                const int q = p0 + row;
                if (q < HW)
                    *reinterpret_cast<u32x4*>(Y + ((size_t)img * HW + q) * dm.Cout + col0 + (lane & 7) * 8) =
                        *reinterpret_cast<const u32x4*>(obuf + row * kOutStride + (lane & 7) * 16);
            }
        }
        __syncthreads();  // the staging is read out before the next tile's halo lands on it
    }
}

// ---- stride 1, Cout >= 128, no split-K: conv3x3_kernel<1, false>'s arithmetic with its requests issued ahead of their use ------------
// In conv3x3_kernel<1, false> every A fragment is read from LDS right in front of the MFMAs that take it, the weights are requested one
// batch (8 MFMAs) ahead, each chunk starts its weights cold, and __syncthreads drains what is in flight.  Here
//   * four waves share one halo.  Cout >= 256: a tile of 96 pixels x 256 channels, a wave = RT = 3 row tiles of 32 pixels x 64 channels, so
//     a weight fragment feeds three MFMAs, not two: the weight stream through the vector cache is what a wave waits for most (without
//     it the kernel runs 1.4-1.6 times faster, without its LDS reads 1.1 times; docs/experiments.md), and 96-pixel tiles deal the
//     headline's layer3 in one round (352 workgroups on 512 slots).  Four row tiles per wave need one wave per SIMD and lose.
//     Cout = 128 / 192: 128 pixels x 128 channels, RT = 2, wave 2 c + h = pixel half h of column half c;
//   * the A fragments of k-step s + 1 are read before the MFMAs of k-step s;
//   * the weights stream through a ring of k-step fragments (six at RT = 2, four at RT = 3), requested about 20 MFMAs ahead.  The ring
//     runs on across chunks and tiles: the weights depend on neither, so the first k-steps of the next chunk are requested before the
//     barriers, not behind them;
//   * the barriers wait for LDS alone (pipe_lds_barrier) and the epilogue orders its staging with ALO_WAVE_LDS_ORDER: neither drains the
//     ring or the staged halo.  Weights and halo come through loads in the global address space, which LDS waits do not count.
// An accumulator sees the k-steps in conv3x3_kernel's order (chunk, tap, channel), one MFMA each, from zero, with the same masking,
// bias, ReLU and rounding, and a lane of the MFMA owns one pixel: the output is that kernel's bit for bit whatever RT is.  The chunk
// body is unrolled (36 k-steps, whole turns of the ring: a ring slot has to be a register name).  Byte offsets inside an image are
// 32-bit (the host checks).
template <int PIX, int RT>   // pixels per workgroup tile; 32-pixel row tiles per wave
struct GeoPipe {
    static constexpr int kWavePix = 32 * RT;                 // pixels per wave
    static_assert(PIX == kWavePix || PIX == 2 * kWavePix, "four waves: 1 x 4 or 2 x 2 (pixels x columns)");
    static constexpr int kCols = PIX == kWavePix ? 256 : 128;   // output channels per workgroup
    static constexpr int kChunk = Geo<1>::kChunk;
    static constexpr int kSteps = 9 * (kChunk / 16);         // k-steps per chunk
    static constexpr int kRing = RT == 3 ? 4 : 6;            // weight fragments (one k-step, two column tiles) in the ring: ~20 MFMAs ahead
    static_assert(kSteps % kRing == 0, "a chunk is a whole number of turns: a slot is the same register name in every chunk");
    static constexpr int kRun = PIX + 2;
    static constexpr int kSlots = 3 * kRun;
    static constexpr int kPixStride = Geo<1>::kPixStride;
    static constexpr int kPieces = kSlots * (kChunk / 8);
    static constexpr int kIters = (kPieces + 255) / 256;     // halo pieces per thread: 10 (PIX = 96), 13 (128)
    static constexpr int kHalo = kSlots * kPixStride;
    static constexpr int kOut = 4 * kWavePix * kOutStride;   // four waves' bf16 output blocks; aliases the halo
    static constexpr int kLds = kHalo > kOut ? kHalo : kOut;
};
constexpr int kPipeThreads = 256;

// waits for this wave's LDS traffic only, then the workgroup barrier (encoder_block.hip's lds_barrier)
__device__ __forceinline__ void pipe_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <int PIX, int RT>
__global__ void __launch_bounds__(kPipeThreads, 2)
conv3x3_pipe_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ Wp, const bf16_t* __restrict__ bias,
                    bf16_t* __restrict__ Y, const ConvDims dm) {   // dm.tiles_per_image counts tiles of PIX pixels
    using G = GeoPipe<PIX, RT>;
    typedef const u32x4 __attribute__((address_space(1))) * global_u32x4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const halo = smem;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;   // wave: known uniform to the compiler
    const int nl = lane & 31, kg = lane >> 5;
    const int wcol = PIX == G::kWavePix ? wave : wave >> 1;              // this wave's 64 columns of the workgroup's
    const int pbase = PIX == G::kWavePix ? 0 : G::kWavePix * (wave & 1);   // and its pixels of the tile
    const int HW = dm.H * dm.W;
    const int col0 = blockIdx.y * G::kCols + wcol * 64;
    const bool has_cols = col0 < dm.Cout;                  // Cout % 64 == 0
    float* const bias_s = reinterpret_cast<float*>(smem + G::kLds);   // the workgroup's bias values, fp32; read after the tile's barriers
    {
        const int c = blockIdx.y * G::kCols + tid;
        bias_s[tid] = (bias != nullptr && tid < G::kCols && c < dm.Cout) ? bf16_to_f32(bias[c].bits) : 0.f;
    }

    // persistent workgroups, one contiguous eighth of the tiles per XCD (see conv3x3_kernel)
    const TileRange range = xcd_tile_range(dm.tiles_per_image * dm.N);
    const int tile_end = range.end, lanes_per_xcd = range.step;
    int tile = range.first;
    if (tile >= tile_end) return;

    const int ksteps_per_tap = dm.Cin / 16;
    const size_t ctile_stride = (size_t)9 * ksteps_per_tap * 512;      // elements between the packed column tiles
    const bf16_t* const wcols = Wp + (size_t)(has_cols ? col0 / 32 : 0) * ctile_stride;   // uniform; + this lane's 16 bytes of a fragment
    const unsigned lane_bytes = lane * 16;
    // k-step s of the chunk at channel c0: tap s / 4, channels c0 + 16 (s % 4) .. (conv3x3_kernel's order), both column tiles
    auto load_w = [&](u32x4 (&f)[2], int c0, int s) {
        const bf16_t* p = wcols + (size_t)((s >> 2) * ksteps_per_tap + (c0 >> 4) + (s & 3)) * 512;
#pragma unroll
        for (int b = 0; b < 2; ++b)
            f[b] = *(global_u32x4)(uintptr_t)(reinterpret_cast<const unsigned char*>(p + b * ctile_stride) + lane_bytes);
    };

    // The halo travels through registers, requested one (tile, chunk) ahead.  Piece i = tid + 256 it is 16 bytes (tid & 7) of staging
    // slot i >> 3 (slots past the last one repeat it and are not parked); every request is made, in-range by clamping.
    u32x4 stage[G::kIters];
    const unsigned piece_bytes = (tid & 7) * 16, row_bytes = dm.Cin * 2;
    auto load_halo = [&](int tl, int c0) {
        const int im = tl / dm.tiles_per_image, first = (tl - im * dm.tiles_per_image) * PIX;
        const unsigned char* ximg = reinterpret_cast<const unsigned char*>(X + (size_t)im * HW * dm.Cin + c0);   // uniform
#pragma unroll
        for (int it = 0; it < G::kIters; ++it) {
            int slot = (tid >> 3) + it * (kPipeThreads / 8);
            slot = slot < G::kSlots ? slot : G::kSlots - 1;
            const int run = slot / G::kRun;
            int q = first + (run - 1) * dm.W - 1 + (slot - run * G::kRun);
            q = q < 0 ? 0 : (q > HW - 1 ? HW - 1 : q);
            stage[it] = *(global_u32x4)(uintptr_t)(ximg + ((unsigned)q * row_bytes + piece_bytes));   // H W Cin < 2^30
        }
    };
    load_halo(tile, 0);

    // k-step n of the wave's stream (kSteps = 36 per chunk, chunks and tiles on end) lives in ring[n % kRing]; a chunk is a whole number
    // of turns, so a slot is the same register name in every chunk.  A wave without columns streams column tile 0 and stores nothing: no branch
    // around the requests, whose count the compiler's waits rely on.
    u32x4 ring[G::kRing][2];   // [slot][column tile]
#pragma unroll
    for (int s = 0; s < G::kRing - 1; ++s) load_w(ring[s], 0, s);
    __builtin_amdgcn_sched_barrier(0);

    const unsigned char* const a_lane = halo + (pbase + nl) * G::kPixStride + kg * 16;
    unsigned char* const obuf = smem + wave * (G::kWavePix * kOutStride);

    for (; tile < tile_end; tile += lanes_per_xcd) {
        const int img = tile / dm.tiles_per_image;
        const int p0 = (tile - img * dm.tiles_per_image) * PIX + pbase;   // this wave's first output pixel inside the image
        const int next_tile = tile + lanes_per_xcd < tile_end ? tile + lanes_per_xcd : tile;

        // which of the 9 taps exist for this lane's pixels (row tile a: output pixel p0 + 32 a + nl)
        unsigned tapmask[RT];
#pragma unroll
        for (int a = 0; a < RT; ++a) {
            const int q = p0 + 32 * a + nl;
            const int y = q / dm.W, x = q - y * dm.W;
            unsigned m = 0;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
                if (q < HW && yy >= 0 && yy < dm.H && xx >= 0 && xx < dm.W) m |= 1u << t;
            }
            tapmask[a] = m;
        }

        f32x16 acc[RT][2];  // [row tile][column tile]
        zero_acc(acc);

#pragma unroll 1
        for (int c0 = 0; c0 < dm.Cin; c0 += G::kChunk) {
#pragma unroll
            for (int it = 0; it < G::kIters; ++it) {
                const int i = tid + it * kPipeThreads;
                if (it < G::kPieces / kPipeThreads || i < G::kPieces)
                    *reinterpret_cast<u32x4*>(halo + (i >> 3) * G::kPixStride + (i & 7) * 16) = stage[it];
            }
            pipe_lds_barrier();
            // the next chunk, of this tile or of the next one (the last tile asks for its own first chunk again: no branch around requests)
            const bool last_chunk = c0 + G::kChunk >= dm.Cin;
            const int c0_next = last_chunk ? 0 : c0 + G::kChunk;
            load_halo(last_chunk ? next_tile : tile, c0_next);
            __builtin_amdgcn_sched_barrier(0);

            u32x4 af[2][RT];   // [k-step parity][row tile]: the fragments of k-step s + 1 are read before the MFMAs of k-step s
#pragma unroll
            for (int a = 0; a < RT; ++a) af[0][a] = *reinterpret_cast<const u32x4*>(a_lane + 32 * a * G::kPixStride);
#pragma unroll
            for (int s = 0; s < G::kSteps; ++s) {   // k-step of the chunk: tap s / 4, channels 16 (s % 4) ..
                // k-step s + kAhead of the stream takes the slot k-step s - 1 left
                constexpr int kAhead = G::kRing - 1;
                if (s + kAhead < G::kSteps) load_w(ring[(s + kAhead) % G::kRing], c0, s + kAhead);
                else load_w(ring[(s + kAhead) % G::kRing], c0_next, s + kAhead - G::kSteps);
                if (s + 1 < G::kSteps) {
                    const int tn = (s + 1) >> 2, slot = (tn / 3) * G::kRun + tn % 3;
#pragma unroll
                    for (int a = 0; a < RT; ++a)
                        af[(s + 1) & 1][a] = *reinterpret_cast<const u32x4*>(a_lane + (slot + 32 * a) * G::kPixStride + ((s + 1) & 3) * 32);
                }
                __builtin_amdgcn_sched_barrier(0);
                const int t = s >> 2;
                u32x4 am[RT];
#pragma unroll
                for (int a = 0; a < RT; ++a) am[a] = ((tapmask[a] >> t) & 1u) ? af[s & 1][a] : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int a = 0; a < RT; ++a) acc[a][b] = mfma_32x32x16<bf16_t>(ring[s % G::kRing][b], am[a], acc[a][b]);
                __builtin_amdgcn_sched_barrier(0);
            }
            pipe_lds_barrier();  // the halo is overwritten by the next channel chunk (and by the epilogue's staging)
        }

        if (has_cols) {
            // lane = output pixel 32 a + nl, registers 4 q .. 4 q + 3 = channels col0 + 32 b + 8 q + 4 kg .. + 3 (see conv3x3_kernel)
            stage_quads<bf16_t, true>(obuf, kOutStride, acc, bias_s + wcol * 64, dm.relu, nl, 0, kg);
            ALO_WAVE_LDS_ORDER();
            // the wave's pixels x 128 B: 8 lanes x 16 B per pixel, 8 pixels per store instruction
#pragma unroll
            for (int pass = 0; pass < G::kWavePix / 8; ++pass) {
                const int row = pass * 8 + (lane >> 3);
                const int q = p0 + row;
                if (q < HW)
                    *reinterpret_cast<u32x4*>(Y + ((size_t)img * HW + q) * dm.Cout + col0 + (lane & 7) * 8) =
                        *reinterpret_cast<const u32x4*>(obuf + row * kOutStride + (lane & 7) * 16);
            }
        }
        pipe_lds_barrier();  // the staging is read out before the next tile's halo lands on it
    }
}

// ---- stride 2, Cout >= 128, no split-K: conv3x3_kernel<2, false>'s arithmetic and halo on conv3x3_pipe_kernel's loop ------------------
// The waves, the tiles, the A fragments one k-step ahead, the weight ring that runs on across chunks and tiles, the barriers and the
// epilogue are conv3x3_pipe_kernel's.  The halo is conv3x3_kernel<2, ...>'s: 32 channels per chunk (at 64 the 96-pixel halo takes 83 KB
// and two workgroups no longer share a CU), per tap row a run of PIX + 1 odd-column and a run of PIX even-column pixels of input row
// 2 y + dy - 1; tap (dy, dx) of tile pixel m reads slot dy kRun + (dx == 0 ? 0 : dx == 1 ? PIX + 1 : 1) + m.  A chunk is 18 k-steps
// (tap s / 2, channels 16 (s % 2) ..), so the unrolled body is two chunks: 36 k-steps, whole turns of either ring.  The pixel behind
// a staging slot depends on the tile alone (slot_pixel<2> divides per piece and chunk): its byte offset is worked out once per tile,
// in the tile's last chunk for the next tile, and kept in registers.  An accumulator sees conv3x3_kernel<2, false>'s k-steps in
// that kernel's order from zero, with its masking, bias, ReLU and rounding: the output is that kernel's bit for bit.
template <int PIX, int RT>
struct GeoPipeS2 {
    static constexpr int kWavePix = 32 * RT;
    static_assert(PIX == kWavePix || PIX == 2 * kWavePix, "four waves: 1 x 4 or 2 x 2 (pixels x columns)");
    static constexpr int kCols = PIX == kWavePix ? 256 : 128;
    static constexpr int kChunk = Geo<2>::kChunk;
    static constexpr int kSteps = 9 * (kChunk / 16);         // k-steps per chunk: 18
    static constexpr int kBody = 2;                          // chunks per unrolled body (Cin % 64 == 0)
    static constexpr int kRing = GeoPipe<PIX, RT>::kRing;
    static_assert((kBody * kSteps) % kRing == 0, "a body is a whole number of turns: a slot is the same register name in every body");
    static constexpr int kRun = 2 * PIX + 1;                 // PIX + 1 odd-column pixels, then PIX even-column ones
    static constexpr int kSlots = 3 * kRun;
    static constexpr int kPixStride = Geo<2>::kPixStride;
    static constexpr int kPieces = kSlots * (kChunk / 8);
    static constexpr int kIters = (kPieces + 255) / 256;     // halo pieces per thread: 10 (PIX = 96), 13 (128)
    static constexpr int kHalo = kSlots * kPixStride;        // 46320 B (PIX = 96), 61680 B (128)
    static constexpr int kOut = 4 * kWavePix * kOutStride;   // four waves' bf16 output blocks; aliases the halo
    static constexpr int kLds = kHalo > kOut ? kHalo : kOut;
    static constexpr int kOffsets = kIters * 256 * 4;        // behind the bias values: the halo pieces' byte offsets inside the image
    static_assert(2 * (kLds + 256 * 4 + kOffsets) <= 160 * 1024, "two workgroups per CU");
};

// slot_pixel<2> for a tile of PIX pixels
template <int PIX>
__device__ __forceinline__ int slot_pixel_s2(int slot, int p0, const ConvDims& dm) {
    constexpr int kRun = 2 * PIX + 1;
    const int dy = slot / kRun, r = slot - dy * kRun;
    const int odd = r < PIX + 1 ? 1 : 0;                         // column parity of this run
    int f = p0 + (odd ? r - 1 : r - (PIX + 1)) - (dy == 0 ? dm.Wo : 0);   // output-index space: (yo + oy) * Wo + xo + ox
    const int last = dm.Ho * dm.Wo - 1;
    f = f < 0 ? 0 : (f > last ? last : f);
    const int yp = f / dm.Wo, xp = f - yp * dm.Wo;
    int iy = 2 * yp + (dy == 1 ? 0 : 1), ix = 2 * xp + odd;
    iy = iy > dm.H - 1 ? dm.H - 1 : iy;
    ix = ix > dm.W - 1 ? dm.W - 1 : ix;
    return iy * dm.W + ix;
}

template <int PIX, int RT>
__global__ void __launch_bounds__(kPipeThreads, 2)
conv3x3_pipe_s2_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ Wp, const bf16_t* __restrict__ bias,
                       bf16_t* __restrict__ Y, const ConvDims dm) {   // dm.tiles_per_image counts tiles of PIX output pixels
    using G = GeoPipeS2<PIX, RT>;
    typedef const u32x4 __attribute__((address_space(1))) * global_u32x4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const halo = smem;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int nl = lane & 31, kg = lane >> 5;
    const int wcol = PIX == G::kWavePix ? wave : wave >> 1;              // this wave's 64 columns of the workgroup's
    const int pbase = PIX == G::kWavePix ? 0 : G::kWavePix * (wave & 1);   // and its pixels of the tile
    const int HWo = dm.Ho * dm.Wo;
    const int col0 = blockIdx.y * G::kCols + wcol * 64;
    const bool has_cols = col0 < dm.Cout;                  // Cout % 64 == 0
    float* const bias_s = reinterpret_cast<float*>(smem + G::kLds);   // the workgroup's bias values, fp32; read after the tile's barriers
    {
        const int c = blockIdx.y * G::kCols + tid;
        bias_s[tid] = (bias != nullptr && tid < G::kCols && c < dm.Cout) ? bf16_to_f32(bias[c].bits) : 0.f;
    }

    // persistent workgroups, one contiguous eighth of the tiles per XCD (see conv3x3_kernel)
    const TileRange range = xcd_tile_range(dm.tiles_per_image * dm.N);
    const int tile_end = range.end, lanes_per_xcd = range.step;
    int tile = range.first;
    if (tile >= tile_end) return;

    const int ksteps_per_tap = dm.Cin / 16;
    const size_t ctile_stride = (size_t)9 * ksteps_per_tap * 512;      // elements between the packed column tiles
    const bf16_t* const wcols = Wp + (size_t)(has_cols ? col0 / 32 : 0) * ctile_stride;   // uniform; + this lane's 16 bytes of a fragment
    const unsigned lane_bytes = lane * 16;
    // k-step s of the chunk at channel c0: tap s / 2, channels c0 + 16 (s % 2) .. (conv3x3_kernel<2>'s order), both column tiles
    auto load_w = [&](u32x4 (&f)[2], int c0, int s) {
        const bf16_t* p = wcols + (size_t)((s >> 1) * ksteps_per_tap + (c0 >> 4) + (s & 1)) * 512;
#pragma unroll
        for (int b = 0; b < 2; ++b)
            f[b] = *(global_u32x4)(uintptr_t)(reinterpret_cast<const unsigned char*>(p + b * ctile_stride) + lane_bytes);
    };

    // The halo travels through registers, requested one (tile, chunk) ahead.  Piece i = tid + 256 it is 16 bytes (tid & 3) of staging
    // slot i >> 2 (slots past the last one repeat it and are not parked); every request is made, in-range by clamping.  aim_halo
    // points ximg / hoff at a tile: the image and, per piece, the byte offset of its pixel inside it (H W Cin < 2^30).
    // The offsets live in LDS, [piece][thread], each thread's own: in registers, next to the staged halo, the ring and the accumulators,
    // they spill (184 / 224 bytes of scratch at RT = 3 / 2).
    u32x4 stage[G::kIters];
    unsigned* const hoff = reinterpret_cast<unsigned*>(smem + G::kLds + kPipeThreads * 4) + tid;
    const unsigned char* ximg;   // uniform
    const unsigned piece_bytes = (tid & 3) * 16, row_bytes = dm.Cin * 2;
    auto aim_halo = [&](int tl) {
        const int im = tl / dm.tiles_per_image, first = (tl - im * dm.tiles_per_image) * PIX;
        ximg = reinterpret_cast<const unsigned char*>(X + (size_t)im * dm.H * dm.W * dm.Cin);
#pragma unroll 1
        for (int it = 0; it < G::kIters; ++it) {
            int slot = (tid >> 2) + it * (kPipeThreads / 4);
            slot = slot < G::kSlots ? slot : G::kSlots - 1;
            hoff[it * kPipeThreads] = (unsigned)slot_pixel_s2<PIX>(slot, first, dm) * row_bytes + piece_bytes;
        }
    };
    auto load_halo = [&](int c0) {
        const unsigned char* xc = ximg + c0 * 2;   // uniform
#pragma unroll
        for (int it = 0; it < G::kIters; ++it) stage[it] = *(global_u32x4)(uintptr_t)(xc + hoff[it * kPipeThreads]);
    };
    aim_halo(tile);
    load_halo(0);

    // k-step n of the wave's stream (36 per body, bodies and tiles on end) lives in ring[n % kRing] (see conv3x3_pipe_kernel)
    u32x4 ring[G::kRing][2];   // [slot][column tile]
#pragma unroll
    for (int s = 0; s < G::kRing - 1; ++s) load_w(ring[s], 0, s);
    __builtin_amdgcn_sched_barrier(0);

    const unsigned char* const a_lane = halo + (pbase + nl) * G::kPixStride + kg * 16;
    unsigned char* const obuf = smem + wave * (G::kWavePix * kOutStride);

    for (; tile < tile_end; tile += lanes_per_xcd) {
        const int img = tile / dm.tiles_per_image;
        const int p0 = (tile - img * dm.tiles_per_image) * PIX + pbase;   // this wave's first output pixel inside the image
        const int next_tile = tile + lanes_per_xcd < tile_end ? tile + lanes_per_xcd : tile;

        // which of the 9 taps exist for this lane's pixels (row tile a: output pixel p0 + 32 a + nl)
        unsigned tapmask[RT];
#pragma unroll
        for (int a = 0; a < RT; ++a) {
            const int q = p0 + 32 * a + nl;
            const int y = q / dm.Wo, x = q - y * dm.Wo;
            unsigned m = 0;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int yy = 2 * y + t / 3 - 1, xx = 2 * x + t % 3 - 1;
                if (q < HWo && yy >= 0 && yy < dm.H && xx >= 0 && xx < dm.W) m |= 1u << t;
            }
            tapmask[a] = m;
        }

        f32x16 acc[RT][2];  // [row tile][column tile]
        zero_acc(acc);

#pragma unroll 1
        for (int c0 = 0; c0 < dm.Cin; c0 += G::kBody * G::kChunk) {
            const bool last_body = c0 + G::kBody * G::kChunk >= dm.Cin;
            const int c0_next = last_body ? 0 : c0 + G::kBody * G::kChunk;
#pragma unroll
            for (int h = 0; h < G::kBody; ++h) {
#pragma unroll
                for (int it = 0; it < G::kIters; ++it) {
                    const int i = tid + it * kPipeThreads;
                    if (it < G::kPieces / kPipeThreads || i < G::kPieces)
                        *reinterpret_cast<u32x4*>(halo + (i >> 2) * G::kPixStride + (i & 3) * 16) = stage[it];
                }
                pipe_lds_barrier();
                // the next chunk, of this tile or of the next one (the last tile asks for its own first chunk again: no branch around
                // requests; the branch below holds integer arithmetic alone)
                if (h + 1 < G::kBody) load_halo(c0 + (h + 1) * G::kChunk);
                else {
                    if (last_body) aim_halo(next_tile);
                    load_halo(c0_next);
                }
                __builtin_amdgcn_sched_barrier(0);

                u32x4 af[2][RT];   // [k-step parity][row tile]: the fragments of k-step s + 1 are read before the MFMAs of k-step s
#pragma unroll
                for (int a = 0; a < RT; ++a) af[0][a] = *reinterpret_cast<const u32x4*>(a_lane + 32 * a * G::kPixStride);
#pragma unroll
                for (int s = 0; s < G::kSteps; ++s) {   // k-step of the chunk: tap s / 2, channels 16 (s % 2) ..
                    // k-step n + kAhead of the body takes the slot k-step n - 1 left
                    constexpr int kAhead = G::kRing - 1, kBodySteps = G::kBody * G::kSteps;
                    const int n = h * G::kSteps + s + kAhead;
                    if (n < kBodySteps) load_w(ring[n % G::kRing], c0 + (n / G::kSteps) * G::kChunk, n % G::kSteps);
                    else load_w(ring[n % G::kRing], c0_next, n - kBodySteps);
                    if (s + 1 < G::kSteps) {
                        const int tn = (s + 1) >> 1, dy = tn / 3, dx = tn % 3;
                        const int slot = dy * G::kRun + (dx == 0 ? 0 : (dx == 1 ? PIX + 1 : 1));
#pragma unroll
                        for (int a = 0; a < RT; ++a)
                            af[(s + 1) & 1][a] = *reinterpret_cast<const u32x4*>(a_lane + (slot + 32 * a) * G::kPixStride + ((s + 1) & 1) * 32);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    const int t = s >> 1;
                    u32x4 am[RT];
#pragma unroll
                    for (int a = 0; a < RT; ++a) am[a] = ((tapmask[a] >> t) & 1u) ? af[s & 1][a] : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
                    for (int b = 0; b < 2; ++b)
#pragma unroll
                        for (int a = 0; a < RT; ++a)
                            acc[a][b] = mfma_32x32x16<bf16_t>(ring[(h * G::kSteps + s) % G::kRing][b], am[a], acc[a][b]);
                    __builtin_amdgcn_sched_barrier(0);
                }
                pipe_lds_barrier();  // the halo is overwritten by the next channel chunk (and by the epilogue's staging)
            }
        }

        if (has_cols) {
            // lane = output pixel 32 a + nl, registers 4 q .. 4 q + 3 = channels col0 + 32 b + 8 q + 4 kg .. + 3 (see conv3x3_kernel)
            stage_quads<bf16_t, true>(obuf, kOutStride, acc, bias_s + wcol * 64, dm.relu, nl, 0, kg);
            ALO_WAVE_LDS_ORDER();
            // the wave's pixels x 128 B: 8 lanes x 16 B per pixel, 8 pixels per store instruction
#pragma unroll
            for (int pass = 0; pass < G::kWavePix / 8; ++pass) {
                const int row = pass * 8 + (lane >> 3);
                const int q = p0 + row;
                if (q < HWo)
                    *reinterpret_cast<u32x4*>(Y + ((size_t)img * HWo + q) * dm.Cout + col0 + (lane & 7) * 8) =
                        *reinterpret_cast<const u32x4*>(obuf + row * kOutStride + (lane & 7) * 16);
            }
        }
        pipe_lds_barrier();  // the staging is read out before the next tile's halo lands on it
    }
}

// y[p][c] = act(sum_z partial[z][p][c] + bias[c]) -> bf16; one thread per 8 channels
__global__ void __launch_bounds__(256)
conv_splitk_finalize_kernel(const float* __restrict__ partial, const bf16_t* __restrict__ bias, bf16_t* __restrict__ Y, long rows,
                            int Cout, int Z, int relu) {
    const long n8 = rows * (Cout / 8);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
        const long e = i * 8;
        const int c = (int)(e % Cout);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = bias ? bf16_to_f32(bias[c + j].bits) : 0.f;
        for (int z = 0; z < Z; ++z) {
            const float* p = partial + (size_t)z * rows * Cout + e;
            const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { v[j] += a[j]; v[4 + j] += b[j]; }
        }
        if (relu)
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = relu_keep_nan(v[j]);
        *reinterpret_cast<u32x4*>(Y + e) = u32x4{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
    }
}

// split-K factor: only when the tiles alone leave most of the chip idle (the 2048 -> 256 input projection: 80 workgroups)
int conv_zsplit(int ntiles, int Cin, int Cout) {
    if (Cout == 64) return 1;
    const int base = ntiles * ((Cout + 127) / 128);
    int z = 1;
    while (base * z * 2 <= 1024 && Cin % (z * 2 * 64) == 0 && Cin / (z * 2) >= 128) z *= 2;
    return z;
}

template <int STRIDE, bool KSPLIT>
int launch_conv(const void* x, const void* w, const void* bias, void* y, void* partial, const ConvDims& dm, hipStream_t stream) {
    constexpr int lds = Geo<STRIDE>::kLds + kThreads * 4;
    void* args[] = {&x, &w, &bias, &y, &partial, const_cast<ConvDims*>(&dm)};
    const unsigned gy = KSPLIT ? dm.Cout / 64 : (dm.Cout + 127) / 128;
    const unsigned gx = xcd_grid(dm.tiles_per_image * dm.N, 128);   // 32 CUs per XCD x up to 4 resident workgroups
    return launch<conv3x3_kernel<STRIDE, KSPLIT>>(dim3(gx, gy, (unsigned)dm.zsplit), kThreads, lds, stream, "alo_conv3x3_nhwc", args);
}

template <bool KSPLIT>
int launch_conv_d2(const void* x, const void* w, const void* bias, void* y, void* partial, const ConvDims& dm, hipStream_t stream) {
    constexpr int lds = GeoD2::kLds + kThreads * 4;
    void* args[] = {&x, &w, &bias, &y, &partial, const_cast<ConvDims*>(&dm)};
    const unsigned gy = KSPLIT ? dm.Cout / 64 : (dm.Cout + 127) / 128;
    const unsigned gx = xcd_grid(dm.tiles_per_image * dm.N, 128);   // as launch_conv
    return launch<conv3x3_d2_kernel<KSPLIT>>(dim3(gx, gy, (unsigned)dm.zsplit), kThreads, lds, stream, "alo_conv3x3_nhwc", args);
}

int launch_conv_c64(const void* x, const void* w, const void* bias, void* y, const ConvDims& dm, hipStream_t stream) {
    void* args[] = {&x, &w, &bias, &y, const_cast<ConvDims*>(&dm)};
    const unsigned gx = xcd_grid(dm.tiles_per_image * dm.N, 64);   // 32 CUs per XCD x 2 resident workgroups (the weights take the registers of a third)
    return launch<conv3x3_c64_kernel>(dim3(gx), kC64Threads, kC64Lds, stream, "alo_conv3x3_nhwc", args);
}

template <int PIX, int RT>
int launch_conv_pipe(const void* x, const void* w, const void* bias, void* y, const ConvDims& dm, hipStream_t stream) {
    using G = GeoPipe<PIX, RT>;
    ConvDims dp = dm;
    dp.tiles_per_image = (dm.H * dm.W + PIX - 1) / PIX;
    void* args[] = {&x, &w, &bias, &y, &dp};
    const unsigned gx = xcd_grid(dp.tiles_per_image * dm.N, 64);   // 32 CUs per XCD x 2 resident workgroups of four waves
    const unsigned gy = (dm.Cout + G::kCols - 1) / G::kCols;
    return launch<conv3x3_pipe_kernel<PIX, RT>>(dim3(gx, gy), kPipeThreads, G::kLds + kPipeThreads * 4, stream, "alo_conv3x3_nhwc", args);
}

template <int PIX, int RT>
int launch_conv_pipe_s2(const void* x, const void* w, const void* bias, void* y, const ConvDims& dm, hipStream_t stream) {
    using G = GeoPipeS2<PIX, RT>;
    ConvDims dp = dm;
    dp.tiles_per_image = (dm.Ho * dm.Wo + PIX - 1) / PIX;
    void* args[] = {&x, &w, &bias, &y, &dp};
    const unsigned gx = xcd_grid(dp.tiles_per_image * dm.N, 64);   // as launch_conv_pipe
    const unsigned gy = (dm.Cout + G::kCols - 1) / G::kCols;
    return launch<conv3x3_pipe_s2_kernel<PIX, RT>>(dim3(gx, gy), kPipeThreads, G::kLds + kPipeThreads * 4 + G::kOffsets, stream, "alo_conv3x3_nhwc", args);
}

}  // namespace
}  // namespace alo

using namespace alo;

extern "C" size_t alo_conv3x3_workspace_bytes(int N, int H, int W, int Cin, int Cout, int stride) {
    // a stride that carries a five-tap flag (ALO_F32 only, conv_f32.hip) answers 0 here as well: those kernels never split K
    if (stride == (1 | ALO_CONV_DILATION_2)) stride = 1;   // the dilated flavour: the same output, the same split
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (stride != 1 && stride != 2)) return 0;
    const long hwo = (long)((H - 1) / stride + 1) * ((W - 1) / stride + 1);
    const int z = conv_zsplit((int)((hwo + kPix - 1) / kPix) * N, Cin, Cout);
    return z > 1 ? (size_t)z * N * hwo * Cout * sizeof(float) : 0;
}

extern "C" int alo_conv3x3_nhwc(const void* x, const void* w_packed, const void* bias, void* y, void* workspace, int N, int H,
                                int W, int Cin, int Cout, int stride, int relu, int dtype, void* stream) {
    ALO_REQUIRE(x && w_packed && y, ALO_ERR_INVALID_ARGUMENT, "alo_conv3x3_nhwc: null pointer argument");
    ALO_REQUIRE(N > 0 && H > 0 && W > 0, ALO_ERR_INVALID_ARGUMENT, "alo_conv3x3_nhwc: N, H, W must be positive");
    // ALO_CONV_TAPS_1X5 / ALO_CONV_TAPS_5X1 / ALO_CONV_DILATION_2 ride above the stride's low byte (a negative stride is no flagged one)
    const int flags = stride > 0 ? stride & ~0xff : 0;
    const int dil2 = flags & ALO_CONV_DILATION_2, taps = flags & ~ALO_CONV_DILATION_2;
    if (flags) stride &= 0xff;
    ALO_REQUIRE(stride == 1 || stride == 2, ALO_ERR_UNSUPPORTED, "alo_conv3x3_nhwc: stride must be 1 or 2 (got %d)", stride);
    ALO_REQUIRE(!taps || taps == ALO_CONV_TAPS_1X5 || taps == ALO_CONV_TAPS_5X1, ALO_ERR_UNSUPPORTED,
                "alo_conv3x3_nhwc: stride carries 0x%x above its low byte: one of ALO_CONV_TAPS_1X5, ALO_CONV_TAPS_5X1 (five taps), ALO_CONV_DILATION_2 or nothing", taps);
    ALO_REQUIRE(!taps || stride == 1, ALO_ERR_UNSUPPORTED, "alo_conv3x3_nhwc: the five-tap flavours (ALO_CONV_TAPS_*) are stride 1 only");
    ALO_REQUIRE(!dil2 || stride == 1, ALO_ERR_UNSUPPORTED, "alo_conv3x3_nhwc: the dilated flavour (ALO_CONV_DILATION_2) is stride 1 only");
    ALO_REQUIRE(!dil2 || !taps, ALO_ERR_UNSUPPORTED,
                "alo_conv3x3_nhwc: ALO_CONV_DILATION_2 does not combine with the five-tap flavours (ALO_CONV_TAPS_*)");
    ALO_REQUIRE(Cin >= 64 && Cin % 64 == 0 && Cout >= 64 && Cout % 64 == 0, ALO_ERR_UNSUPPORTED,
                "alo_conv3x3_nhwc: Cin and Cout must be multiples of 64 (Cin=%d Cout=%d)", Cin, Cout);
    // ALO_F32 (conv_f32.hip) is held to the checks of a bf16 call; every other dtype meets the refusal it always met
    ALO_REQUIRE(dtype == ALO_BF16 || dtype == ALO_F32, ALO_ERR_UNSUPPORTED, "alo_conv3x3_nhwc: bf16 only (dtype %d)", dtype);
    ALO_REQUIRE(!taps || dtype == ALO_F32, ALO_ERR_UNSUPPORTED, "alo_conv3x3_nhwc: the five-tap flavours (ALO_CONV_TAPS_*) take ALO_F32 only");
    ALO_REQUIRE(aligned16(x, w_packed, y, workspace), ALO_ERR_INVALID_ARGUMENT, "alo_conv3x3_nhwc: pointers must be 16-byte aligned");
    ALO_REQUIRE((long)H * W < (1L << 24) && (long)N * H * W * (long)(Cin > Cout ? Cin : Cout) < (1L << 40), ALO_ERR_UNSUPPORTED,
                "alo_conv3x3_nhwc: image too large");
    if (dtype == ALO_F32) {
        ALO_REQUIRE(workspace, ALO_ERR_INVALID_ARGUMENT,
                    "alo_conv3x3_nhwc: a workspace is required (alo_conv3x3_workspace_bytes + 4 N rounded up to 256 bytes)");
        ALO_REQUIRE(N <= 65535, ALO_ERR_UNSUPPORTED, "alo_conv3x3_nhwc: image too large");
        // the per-image magnitudes sit behind the bytes alo_conv3x3_workspace_bytes reports (split-K partial sums: unused here)
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (taps) return conv_taps_f32(x, w_packed, bias, y, workspace, N, H, W, Cin, Cout, taps == ALO_CONV_TAPS_5X1, relu, s);
        void* const image_mag = static_cast<char*>(workspace) + alo_conv3x3_workspace_bytes(N, H, W, Cin, Cout, stride);
        return conv3x3_f32(x, w_packed, bias, y, image_mag, N, H, W, Cin, Cout, stride, dil2 ? 2 : 1, relu, s);
    }
    ConvDims dm;
    dm.N = N; dm.H = H; dm.W = W; dm.Cin = Cin; dm.Cout = Cout; dm.relu = relu;
    dm.Ho = (H - 1) / stride + 1;
    dm.Wo = (W - 1) / stride + 1;
    dm.tiles_per_image = (dm.Ho * dm.Wo + kPix - 1) / kPix;
    dm.zsplit = workspace ? conv_zsplit(dm.tiles_per_image * N, Cin, Cout) : 1;   // no workspace: no split-K
    dm.cin_per_z = Cin / dm.zsplit;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // ALO_CONV3X3_C64 = "stream" keeps the 64 -> 64 stride-1 shape on conv3x3_kernel<1, true> (measurement knob; read per call: a test
    // flips it inside one process)
    const char* knob = getenv("ALO_CONV3X3_C64");
    if (!dil2 && stride == 1 && Cin == 64 && Cout == 64 && dm.zsplit == 1 && !(knob && !strcmp(knob, "stream")))
        return launch_conv_c64(x, w_packed, bias, y, dm, s);
    // ALO_CONV3X3_PIPE = "off" keeps the stride-1 shapes of 128 and more output channels on conv3x3_kernel<1, false> (measurement knob,
    // read per call like ALO_CONV3X3_C64); the two kernels agree bit for bit.  Measured in the headline's graph replay, knob off then on
    // (profiles/conv3x3_pipe_{parent,change}_kernel_stats.csv, split by grid in the traces; avg (min-max) over 37 passes, us):
    //   128 ch 100 x 167: 62.9 (60.4-69.0) -> 54.7 (52.4-62.3);  256 ch 50 x 84: 73.3 (68.3-82.8) -> 50.3 (47.6-59.4);
    //   512 ch 25 x 42: 77.4 (67.2-86.8) -> 60.7 (58.9-70.3).  Faster in every one of the 37 passes, and max below min over the 30
    //   timed passes for all three (56.1 < 60.7, 53.5 < 70.3, 62.7 < 74.7); over all 37 passes max is below min for 256 channels only:
    //   at 128 and 512 the new kernel's slowest warm-up launch (pass 1) is above the old kernel's fastest eager launch (pass 0).
    //   Eager, per tag (LaunchTimer, the backbone alone, 10 forwards per leg): 128 ch 65.4 (63.7-68.4) -> 58.2 (56.7-61.2), 256 ch 75.5
    //   (73.4-79.9) -> 53.1 (52.0-57.2), 512 ch 79.5 (77.9-81.9) -> 63.9 (62.1-67.8): max below min for all three.
    // Tile shapes tried at 256 / 512 channels (us per launch, back to back): 64 x 256 two row tiles 57.9 / 62.5, 128 x 128 two row
    // tiles 61.7 / 66.5, 128 x 256 four row tiles (one wave per SIMD) 83 / 77, 96 x 256 three row tiles 49.3 / 56: the last is routed.
    const char* pipe = getenv("ALO_CONV3X3_PIPE");
    if (!dil2 && stride == 1 && Cout >= 128 && dm.zsplit == 1 && (long)H * W * Cin < (1L << 30) && !(pipe && !strcmp(pipe, "off")))
        return Cout >= 256 ? launch_conv_pipe<96, 3>(x, w_packed, bias, y, dm, s) : launch_conv_pipe<128, 2>(x, w_packed, bias, y, dm, s);
    // Stride 2 of 128 and more output channels goes to conv3x3_pipe_s2_kernel on the same terms; "off" keeps it on conv3x3_kernel<2, false>
    // as well, and ALO_CONV3X3_PIPE = "stride1" keeps it there alone (stride 1 pipelined: the routing before the stride-2 kernel).
    // Measured in the headline's graph replay, parent then change (profiles/conv3x3_pipe_s2_{parent,change}_kernel_stats.csv, split by
    // grid in the traces; avg (min-max) over 37 passes, us):
    //   128 ch 200 x 334: 111.8 (109.2-115.5) -> 77.9 (75.6-83.0);  256 ch 100 x 167: 105.6 (102.6-115.2) -> 57.7 (55.7-66.9);
    //   512 ch 50 x 84: 102.6 (93.1-111.8) -> 66.0 (63.4-76.0).  Max below min for all three, over all 37 passes and over the 30 timed
    //   ones (79.8 < 110.2, 58.1 < 104.1, 67.3 < 99.4): no shape is sent back.  The split-K call (2048 -> 256, 60.5 us) is not the route's.
    // Back to back at 256 / 512 channels: 128 x 128 two row tiles 77.1 / 79.1, 64 x 256 two row tiles 64.7 / 69.6, 96 x 256 three row
    // tiles 60.4 / 59.8 (routed); at 128 channels 128 x 128 with a ring of 6 / 4 / 3: 74.6 / 75.6 / 78.8 (docs/experiments.md).
    if (!dil2 && stride == 2 && Cout >= 128 && dm.zsplit == 1 && (long)H * W * Cin < (1L << 30) &&
        !(pipe && (!strcmp(pipe, "off") || !strcmp(pipe, "stride1"))))
        return Cout >= 256 ? launch_conv_pipe_s2<96, 3>(x, w_packed, bias, y, dm, s) : launch_conv_pipe_s2<128, 2>(x, w_packed, bias, y, dm, s);
    const bool ksplit = Cout == 64;
    const int rc = dil2 ? (ksplit ? launch_conv_d2<true>(x, w_packed, bias, y, workspace, dm, s) : launch_conv_d2<false>(x, w_packed, bias, y, workspace, dm, s))
                 : stride == 1 ? (ksplit ? launch_conv<1, true>(x, w_packed, bias, y, workspace, dm, s) : launch_conv<1, false>(x, w_packed, bias, y, workspace, dm, s))
                               : (ksplit ? launch_conv<2, true>(x, w_packed, bias, y, workspace, dm, s) : launch_conv<2, false>(x, w_packed, bias, y, workspace, dm, s));
    if (rc != ALO_OK || dm.zsplit == 1) return rc;
    const long rows = (long)N * dm.Ho * dm.Wo;
    const float* part = static_cast<const float*>(workspace);
    int z = dm.zsplit;
    long blocks = (rows * (Cout / 8) + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    void* args[] = {&part, &bias, &y, const_cast<long*>(&rows), &Cout, &z, &relu};
    return launch<conv_splitk_finalize_kernel>((unsigned)blocks, 256, 0, s, "alo_conv3x3_nhwc (finalize)", args);
}
