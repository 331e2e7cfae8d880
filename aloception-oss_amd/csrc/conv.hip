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
// That is the streaming kernel, conv3x3_kernel<Plan, KSPLIT>.  What it stages and where a tap reads is the plan's: PlanS1<1> and
// PlanS2 as above, PlanS1<2> = PlanD2 for ALO_CONV_DILATION_2 in `stride` (dilation 2, padding 2, stride 1: layer4 of a DC5
// backbone), runs of 68 pixels two rows apart with the taps two slots apart.  Two more kernels take its shapes where they win:
//   * Cin == Cout == 64 at stride 1 goes to conv3x3_c64_kernel, the same split on four waves with the weights kept in registers;
//   * Cout >= 128 without split-K and without dilation goes to the pipelined kernel, conv3x3_pipe_kernel<Plan>: this arithmetic on
//     four waves per halo, with the LDS reads and the weight requests issued ahead of the MFMAs that use them.  PipeS1<PIX, RT> is the
//     stride-1 halo of PIX pixels, PipeS2<PIX, RT> the stride-2 one with 32 channels per chunk.
// Each loop is written once; a halo (HaloS1, HaloS2) is written once for both.  Until the plans the kernels went by other names, which
// profiles/ and docs/experiments.md keep: conv3x3_kernel<1 | 2, K> = <PlanS1<1> | PlanS2, K>, conv3x3_d2_kernel<K> = conv3x3_kernel<PlanS1<2>, K>,
// conv3x3_pipe_kernel<PIX, RT> = <PipeS1<PIX, RT>>, conv3x3_pipe_s2_kernel<PIX, RT> = conv3x3_pipe_kernel<PipeS2<PIX, RT>>.
#include <cstdlib>
#include <cstring>

#include "mfma_tile.hpp"

namespace alo {
namespace {

constexpr int kPix = 64;                     // output pixels per tile
constexpr int kThreads = 128;                // two waves
constexpr int kOutStride = 64 * 2 + 16;      // LDS bytes per pixel of a wave's 64 x 64 output block
constexpr int kRedOffset = kPix * kOutStride;  // K-split: wave 1's fp32 partial sums [64 regs][64 lanes] sit behind wave 0's output block

struct ConvDims {
    int N, H, W, Ho, Wo, Cin, Cout;
    int tiles_per_image;
    int relu;
    int zsplit, cin_per_z;   // split-K over gridDim.z: workgroup z reduces input channels [z * cin_per_z, + cin_per_z)
};

struct WFrag { u32x4 v[2][2]; };    // [k-step of the batch][column tile]

// ---- halos: which input pixels a tile of PIX output pixels stages, and where a tap finds them ------------------------------------------
// Both kernels below run over these.  A halo is kChunk channels of three runs (one per tap row) of kRun pixels and gives
//   kStride, kDil   for the tap mask: constants, and the kernels spell the tap coordinates out themselves (as functions of the halo they
//                   change the code, as does the tap-mask loop as a helper: docs/experiments.md);
//   slot_pixel      the flattened input pixel, clamped into the image, behind staging slot `slot` of the tile whose first output pixel is p0;
//   tap_slot        the slot tap (dy, dx) of tile pixel 0 reads; pixel m reads m slots further on.

// stride 1, dilation DIL (padding DIL): runs of PIX + 2 DIL consecutive input pixels, rows y - DIL, y, y + DIL (flattened index
// p - DIL .. p + PIX - 1 + DIL); the taps of a row sit DIL slots apart
template <int PIX, int DIL>
struct HaloS1 {
    static constexpr int kStride = 1, kDil = DIL, kChunk = 64, kRun = PIX + 2 * DIL;
    static __device__ __forceinline__ int slot_pixel(int slot, int p0, const ConvDims& dm) {
        const int run = slot / kRun, pix = slot - run * kRun;
        const int q = p0 + (run - 1) * DIL * dm.W - DIL + pix;
        const int last = dm.H * dm.W - 1;
        return q < 0 ? 0 : (q > last ? last : q);
    }
    static __device__ __forceinline__ int tap_slot(int dy, int dx) { return dy * kRun + DIL * dx; }
};

// stride 2: per tap row dy a run of PIX + 1 odd-column and a run of PIX even-column pixels of input row 2 y + dy - 1 (in the four parity
// phases of the input a stride-2 tap is a shift of the flattened OUTPUT index); 32 channels, or the halo of twice the pixels outgrows LDS
template <int PIX>
struct HaloS2 {
    static constexpr int kStride = 2, kDil = 1, kChunk = 32, kRun = 2 * PIX + 1;
    static __device__ __forceinline__ int slot_pixel(int slot, int p0, const ConvDims& dm) {
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
    static __device__ __forceinline__ int tap_slot(int dy, int dx) { return dy * kRun + (dx == 0 ? 0 : (dx == 1 ? PIX + 1 : 1)); }
};

// ---- the streaming kernel: two waves, the weights one batch ahead (the head of the file describes it) --------------------------------
// Its plans: a halo for kPix pixels and the LDS frame around it.
template <class HALO>
struct StreamPlan : HALO {
    using HALO::kChunk;                                      // input channels staged at once
    using HALO::kRun;                                        // staged pixels per tap row
    static constexpr int kBpt = kChunk / 32;                 // weight batches (two k-steps each) per tap and chunk
    static constexpr int kSlots = 3 * kRun;
    static constexpr int kPixStride = kChunk * 2 + 16;       // LDS bytes per staged pixel (+16: conflict-free 16-byte reads)
    static constexpr int kPieces = kSlots * (kChunk / 8);    // 16-byte pieces per chunk
    static constexpr int kIters = (kPieces + kThreads - 1) / kThreads;
    static constexpr int kLds = kSlots * kPixStride;
    static_assert(kLds >= kRedOffset + 64 * 64 * 4, "the epilogue's staging aliases the halo");
};
template <int DIL> struct PlanS1 : StreamPlan<HaloS1<kPix, DIL>> {};   // named structs, not aliases: a profile shows conv3x3_kernel<PlanS1<1>, ..>
struct PlanS2 : StreamPlan<HaloS2<kPix>> {};
using PlanD2 = PlanS1<2>;   // layer4.1 / layer4.2 conv2 of a DC5 backbone
static_assert(PlanD2::kIters == PlanS1<1>::kIters, "as many halo registers in flight as undilated (<PlanS1<1>, false> sits at 256 registers)");

template <class P, bool KSPLIT>
__global__ void __launch_bounds__(kThreads, 2)
conv3x3_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ Wp, const bf16_t* __restrict__ bias,
               bf16_t* __restrict__ Y, float* __restrict__ partial, const ConvDims dm) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const halo = smem;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nl = lane & 31, kg = lane >> 5;
    const int HWo = dm.Ho * dm.Wo;
    const int col0 = KSPLIT ? blockIdx.y * 64 : blockIdx.y * 128 + wave * 64;  // this wave's 64 output channels
    const bool has_cols = col0 < dm.Cout;                               // Cout % 64 == 0
    float* const bias_s = reinterpret_cast<float*>(smem + P::kLds);     // the workgroup's 128 (K-split: 64) bias values, fp32
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
    constexpr int kBatches = 9 * P::kBpt;
    const int my_batches = KSPLIT ? (kBatches - wave + 1) / 2 : kBatches;
    auto batch = [&](int i) { return KSPLIT ? wave + 2 * i : i; };

    // halo pieces travel through registers and are requested one (tile, chunk) AHEAD of their use
    u32x4 stage[P::kIters];
    auto load_halo = [&](int tl, int c0) {
        const int im = tl / dm.tiles_per_image, first = (tl - im * dm.tiles_per_image) * kPix;
        const bf16_t* ximg = X + (size_t)im * dm.H * dm.W * dm.Cin + c0;
#pragma unroll
        for (int it = 0; it < P::kIters; ++it) {
            const int i = tid + it * kThreads;
            const int piece = i % (P::kChunk / 8), slot = i / (P::kChunk / 8);
            if (i < P::kPieces)
                stage[it] = *reinterpret_cast<const u32x4*>(ximg + (size_t)P::slot_pixel(slot, first, dm) * dm.Cin + piece * 8);
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
                const int yy = y * P::kStride + P::kDil * (t / 3) - P::kDil, xx = x * P::kStride + P::kDil * (t % 3) - P::kDil;
                if (q < HWo && yy >= 0 && yy < dm.H && xx >= 0 && xx < dm.W) m |= 1u << t;
            }
            tapmask[a] = m;
        }

        // zeroing, quad epilogue and row store stay this kernel's own: with zero_acc / stage_quads (mfma_tile.hpp) in their place the
        // <PlanS1<1>, false> instantiation (256 registers, 36 bytes of scratch) gains an instruction or 260 bytes of scratch
        f32x16 acc[2][2];  // [row tile][column tile]
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

        for (int c0 = cbeg; c0 < cend; c0 += P::kChunk) {
            // weights of batch kb of this chunk: tap kb / kBpt, k-steps 2 (kb % kBpt) and + 1 of the chunk
            auto load_w = [&](WFrag& f, int kb) {
                const bf16_t* p = wfrag + (size_t)((kb / P::kBpt) * ksteps_per_tap + c0 / 16 + 2 * (kb % P::kBpt)) * 512;
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
                        f.v[j][b] = *reinterpret_cast<const u32x4*>(p + (size_t)j * 512 + b * ctile_stride);
            };
            auto compute = [&](const WFrag& f, int kb) {
                const int t = kb / P::kBpt, dy = t / 3, dx = t - 3 * dy;
                const int slot = P::tap_slot(dy, dx);
                const bool ok0 = (tapmask[0] >> t) & 1u, ok1 = (tapmask[1] >> t) & 1u;
                const unsigned char* a_base = halo + (slot + nl) * P::kPixStride + kg * 16 + (kb % P::kBpt) * 64;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    u32x4 a0 = *reinterpret_cast<const u32x4*>(a_base + j * 32);
                    u32x4 a1 = *reinterpret_cast<const u32x4*>(a_base + 32 * P::kPixStride + j * 32);
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
            for (int it = 0; it < P::kIters; ++it) {
                const int i = tid + it * kThreads;
                const int piece = i % (P::kChunk / 8), slot = i / (P::kChunk / 8);
                if (i < P::kPieces) *reinterpret_cast<u32x4*>(halo + slot * P::kPixStride + piece * 16) = stage[it];
            }
            __syncthreads();
            if (c0 + P::kChunk < cend) load_halo(tile, c0 + P::kChunk);
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
// Same tile, same halo and the same K split as conv3x3_kernel<PlanS1<1>, true>, on four waves instead of two: wave 2 h + p takes K-half h
// (that kernel's weight batches h, h + 2, .., h + 16 = channels 32 h .. 32 h + 31 of every tap, in its order) of pixels 32 p .. 32 p + 31
// of the tile.  A wave's share of the packed matrix is 9 taps x 2 k-steps x 2 column tiles x 16 B per lane = 144 registers: loaded
// once per persistent workgroup, so the tile loop has no weight traffic left.  Waves 2 and 3 hand their sums to waves 0 and 1, which
// add them (own half first) and run the epilogue for their 32 pixels each: every output is summed exactly as that kernel
// sums it, bit for bit.  The halo, the output staging and the partial sums have LDS of their own, which leaves two barriers per tile.
constexpr int kC64Threads = 256;
constexpr int kC64Iters = (PlanS1<1>::kPieces + kC64Threads - 1) / kC64Threads;   // halo pieces per thread: 7
constexpr int kC64Out = PlanS1<1>::kLds;                                          // bf16 output block [64 pixels][kOutStride]
constexpr int kC64Red = kC64Out + kPix * kOutStride;                           // fp32 sums of waves 2, 3: [2][32 regs][64 lanes]
constexpr int kC64Bias = kC64Red + 2 * 32 * 64 * 4;                            // 64 bias values, fp32
constexpr int kC64Lds = kC64Bias + 64 * 4;
static_assert(kC64Out % 16 == 0 && kC64Red % 16 == 0 && kC64Bias % 16 == 0, "16-byte LDS accesses");

__global__ void __launch_bounds__(kC64Threads, 2)
conv3x3_c64_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ Wp, const bf16_t* __restrict__ bias,
                   bf16_t* __restrict__ Y, const ConvDims dm) {
    using G = PlanS1<1>;
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

// ---- the pipelined kernel (Cout >= 128, no split-K): the streaming kernel's arithmetic with its requests issued ahead of their use --
// In conv3x3_kernel every A fragment is read from LDS right in front of the MFMAs that take it, the weights are requested one batch
// (8 MFMAs) ahead, each chunk starts its weights cold, and __syncthreads drains what is in flight.  Here
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
// bias, ReLU and rounding, and a lane of the MFMA owns one pixel: the output is that kernel's bit for bit whatever RT is.  The loop
// body is unrolled (36 k-steps, whole turns of the ring: a ring slot has to be a register name).  Byte offsets inside an image are
// 32-bit (the host checks).
//
// Its plans: a halo for PIX pixels, the LDS frame around it, kBody (chunks per unrolled body), kOffsets (LDS bytes for the halo pieces'
// addresses, see load_halo) and the output's width and pixel count, so that a stride-1 instantiation reads the W, H W it always read.
template <class HALO, int PIX, int RT, int BODY>   // pixels per workgroup tile; 32-pixel row tiles per wave
struct PipePlan : HALO {
    using HALO::kChunk;
    using HALO::kRun;
    static constexpr int kPix = PIX, kRowTiles = RT;
    static constexpr int kWavePix = 32 * RT;                 // pixels per wave
    static_assert(PIX == kWavePix || PIX == 2 * kWavePix, "four waves: 1 x 4 or 2 x 2 (pixels x columns)");
    static constexpr int kCols = PIX == kWavePix ? 256 : 128;   // output channels per workgroup
    static constexpr int kSpt = kChunk / 16;                 // k-steps per tap and chunk
    static constexpr int kSteps = 9 * kSpt;                  // k-steps per chunk
    static constexpr int kBody = BODY;                       // chunks per unrolled body (Cin % 64 == 0)
    static constexpr int kRing = RT == 3 ? 4 : 6;            // weight fragments (one k-step, two column tiles) in the ring: ~20 MFMAs ahead
    static_assert((kBody * kSteps) % kRing == 0, "a body is a whole number of turns: a slot is the same register name in every body");
    static constexpr int kSlots = 3 * kRun;
    static constexpr int kPixStride = kChunk * 2 + 16;
    static constexpr int kPps = kChunk / 8;                  // 16-byte pieces per staged pixel
    static constexpr int kPieces = kSlots * kPps;
    static constexpr int kIters = (kPieces + 255) / 256;     // halo pieces per thread: 10 (PIX = 96), 13 (128), either stride
    static constexpr int kHalo = kSlots * kPixStride;        // stride 2: 46320 B (PIX = 96), 61680 B (128)
    static constexpr int kOut = 4 * kWavePix * kOutStride;   // four waves' bf16 output blocks; aliases the halo
    static constexpr int kLds = kHalo > kOut ? kHalo : kOut;
};
constexpr int kPipeThreads = 256;

// stride 1: 64 channels per chunk, a body of one.  A piece's pixel is the tile's first plus a constant, clamped: worked out per request
template <int PIX, int RT>
struct PipeS1 : PipePlan<HaloS1<PIX, 1>, PIX, RT, 1> {
    static constexpr int kOffsets = 0;
    static __device__ __forceinline__ int out_w(const ConvDims& dm) { return dm.W; }
    static __device__ __forceinline__ int out_pixels(const ConvDims& dm) { return dm.H * dm.W; }
};

// stride 2: 32 channels per chunk (at 64 the 96-pixel halo takes 83 KB and two workgroups no longer share a CU), so a chunk is 18
// k-steps and the unrolled body two chunks.  The pixel behind a staging slot takes divisions and depends on the tile alone: its byte
// offset is worked out once per tile, in the tile's last chunk for the next tile, and kept in LDS, [piece][thread], each thread's own
// (in registers, next to the staged halo, the ring and the accumulators, they spill: 184 / 224 bytes of scratch at RT = 3 / 2).
template <int PIX, int RT>
struct PipeS2 : PipePlan<HaloS2<PIX>, PIX, RT, 2> {
    using F = PipePlan<HaloS2<PIX>, PIX, RT, 2>;
    static constexpr int kOffsets = F::kIters * 256 * 4;     // behind the bias values
    static_assert(2 * (F::kLds + 256 * 4 + kOffsets) <= 160 * 1024, "two workgroups per CU");
    static __device__ __forceinline__ int out_w(const ConvDims& dm) { return dm.Wo; }
    static __device__ __forceinline__ int out_pixels(const ConvDims& dm) { return dm.Ho * dm.Wo; }
};

// waits for this wave's LDS traffic only, then the workgroup barrier (encoder_block.hip's lds_barrier)
__device__ __forceinline__ void pipe_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <class P>
__global__ void __launch_bounds__(kPipeThreads, 2)
conv3x3_pipe_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ Wp, const bf16_t* __restrict__ bias,
                    bf16_t* __restrict__ Y, const ConvDims dm) {   // dm.tiles_per_image counts tiles of P::kPix output pixels
    constexpr int PIX = P::kPix, RT = P::kRowTiles;
    typedef const u32x4 __attribute__((address_space(1))) * global_u32x4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const halo = smem;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;   // wave: known uniform to the compiler
    const int nl = lane & 31, kg = lane >> 5;
    const int wcol = PIX == P::kWavePix ? wave : wave >> 1;              // this wave's 64 columns of the workgroup's
    const int pbase = PIX == P::kWavePix ? 0 : P::kWavePix * (wave & 1);   // and its pixels of the tile
    const int HW = dm.H * dm.W, HWo = P::out_pixels(dm), Wo = P::out_w(dm);
    const int col0 = blockIdx.y * P::kCols + wcol * 64;
    const bool has_cols = col0 < dm.Cout;                  // Cout % 64 == 0
    float* const bias_s = reinterpret_cast<float*>(smem + P::kLds);   // the workgroup's bias values, fp32; read after the tile's barriers
    {
        const int c = blockIdx.y * P::kCols + tid;
        bias_s[tid] = (bias != nullptr && tid < P::kCols && c < dm.Cout) ? bf16_to_f32(bias[c].bits) : 0.f;
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
    // k-step s of the chunk at channel c0: tap s / kSpt, channels c0 + 16 (s % kSpt) .. (conv3x3_kernel's order), both column tiles
    auto load_w = [&](u32x4 (&f)[2], int c0, int s) {
        const bf16_t* p = wcols + (size_t)((s / P::kSpt) * ksteps_per_tap + (c0 >> 4) + (s % P::kSpt)) * 512;
#pragma unroll
        for (int b = 0; b < 2; ++b)
            f[b] = *(global_u32x4)(uintptr_t)(reinterpret_cast<const unsigned char*>(p + b * ctile_stride) + lane_bytes);
    };

    // The halo travels through registers, requested one (tile, chunk) ahead.  Piece i = tid + 256 it is 16 bytes (tid % kPps) of staging
    // slot i / kPps (slots past the last one repeat it and are not parked); every request is made, in-range by clamping.  A plan with
    // kOffsets keeps the byte offset of each piece's pixel inside the image (H W Cin < 2^30) in hoff: aim_halo points ximg / hoff at a
    // tile, load_halo then only adds the chunk.  Without, aim_halo is empty and load_halo works the pixel out per request.  This is the
    // one part of the loop the plans do not share.
    u32x4 stage[P::kIters];
    unsigned* const hoff = reinterpret_cast<unsigned*>(smem + P::kLds + kPipeThreads * 4) + tid;
    const unsigned char* ximg = nullptr;   // uniform
    const unsigned piece_bytes = (tid % P::kPps) * 16, row_bytes = dm.Cin * 2;
    auto aim_halo = [&](int tl) {
        if constexpr (P::kOffsets != 0) {
            const int im = tl / dm.tiles_per_image, first = (tl - im * dm.tiles_per_image) * PIX;
            ximg = reinterpret_cast<const unsigned char*>(X + (size_t)im * dm.H * dm.W * dm.Cin);
#pragma unroll 1
            for (int it = 0; it < P::kIters; ++it) {
                int slot = tid / P::kPps + it * (kPipeThreads / P::kPps);
                slot = slot < P::kSlots ? slot : P::kSlots - 1;
                hoff[it * kPipeThreads] = (unsigned)P::slot_pixel(slot, first, dm) * row_bytes + piece_bytes;
            }
        }
    };
    auto load_halo = [&](int tl, int c0) {   // tl: the tile aim_halo was given last
        if constexpr (P::kOffsets != 0) {
            const unsigned char* xc = ximg + c0 * 2;   // uniform
#pragma unroll
            for (int it = 0; it < P::kIters; ++it) stage[it] = *(global_u32x4)(uintptr_t)(xc + hoff[it * kPipeThreads]);
        } else {
            const int im = tl / dm.tiles_per_image, first = (tl - im * dm.tiles_per_image) * PIX;
            const unsigned char* xc = reinterpret_cast<const unsigned char*>(X + (size_t)im * HW * dm.Cin + c0);   // uniform
#pragma unroll
            for (int it = 0; it < P::kIters; ++it) {
                int slot = tid / P::kPps + it * (kPipeThreads / P::kPps);
                slot = slot < P::kSlots ? slot : P::kSlots - 1;
                // HaloS1::slot_pixel, spelled out: through the function four unsigned compares of <128, 2> (three of <96, 3>) turn round
                const int run = slot / P::kRun;
                int q = first + (run - 1) * dm.W - 1 + (slot - run * P::kRun);
                q = q < 0 ? 0 : (q > HW - 1 ? HW - 1 : q);
                stage[it] = *(global_u32x4)(uintptr_t)(xc + ((unsigned)q * row_bytes + piece_bytes));   // H W Cin < 2^30
            }
        }
    };
    aim_halo(tile);
    load_halo(tile, 0);

    // k-step n of the wave's stream (36 per body, bodies and tiles on end) lives in ring[n % kRing]; a body is a whole number of turns,
    // so a slot is the same register name in every body.  A wave without columns streams column tile 0 and stores nothing: no branch
    // around the requests, whose count the compiler's waits rely on.
    u32x4 ring[P::kRing][2];   // [slot][column tile]
#pragma unroll
    for (int s = 0; s < P::kRing - 1; ++s) load_w(ring[s], 0, s);
    __builtin_amdgcn_sched_barrier(0);

    const unsigned char* const a_lane = halo + (pbase + nl) * P::kPixStride + kg * 16;
    unsigned char* const obuf = smem + wave * (P::kWavePix * kOutStride);

    for (; tile < tile_end; tile += lanes_per_xcd) {
        const int img = tile / dm.tiles_per_image;
        const int p0 = (tile - img * dm.tiles_per_image) * PIX + pbase;   // this wave's first output pixel inside the image
        const int next_tile = tile + lanes_per_xcd < tile_end ? tile + lanes_per_xcd : tile;

        // which of the 9 taps exist for this lane's pixels (row tile a: output pixel p0 + 32 a + nl)
        unsigned tapmask[RT];
#pragma unroll
        for (int a = 0; a < RT; ++a) {
            const int q = p0 + 32 * a + nl;
            const int y = q / Wo, x = q - y * Wo;
            unsigned m = 0;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int yy = y * P::kStride + t / 3 - 1, xx = x * P::kStride + t % 3 - 1;
                if (q < HWo && yy >= 0 && yy < dm.H && xx >= 0 && xx < dm.W) m |= 1u << t;
            }
            tapmask[a] = m;
        }

        f32x16 acc[RT][2];  // [row tile][column tile]
        zero_acc(acc);

#pragma unroll 1
        for (int c0 = 0; c0 < dm.Cin; c0 += P::kBody * P::kChunk) {
            const bool last_body = c0 + P::kBody * P::kChunk >= dm.Cin;
            const int c0_next = last_body ? 0 : c0 + P::kBody * P::kChunk;
#pragma unroll
            for (int h = 0; h < P::kBody; ++h) {
#pragma unroll
                for (int it = 0; it < P::kIters; ++it) {
                    const int i = tid + it * kPipeThreads;
                    if (it < P::kPieces / kPipeThreads || i < P::kPieces)
                        *reinterpret_cast<u32x4*>(halo + (i / P::kPps) * P::kPixStride + (i % P::kPps) * 16) = stage[it];
                }
                pipe_lds_barrier();
                // the next chunk, of this tile or of the next one (the last tile asks for its own first chunk again: no branch around
                // requests; aiming holds integer arithmetic alone)
                if (h + 1 < P::kBody) load_halo(tile, c0 + (h + 1) * P::kChunk);
                else {
                    if (last_body) aim_halo(next_tile);
                    load_halo(last_body ? next_tile : tile, c0_next);
                }
                __builtin_amdgcn_sched_barrier(0);

                u32x4 af[2][RT];   // [k-step parity][row tile]: the fragments of k-step s + 1 are read before the MFMAs of k-step s
#pragma unroll
                for (int a = 0; a < RT; ++a) af[0][a] = *reinterpret_cast<const u32x4*>(a_lane + 32 * a * P::kPixStride);
#pragma unroll
                for (int s = 0; s < P::kSteps; ++s) {   // k-step of the chunk: tap s / kSpt, channels 16 (s % kSpt) ..
                    // k-step n + kAhead of the body takes the slot k-step n - 1 left
                    constexpr int kAhead = P::kRing - 1, kBodySteps = P::kBody * P::kSteps;
                    const int n = h * P::kSteps + s + kAhead;
                    if (n < kBodySteps) load_w(ring[n % P::kRing], c0 + (n / P::kSteps) * P::kChunk, n % P::kSteps);
                    else load_w(ring[n % P::kRing], c0_next, n - kBodySteps);
                    if (s + 1 < P::kSteps) {
                        const int tn = (s + 1) / P::kSpt, slot = P::tap_slot(tn / 3, tn % 3);
#pragma unroll
                        for (int a = 0; a < RT; ++a)
                            af[(s + 1) & 1][a] =
                                *reinterpret_cast<const u32x4*>(a_lane + (slot + 32 * a) * P::kPixStride + ((s + 1) % P::kSpt) * 32);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    const int t = s / P::kSpt;
                    u32x4 am[RT];
#pragma unroll
                    for (int a = 0; a < RT; ++a) am[a] = ((tapmask[a] >> t) & 1u) ? af[s & 1][a] : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
                    for (int b = 0; b < 2; ++b)
#pragma unroll
                        for (int a = 0; a < RT; ++a)
                            acc[a][b] = mfma_32x32x16<bf16_t>(ring[(h * P::kSteps + s) % P::kRing][b], am[a], acc[a][b]);
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
            for (int pass = 0; pass < P::kWavePix / 8; ++pass) {
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

template <class P, bool KSPLIT>
int launch_conv(const void* x, const void* w, const void* bias, void* y, void* partial, const ConvDims& dm, hipStream_t stream) {
    constexpr int lds = P::kLds + kThreads * 4;
    void* args[] = {&x, &w, &bias, &y, &partial, const_cast<ConvDims*>(&dm)};
    const unsigned gy = KSPLIT ? dm.Cout / 64 : (dm.Cout + 127) / 128;
    const unsigned gx = xcd_grid(dm.tiles_per_image * dm.N, 128);   // 32 CUs per XCD x up to 4 resident workgroups
    return launch<conv3x3_kernel<P, KSPLIT>>(dim3(gx, gy, (unsigned)dm.zsplit), kThreads, lds, stream, "alo_conv3x3_nhwc", args);
}

int launch_conv_c64(const void* x, const void* w, const void* bias, void* y, const ConvDims& dm, hipStream_t stream) {
    void* args[] = {&x, &w, &bias, &y, const_cast<ConvDims*>(&dm)};
    const unsigned gx = xcd_grid(dm.tiles_per_image * dm.N, 64);   // 32 CUs per XCD x 2 resident workgroups (the weights take the registers of a third)
    return launch<conv3x3_c64_kernel>(dim3(gx), kC64Threads, kC64Lds, stream, "alo_conv3x3_nhwc", args);
}

template <class P>
int launch_conv_pipe(const void* x, const void* w, const void* bias, void* y, const ConvDims& dm, hipStream_t stream) {
    ConvDims dp = dm;
    dp.tiles_per_image = (dm.Ho * dm.Wo + P::kPix - 1) / P::kPix;
    void* args[] = {&x, &w, &bias, &y, &dp};
    const unsigned gx = xcd_grid(dp.tiles_per_image * dm.N, 64);   // 32 CUs per XCD x 2 resident workgroups of four waves
    const unsigned gy = (dm.Cout + P::kCols - 1) / P::kCols;
    return launch<conv3x3_pipe_kernel<P>>(dim3(gx, gy), kPipeThreads, P::kLds + kPipeThreads * 4 + P::kOffsets, stream, "alo_conv3x3_nhwc", args);
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
    // ALO_CONV3X3_C64 = "stream" keeps the 64 -> 64 stride-1 shape on conv3x3_kernel<PlanS1<1>, true> (measurement knob; read per call: a test
    // flips it inside one process)
    const char* knob = getenv("ALO_CONV3X3_C64");
    if (!dil2 && stride == 1 && Cin == 64 && Cout == 64 && dm.zsplit == 1 && !(knob && !strcmp(knob, "stream")))
        return launch_conv_c64(x, w_packed, bias, y, dm, s);
    // ALO_CONV3X3_PIPE = "off" keeps the stride-1 shapes of 128 and more output channels on conv3x3_kernel<PlanS1<1>, false> (measurement knob,
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
        return Cout >= 256 ? launch_conv_pipe<PipeS1<96, 3>>(x, w_packed, bias, y, dm, s) : launch_conv_pipe<PipeS1<128, 2>>(x, w_packed, bias, y, dm, s);
    // Stride 2 of 128 and more output channels goes to conv3x3_pipe_kernel<PipeS2<..>> on the same terms; "off" keeps it on conv3x3_kernel<PlanS2, false>
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
        return Cout >= 256 ? launch_conv_pipe<PipeS2<96, 3>>(x, w_packed, bias, y, dm, s) : launch_conv_pipe<PipeS2<128, 2>>(x, w_packed, bias, y, dm, s);
    const bool ksplit = Cout == 64;
    const int rc = dil2 ? (ksplit ? launch_conv<PlanD2, true>(x, w_packed, bias, y, workspace, dm, s) : launch_conv<PlanD2, false>(x, w_packed, bias, y, workspace, dm, s))
                 : stride == 1 ? (ksplit ? launch_conv<PlanS1<1>, true>(x, w_packed, bias, y, workspace, dm, s) : launch_conv<PlanS1<1>, false>(x, w_packed, bias, y, workspace, dm, s))
                               : (ksplit ? launch_conv<PlanS2, true>(x, w_packed, bias, y, workspace, dm, s) : launch_conv<PlanS2, false>(x, w_packed, bias, y, workspace, dm, s));
    if (rc != ALO_OK || dm.zsplit == 1) return rc;
    const long rows = (long)N * dm.Ho * dm.Wo;
    const float* part = static_cast<const float*>(workspace);
    int z = dm.zsplit;
    long blocks = (rows * (Cout / 8) + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    void* args[] = {&part, &bias, &y, const_cast<long*>(&rows), &Cout, &z, &relu};
    return launch<conv_splitk_finalize_kernel>((unsigned)blocks, 256, 0, s, "alo_conv3x3_nhwc (finalize)", args);
}
