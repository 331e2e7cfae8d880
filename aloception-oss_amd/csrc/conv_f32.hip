// 3x3 convolution (padding 1, stride 1 or 2) and the five-tap convolutions 1x5 (padding (0, 2)) and 5x1 (padding (2, 0)) at stride 1,
// NHWC fp32 in and out, on the fp16 matrix cores at fp32-class accuracy: the two-term split
// arithmetic of split_f16.hpp (scale, split, non-finite rule, term order, undo) in the frame of conv3x3_kernel (conv.hip's header) —
// RAFT's update block is fp32 end to end.
//
//   * scale: one power of two per IMAGE (conv_f32_absmax_kernel: the image's largest finite magnitude), so an image's result does not
//     depend on its batch neighbours.  The raw fp32 pixels travel through registers one chunk ahead, as in conv3x3_kernel, and are split
//     where a tile's halo is parked in LDS; a non-finite element spoils exactly the outputs whose window holds it.
//   * weights: split once by the caller as a (Cout, 9 Cin) matrix, one power of two per output channel (alo_hotpath.h).
//   * epilogue: the undo by k_image + k_channel, + bias, ReLU, fp32 stores in whole 256-byte runs through LDS.
//
// Tile: 64 consecutive output pixels x 128 output channels on two waves (64 each, 2 x 2 MFMA tiles), as conv3x3_kernel; the halo is
// staged 16 input channels (one k-step per tap) at a time, a pixel's hi terms and lo terms side by side (the 80-byte pixel stride of
// conv3x3_kernel<2>): 28 registers of raw pixels in flight at stride 1, and no spill next to 64 accumulators and both weight terms.  Cout == 64: the two waves take every other (tap, k-step) and wave 0 adds wave 1's sums (a fixed order).
//
// The five-tap flavours (RAFT's SepConvGRU; conv_taps_f32_kernel) are the same loop over another halo plan (Plan5): which input pixel
// stands behind a staging slot, at which slot a tap's 64 pixels begin, and whether a tap lies inside the image for an output pixel.
// 1x5: one run of 64 + 4 pixels; 5x1: five runs of 64 pixels, W pixels apart.  The weight is a (Cout, 5 Cin) tap-major matrix.  The loop
// is written over the plan; conv3x3_f32_kernel keeps its own copy of it: as an instantiation of the shared loop over a 3x3 plan its
// code changes (stride 1: 2422 -> 2441 instructions, stride 2: 4225 -> 4238, tools/isa_diff.py), and the rule of mfma_tile.hpp is that
// a kernel's code moves only with a measurement.
//
// The dilated 3x3 (ALO_CONV_DILATION_2: dilation 2, padding 2, stride 1; conv3x3_d2_f32_kernel) is that shared loop over a nine-tap plan
// (Plan3x3D2) and the undilated call's (Cout, 9 Cin) matrix.
#include "mfma_tile.hpp"
#include "split_f16.hpp"

namespace alo {
namespace {

constexpr int kPix = 64;                          // output pixels per tile
constexpr int kThreads = 128;                     // two waves

// what a kernel stages per chunk for a halo plan of SLOTS pixels
template <int SLOTS>
struct Staging {
    static constexpr int kChunk = 16;                       // input channels staged at once: one k-step per tap
    static constexpr int kSteps = kChunk / 16;              // k-steps per tap and chunk
    static constexpr int kSlots = SLOTS;
    static constexpr int kLoOffset = kChunk * 2;            // a staged pixel: kChunk hi terms, then kChunk lo terms
    static constexpr int kPixStride = kChunk * 4 + 16;      // (+16: conflict-free 16-byte reads)
    static constexpr int kPieces = kSlots * (kChunk / 4);   // 16-byte pieces (four fp32 channels) per chunk
    static constexpr int kIters = (kPieces + kThreads - 1) / kThreads;
    static constexpr int kHalo = kSlots * kPixStride;
    static constexpr int kStaging = kRedOffset + 64 * 64 * 4;   // the epilogue's staging aliases the halo (and 2 kOutBytes fit in it)
    static constexpr int kLds = kHalo > kStaging ? kHalo : kStaging;
    static_assert(kLds % 16 == 0 && kStaging >= 2 * kOutBytes, "16-byte LDS accesses; both waves' output blocks");
};
template <int STRIDE>
struct Geo : Staging<3 * (STRIDE == 1 ? kPix + 2 : 2 * kPix + 1)> {
    static constexpr int kRun = STRIDE == 1 ? kPix + 2 : 2 * kPix + 1;  // staged pixels per tap row (conv.hip's header)
};

struct ConvF32Dims {
    int N, H, W, Ho, Wo, Cin, Cout;
    int tiles_per_image;
    int relu;
};

// flattened input pixel (clamped into the image) behind staging slot `slot` of the tile whose first output pixel is p0: the halo plan of
// conv3x3_kernel (conv.hip, slot_pixel)
template <int STRIDE>
__device__ __forceinline__ int slot_pixel(int slot, int p0, const ConvF32Dims& dm) {
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

// mag[image] = bit pattern of the image's largest finite magnitude (zero on entry): per_image fp32 values per image, a multiple of 4
__global__ void __launch_bounds__(256)
conv_f32_absmax_kernel(const float* __restrict__ X, unsigned* __restrict__ mag, long per_image) {
    const f32x4* p = reinterpret_cast<const f32x4*>(X + (size_t)blockIdx.y * per_image);
    const long n4 = per_image / 4;
    auto fin = [](float v) { v = fabsf(v); return v < INFINITY ? v : 0.f; };   // Inf / NaN do not take part
    float m = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 v = p[i];
        m = fmaxf(fmaxf(m, fmaxf(fin(v[0]), fin(v[1]))), fmaxf(fin(v[2]), fin(v[3])));
    }
    unsigned w = __float_as_uint(m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) w = max(w, (unsigned)__shfl_xor((int)w, o, 64));
    if ((threadIdx.x & 63) == 0 && w) atomicMax(mag + blockIdx.y, w);
}

template <int STRIDE, bool KSPLIT>
__global__ void __launch_bounds__(kThreads, STRIDE == 1 ? 2 : 1)   // stride 2 stages twice the halo: it takes the registers of a second wave
conv3x3_f32_kernel(const float* __restrict__ X, const f16_t* __restrict__ Wp, const float* __restrict__ bias, float* __restrict__ Y,
                   const unsigned* __restrict__ mag, const ConvF32Dims dm) {
    using G = Geo<STRIDE>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const halo = smem;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nl = lane & 31, kg = lane >> 5;
    const int HWo = dm.Ho * dm.Wo;
    const int col0 = KSPLIT ? blockIdx.y * 64 : blockIdx.y * 128 + wave * 64;  // this wave's 64 output channels
    const bool has_cols = col0 < dm.Cout;                               // Cout % 64 == 0
    const size_t term_stride = (size_t)dm.Cout * 9 * dm.Cin;            // elements between the packed hi and lo matrices
    // the workgroup's 128 (K-split: 64) bias values and channel exponents
    float* const bias_s = reinterpret_cast<float*>(smem + G::kLds);
    int* const kc_s = reinterpret_cast<int*>(smem + G::kLds + kThreads * 4);
    fill_channel_tables<KSPLIT>(bias_s, kc_s, bias, reinterpret_cast<const int*>(Wp + 2 * term_stride), KSPLIT ? blockIdx.y * 64 : blockIdx.y * 128,
                                dm.Cout, tid);

    // persistent workgroups, one contiguous eighth of the tiles per XCD (see conv3x3_kernel)
    const TileRange range = xcd_tile_range(dm.tiles_per_image * dm.N);
    const int tile_end = range.end, lanes_per_xcd = range.step;
    int tile = range.first;
    if (tile >= tile_end) return;

    const int ksteps_per_tap = dm.Cin / 16;
    const size_t ctile_stride = (size_t)9 * ksteps_per_tap * 512;      // elements between the packed column tiles
    const f16_t* wfrag = Wp + (size_t)(col0 / 32) * ctile_stride + lane * 8;

    // this wave's (tap, k-step) pairs of a chunk: all 9 kSteps of them, or every other one when the two waves split K
    constexpr int kBatches = 9 * G::kSteps;
    const int my_batches = KSPLIT ? (kBatches - wave + 1) / 2 : kBatches;
    auto batch = [&](int i) { return KSPLIT ? wave + 2 * i : i; };

    // raw fp32 halo pieces travel through registers and are requested one (tile, chunk) AHEAD of their use
    u32x4 stage[G::kIters];
    auto load_halo = [&](int tl, int c0) {
        const int im = tl / dm.tiles_per_image, first = (tl - im * dm.tiles_per_image) * kPix;
        const float* ximg = X + (size_t)im * dm.H * dm.W * dm.Cin + c0;
#pragma unroll
        for (int it = 0; it < G::kIters; ++it) {
            const int i = tid + it * kThreads;
            const int piece = i % (G::kChunk / 4), slot = i / (G::kChunk / 4);
            if (i < G::kPieces)
                stage[it] = *reinterpret_cast<const u32x4*>(ximg + (size_t)slot_pixel<STRIDE>(slot, first, dm) * dm.Cin + piece * 4);
        }
    };
    load_halo(tile, 0);

    for (; tile < tile_end; tile += lanes_per_xcd) {
        const int img = tile / dm.tiles_per_image;
        const int p0 = (tile - img * dm.tiles_per_image) * kPix;       // first output pixel of the tile inside the image
        const int kimg = split_exponent(mag[img]);
        const float down = ldexpf(1.0f, -kimg);

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

        f32x16 acc[2][2];  // [row tile][column tile]
        zero_acc(acc);

        for (int c0 = 0; c0 < dm.Cin; c0 += G::kChunk) {
            // weights of pair kb of this chunk: tap kb / kSteps, k-step kb % kSteps of the chunk, both terms
            auto load_w = [&](WFrag& f, int kb) {
                load_wfrag(f, wfrag + (size_t)((kb / G::kSteps) * ksteps_per_tap + c0 / 16 + kb % G::kSteps) * 512, term_stride, ctile_stride);
            };
            auto compute = [&](const WFrag& f, int kb) {
                const int t = kb / G::kSteps, dy = t / 3, dx = t - 3 * dy;
                const int slot = STRIDE == 1 ? dy * G::kRun + dx : dy * G::kRun + (dx == 0 ? 0 : (dx == 1 ? kPix + 1 : 1));
                const bool ok0 = (tapmask[0] >> t) & 1u, ok1 = (tapmask[1] >> t) & 1u;
                const unsigned char* a_base = halo + (slot + nl) * G::kPixStride + kg * 16 + (kb % G::kSteps) * 32;
                XFrag x;
#pragma unroll
                for (int term = 0; term < 2; ++term) {
                    x.v[term][0] = *reinterpret_cast<const u32x4*>(a_base + term * G::kLoOffset);
                    x.v[term][1] = *reinterpret_cast<const u32x4*>(a_base + 32 * G::kPixStride + term * G::kLoOffset);
                    if (!ok0) x.v[term][0] = u32x4{0u, 0u, 0u, 0u};
                    if (!ok1) x.v[term][1] = u32x4{0u, 0u, 0u, 0u};
                }
                mma_split(acc, f, x);
            };
            WFrag w0, w1;
            if (has_cols) load_w(w0, batch(0));

            // park the chunk: four channels of one staged pixel -> four hi terms and four lo terms
#pragma unroll
            for (int it = 0; it < G::kIters; ++it) {
                const int i = tid + it * kThreads;
                const int piece = i % (G::kChunk / 4), slot = i / (G::kChunk / 4);
                if (i < G::kPieces) park4(halo + slot * G::kPixStride + piece * 8, G::kLoOffset, stage[it], down);
            }
            __syncthreads();
            if (c0 + G::kChunk < dm.Cin) load_halo(tile, c0 + G::kChunk);
            else if (tile + lanes_per_xcd < tile_end) load_halo(tile + lanes_per_xcd, 0);

            if (has_cols) {   // (linear_f32_kernel's loop; as a shared function it costs that kernel 14 VGPRs and changes three of these four)
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

        if (has_cols && !(KSPLIT && wave == 1)) {
            unsigned char* const obuf = smem + (KSPLIT ? 0 : wave) * kOutBytes;
            const int cs0 = (KSPLIT ? 0 : wave) * 64;    // this wave's first channel in bias_s / kc_s
            // one row tile (32 output pixels) at a time: 2^(k_image + k_channel), bias, ReLU -> LDS; then 16 lanes x 16 B per pixel.  (The
            // row store as a shared function too: layer2.x.conv2 273.5 -> 275.2 us against spreads of 0.9 and 1.5.)
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                stage_scaled_quads(obuf, acc[a], kimg, bias_s + cs0, kc_s + cs0, dm.relu, nl, kg);
                wave_lds_fence();
#pragma unroll
                for (int pass = 0; pass < 8; ++pass) {
                    const int row = pass * 4 + (lane >> 4);
                    const int q = p0 + 32 * a + row;
                    if (q < HWo)
                        *reinterpret_cast<f32x4*>(Y + ((size_t)img * HWo + q) * dm.Cout + col0 + (lane & 15) * 4) =
                            *reinterpret_cast<const f32x4*>(obuf + row * kOutStride + (lane & 15) * 16);
                }
                wave_lds_fence();   // the block is read out before the second row tile lands on it
            }
        }
        __syncthreads();  // the staging is read out before the next tile's halo lands on it
    }
}

// ---- the five-tap halo plans ----------------------------------------------------------------------------------------------------------
// slot_pixel: the flattened input pixel (clamped into the image) behind staging slot `slot` of the tile whose first output pixel is p0;
// tap_slot: the slot of tap t's pixel for the tile's first output pixel (output pixel i reads slot tap_slot + i);
// tap_inside: does tap t of output pixel (y, x) lie inside the image (outside: it contributes zero).
// 1x5, padding (0, 2): one run of 64 + 4 pixels, tap t at column x + t - 2.  5x1, padding (2, 0): five runs of 64 pixels, tap t's run
// (t - 2) W pixels from the tile's own.  Stride 1: Ho = H, Wo = W.
template <bool VERTICAL>
struct Plan5 {
    static constexpr int kTaps = 5;
    static constexpr int kSlots = VERTICAL ? 5 * kPix : kPix + 4;
    static constexpr int kMinBlocks = 2;
    static __device__ __forceinline__ int slot_pixel(int slot, int p0, const ConvF32Dims& dm) {
        const int q = VERTICAL ? p0 + (slot / kPix - 2) * dm.W + slot % kPix : p0 - 2 + slot;
        const int last = dm.H * dm.W - 1;
        return q < 0 ? 0 : (q > last ? last : q);
    }
    static __device__ __forceinline__ int tap_slot(int t) { return VERTICAL ? t * kPix : t; }
    static __device__ __forceinline__ bool tap_inside(int t, int y, int x, const ConvF32Dims& dm) {
        const int v = (VERTICAL ? y : x) + t - 2;
        return v >= 0 && v < (VERTICAL ? dm.H : dm.W);
    }
};

// The dilated 3x3 (ALO_CONV_DILATION_2: dilation 2, zero padding 2, stride 1) is a third plan: three runs of 64 + 4 pixels, 2 W pixels
// apart (rows y - 2, y, y + 2; flattened index p - 2 .. p + 65); tap t = 3 dy + dx at row y + 2 (dy - 1), column x + 2 (dx - 1) begins at
// slot kRun dy + 2 dx.  The weight is the undilated call's (Cout, 9 Cin) matrix.
struct Plan3x3D2 {
    static constexpr int kTaps = 9;
    static constexpr int kRun = kPix + 4;
    static constexpr int kSlots = 3 * kRun;
    static constexpr int kMinBlocks = 2;
    static __device__ __forceinline__ int slot_pixel(int slot, int p0, const ConvF32Dims& dm) {
        const int run = slot / kRun, pix = slot - run * kRun;
        const int q = p0 + (run - 1) * 2 * dm.W - 2 + pix;
        const int last = dm.H * dm.W - 1;
        return q < 0 ? 0 : (q > last ? last : q);
    }
    static __device__ __forceinline__ int tap_slot(int t) { return (t / 3) * kRun + 2 * (t % 3); }
    static __device__ __forceinline__ bool tap_inside(int t, int y, int x, const ConvF32Dims& dm) {
        const int yy = y + 2 * (t / 3 - 1), xx = x + 2 * (t % 3 - 1);
        return yy >= 0 && yy < dm.H && xx >= 0 && xx < dm.W;
    }
};

// conv3x3_f32_kernel's loop over halo plan P
template <class P, bool KSPLIT>
__device__ __forceinline__ void conv_f32_tiles(const float* __restrict__ X, const f16_t* __restrict__ Wp, const float* __restrict__ bias,
                                               float* __restrict__ Y, const unsigned* __restrict__ mag, const ConvF32Dims dm) {
    using G = Staging<P::kSlots>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const halo = smem;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nl = lane & 31, kg = lane >> 5;
    const int HWo = dm.Ho * dm.Wo;
    const int col0 = KSPLIT ? blockIdx.y * 64 : blockIdx.y * 128 + wave * 64;  // this wave's 64 output channels
    const bool has_cols = col0 < dm.Cout;                               // Cout % 64 == 0
    const size_t term_stride = (size_t)dm.Cout * P::kTaps * dm.Cin;            // elements between the packed hi and lo matrices
    // the workgroup's 128 (K-split: 64) bias values and channel exponents
    float* const bias_s = reinterpret_cast<float*>(smem + G::kLds);
    int* const kc_s = reinterpret_cast<int*>(smem + G::kLds + kThreads * 4);
    fill_channel_tables<KSPLIT>(bias_s, kc_s, bias, reinterpret_cast<const int*>(Wp + 2 * term_stride), KSPLIT ? blockIdx.y * 64 : blockIdx.y * 128,
                                dm.Cout, tid);

    // persistent workgroups, one contiguous eighth of the tiles per XCD (see conv3x3_kernel)
    const TileRange range = xcd_tile_range(dm.tiles_per_image * dm.N);
    const int tile_end = range.end, lanes_per_xcd = range.step;
    int tile = range.first;
    if (tile >= tile_end) return;

    const int ksteps_per_tap = dm.Cin / 16;
    const size_t ctile_stride = (size_t)P::kTaps * ksteps_per_tap * 512;      // elements between the packed column tiles
    const f16_t* wfrag = Wp + (size_t)(col0 / 32) * ctile_stride + lane * 8;

    // this wave's (tap, k-step) pairs of a chunk: all kTaps kSteps of them, or every other one when the two waves split K
    constexpr int kBatches = P::kTaps * G::kSteps;
    const int my_batches = KSPLIT ? (kBatches - wave + 1) / 2 : kBatches;
    auto batch = [&](int i) { return KSPLIT ? wave + 2 * i : i; };

    // raw fp32 halo pieces travel through registers and are requested one (tile, chunk) AHEAD of their use
    u32x4 stage[G::kIters];
    auto load_halo = [&](int tl, int c0) {
        const int im = tl / dm.tiles_per_image, first = (tl - im * dm.tiles_per_image) * kPix;
        const float* ximg = X + (size_t)im * dm.H * dm.W * dm.Cin + c0;
#pragma unroll
        for (int it = 0; it < G::kIters; ++it) {
            const int i = tid + it * kThreads;
            const int piece = i % (G::kChunk / 4), slot = i / (G::kChunk / 4);
            if (i < G::kPieces)
                stage[it] = *reinterpret_cast<const u32x4*>(ximg + (size_t)P::slot_pixel(slot, first, dm) * dm.Cin + piece * 4);
        }
    };
    load_halo(tile, 0);

    for (; tile < tile_end; tile += lanes_per_xcd) {
        const int img = tile / dm.tiles_per_image;
        const int p0 = (tile - img * dm.tiles_per_image) * kPix;       // first output pixel of the tile inside the image
        const int kimg = split_exponent(mag[img]);
        const float down = ldexpf(1.0f, -kimg);

        // which of the taps exist for this lane's two pixels (row tiles a = 0, 1: output pixel p0 + 32 a + nl)
        unsigned tapmask[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int q = p0 + 32 * a + nl;
            const int y = q / dm.Wo, x = q - y * dm.Wo;
            unsigned m = 0;
#pragma unroll
            for (int t = 0; t < P::kTaps; ++t) {
                if (q < HWo && P::tap_inside(t, y, x, dm)) m |= 1u << t;
            }
            tapmask[a] = m;
        }

        f32x16 acc[2][2];  // [row tile][column tile]
        zero_acc(acc);

        for (int c0 = 0; c0 < dm.Cin; c0 += G::kChunk) {
            // weights of pair kb of this chunk: tap kb / kSteps, k-step kb % kSteps of the chunk, both terms
            auto load_w = [&](WFrag& f, int kb) {
                load_wfrag(f, wfrag + (size_t)((kb / G::kSteps) * ksteps_per_tap + c0 / 16 + kb % G::kSteps) * 512, term_stride, ctile_stride);
            };
            auto compute = [&](const WFrag& f, int kb) {
                const int t = kb / G::kSteps, slot = P::tap_slot(t);
                const bool ok0 = (tapmask[0] >> t) & 1u, ok1 = (tapmask[1] >> t) & 1u;
                const unsigned char* a_base = halo + (slot + nl) * G::kPixStride + kg * 16 + (kb % G::kSteps) * 32;
                XFrag x;
#pragma unroll
                for (int term = 0; term < 2; ++term) {
                    x.v[term][0] = *reinterpret_cast<const u32x4*>(a_base + term * G::kLoOffset);
                    x.v[term][1] = *reinterpret_cast<const u32x4*>(a_base + 32 * G::kPixStride + term * G::kLoOffset);
                    if (!ok0) x.v[term][0] = u32x4{0u, 0u, 0u, 0u};
                    if (!ok1) x.v[term][1] = u32x4{0u, 0u, 0u, 0u};
                }
                mma_split(acc, f, x);
            };
            WFrag w0, w1;
            if (has_cols) load_w(w0, batch(0));

            // park the chunk: four channels of one staged pixel -> four hi terms and four lo terms
#pragma unroll
            for (int it = 0; it < G::kIters; ++it) {
                const int i = tid + it * kThreads;
                const int piece = i % (G::kChunk / 4), slot = i / (G::kChunk / 4);
                if (i < G::kPieces) park4(halo + slot * G::kPixStride + piece * 8, G::kLoOffset, stage[it], down);
            }
            __syncthreads();
            if (c0 + G::kChunk < dm.Cin) load_halo(tile, c0 + G::kChunk);
            else if (tile + lanes_per_xcd < tile_end) load_halo(tile + lanes_per_xcd, 0);

            if (has_cols) {   // (linear_f32_kernel's loop; as a shared function it costs that kernel 14 VGPRs and changes three of these four)
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

        if (has_cols && !(KSPLIT && wave == 1)) {
            unsigned char* const obuf = smem + (KSPLIT ? 0 : wave) * kOutBytes;
            const int cs0 = (KSPLIT ? 0 : wave) * 64;    // this wave's first channel in bias_s / kc_s
            // one row tile (32 output pixels) at a time: 2^(k_image + k_channel), bias, ReLU -> LDS; then 16 lanes x 16 B per pixel.  (The
            // row store as a shared function too: layer2.x.conv2 273.5 -> 275.2 us against spreads of 0.9 and 1.5.)
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                stage_scaled_quads(obuf, acc[a], kimg, bias_s + cs0, kc_s + cs0, dm.relu, nl, kg);
                wave_lds_fence();
#pragma unroll
                for (int pass = 0; pass < 8; ++pass) {
                    const int row = pass * 4 + (lane >> 4);
                    const int q = p0 + 32 * a + row;
                    if (q < HWo)
                        *reinterpret_cast<f32x4*>(Y + ((size_t)img * HWo + q) * dm.Cout + col0 + (lane & 15) * 4) =
                            *reinterpret_cast<const f32x4*>(obuf + row * kOutStride + (lane & 15) * 16);
                }
                wave_lds_fence();   // the block is read out before the second row tile lands on it
            }
        }
        __syncthreads();  // the staging is read out before the next tile's halo lands on it
    }
}

template <bool VERTICAL, bool KSPLIT>
__global__ void __launch_bounds__(kThreads, Plan5<VERTICAL>::kMinBlocks)
conv_taps_f32_kernel(const float* __restrict__ X, const f16_t* __restrict__ Wp, const float* __restrict__ bias, float* __restrict__ Y,
                     const unsigned* __restrict__ mag, const ConvF32Dims dm) {
    conv_f32_tiles<Plan5<VERTICAL>, KSPLIT>(X, Wp, bias, Y, mag, dm);
}

template <bool KSPLIT>
__global__ void __launch_bounds__(kThreads, Plan3x3D2::kMinBlocks)
conv3x3_d2_f32_kernel(const float* __restrict__ X, const f16_t* __restrict__ Wp, const float* __restrict__ bias, float* __restrict__ Y,
                      const unsigned* __restrict__ mag, const ConvF32Dims dm) {
    conv_f32_tiles<Plan3x3D2, KSPLIT>(X, Wp, bias, Y, mag, dm);
}

template <class G, auto KERNEL, bool KSPLIT>
int launch_conv_f32(const void* x, const void* w, const void* bias, void* y, const void* mag, const ConvF32Dims& dm, hipStream_t stream) {
    constexpr int lds = G::kLds + kThreads * 8;
    void* args[] = {&x, &w, &bias, &y, &mag, const_cast<ConvF32Dims*>(&dm)};
    const unsigned gy = KSPLIT ? dm.Cout / 64 : (dm.Cout + 127) / 128;
    const unsigned gx = xcd_grid(dm.tiles_per_image * dm.N, 128);   // 32 CUs per XCD x up to 4 resident workgroups
    return launch<KERNEL>(dim3(gx, gy), kThreads, lds, stream, "alo_conv3x3_nhwc", args);
}

// the per-image magnitudes of x (N images of per_image fp32 values) -> image_mag
int image_magnitudes(const void* x, void* image_mag, int N, long per_image, hipStream_t stream) {
    const hipError_t e = hipMemsetAsync(image_mag, 0, (size_t)N * sizeof(unsigned), stream);
    if (e != hipSuccess) return fail(ALO_ERR_LAUNCH, "alo_conv3x3_nhwc (magnitudes): %s", hipGetErrorString(e));
    long blocks = (per_image / 4 + 256 * 8 - 1) / (256 * 8);
    if (blocks > 256) blocks = 256;
    void* args[] = {&x, &image_mag, &per_image};
    return launch<conv_f32_absmax_kernel>(dim3((unsigned)blocks, (unsigned)N), 256, 0, stream, "alo_conv3x3_nhwc (magnitudes)", args);
}

}  // namespace

int conv3x3_f32(const void* x, const void* w_split, const void* bias, void* y, void* image_mag, int N, int H, int W, int Cin, int Cout,
                int stride, int dilation, int relu, hipStream_t stream) {
    ConvF32Dims dm;
    dm.N = N; dm.H = H; dm.W = W; dm.Cin = Cin; dm.Cout = Cout; dm.relu = relu;
    dm.Ho = (H - 1) / stride + 1;
    dm.Wo = (W - 1) / stride + 1;
    dm.tiles_per_image = (dm.Ho * dm.Wo + kPix - 1) / kPix;
    const int rc = image_magnitudes(x, image_mag, N, (long)H * W * Cin, stream);
    if (rc != ALO_OK) return rc;
    const bool ksplit = Cout == 64;
    if (dilation == 2)   // stride 1 (checked by the caller)
        return ksplit ? launch_conv_f32<Staging<Plan3x3D2::kSlots>, conv3x3_d2_f32_kernel<true>, true>(x, w_split, bias, y, image_mag, dm, stream)
                      : launch_conv_f32<Staging<Plan3x3D2::kSlots>, conv3x3_d2_f32_kernel<false>, false>(x, w_split, bias, y, image_mag, dm, stream);
    return stride == 1 ? (ksplit ? launch_conv_f32<Geo<1>, conv3x3_f32_kernel<1, true>, true>(x, w_split, bias, y, image_mag, dm, stream)
                                 : launch_conv_f32<Geo<1>, conv3x3_f32_kernel<1, false>, false>(x, w_split, bias, y, image_mag, dm, stream))
                       : (ksplit ? launch_conv_f32<Geo<2>, conv3x3_f32_kernel<2, true>, true>(x, w_split, bias, y, image_mag, dm, stream)
                                 : launch_conv_f32<Geo<2>, conv3x3_f32_kernel<2, false>, false>(x, w_split, bias, y, image_mag, dm, stream));
}

// 1x5 / padding (0, 2) (vertical = 0) or 5x1 / padding (2, 0) (vertical = 1), stride 1; w_split: the (Cout, 5 Cin) tap-major matrix
int conv_taps_f32(const void* x, const void* w_split, const void* bias, void* y, void* image_mag, int N, int H, int W, int Cin, int Cout,
                  int vertical, int relu, hipStream_t stream) {
    ConvF32Dims dm;
    dm.N = N; dm.H = H; dm.W = W; dm.Cin = Cin; dm.Cout = Cout; dm.relu = relu;
    dm.Ho = H;
    dm.Wo = W;
    dm.tiles_per_image = (H * W + kPix - 1) / kPix;
    const int rc = image_magnitudes(x, image_mag, N, (long)H * W * Cin, stream);
    if (rc != ALO_OK) return rc;
    const bool ksplit = Cout == 64;
    return vertical ? (ksplit ? launch_conv_f32<Staging<Plan5<true>::kSlots>, conv_taps_f32_kernel<true, true>, true>(x, w_split, bias, y, image_mag, dm, stream)
                              : launch_conv_f32<Staging<Plan5<true>::kSlots>, conv_taps_f32_kernel<true, false>, false>(x, w_split, bias, y, image_mag, dm, stream))
                    : (ksplit ? launch_conv_f32<Staging<Plan5<false>::kSlots>, conv_taps_f32_kernel<false, true>, true>(x, w_split, bias, y, image_mag, dm, stream)
                              : launch_conv_f32<Staging<Plan5<false>::kSlots>, conv_taps_f32_kernel<false, false>, false>(x, w_split, bias, y, image_mag, dm, stream));
}

}  // namespace alo
