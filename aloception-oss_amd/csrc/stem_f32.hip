// The fp32 flavour of alo_stem_conv_pool (stem.hip's header: 7x7 / stride 2 / padding 3 convolution of a 3-channel image, bias, ReLU and
// the 3x3 / stride 2 / padding 1 max-pool in one launch) on the fp16 matrix cores at fp32-class accuracy: the two-term split arithmetic
// of split_f16.hpp (scale, split, non-finite rule, term order, undo) in the tile of stem_conv_pool_kernel — 17 x 15 convolution outputs
// behind 8 x 7 pooled pixels, K = 7 tap rows x 24, persistent workgroups.
//
//   * scale: one power of two per staged WINDOW (the 39 rows x 35 pixels x 3 channels a tile reads, zero outside the image), from the
//     window's largest finite magnitude, found while the window sits in the staging registers: no pre-pass, and a tile's result depends
//     on its own window only.  A dim region next to a bright one keeps its own accuracy as soon as the tile does not see both.
//   * the window is split where it is parked in LDS, as two planes (high terms, low terms) in stem_conv_pool_kernel's row layout, so an
//     A fragment is again 16 contiguous bytes of a plane.  A non-finite pixel is parked as hi = 0, lo = the pixel.
//   * weights: split by the caller as the (64, 176) matrix of stem.hip, one power of two per output channel (alo_hotpath.h).  Both terms
//     are 2 x 22 u32x4 per lane, which do not fit next to 64 accumulators: they live in LDS (45 KB, loaded once per workgroup), in
//     fragment order, and every fragment a wave reads feeds BOTH of its pixel tiles (6 MFMAs).
//   * epilogue: the undo by k_window + k_channel (ldexp, exact), + bias, ReLU (NaN kept) -> fp32 convolution outputs in LDS (69 KB); the
//     pool is a fp32 max that lets a NaN through, as torch's.
// LDS: 45056 weights + 2 x 8960 window planes + 69360 convolution outputs + 528 tables = 132864 bytes: one workgroup of four waves per CU.
#include "mfma_tile.hpp"
#include "split_f16.hpp"

namespace alo {
namespace {

constexpr int kPoolRows = 8, kPoolCols = 7;                          // pooled pixels per tile
constexpr int kConvRows = 2 * kPoolRows + 1, kConvCols = 2 * kPoolCols + 1;   // 17 x 15 convolution outputs
constexpr int kConvPix = kConvRows * kConvCols;                      // 255
constexpr int kWinRows = 2 * kConvRows + 5;                          // 39 input rows
constexpr int kInCols = 2 * kConvCols + 5;                           // 35 input pixels per row
constexpr int kInElems = kInCols * 3;                                // 105 staged elements per row
constexpr int kInStride = 224;                                       // LDS bytes per row of a plane (112 fp16 elements)
constexpr int kPlaneRows = kWinRows + 1;                             // + the row k-group 21 reads (and then replaces by zeros)
constexpr int kPlane = kPlaneRows * kInStride;                       // 8960
constexpr int kConvStride = 64 * 4 + 16;                             // LDS bytes per convolution output pixel
constexpr int kKsteps = 11;                                          // 21 k-groups of 8 (+1 of zeros)
constexpr int kThreads = 256;
constexpr int kTermBytes = 64 * 176 * 2;                             // one packed weight term
constexpr int kWOff = 0, kInOff = 2 * kTermBytes, kConvOff = kInOff + 2 * kPlane, kTabOff = kConvOff + kConvPix * kConvStride;
constexpr int kLds = kTabOff + 64 * 4 + 64 * 4 + 4 * 4;              // bias, channel exponents, the waves' magnitudes
static_assert(kConvPix <= 8 * 32, "8 MFMA row tiles");
static_assert(kInOff % 16 == 0 && kConvOff % 16 == 0 && kTabOff % 16 == 0, "16-byte LDS accesses");

struct StemF32Dims {
    int N, H, W, Hc, Wc, Hp, Wp;
    long sN, sC, sH, sW;   // element strides of the (N, 3, H, W) input
    int tiles_y, tiles_x;
};

// torch's max-pool update: a NaN is taken and then stays
__device__ __forceinline__ float max_keep_nan(float m, float v) { return (v > m || v != v) ? v : m; }

__global__ void __launch_bounds__(kThreads, 1)
stem_conv_pool_f32_kernel(const float* __restrict__ X, const unsigned char* __restrict__ Wsplit, const float* __restrict__ bias,
                          float* __restrict__ Y, const StemF32Dims dm) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const w_lds = smem + kWOff;
    unsigned char* const in_lds = smem + kInOff;          // the plane of high terms; the low terms are kPlane behind
    unsigned char* const conv_lds = smem + kConvOff;
    float* const bias_s = reinterpret_cast<float*>(smem + kTabOff);
    int* const kc_s = reinterpret_cast<int*>(smem + kTabOff + 256);
    unsigned* const mag_s = reinterpret_cast<unsigned*>(smem + kTabOff + 512);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nl = lane & 31, kg = lane >> 5;

    // both packed weight terms, [term][2 column tiles][11 k-steps][64 lanes][8 fp16], as they lie in memory
    for (int i = tid; i < 2 * kTermBytes / 16; i += kThreads)
        *reinterpret_cast<u32x4*>(w_lds + i * 16) = *reinterpret_cast<const u32x4*>(Wsplit + (size_t)i * 16);
    if (tid < 64) {
        bias_s[tid] = bias ? bias[tid] : 0.f;
        kc_s[tid] = reinterpret_cast<const int*>(Wsplit + 2 * kTermBytes)[tid];
    }
    // elements 105..111 of every plane row and the whole last row are read (against zero weights, and masked) but never staged
    for (int i = tid; i < 2 * kPlaneRows * (kInStride / 2); i += kThreads) {
        const int row = (i / (kInStride / 2)) % kPlaneRows, e = i % (kInStride / 2);
        if (e >= kInElems || row == kWinRows) *reinterpret_cast<uint16_t*>(in_lds + i * 2) = 0;
    }

    const int tiles_per_image = dm.tiles_y * dm.tiles_x;
    const int ntiles = tiles_per_image * dm.N;

    // 39 rows x 35 pixels x 3 channels of the image per tile, requested one tile AHEAD (register staged), interleaved [row][x * 3 + c],
    // zero outside the image (the convolution's padding)
    constexpr int kStageIters = (kWinRows * kInElems + kThreads - 1) / kThreads;   // 16
    float sv[kStageIters];
    auto load_tile = [&](int tl) {
        const int n = tl / tiles_per_image, trem = tl - n * tiles_per_image;
        const int ty = trem / dm.tiles_x, tx = trem - ty * dm.tiles_x;
        const int iy0 = 4 * ty * kPoolRows - 5, ix0 = 4 * tx * kPoolCols - 5;
        const float* xn = X + (size_t)n * dm.sN;
#pragma unroll
        for (int it = 0; it < kStageIters; ++it) {
            const int i = tid + it * kThreads;
            const int row = i / kInElems, e = i - row * kInElems, xc = e / 3, c = e - 3 * xc;
            const int iy = iy0 + row, ix = ix0 + xc;
            const bool ok = i < kWinRows * kInElems && iy >= 0 && iy < dm.H && ix >= 0 && ix < dm.W;
            sv[it] = ok ? xn[c * dm.sC + iy * dm.sH + ix * dm.sW] : 0.f;
        }
    };
    if ((int)blockIdx.x < ntiles) load_tile(blockIdx.x);

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int n = tile / tiles_per_image, trem = tile - n * tiles_per_image;
        const int ty = trem / dm.tiles_x, tx = trem - ty * dm.tiles_x;
        const int py0 = ty * kPoolRows, px0 = tx * kPoolCols;          // first pooled pixel
        const int cy0 = 2 * py0 - 1, cx0 = 2 * px0 - 1;                // first convolution output

        // ---- the window's exponent: largest finite magnitude of the staged values, over the four waves --------------------------------
        unsigned mg = 0u;
#pragma unroll
        for (int it = 0; it < kStageIters; ++it) mg = max(mg, finite_mag(__float_as_uint(sv[it])));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mg = max(mg, (unsigned)__shfl_xor((int)mg, o, 64));
        if (lane == 0) mag_s[wave] = mg;
        __syncthreads();
        const int kwin = split_exponent(max(max(mag_s[0], mag_s[1]), max(mag_s[2], mag_s[3])));
        const float down = ldexpf(1.0f, -kwin);

        // ---- park the window: a high and a low term per element -----------------------------------------------------------------------
#pragma unroll
        for (int it = 0; it < kStageIters; ++it) {
            const int i = tid + it * kThreads;
            const int row = i / kInElems, e = i - row * kInElems;
            _Float16 hi, lo;
            split2(sv[it], down, hi, lo);
            if (i < kWinRows * kInElems) {
                *reinterpret_cast<_Float16*>(in_lds + row * kInStride + e * 2) = hi;
                *reinterpret_cast<_Float16*>(in_lds + kPlane + row * kInStride + e * 2) = lo;
            }
        }
        __syncthreads();
        if (tile + (int)gridDim.x < ntiles) load_tile(tile + gridDim.x);

        // ---- implicit GEMM, channels x pixels: wave w owns pixel tiles w and w + 4 (32 convolution outputs each) x both channel tiles.
        // The WEIGHTS are the MFMA's row operand, so a lane ends up holding 2 x 16 channels of ONE pixel per pixel tile --------------------
        int m_raw[2], m[2], lr[2], lc[2];
        const unsigned char* a_base[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            m_raw[a] = (wave + 4 * a) * 32 + nl;
            m[a] = m_raw[a] < kConvPix ? m_raw[a] : kConvPix - 1;
            lr[a] = m[a] / kConvCols;
            lc[a] = m[a] - lr[a] * kConvCols;
            a_base[a] = in_lds + (2 * lr[a]) * kInStride + lc[a] * 12;
        }
        f32x16 acc[2][2];   // [pixel tile][channel tile]
        zero_acc(acc);
#pragma unroll
        for (int s = 0; s < kKsteps; ++s) {
            // k-group G = 2 s + kg is tap row G / 3, elements 8 (G % 3) .. + 7 of its 24
            const int g0 = 2 * s, g1 = 2 * s + 1;
            const int off = kg ? (g1 / 3) * kInStride + (g1 % 3) * 16 : (g0 / 3) * kInStride + (g0 % 3) * 16;
            const int G = kg ? g1 : g0;
            WFrag w;
            XFrag x;
#pragma unroll
            for (int term = 0; term < 2; ++term) {
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
                    w.v[term][ct] = *reinterpret_cast<const u32x4*>(w_lds + term * kTermBytes + ((ct * kKsteps + s) * 64 + lane) * 16);
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const unsigned* ap = reinterpret_cast<const unsigned*>(a_base[a] + term * kPlane + off);
                    u32x4 v = {ap[0], ap[1], ap[2], ap[3]};
                    // the zero-weight columns must contribute 0, not 0 x Inf / 0 x NaN (stem_conv_pool_kernel): elements 21..23 of a tap
                    // row hold the real pixel 2 lc + 7, and k-group 21 reads input row 2 lr + 7
                    if (G == 21) v = u32x4{0u, 0u, 0u, 0u};
                    else if (G % 3 == 2) { v.z &= 0x0000ffffu; v.w = 0u; }
                    x.v[term][a] = v;
                }
            }
            mma_split(acc, w, x);
        }

        // the undo, + bias, ReLU -> fp32 into the convolution buffer, 4 consecutive channels per write; pixels outside the convolution's
        // output are the pool's padding (0 is neutral for a max over ReLU outputs)
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int cy = cy0 + lr[a], cx = cx0 + lc[a];
            const bool ok = cy >= 0 && cy < dm.Hc && cx >= 0 && cx < dm.Wc;
            if (m_raw[a] < kConvPix) {
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int c = 32 * ct + 8 * q + 4 * kg;
                        f32x4 v = {0.f, 0.f, 0.f, 0.f};
                        if (ok) {
                            const f32x4 bb = *reinterpret_cast<const f32x4*>(bias_s + c);
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] = relu_keep_nan(ldexpf(acc[a][ct][4 * q + e], kwin + kc_s[c + e]) + bb[e]);
                        }
                        *reinterpret_cast<f32x4*>(conv_lds + m[a] * kConvStride + c * 4) = v;
                    }
            }
        }
        __syncthreads();

        // ---- 3x3 / stride 2 max-pool out of LDS: item = (pooled pixel, 4 channels) ------------------------------------------------------
        for (int i = tid; i < kPoolRows * kPoolCols * 16; i += kThreads) {
            const int pp = i >> 4, cq = i & 15;
            const int lpy = pp / kPoolCols, lpx = pp - lpy * kPoolCols;
            f32x4 best = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(conv_lds + ((2 * lpy + dy) * kConvCols + 2 * lpx + dx) * kConvStride + cq * 16);
#pragma unroll
                    for (int e = 0; e < 4; ++e) best[e] = max_keep_nan(best[e], v[e]);
                }
            const int py = py0 + lpy, px = px0 + lpx;
            if (py < dm.Hp && px < dm.Wp)
                *reinterpret_cast<f32x4*>(Y + (((size_t)n * dm.Hp + py) * dm.Wp + px) * 64 + cq * 4) = best;
        }
        __syncthreads();  // the planes, the convolution buffer and the magnitudes are rewritten by the next tile
    }
}

}  // namespace

int stem_conv_pool_f32(const void* x, const void* w_split, const void* bias, void* y, int N, int H, int W, long stride_n, long stride_c,
                       long stride_h, long stride_w, hipStream_t stream) {
    StemF32Dims dm;
    dm.N = N; dm.H = H; dm.W = W;
    dm.Hc = (H - 1) / 2 + 1; dm.Wc = (W - 1) / 2 + 1;
    dm.Hp = (dm.Hc - 1) / 2 + 1; dm.Wp = (dm.Wc - 1) / 2 + 1;
    dm.sN = stride_n; dm.sC = stride_c; dm.sH = stride_h; dm.sW = stride_w;
    dm.tiles_y = (dm.Hp + kPoolRows - 1) / kPoolRows;
    dm.tiles_x = (dm.Wp + kPoolCols - 1) / kPoolCols;
    const long ntiles = (long)dm.tiles_y * dm.tiles_x * N;
    ALO_REQUIRE(ntiles < (1L << 30), ALO_ERR_UNSUPPORTED, "alo_stem_conv_pool: image batch too large");
    void* args[] = {&x, &w_split, &bias, &y, &dm};
    const unsigned grid = (unsigned)(ntiles < 256 ? ntiles : 256);   // 256 CUs x 1 resident workgroup
    return launch<stem_conv_pool_f32_kernel>(grid, kThreads, kLds, stream, "alo_stem_conv_pool", args);
}

}  // namespace alo
