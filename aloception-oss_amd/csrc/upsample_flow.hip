// RAFT's flow up-sampling (alonet/raft/raft.py RAFTBase.upsample_flow, utils.upflow8): the fp32 flavour of alo_upsample_add_nhwc.
// Planar (NCHW) fp32 in and out, x8 in both directions; the convex mode has a backward (ALO_UPSAMPLE_GRAD, below).
//
// Convex (mask given): every fine pixel is a softmax-weighted mix of the 3x3 coarse neighbourhood of its cell,
//   out[n, c, 8y+i, 8x+j] = sum_k softmax_k(mask[n, k*64 + i*8 + j, y, x]) * 8 * flow[n, c, y + k/3 - 1, x + k%3 - 1]
// where a neighbour outside the image has value 0 and KEEPS its weight (F.unfold pads with zeros; nothing is renormalised).  The
// stock chain (softmax, unfold, multiply, sum, permute + reshape) passes over the (N, 576, h, w) mask several times; here it is read
// once and nothing of its size is written.
//   * lanes run over the flattened coarse pixel p = y * w + x, so every mask plane is read as contiguous 256-byte wave segments for
//     any w, row ends included;
//   * a thread owns one (n, p, sub-row i): 72 independent 4-byte mask loads (9 taps x 8 columns j) through a buffer resource over
//     the image's 576 planes, the plane offset in a scalar register; its 9 x C flow neighbours come from cache, the out-of-image
//     ones as the zero a buffer load returns for an offset past the resource;
//   * 8 softmaxes over k (max-subtracted, fp32), then per channel 8 outputs as two 16-byte stores: adjacent lanes write adjacent
//     32 bytes of one output row;
//   * sub-row i is the fastest block coordinate: block b runs on XCD b % 8, so each XCD streams the 72 planes of one i.
// Non-finite values behave as the arithmetic says, which is what the stock chain gives: a +inf logit or nine -inf logits make their
// own fine pixel NaN, a -inf logit is weight 0, a NaN flow value reaches the fine pixels of the cells it neighbours.  exp is the
// hardware's 2^x of (l - max) * log2(e): a weight below 2^-126 is 0.
//
// Bilinear (no mask): 8 * F.interpolate(flow, (8h, 8w), mode="bilinear", align_corners=True) in ATen's arithmetic
// (UpSampleBilinear2d.cu: source = dst * (in - 1) / (out - 1), the scale a float quotient; lambda = source - floor).
#include "common.hpp"

namespace alo {
namespace {

constexpr int kUpThreads = 128;   // two waves: the (1, 2, 55, 128) map still gives 440 workgroups

struct UpFlowDims {
    int C, h, w, hw, chunks;   // chunks = ceil(hw / kUpThreads)
};

// the 9 neighbours of coarse pixel (y, x) in channels c0 .. c0 + NC - 1, times 8; a channel past C reads as 0 and is never stored
template <int NC>
__device__ __forceinline__ void load_neighbours(__amdgpu_buffer_rsrc_t flow_r, const UpFlowDims& dm, int c0, int y, int x, float (&v)[NC][9]) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
            // one select, no short-circuit: with && the compiler branches around each load and they stop overlapping
            const bool in = ((unsigned)yy < (unsigned)dm.h) & ((unsigned)xx < (unsigned)dm.w) & (c0 + c < dm.C);
            const unsigned off = in ? (unsigned)((c0 + c) * dm.hw + yy * dm.w + xx) * 4u : kOutOfRange;
            v[c][k] = 8.f * __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(flow_r, off, 0, 0));
        }
}

template <int NC>
__global__ void __launch_bounds__(kUpThreads)
upsample_flow_convex_kernel(const float* __restrict__ flow, const float* __restrict__ mask, float* __restrict__ out, const UpFlowDims dm) {
    const unsigned b = blockIdx.x;
    const int i = b & 7;
    const int chunk = (b >> 3) % dm.chunks;
    const long n = (b >> 3) / dm.chunks;
    const int p = chunk * kUpThreads + threadIdx.x;
    if (p >= dm.hw) return;
    const int y = p / dm.w, x = p - y * dm.w;

    // one image's planes per resource: 576 * hw * 4 bytes < 4 GiB is the launcher's check
    const __amdgpu_buffer_rsrc_t mask_r = make_rsrc(mask + n * 576 * dm.hw, 576u * (unsigned)dm.hw * 4u);
    const __amdgpu_buffer_rsrc_t flow_r = make_rsrc(flow + n * dm.C * dm.hw, (unsigned)(dm.C * dm.hw) * 4u);

    float v[NC][9];
    load_neighbours<NC>(flow_r, dm, 0, y, x, v);

    float e[9][8];   // logits, then exp(logit - max)
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j)
            e[k][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(mask_r, (unsigned)p * 4u, (int)((unsigned)(k * 64 + i * 8 + j) * (unsigned)dm.hw * 4u), 0));

    float rs[8];     // 1 / sum_k e[k][j]: the sum lies in [1, 9]
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float m = e[0][j];
#pragma unroll
        for (int k = 1; k < 9; ++k) m = fmaxf(m, e[k][j]);
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            e[k][j] = __expf(e[k][j] - m);
            s += e[k][j];
        }
        rs[j] = __builtin_amdgcn_rcpf(s);
    }

    const int W = 8 * dm.w;
    float* const orow = out + ((n * dm.C * 8 * dm.h + 8 * y + i) * (long)W + 8 * x);
    const long cstride = 64L * dm.hw;
    for (int c0 = 0;;) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float acc = e[0][j] * v[c][0];
#pragma unroll
                for (int k = 1; k < 9; ++k) acc = fmaf(e[k][j], v[c][k], acc);
                o[j] = acc * rs[j];
            }
            if (c0 + c < dm.C) {
                float* const po = orow + (c0 + c) * cstride;
                *reinterpret_cast<f32x4*>(po) = f32x4{o[0], o[1], o[2], o[3]};
                *reinterpret_cast<f32x4*>(po + 4) = f32x4{o[4], o[5], o[6], o[7]};
            }
        }
        c0 += NC;
        if (c0 >= dm.C) break;
        load_neighbours<NC>(flow_r, dm, c0, y, x, v);
    }
}

struct UpBilinearDims {
    int h, w;
    long total;      // BQ * C * 8h * 2w: a thread writes four consecutive fine pixels of one row
    float ry, rx;    // (in - 1) / (out - 1), the float quotient ATen forms
};

__global__ void __launch_bounds__(256)
upsample_flow_bilinear_kernel(const float* __restrict__ flow, float* __restrict__ out, const UpBilinearDims dm) {
    const long idx = blockIdx.x * 256L + threadIdx.x;
    if (idx >= dm.total) return;
    const int W4 = 2 * dm.w, H = 8 * dm.h;
    const int X0 = (int)(idx % W4) * 4;
    const long row = idx / W4;
    const int Y = (int)(row % H);
    const float* const src = flow + (row / H) * dm.h * dm.w;
    const float ysrc = dm.ry * (float)Y;
    const int y0 = min((int)ysrc, dm.h - 1), y1 = y0 + (y0 < dm.h - 1 ? 1 : 0);
    const float ly1 = ysrc - (float)y0, ly0 = 1.f - ly1;
    float o[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float xsrc = dm.rx * (float)(X0 + t);
        const int x0 = min((int)xsrc, dm.w - 1), x1 = x0 + (x0 < dm.w - 1 ? 1 : 0);
        const float lx1 = xsrc - (float)x0, lx0 = 1.f - lx1;
        o[t] = 8.f * (ly0 * (lx0 * src[y0 * dm.w + x0] + lx1 * src[y0 * dm.w + x1])
                      + ly1 * (lx0 * src[y1 * dm.w + x0] + lx1 * src[y1 * dm.w + x1]));
    }
    *reinterpret_cast<f32x4*>(out + idx * 4) = f32x4{o[0], o[1], o[2], o[3]};
}

// ---- the backward of the convex mode (ALO_UPSAMPLE_GRAD) ----------------------------------------------------------------------------
// With w_k the forward's weights (the same max-subtracted softmax, the same exp and reciprocal) and G_c = grad_up[n, c, 8y+i, 8x+j]:
//   t_k                                = sum_c G_c * 8 * flow[n, c, y + k/3 - 1, x + k%3 - 1]
//   grad_mask[n, k*64 + i*8 + j, y, x] = w_k * (t_k - sum_k' w_k' t_k')
//   taps[n, c*9 + k, y, x]             = 8 * sum_{i, j} w_k * G_c        (the columns of F.unfold's adjoint: the caller folds them)
// The forward's access pattern: lanes run over the flattened coarse pixel, a thread owns one (n, p, sub-row i), 72 mask loads and 72
// grad_mask stores through buffer resources with the plane offset in a scalar register, grad_up as two 16-byte loads per channel,
// out-of-image neighbours as the zero of a buffer load past its resource.
//   * All channels of a thread's grad_up sub-row and flow neighbours stay in registers (NC = 1, 2, 4 or 8 >= C, the rest zeros), so
//     t_k is formed column by column and never stored.
//   * The sum over i of `taps` is what the forward has no counterpart for.  A workgroup is the eight sub-rows of PX pixels; the
//     partial sums of a pixel meet in LDS, two channels at a time, and are added in the order i = 0..7: no atomics, the same bits on
//     every run.  A thread that owned all eight sub-rows would need no LDS, but a training crop (6 x 46 x 62 = 17k coarse pixels)
//     would then be 270 waves on 256 CUs; this way it is 2160.  Measured (docs/experiments.md): that variant is 14 % faster on
//     4 x 90 x 160 maps and 25 % slower on the crop.
//   * PX = 64 (512 threads, wave i is sub-row i) for C <= 4; PX = 32 (256 threads) for C > 4, where a wave then has the whole
//     register file and nothing goes to scratch.
//   * A lane past the map's end works on the last pixel's values and stores nothing.

// grad_up[n, c, 8y+i, 8x .. 8x+7] for c < NC; a channel past C reads the last one's row (in bounds) and counts as 0
template <int NC>
__device__ __forceinline__ void load_grad_rows(const float* __restrict__ grow, const UpFlowDims& dm, float (&g)[NC][8]) {
    const long cstride = 64L * dm.hw;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const bool in = c < dm.C;
        const float* const pg = grow + (in ? c : dm.C - 1) * cstride;
        const f32x4 a = *reinterpret_cast<const f32x4*>(pg), b = *reinterpret_cast<const f32x4*>(pg + 4);
        const float r[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) g[c][j] = in ? r[j] : 0.f;
    }
}

template <int NC, int PX>
__global__ void __launch_bounds__(8 * PX)
upsample_flow_grad_kernel(const float* __restrict__ flow, const float* __restrict__ grad_up, const float* __restrict__ mask,
                          float* __restrict__ grad_mask, float* __restrict__ taps, const UpFlowDims dm) {
    constexpr int PC = NC < 2 ? NC : 2;   // channels per pass through LDS
    __shared__ float part[8][9 * PC][PX];
    const unsigned b = blockIdx.x;
    const int chunk = b % dm.chunks;
    const long n = b / dm.chunks;
    const int i = threadIdx.x / PX, lane = threadIdx.x % PX;
    const bool active = chunk * PX + lane < dm.hw;
    const int p = active ? chunk * PX + lane : dm.hw - 1;
    const int y = p / dm.w, x = p - y * dm.w;

    const __amdgpu_buffer_rsrc_t mask_r = make_rsrc(mask + n * 576 * dm.hw, 576u * (unsigned)dm.hw * 4u);
    const __amdgpu_buffer_rsrc_t gmask_r = make_rsrc(grad_mask + n * 576 * dm.hw, 576u * (unsigned)dm.hw * 4u);
    const __amdgpu_buffer_rsrc_t flow_r = make_rsrc(flow + n * dm.C * dm.hw, (unsigned)(dm.C * dm.hw) * 4u);
    const float* const grow = grad_up + ((n * dm.C * 8 * dm.h + 8 * y + i) * (8L * dm.w) + 8 * x);

    float e[9][8];   // logits, then the weights
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j)
            e[k][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(mask_r, (unsigned)p * 4u, (int)((unsigned)(k * 64 + i * 8 + j) * (unsigned)dm.hw * 4u), 0));
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float m = e[0][j];
#pragma unroll
        for (int k = 1; k < 9; ++k) m = fmaxf(m, e[k][j]);
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            e[k][j] = __expf(e[k][j] - m);
            s += e[k][j];
        }
        const float rs = __builtin_amdgcn_rcpf(s);
#pragma unroll
        for (int k = 0; k < 9; ++k) e[k][j] *= rs;
    }

    float v[NC][9], g[NC][8];
    load_neighbours<NC>(flow_r, dm, 0, y, x, v);
    load_grad_rows<NC>(grow, dm, g);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float t[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            t[k] = g[0][j] * v[0][k];
#pragma unroll
            for (int c = 1; c < NC; ++c) t[k] = fmaf(g[c][j], v[c][k], t[k]);
        }
        float s = e[0][j] * t[0];
#pragma unroll
        for (int k = 1; k < 9; ++k) s = fmaf(e[k][j], t[k], s);
        if (active) {
#pragma unroll
            for (int k = 0; k < 9; ++k)
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(e[k][j] * (t[k] - s)), gmask_r, (unsigned)p * 4u,
                                                      (int)((unsigned)(k * 64 + i * 8 + j) * (unsigned)dm.hw * 4u), 0);
        }
    }

    float* const timg = taps + n * 9 * dm.C * dm.hw;
#pragma unroll
    for (int c0 = 0; c0 < NC; c0 += PC) {
        if (c0 >= dm.C) break;   // uniform
#pragma unroll
        for (int c = 0; c < PC; ++c)
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                float acc = e[k][0] * g[c0 + c][0];
#pragma unroll
                for (int j = 1; j < 8; ++j) acc = fmaf(e[k][j], g[c0 + c][j], acc);
                part[i][c * 9 + k][lane] = 8.f * acc;
            }
        __syncthreads();
        for (int idx = threadIdx.x; idx < 9 * PC * PX; idx += 8 * PX) {
            const int ck = idx / PX, l = idx % PX;
            float s = part[0][ck][l];
#pragma unroll
            for (int r = 1; r < 8; ++r) s += part[r][ck][l];
            if (c0 * 9 + ck < 9 * dm.C && chunk * PX + l < dm.hw) timg[(long)(c0 * 9 + ck) * dm.hw + chunk * PX + l] = s;
        }
        __syncthreads();
    }
}

}  // namespace

int upsample_flow_f32(const void* flow, const void* mask, void* out, int BQ, int C, int h, int w, hipStream_t stream, const char* what) {
    const long hw = (long)h * w;
    void* args[4];
    if (mask == nullptr) {
        UpBilinearDims dm;
        dm.h = h; dm.w = w;
        dm.total = (long)BQ * C * hw * 16;
        dm.ry = (float)(h - 1) / (float)(8 * h - 1); dm.rx = (float)(w - 1) / (float)(8 * w - 1);
        const long blocks = (dm.total + 255) / 256;
        ALO_REQUIRE(hw < (1L << 24) && blocks < (1L << 31), ALO_ERR_UNSUPPORTED, "%s: map too large (BQ=%d C=%d h=%d w=%d)", what, BQ, C, h, w);
        args[0] = &flow; args[1] = &out; args[2] = &dm;
        return launch<upsample_flow_bilinear_kernel>((unsigned)blocks, 256, 0, stream, what, args);
    }
    // 576 planes of one image behind one buffer resource, byte offsets in 32 bits
    ALO_REQUIRE(hw * 576 * 4 < (1L << 32), ALO_ERR_UNSUPPORTED, "%s: the mask of one image must stay below 4 GiB (h=%d w=%d)", what, h, w);
    UpFlowDims dm;
    dm.C = C; dm.h = h; dm.w = w; dm.hw = (int)hw; dm.chunks = (int)((hw + kUpThreads - 1) / kUpThreads);
    const long blocks = 8L * dm.chunks * BQ;
    ALO_REQUIRE(blocks < (1L << 31), ALO_ERR_UNSUPPORTED, "%s: map too large (BQ=%d C=%d h=%d w=%d)", what, BQ, C, h, w);
    args[0] = &flow; args[1] = &mask; args[2] = &out; args[3] = &dm;
    return C % 2 == 0 ? launch<upsample_flow_convex_kernel<2>>((unsigned)blocks, kUpThreads, 0, stream, what, args)
                      : launch<upsample_flow_convex_kernel<1>>((unsigned)blocks, kUpThreads, 0, stream, what, args);
}

int upsample_flow_grad_f32(const void* flow_and_grad, const void* mask, void* out, int BQ, int C, int h, int w, hipStream_t stream, const char* what) {
    const long hw = (long)h * w;
    ALO_REQUIRE(hw * 576 * 4 < (1L << 32), ALO_ERR_UNSUPPORTED, "%s: the mask of one image must stay below 4 GiB (h=%d w=%d)", what, h, w);
    UpFlowDims dm;
    dm.C = C; dm.h = h; dm.w = w; dm.hw = (int)hw; const int px = C <= 4 ? 64 : 32;   // coarse pixels per workgroup
    dm.chunks = (int)((hw + px - 1) / px);
    const long blocks = (long)dm.chunks * BQ;
    ALO_REQUIRE(blocks < (1L << 31), ALO_ERR_UNSUPPORTED, "%s: map too large (BQ=%d C=%d h=%d w=%d)", what, BQ, C, h, w);
    // x_low: flow, then grad_up from the next multiple of 4 elements; out: grad_mask, then taps
    const float* flow = static_cast<const float*>(flow_and_grad);
    const float* grad_up = flow + ((long)BQ * C * hw + 3) / 4 * 4;
    float* grad_mask = static_cast<float*>(out);
    float* taps = grad_mask + (long)BQ * 576 * hw;
    void* args[6] = {&flow, &grad_up, &mask, &grad_mask, &taps, &dm};
    const unsigned grid = (unsigned)blocks;
    return C == 1 ? launch<upsample_flow_grad_kernel<1, 64>>(grid, 512, 0, stream, what, args)
         : C == 2 ? launch<upsample_flow_grad_kernel<2, 64>>(grid, 512, 0, stream, what, args)
         : C <= 4 ? launch<upsample_flow_grad_kernel<4, 64>>(grid, 512, 0, stream, what, args)
                  : launch<upsample_flow_grad_kernel<8, 32>>(grid, 256, 0, stream, what, args);
}

}  // namespace alo
