// RAFT's flow up-sampling (alonet/raft/raft.py RAFTBase.upsample_flow, utils.upflow8): the fp32 flavour of alo_upsample_add_nhwc.
// Planar (NCHW) fp32 in and out, x8 in both directions, forward only.
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

}  // namespace alo
