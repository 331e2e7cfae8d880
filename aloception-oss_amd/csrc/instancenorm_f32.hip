// InstanceNorm (+ ReLU) over channels-last fp32 rows (B, HW, C): the ALO_F32 flavour of alo_groupnorm_rows_act (groups == C, no affine)
// — nn.InstanceNorm2d of RAFT's feature encoder (alonet/raft/extractor.py) between channels-last convolutions, where ATen's batch-norm
// kernels want NCHW.
//
// Three launches, deterministic, no atomics:
//   statistics  one workgroup per 256-row chunk of one image; a thread owns 4 channels of every (256 / (C / 4))-th row.  It takes its
//               rows 16 at a time: a channel's mean is its first value + the mean distance to it, and the squared distances to THAT
//               mean are summed (two passes over registers, nothing subtracted from a sum of squares); batches, then the threads of
//               a channel, are combined with Chan's formula.  workspace[b][chunk][c] = (n, mean, M2).
//   merge       one workgroup per 4 channels of one image: 64 stripes of chunk triples, then the 64 stripes.  The finished
//               (mean, 1 / sqrt(M2 / n + eps)) overwrite the first two words of workspace[b][0][c], which no other workgroup reads.
//   normalise   the chunk grid again: y = (x - mean) * rstd, read from those words; the chunk list is not looked at.
// The workspace is alo_groupnorm_rows_workspace_bytes(B, HW, C): ceil(HW / 256) * C triples per image.
#include "common.hpp"

// every product and sum below rounds on its own: tests/instancenorm_f32_ref.py restates this file operation by operation
#pragma clang fp contract(off)

namespace alo {
namespace {

constexpr int kInThreads = 256;
constexpr int kInRows = 256;     // rows per workgroup, statistics and normalise pass (the chunk of the workspace's answer)
constexpr int kInBatch = 16;     // rows a thread holds in registers at a time
constexpr int kInStripes = 64;   // merge pass: kInThreads / 4 channels

// Chan et al.: merge (nb, mb, m2b) into (n, mean, m2); an empty side leaves the other untouched, bit for bit
__device__ __forceinline__ void chan_merge(float& n, float& mean, float& m2, float nb, float mb, float m2b) {
    if (nb == 0.f) return;
    if (n == 0.f) { n = nb; mean = mb; m2 = m2b; return; }
    const float nn = n + nb, d = mb - mean;
    mean += d * (nb / nn);
    m2 += m2b + d * d * (n * nb / nn);
    n = nn;
}

struct InDims {
    int HW, C, nchunks;
    long y_batch_stride;   // elements between the images of the output
    float eps;
    int relu;
};

__global__ void __launch_bounds__(kInThreads)
instancenorm_f32_stats_kernel(const float* __restrict__ X, float* __restrict__ ws, const InDims dm) {
    __shared__ float part[kInThreads][4][3];
    const int tid = threadIdx.x, tpr = dm.C / 4, rpp = kInThreads / tpr;   // threads per row, rows per pass
    const int cg = tid % tpr, r0 = tid / tpr;
    const int b = blockIdx.y, row_begin = blockIdx.x * kInRows;
    const int row_end = row_begin + kInRows < dm.HW ? row_begin + kInRows : dm.HW;
    const float* xb = X + ((size_t)b * dm.HW) * dm.C + cg * 4;
    float n = 0.f, mean[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f};
    for (int base = row_begin + r0; base < row_end; base += kInBatch * rpp) {
        f32x4 v[kInBatch];
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < kInBatch; ++j) {
            const int r = base + j * rpp;
            const bool valid = r < row_end;
            v[j] = valid ? *reinterpret_cast<const f32x4*>(xb + (size_t)r * dm.C) : f32x4{0.f, 0.f, 0.f, 0.f};
            cnt += valid ? 1 : 0;
        }
        const float nb = (float)cnt;
        f32x4 s = {0.f, 0.f, 0.f, 0.f};   // the batch's sum of distances to its first row: rounds at the spread's size, not the mean's
#pragma unroll
        for (int j = 1; j < kInBatch; ++j)
            if (j < cnt) s += v[j] - v[0];
        const f32x4 mb = v[0] + s / nb;
        f32x4 q = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < kInBatch; ++j) {
            const f32x4 d = v[j] - mb;
            if (j < cnt) q += d * d;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float ni = n;
            chan_merge(ni, mean[i], m2[i], nb, mb[i], q[i]);
        }
        n += nb;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { part[tid][i][0] = n; part[tid][i][1] = mean[i]; part[tid][i][2] = m2[i]; }
    __syncthreads();
    if (tid < dm.C) {   // channel tid = word tid % 4 of slice tid / 4, over every row slot
        const int slice = tid / 4, sub = tid % 4;
        float gn = 0.f, gm = 0.f, g2 = 0.f;
        for (int rr = 0; rr < rpp; ++rr) {
            const int t = rr * tpr + slice;
            chan_merge(gn, gm, g2, part[t][sub][0], part[t][sub][1], part[t][sub][2]);
        }
        float* o = ws + (((size_t)b * dm.nchunks + blockIdx.x) * dm.C + tid) * 3;
        o[0] = gn; o[1] = gm; o[2] = g2;
    }
}

// grid (C / 4, B): thread = (stripe, channel % 4)
__global__ void __launch_bounds__(kInThreads)
instancenorm_f32_merge_kernel(float* ws, const InDims dm) {
    __shared__ float part[kInThreads][3];
    const int tid = threadIdx.x, sub = tid % 4, stripe = tid / 4, b = blockIdx.y, c = blockIdx.x * 4 + sub;
    float* image = ws + (size_t)b * dm.nchunks * dm.C * 3;
    float gn = 0.f, gm = 0.f, g2 = 0.f;
    for (int k = stripe; k < dm.nchunks; k += kInStripes) {
        const float* p = image + ((size_t)k * dm.C + c) * 3;
        chan_merge(gn, gm, g2, p[0], p[1], p[2]);
    }
    part[tid][0] = gn; part[tid][1] = gm; part[tid][2] = g2;
    __syncthreads();   // every read of the image's triples of these 4 channels is done: chunk 0's are overwritten below
    if (tid < 4) {
        gn = 0.f; gm = 0.f; g2 = 0.f;
        for (int st = 0; st < kInStripes; ++st) {
            const int t = st * 4 + tid;
            chan_merge(gn, gm, g2, part[t][0], part[t][1], part[t][2]);
        }
        float* o = image + (size_t)c * 3;
        o[0] = gm;
        o[1] = 1.f / sqrtf(g2 / gn + dm.eps);   // biased variance; correctly rounded division and root
    }
}

// X may be Y (in place): an element is read and written by the same thread
__global__ void __launch_bounds__(kInThreads)
instancenorm_f32_apply_kernel(const float* X, const float* __restrict__ ws, float* Y, const InDims dm) {
    const int tid = threadIdx.x, tpr = dm.C / 4, rpp = kInThreads / tpr, cg = tid % tpr, r0 = tid / tpr;
    const int b = blockIdx.y, row_begin = blockIdx.x * kInRows;
    const int row_end = row_begin + kInRows < dm.HW ? row_begin + kInRows : dm.HW;
    const float* st = ws + ((size_t)b * dm.nchunks * dm.C + cg * 4) * 3;
    const f32x4 mean = {st[0], st[3], st[6], st[9]}, rstd = {st[1], st[4], st[7], st[10]};
    const bool relu = dm.relu != 0;
    const float* xb = X + ((size_t)b * dm.HW) * dm.C + cg * 4;
    float* yb = Y + (size_t)b * dm.y_batch_stride + cg * 4;
#pragma unroll 4
    for (int r = row_begin + r0; r < row_end; r += rpp) {
        f32x4 v = (*reinterpret_cast<const f32x4*>(xb + (size_t)r * dm.C) - mean) * rstd;
        if (relu) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = v[i] < 0.f ? 0.f : v[i];   // NaN kept, as torch's relu keeps it
        }
        *reinterpret_cast<f32x4*>(yb + (size_t)r * dm.C) = v;
    }
}

}  // namespace

int instancenorm_f32(const void* x, void* y, void* workspace, int B, int HW, int C, float eps, long y_batch_stride, int relu,
                     hipStream_t stream, const char* what) {
    InDims dm;
    dm.HW = HW; dm.C = C; dm.nchunks = (HW + kInRows - 1) / kInRows;
    dm.y_batch_stride = y_batch_stride; dm.eps = eps; dm.relu = relu ? 1 : 0;
    const dim3 grid(dm.nchunks, B);
    void* stats_args[] = {&x, &workspace, &dm};
    if (int rc = launch<instancenorm_f32_stats_kernel>(grid, kInThreads, 0, stream, what, stats_args)) return rc;
    void* merge_args[] = {&workspace, &dm};
    if (int rc = launch<instancenorm_f32_merge_kernel>(dim3(C / 4, B), kInThreads, 0, stream, what, merge_args)) return rc;
    void* apply_args[] = {&x, &workspace, &y, &dm};
    return launch<instancenorm_f32_apply_kernel>(grid, kInThreads, 0, stream, what, apply_args);
}

}  // namespace alo
