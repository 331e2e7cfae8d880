// Two-stage Deformable-DETR: the three data-movement passes between the encoder and the decoder (include/alo_two_stage.h).
//
// Stock, gen_encoder_output_proposals (alonet/deformable_detr/deformable_transformer.py:145-177) is a host loop over the levels
// (meshgrid, cat, divide, cat per level), a window test, a log and two masked_fill pairs over (B, S, 4) and (B, S, C);
// the decoder-input branch (:259-262 + get_proposal_pos_embed :130-143) is gather, sigmoid, divide, sin, cos, stack, flatten.
// All of it streams: a token's proposal depends on its (level, y, x) and two counts per (image, level), a memory row on one
// byte of `keep`, a query on one gathered 16-byte row.  Three launches, or two with the first two folded (what the module uses), no temporaries.
#include "common.hpp"

#include "../../include/alo_two_stage.h"

namespace alo {
namespace {

constexpr int kMaxLevels = 8;
constexpr int kPropThreads = 256;
constexpr int kPropTokens = 512;   // tokens per block: the per-(image, level) counts are re-reduced once per block

struct PropDims {
    int B, L, S, chunks;           // chunks: blocks per image
    int h[kMaxLevels], w[kMaxLevels], start[kMaxLevels], chunk0[kMaxLevels];   // chunk0[l]: first block (within an image) of level l
};

// valid_W / valid_H of one (image, level): the un-padded tokens of the level's first row / first column (:152-153), counted by the
// whole block (256 threads) from m, the level's first mask byte.  Ends in a barrier; every thread gets both counts.
__device__ __forceinline__ void level_counts(const unsigned char* __restrict__ m, int hl, int wl, float& fw, float& fh) {
    __shared__ int counts[2][kPropThreads / 64];
    int vw = 0, vh = 0;
    for (int x = threadIdx.x; x < wl; x += kPropThreads) vw += m[x] ? 0 : 1;
    for (int y = threadIdx.x; y < hl; y += kPropThreads) vh += m[(size_t)y * wl] ? 0 : 1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { vw += __shfl_xor(vw, o, 64); vh += __shfl_xor(vh, o, 64); }
    if ((threadIdx.x & 63) == 0) { counts[0][threadIdx.x >> 6] = vw; counts[1][threadIdx.x >> 6] = vh; }
    __syncthreads();
    vw = vh = 0;
#pragma unroll
    for (int i = 0; i < kPropThreads / 64; ++i) { vw += counts[0][i]; vh += counts[1][i]; }
    fw = (float)vw;
    fh = (float)vh;
}

// Proposal of token p = (y, x) of level l -> its four logits (+inf when dropped); returns keep.
__device__ __forceinline__ bool token_proposal(int l, int p, int wl, float fw, float fh, bool padded, f32x4& o) {
    const float wh = ldexpf(0.05f, l);                       // 0.05 * 2^l, exact scaling of float32(0.05)
    const bool wh_ok = wh > 0.01f && wh < 0.99f;
    const float inf = __builtin_huge_valf();
    const int y = p / wl, x = p - y * wl;
    // (x + 0.5) / valid_W with IEEE division, as the float32 torch formulation; a zero count gives +inf, outside the window
    const float px = __fdiv_rn((float)x + 0.5f, fw), py = __fdiv_rn((float)y + 0.5f, fh);
    const bool ok = wh_ok && px > 0.01f && px < 0.99f && py > 0.01f && py < 0.99f && !padded;
    o = f32x4{inf, inf, inf, inf};
    if (ok) {
        const float wh_logit = logf(__fdiv_rn(wh, 1.f - wh));
        o = f32x4{logf(__fdiv_rn(px, 1.f - px)), logf(__fdiv_rn(py, 1.f - py)), wh_logit, wh_logit};
    }
    return ok;
}

__device__ __forceinline__ int level_of_chunk(const PropDims& dm, int c) {
    int l = 0;
#pragma unroll
    for (int i = 1; i < kMaxLevels; ++i)
        if (i < dm.L && c >= dm.chunk0[i]) l = i;
    return l;
}

// One block = up to kPropTokens consecutive tokens of one (image, level); the block counts valid_W / valid_H itself: h + w byte
// loads against 512 tokens x 17 bytes written.
__global__ void __launch_bounds__(kPropThreads)
encoder_proposals_kernel(const unsigned char* __restrict__ mask, float* __restrict__ proposals, unsigned char* __restrict__ keep,
                         const PropDims dm) {
    const int b = blockIdx.x / dm.chunks, c = blockIdx.x - b * dm.chunks;
    const int l = level_of_chunk(dm, c);
    const int hl = dm.h[l], wl = dm.w[l], n = hl * wl;
    const size_t base = (size_t)b * dm.S + dm.start[l];
    const unsigned char* m = mask + base;
    float fw, fh;
    level_counts(m, hl, wl, fw, fh);
    const int p0 = (c - dm.chunk0[l]) * kPropTokens;
#pragma unroll
    for (int j = 0; j < kPropTokens / kPropThreads; ++j) {
        const int p = p0 + j * kPropThreads + threadIdx.x;
        if (p >= n) break;
        f32x4 o;
        const bool ok = token_proposal(l, p, wl, fw, fh, m[p] != 0, o);
        *reinterpret_cast<f32x4*>(proposals + (base + p) * 4) = o;
        keep[base + p] = ok ? 1 : 0;
    }
}

// out = keep ? memory : 0 in 16-byte vectors.  2^shift lanes share a row (the host picks the power of two that covers the row's vpr
// vectors, at most the block), so row and column come from shifts and masks, and one byte of `keep` decides the row's loads: a
// dropped row is not read.
__global__ void __launch_bounds__(256)
mask_rows_kernel(const u32x4* __restrict__ memory, const unsigned char* __restrict__ keep, u32x4* __restrict__ out, long rows,
                 int vpr, int shift) {
    const int col0 = threadIdx.x & ((1 << shift) - 1), rows_per_block = 256 >> shift;
    for (long r = (long)blockIdx.x * rows_per_block + (threadIdx.x >> shift); r < rows; r += (long)gridDim.x * rows_per_block) {
        const bool k = keep[r] != 0;
        for (int c = col0; c < vpr; c += 1 << shift) {
            u32x4 v = {0u, 0u, 0u, 0u};
            if (k) v = memory[r * vpr + c];
            out[r * vpr + c] = v;
        }
    }
}

// The two passes above folded into one launch: a block takes kFoldTokens consecutive tokens of one (image, level), counts, writes
// their proposals and keeps the decisions in LDS, then streams the tokens' rows as mask_rows_kernel does (2^shift lanes per row).
constexpr int kFoldTokens = 64;

__global__ void __launch_bounds__(kPropThreads)
encoder_proposals_masked_kernel(const unsigned char* __restrict__ mask, float* __restrict__ proposals, unsigned char* __restrict__ keep,
                                const u32x4* __restrict__ memory, u32x4* __restrict__ out, const PropDims dm, int vpr, int shift) {
    __shared__ unsigned char kept[kFoldTokens];
    const int b = blockIdx.x / dm.chunks, c = blockIdx.x - b * dm.chunks;
    const int l = level_of_chunk(dm, c);
    const int hl = dm.h[l], wl = dm.w[l], n = hl * wl;
    const size_t base = (size_t)b * dm.S + dm.start[l];
    const unsigned char* m = mask + base;
    float fw, fh;
    level_counts(m, hl, wl, fw, fh);
    const int p0 = (c - dm.chunk0[l]) * kFoldTokens;
    const int tokens = n - p0 < kFoldTokens ? n - p0 : kFoldTokens;
    if ((int)threadIdx.x < tokens) {
        const int p = p0 + threadIdx.x;
        f32x4 o;
        const bool ok = token_proposal(l, p, wl, fw, fh, m[p] != 0, o);
        *reinterpret_cast<f32x4*>(proposals + (base + p) * 4) = o;
        keep[base + p] = kept[threadIdx.x] = ok ? 1 : 0;
    }
    __syncthreads();
    const int col0 = threadIdx.x & ((1 << shift) - 1);
    for (int t = threadIdx.x >> shift; t < tokens; t += kPropThreads >> shift) {
        const bool k = kept[t] != 0;
        const size_t row = (base + p0 + t) * vpr;
        for (int cc = col0; cc < vpr; cc += 1 << shift) {
            u32x4 v = {0u, 0u, 0u, 0u};
            if (k) v = memory[row + cc];
            out[row + cc] = v;
        }
    }
}

constexpr int kEmbed = 512;   // 4 components x 128 features (num_pos_feats of :131, fixed by the reference)

// One wave per query: lane t produces the 8 consecutive embedding values [8t, 8t + 8) = component t / 16, features
// 8 (t % 16) ... + 7, i.e. four (sin, cos) pairs of frequencies k = 4 (t % 16) ... + 3.  All lanes read the same gathered row.
// The angle is evaluated in double: near a zero crossing of sin / cos a float32 angle (error ~ 3e-7 at pi) is off by more than one
// bf16 / fp16 ulp of the (tiny) result.  2 400 waves x 12 double transcendentals per lane cost less than the launch.
template <typename T>
__global__ void __launch_bounds__(256)
proposal_queries_kernel(const float* __restrict__ coords, const long long* __restrict__ topk, const float* __restrict__ dim_t,
                        float* __restrict__ ref, T* __restrict__ embed, int S, int K, long queries) {
    const long q = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= queries) return;
    const int lane = threadIdx.x & 63;
    const long b = q / K;
    const long long idx = topk[q];
    const bool in_range = idx >= 0 && idx < (long long)S;
    // an index topk cannot produce: read row 0 of the image (always there) and use zeros instead
    const f32x4 raw = *reinterpret_cast<const f32x4*>(coords + ((size_t)b * S + (in_range ? (size_t)idx : 0)) * 4);
    const float row[4] = {in_range ? raw.x : 0.f, in_range ? raw.y : 0.f, in_range ? raw.z : 0.f, in_range ? raw.w : 0.f};
    double sg[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) sg[i] = 1.0 / (1.0 + exp(-(double)row[i]));   // +inf -> 1, -inf -> 0
    if (lane == 0) *reinterpret_cast<f32x4*>(ref + (size_t)q * 4) = f32x4{(float)sg[0], (float)sg[1], (float)sg[2], (float)sg[3]};

    const int comp = lane >> 4, k0 = (lane & 15) * 4;
    const double s = (comp == 0 ? sg[0] : comp == 1 ? sg[1] : comp == 2 ? sg[2] : sg[3]) * 6.283185307179586;
    const f32x4 freq = *reinterpret_cast<const f32x4*>(dim_t + k0);
    const float f[4] = {freq.x, freq.y, freq.z, freq.w};
    float v[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double a = s / (double)f[j];
        v[2 * j] = (float)sin(a);
        v[2 * j + 1] = (float)cos(a);
    }
    T* o = embed + (size_t)q * kEmbed + lane * 8;
    if constexpr (sizeof(T) == 2) {
        store_vec<T, float, 8>(o, v);
    } else {
        const float lo[4] = {v[0], v[1], v[2], v[3]}, hi[4] = {v[4], v[5], v[6], v[7]};
        store_vec<T, float, 4>(o, lo);
        store_vec<T, float, 4>(o + 4, hi);
    }
}

}  // namespace
}  // namespace alo

using namespace alo;

// Level geometry of a launch whose blocks take `tokens_per_block` tokens of one (image, level); 0 or an error code.
static int prop_dims(PropDims& dm, int B, int L, const int* level_shapes_host, int tokens_per_block, const char* what) {
    ALO_REQUIRE(B > 0 && L > 0 && L <= kMaxLevels, ALO_ERR_INVALID_ARGUMENT, "%s: needs B >= 1 and 1 <= L <= %d (got B = %d, L = %d)", what, kMaxLevels, B, L);
    dm.B = B; dm.L = L;
    long s = 0, chunks = 0;
    for (int l = 0; l < kMaxLevels; ++l) {
        dm.h[l] = l < L ? level_shapes_host[2 * l] : 1;
        dm.w[l] = l < L ? level_shapes_host[2 * l + 1] : 1;
        dm.start[l] = (int)s;
        dm.chunk0[l] = (int)chunks;
        if (l < L) {
            ALO_REQUIRE(dm.h[l] > 0 && dm.w[l] > 0, ALO_ERR_INVALID_ARGUMENT, "%s: level %d has an empty shape", what, l);
            const long n = (long)dm.h[l] * dm.w[l];
            s += n;
            chunks += (n + tokens_per_block - 1) / tokens_per_block;
            ALO_REQUIRE(s * B < (1l << 31) && chunks * B < (1l << 31), ALO_ERR_UNSUPPORTED, "%s: B * S must stay below 2^31 tokens", what);
        }
    }
    dm.S = (int)s;
    dm.chunks = (int)chunks;
    return ALO_OK;
}

// lanes per row of the row-masking loops: the power of two that covers vpr vectors, at most the block
static int row_shift(int vpr) {
    int shift = 0;
    while (shift < 8 && (1 << shift) < vpr) ++shift;
    return shift;
}

extern "C" int alo_encoder_proposals(const unsigned char* mask_flatten, float* proposals, unsigned char* keep, int B, int L,
                                     const int* level_shapes_host, void* stream) {
    ALO_REQUIRE(mask_flatten && proposals && keep && level_shapes_host, ALO_ERR_INVALID_ARGUMENT, "alo_encoder_proposals: null pointer argument");
    ALO_REQUIRE(aligned16(proposals), ALO_ERR_INVALID_ARGUMENT, "alo_encoder_proposals: proposals must be 16-byte aligned");
    PropDims dm;
    if (const int rc = prop_dims(dm, B, L, level_shapes_host, kPropTokens, "alo_encoder_proposals")) return rc;
    void* args[] = {&mask_flatten, &proposals, &keep, &dm};
    return launch<encoder_proposals_kernel>((unsigned)dm.chunks * (unsigned)B, kPropThreads, 0, static_cast<hipStream_t>(stream), "alo_encoder_proposals", args);
}

extern "C" int alo_encoder_proposals_masked(const unsigned char* mask_flatten, float* proposals, unsigned char* keep, const void* memory,
                                            void* out, int B, int L, const int* level_shapes_host, int C, int dtype, void* stream) {
    const char* what = "alo_encoder_proposals_masked";
    ALO_REQUIRE(dtype == ALO_F32 || dtype == ALO_BF16 || dtype == ALO_F16, ALO_ERR_UNSUPPORTED, "%s: dtype must be ALO_F32, ALO_BF16 or ALO_F16", what);
    ALO_REQUIRE(mask_flatten && proposals && keep && memory && out && level_shapes_host, ALO_ERR_INVALID_ARGUMENT, "%s: null pointer argument", what);
    const long row_bytes = (long)C * (dtype == ALO_F32 ? 4 : 2);
    ALO_REQUIRE(C > 0 && row_bytes % 16 == 0, ALO_ERR_UNSUPPORTED, "%s: needs rows of a multiple of 16 bytes (C = %d)", what, C);
    ALO_REQUIRE(aligned16(proposals, memory, out), ALO_ERR_INVALID_ARGUMENT, "%s: proposals, memory and out must be 16-byte aligned", what);
    ALO_REQUIRE(memory != out, ALO_ERR_INVALID_ARGUMENT, "%s: out must not alias memory", what);
    PropDims dm;
    if (const int rc = prop_dims(dm, B, L, level_shapes_host, kFoldTokens, what)) return rc;
    int vpr = (int)(row_bytes / 16), shift = row_shift(vpr);
    void* args[] = {&mask_flatten, &proposals, &keep, &memory, &out, &dm, &vpr, &shift};
    return launch<encoder_proposals_masked_kernel>((unsigned)dm.chunks * (unsigned)B, kPropThreads, 0, static_cast<hipStream_t>(stream), what, args);
}

extern "C" int alo_mask_rows(const void* memory, const unsigned char* keep, void* out, long rows, int C, int dtype, void* stream) {
    ALO_REQUIRE(dtype == ALO_F32 || dtype == ALO_BF16 || dtype == ALO_F16, ALO_ERR_UNSUPPORTED, "alo_mask_rows: dtype must be ALO_F32, ALO_BF16 or ALO_F16");
    ALO_REQUIRE(memory && keep && out, ALO_ERR_INVALID_ARGUMENT, "alo_mask_rows: null pointer argument");
    const long row_bytes = (long)C * (dtype == ALO_F32 ? 4 : 2);
    ALO_REQUIRE(rows > 0 && C > 0 && row_bytes % 16 == 0, ALO_ERR_UNSUPPORTED, "alo_mask_rows: needs rows >= 1 and rows of a multiple of 16 bytes (C = %d)", C);
    ALO_REQUIRE(aligned16(memory, out), ALO_ERR_INVALID_ARGUMENT, "alo_mask_rows: memory and out must be 16-byte aligned");
    ALO_REQUIRE(memory != out, ALO_ERR_INVALID_ARGUMENT, "alo_mask_rows: out must not alias memory");
    const int vpr = (int)(row_bytes / 16);
    int shift = row_shift(vpr);
    const long rows_per_block = 256 >> shift;
    long blocks = (rows + rows_per_block - 1) / rows_per_block;
    blocks = blocks > 8192 ? 8192 : blocks;
    void* args[] = {&memory, &keep, &out, &rows, const_cast<int*>(&vpr), &shift};
    return launch<mask_rows_kernel>((unsigned)blocks, 256, 0, static_cast<hipStream_t>(stream), "alo_mask_rows", args);
}

extern "C" int alo_proposal_queries(const float* coords_unact, const long long* topk, const float* dim_t, float* reference_points,
                                    void* embed, int B, int S, int K, int dtype, void* stream) {
    ALO_REQUIRE(dtype == ALO_F32 || dtype == ALO_BF16 || dtype == ALO_F16, ALO_ERR_UNSUPPORTED, "alo_proposal_queries: dtype must be ALO_F32, ALO_BF16 or ALO_F16");
    ALO_REQUIRE(coords_unact && topk && dim_t && reference_points && embed, ALO_ERR_INVALID_ARGUMENT, "alo_proposal_queries: null pointer argument");
    ALO_REQUIRE(B > 0 && S > 0 && K > 0 && (long)B * K < (1l << 31) && (long)B * S < (1l << 31), ALO_ERR_INVALID_ARGUMENT,
                "alo_proposal_queries: needs B, S, K >= 1 and B * K, B * S below 2^31");
    ALO_REQUIRE(aligned16(coords_unact, dim_t, reference_points, embed), ALO_ERR_INVALID_ARGUMENT, "alo_proposal_queries: coords_unact, dim_t, reference_points and embed must be 16-byte aligned");
    const long queries = (long)B * K;
    const unsigned blocks = (unsigned)((queries + 3) / 4);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == ALO_F32) {
        float* e = static_cast<float*>(embed);
        void* args[] = {&coords_unact, &topk, &dim_t, &reference_points, &e, &S, &K, const_cast<long*>(&queries)};
        return launch<proposal_queries_kernel<float>>(blocks, 256, 0, s, "alo_proposal_queries", args);
    }
    return with_storage_type(dtype, [&](auto t) {
        using T = decltype(t);
        T* e = static_cast<T*>(embed);
        void* args[] = {&coords_unact, &topk, &dim_t, &reference_points, &e, &S, &K, const_cast<long*>(&queries)};
        return launch<proposal_queries_kernel<T>>(blocks, 256, 0, s, "alo_proposal_queries", args);
    });
}
