// RAFT's memory-light correlation block (AlternateCorrBlock) for gfx950 (MI355X).
//
// Reference semantics: alonet/raft/corr.py:63-91.  The reference keeps the 2x2-mean pyramid of fmap2 and, per lookup and level,
// calls the third-party alt_cuda_corr extension on channels-last copies; the value it stands for is CorrBlock's: the bilinear
// sample at (x/2^l + i - r, y/2^l + j - r) of <fmap1[:, query], fmap2_l[:, .]> / sqrt(C), zero outside the map, the first window
// axis offsetting x.  A 2x2 mean commutes with the inner product, so this equals alo_corr_lookup on alo_corr_build's pyramid up to
// fp32 rounding, without the O((HW)^2) volume: only the feature maps are stored.
//
// Prepare (once per block): fmap1 and every level of fmap2 are laid out channels-last, channels zero-padded to a multiple of 16
// (corr_alt_relayout_kernel).  The reference re-permutes on every lookup.
//
// Lookup: a workgroup serves an 8x8 tile of query pixels on one level.  The (2r+2)^2 integer lattice points under each query's
// window are the inner products it needs; the bilinear weights are one (fx, fy) per query and level.  With smooth flow the
// lattices of a tile cover a small shared FOOTPRINT of fmap2_l (about 18x18 pixels at level 0, r = 4, against 6,400 lattice
// reads), so the footprint is staged in LDS 16 channels at a time and every lattice read is a ds_read_b128 from LDS.  The
// footprint is the bounding box of the lattices CLIPPED to the map, over the queries whose lattice touches the map: a NaN, inf
// or far-away coordinate reads as an all-zero window and never widens it.  A tile whose footprint exceeds the LDS budget
// (discontinuous or random motion) reads its lattice points straight from global memory instead: same arithmetic, same order,
// same result.  The lattice values then meet in LDS and each (query, tap) output is their bilinear mix.
//
// Arithmetic: exact fp32 (one fmaf chain per lattice point over the channels), so a non-finite feature spoils exactly the
// lattice points — and through them the taps — that touch it, as in the reference's fp32 arithmetic.
//
// Adjoint (alo_corr_alt_lookup with ALO_CORR_ALT_GRAD in num_levels, TrainableAlternateCorrBlock): corr_alt_lookup_bwd_kernel adds
// the gradients of one lookup with respect to fmap1 and to every level of fmap2 into the GRADIENT REGION the flagged workspace
// carries behind the prepared maps: one channels-last grad_fmap1 plane per level, then every level's gradient slice-major,
// (Cp/16, B, h*w, 16).  Same tiles, footprint and staged / direct decision as the lookup; the comment above the kernel has the rest.
#include "common.hpp"

#include "../../include/alo_corr_alt.h"

namespace alo {
namespace {

constexpr int kAltMaxLevels = 8;
constexpr int kAltCS = 16;                                 // channels per staged slice (= the channel padding)
constexpr int kAltTile = 8, kAltTQ = kAltTile * kAltTile;  // 8x8 queries per workgroup: lane = query, wave = a quarter of the lattice
constexpr int kAltThreads = 256;
constexpr int kAltMaxFp = 768;                             // footprint budget in pixels: 768 x 16 channels x 4 B = 48 KB of LDS
constexpr int kAltStageItems = kAltMaxFp * (kAltCS / 4) / kAltThreads;   // 16-byte pieces one thread stages per slice

struct AltArgs {
    const float* f1;                    // (B, H*W, Cp)
    const float* f2[kAltMaxLevels];     // level l: (B, h_l*w_l, Cp)
    int h[kAltMaxLevels], w[kAltMaxLevels];
    const float* coords;                // (B, 2, H, W)
    float* out;                         // (B, L*(2r+1)^2, H, W)
    int H, W, Cp, num_levels, tiles_x, tiles;
    unsigned nblocks;
    float scale;
};

// ------------------------------------------------------------------------------------------------------------------
// (B, C, n) -> (B, n, Cp) channels-last, channels C..Cp-1 zero.  A workgroup moves 64 pixels x 16 channels through LDS: the
// reads are 256-byte rows of one channel, the writes one contiguous 4 KB run.
// ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
corr_alt_relayout_kernel(const float* __restrict__ in, float* __restrict__ out, int C, int Cp, long n) {
    __shared__ float tile[kAltCS][65];
    const int b = blockIdx.z, c0 = blockIdx.y * kAltCS, t = threadIdx.x;
    const long p0 = (long)blockIdx.x * 64;
#pragma unroll
    for (int i = 0; i < kAltCS / 4; ++i) {
        const int c = (t >> 6) + 4 * i, px = t & 63;
        const long p = p0 + px;
        tile[c][px] = (c0 + c < C && p < n) ? in[((long)b * C + c0 + c) * n + p] : 0.f;
    }
    __syncthreads();
    const int px = t >> 2, c4 = t & 3;
    const long p = p0 + px;
    if (p < n) {
        const f32x4 v = {tile[4 * c4][px], tile[4 * c4 + 1][px], tile[4 * c4 + 2][px], tile[4 * c4 + 3][px]};
        *reinterpret_cast<f32x4*>(out + ((long)b * n + p) * Cp + c0 + 4 * c4) = v;
    }
}

template <int R>
constexpr int alt_lds_floats() {
    return kAltMaxFp * kAltCS > kAltTQ * (2 * R + 2) * (2 * R + 2) ? kAltMaxFp * kAltCS : kAltTQ * (2 * R + 2) * (2 * R + 2);
}

__device__ __forceinline__ float dot4(const f32x4 a, const f32x4 v, float acc) {
    acc = fmaf(a.x, v.x, acc);
    acc = fmaf(a.y, v.y, acc);
    acc = fmaf(a.z, v.z, acc);
    return fmaf(a.w, v.w, acc);
}

// ------------------------------------------------------------------------------------------------------------------
// One workgroup = one (8x8 query tile, level, batch item).  Lane q of every wave is query q of the tile; wave wv owns the lattice
// points k = wv, wv + 4, ... (row k / S, column k % S, S = 2r + 2) of that query.
// ------------------------------------------------------------------------------------------------------------------
template <int R>
__global__ void __launch_bounds__(kAltThreads)
corr_alt_lookup_kernel(const AltArgs a) {
    constexpr int S = 2 * R + 2, WIN = 2 * R + 1, NP = S * S / 4;
    static_assert(NP <= 64, "lattice mask is 64 bits");
    __shared__ f32x4 lds4[alt_lds_floats<R>() / 4];
    float* lds = reinterpret_cast<float*>(lds4);

    const unsigned id = xcd_contiguous_block(blockIdx.x, a.nblocks);   // neighbouring tiles share an XCD's L2
    const int tile = (int)(id % (unsigned)a.tiles);
    const int l = (int)((id / (unsigned)a.tiles) % (unsigned)a.num_levels);
    const int b = (int)(id / (unsigned)a.tiles / (unsigned)a.num_levels);
    const int tid = threadIdx.x, q = tid & (kAltTQ - 1), wv = tid >> 6;
    const int qx = (tile % a.tiles_x) * kAltTile + (q & (kAltTile - 1));
    const int qy = (tile / a.tiles_x) * kAltTile + q / kAltTile;
    const int h = a.h[l], w = a.w[l];
    const long HW = (long)a.H * a.W;
    const bool inside = qx < a.W && qy < a.H;
    const long qpix = inside ? (long)qy * a.W + qx : 0;

    // the query on this level (every wave derives the same values for its 64 lanes: no LDS, no barrier)
    const float inv = 1.0f / (float)(1 << l);
    float cx = 0.f, cy = 0.f;
    if (inside) {
        cx = a.coords[((long)b * 2 + 0) * HW + qpix] * inv;   // exact: power-of-two scale
        cy = a.coords[((long)b * 2 + 1) * HW + qpix] * inv;
    }
    const bool valid = inside && fabsf(cx) < 1e6f && fabsf(cy) < 1e6f;   // NaN fails too: an all-zero window
    const float flx = valid ? floorf(cx) : 0.f, fly = valid ? floorf(cy) : 0.f;
    const float fx = valid ? cx - flx : 0.f, fy = valid ? cy - fly : 0.f;
    const int x0 = (int)flx - R, y0 = (int)fly - R;   // the lattice's first column / row
    const int xlo = max(x0, 0), xhi = min(x0 + S - 1, w - 1), ylo = max(y0, 0), yhi = min(y0 + S - 1, h - 1);
    const bool touches = valid && xlo <= xhi && ylo <= yhi;
    int mnx = touches ? xlo : INT_MAX, mxx = touches ? xhi : INT_MIN;
    int mny = touches ? ylo : INT_MAX, mxy = touches ? yhi : INT_MIN;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mnx = min(mnx, __shfl_xor(mnx, o, 64));
        mxx = max(mxx, __shfl_xor(mxx, o, 64));
        mny = min(mny, __shfl_xor(mny, o, 64));
        mxy = max(mxy, __shfl_xor(mxy, o, 64));
    }
    const bool any = mnx <= mxx;   // workgroup-uniform from here on
    const int fw = any ? mxx - mnx + 1 : 0, fh = any ? mxy - mny + 1 : 0;
    // LDS row pitch = 8 mod 16 pixels: the 16 lanes of a ds_read_b128 group (rows of 4 queries of 2-4 tile rows) then hit 16
    // different bank quads when the flow is locally constant; the unpadded pitch where only that fits the budget
    int F = fw <= 8 ? 8 : ((fw - 9) / 16 + 1) * 16 + 8;
    if ((long)fh * F > kAltMaxFp) F = fw;
    const bool staged = (long)fh * F <= kAltMaxFp;

    // this thread's lattice points: staged -> LDS pixel index, otherwise the pixel index in the level; points off the map -> 0
    // with their mask bit clear (their value is replaced by zero, never multiplied by it: an inf elsewhere must not turn into NaN)
    int off[NP];
    unsigned long long mask = 0;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int k = wv + 4 * j, px = x0 + k % S, py = y0 + k / S;
        const bool in = valid && px >= 0 && px < w && py >= 0 && py < h;
        off[j] = !in ? 0 : (staged ? (py - mny) * F + (px - mnx) : py * w + px);
        mask |= (unsigned long long)in << j;
    }

    float acc[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) acc[j] = 0.f;
    const float* f1q = a.f1 + ((long)b * HW + qpix) * a.Cp;
    const float* f2b = a.f2[l] + (long)b * h * w * a.Cp;
    if (any && staged) {
        // pieces this thread stages every slice: footprint pixel (tid >> 2) + 64 i, channels 4 (tid & 3) .. + 3
        const int c4s = tid & 3;
        int gpix[kAltStageItems];
#pragma unroll
        for (int i = 0; i < kAltStageItems; ++i) {
            const int pix = (tid >> 2) + 64 * i, py = pix / F, px = pix - py * F;
            gpix[i] = (py < fh && px < fw) ? (mny + py) * w + mnx + px : -1;
        }
        f32x4 st[kAltStageItems];
        auto load_slice = [&](int c0) {
#pragma unroll
            for (int i = 0; i < kAltStageItems; ++i)
                if (gpix[i] >= 0) st[i] = *reinterpret_cast<const f32x4*>(f2b + (long)gpix[i] * a.Cp + c0 + 4 * c4s);
        };
        load_slice(0);
        for (int c0 = 0; c0 < a.Cp; c0 += kAltCS) {
            __syncthreads();   // the previous slice has been consumed
#pragma unroll
            for (int i = 0; i < kAltStageItems; ++i)
                if (gpix[i] >= 0) lds4[c4s * kAltMaxFp + (tid >> 2) + 64 * i] = st[i];
            __syncthreads();
            if (c0 + kAltCS < a.Cp) load_slice(c0 + kAltCS);   // in flight while this slice is computed
            f32x4 av[kAltCS / 4];
#pragma unroll
            for (int c = 0; c < kAltCS / 4; ++c)
                av[c] = valid ? *reinterpret_cast<const f32x4*>(f1q + c0 + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                float s = acc[j];
#pragma unroll
                for (int c = 0; c < kAltCS / 4; ++c) s = dot4(av[c], lds4[c * kAltMaxFp + off[j]], s);
                acc[j] = s;
            }
        }
    } else if (any) {
        // over the LDS budget: every lattice point straight from global memory (L2 / L1), same channel order
        for (int c0 = 0; c0 < a.Cp; c0 += kAltCS) {
            f32x4 av[kAltCS / 4];
#pragma unroll
            for (int c = 0; c < kAltCS / 4; ++c)
                av[c] = valid ? *reinterpret_cast<const f32x4*>(f1q + c0 + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const f32x4* p = reinterpret_cast<const f32x4*>(f2b + (long)off[j] * a.Cp + c0);
                float s = acc[j];
#pragma unroll
                for (int c = 0; c < kAltCS / 4; ++c) s = dot4(av[c], p[c], s);
                acc[j] = s;
            }
        }
    }

    // the lattice meets in LDS ([point][query]: conflict-free), then every (query, tap) is a bilinear mix of four points.  A thread
    // mixes for its own query (the loop strides by the workgroup size, a multiple of 64)
    __syncthreads();   // the stage buffer becomes the lattice buffer
#pragma unroll
    for (int j = 0; j < NP; ++j) lds[(wv + 4 * j) * kAltTQ + q] = ((mask >> j) & 1) ? acc[j] : 0.f;
    __syncthreads();
    if (!inside) return;
    const int CH = a.num_levels * WIN * WIN;
    float* outq = a.out + ((long)b * CH + (long)l * WIN * WIN) * HW + qpix;
    for (int rem = wv; rem < WIN * WIN; rem += kAltThreads / kAltTQ) {
        const int ax = rem / WIN, ay = rem % WIN;   // first window axis -> x offset, second -> y offset
        const int k = ay * S + ax;
        const float l00 = lds[k * kAltTQ + q], l01 = lds[(k + 1) * kAltTQ + q];
        const float l10 = lds[(k + S) * kAltTQ + q], l11 = lds[(k + S + 1) * kAltTQ + q];
        const float top = (1.0f - fx) * l00 + fx * l01, bot = (1.0f - fx) * l10 + fx * l11;
        outq[(long)rem * HW] = valid ? ((1.0f - fy) * top + fy * bot) * a.scale : 0.f;
    }
}

template <int R>
int launch_alt_lookup(AltArgs a, hipStream_t stream) {
    void* args[] = {&a};
    return launch<corr_alt_lookup_kernel<R>>(a.nblocks, kAltThreads, 0, stream, "alo_corr_alt_lookup", args);
}

// ------------------------------------------------------------------------------------------------------------------
// The adjoint of one lookup with respect to both feature maps (alo_corr_alt_lookup with ALO_CORR_ALT_GRAD).  Same workgroups, same
// footprint and same staged / direct decision as the forward.  With gL[k] = the bilinear adjoint of grad_out at lattice point k
// (times 1/sqrt(C); 0 off the map and for a query that reads an all-zero window), kept in registers like the forward's sums:
//   dF1[q, :]      += sum_k gL[k] * f2_l[pix(k), :]   the forward's inner loop with gL in place of the accumulators; the four waves'
//                     partial sums meet in LDS and are added to the level's OWN grad_fmap1 plane with plain loads and stores (a
//                     (query, level) belongs to one workgroup, launches on one stream are ordered): no atomics, reproducible;
//   dF2_l[pix(k),:] += gL[k] * f1[q, :]               a scatter.  Many (query, point) pairs of a tile hit the same pixel, so the slice
//                     of the footprint is summed in LDS (ds_add_f32 on a [channel][pixel] image: lanes = queries = neighbouring
//                     pixels = neighbouring banks) and every footprint row is flushed once per tile and slice with
//                     global_atomic_add_f32.  The gradient of a level is stored SLICE-MAJOR, (Cp/16, B, h*w, 16), so that a
//                     footprint row of a slice is one contiguous run: a wave's atomic instruction covers 256 contiguous bytes.
// Per 16-channel slice the 48 KB stage buffer is used three times (fmap2 slice -> the waves' dF1 partials -> dF2 accumulator), so the
// kernel stays under the forward's LDS budget at every radius.  A tile over the footprint budget reads fmap2 and adds into dF2
// straight in global memory, one atomic per (query, point, channel): slower, the same value up to the order of the sums.
// ------------------------------------------------------------------------------------------------------------------
constexpr int kAltAccPitch = kAltMaxFp + 1;   // accumulator [channel][pixel]: an odd pitch, the flush reads 16 channels of a pixel

struct AltGradArgs {
    float* g1[kAltMaxLevels];   // level l's plane of grad_fmap1: (B, H*W, Cp)
    float* g2[kAltMaxLevels];   // gradient of fmap2's level l: (Cp/16, B, h_l*w_l, 16)
    int B;
};

template <int R>
__global__ void __launch_bounds__(kAltThreads)
corr_alt_lookup_bwd_kernel(const AltArgs a, const AltGradArgs ga) {
    constexpr int S = 2 * R + 2, WIN = 2 * R + 1, NP = S * S / 4;
    static_assert(NP <= 64, "lattice mask is 64 bits");
    constexpr int kLds4 = (kAltAccPitch * kAltCS + 3) / 4;
    static_assert(kLds4 >= kAltAccPitch * (kAltCS / 4) && kLds4 >= kAltThreads * (kAltCS / 4), "stage buffer and partial sums fit");
    __shared__ f32x4 lds4[kLds4];
    float* lds = reinterpret_cast<float*>(lds4);

    const unsigned id = xcd_contiguous_block(blockIdx.x, a.nblocks);
    const int tile = (int)(id % (unsigned)a.tiles);
    const int l = (int)((id / (unsigned)a.tiles) % (unsigned)a.num_levels);
    const int b = (int)(id / (unsigned)a.tiles / (unsigned)a.num_levels);
    const int tid = threadIdx.x, q = tid & (kAltTQ - 1), wv = tid >> 6;
    const int tx0 = (tile % a.tiles_x) * kAltTile, ty0 = (tile / a.tiles_x) * kAltTile;
    const int qx = tx0 + (q & (kAltTile - 1)), qy = ty0 + q / kAltTile;
    const int h = a.h[l], w = a.w[l];
    const long HW = (long)a.H * a.W;
    const bool inside = qx < a.W && qy < a.H;
    const long qpix = inside ? (long)qy * a.W + qx : 0;

    // the query on this level, its lattice and the tile's footprint: the forward's, line for line
    const float inv = 1.0f / (float)(1 << l);
    float cx = 0.f, cy = 0.f;
    if (inside) {
        cx = a.coords[((long)b * 2 + 0) * HW + qpix] * inv;
        cy = a.coords[((long)b * 2 + 1) * HW + qpix] * inv;
    }
    const bool valid = inside && fabsf(cx) < 1e6f && fabsf(cy) < 1e6f;
    const float flx = valid ? floorf(cx) : 0.f, fly = valid ? floorf(cy) : 0.f;
    const float fx = valid ? cx - flx : 0.f, fy = valid ? cy - fly : 0.f;
    const int x0 = (int)flx - R, y0 = (int)fly - R;
    const int xlo = max(x0, 0), xhi = min(x0 + S - 1, w - 1), ylo = max(y0, 0), yhi = min(y0 + S - 1, h - 1);
    const bool touches = valid && xlo <= xhi && ylo <= yhi;
    int mnx = touches ? xlo : INT_MAX, mxx = touches ? xhi : INT_MIN;
    int mny = touches ? ylo : INT_MAX, mxy = touches ? yhi : INT_MIN;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mnx = min(mnx, __shfl_xor(mnx, o, 64));
        mxx = max(mxx, __shfl_xor(mxx, o, 64));
        mny = min(mny, __shfl_xor(mny, o, 64));
        mxy = max(mxy, __shfl_xor(mxy, o, 64));
    }
    if (mnx > mxx) return;   // workgroup-uniform: no window of the tile touches the map, nothing to add
    const int fw = mxx - mnx + 1, fh = mxy - mny + 1;
    int F = fw <= 8 ? 8 : ((fw - 9) / 16 + 1) * 16 + 8;
    if ((long)fh * F > kAltMaxFp) F = fw;
    const bool staged = (long)fh * F <= kAltMaxFp;

    // this thread's lattice points and their gL: point (row, col) feeds the taps (col - dx, row - dy), dx, dy in {0, 1}, with the
    // weights the forward mixed them with.  A point off the map, or of a query whose window reads as zero, has no bit and gL = 0
    const float* gq = a.out + ((long)b * a.num_levels + l) * (WIN * WIN) * HW + qpix;   // grad_out of this query's level
    const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
    auto point_grad = [&](int row, int col) {
        float s = 0.f;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int ax = col - dx, ay = row - dy;
                if (ax >= 0 && ax < WIN && ay >= 0 && ay < WIN) s = fmaf(wy[dy] * wx[dx], gq[(long)(ax * WIN + ay) * HW], s);
            }
        return s * a.scale;
    };

    const float* f1q = a.f1 + ((long)b * HW + qpix) * a.Cp;
    const float* f2b = a.f2[l] + (long)b * h * w * a.Cp;
    // the plane of grad_fmap1: thread -> query tid / 4, channels 4 (tid & 3) .. + 3 of the slice
    const int c4s = tid & 3, q2 = tid >> 2;
    const int q2x = tx0 + (q2 & (kAltTile - 1)), q2y = ty0 + q2 / kAltTile;
    const bool inside2 = q2x < a.W && q2y < a.H;
    float* g1q = ga.g1[l] + ((long)b * HW + (inside2 ? (long)q2y * a.W + q2x : 0)) * a.Cp + 4 * c4s;
    const long slice_stride = (long)ga.B * h * w * kAltCS;                 // floats between two slices of the level's gradient
    float* g2b = ga.g2[l] + (long)b * h * w * kAltCS;

    // the four waves' partial sums of dF1 meet in LDS; a thread then adds one query's four channels to the plane
    auto add_f1 = [&](const f32x4 (&p)[kAltCS / 4], int c0) {
        __syncthreads();   // every wave is done with the buffer's previous contents
#pragma unroll
        for (int c = 0; c < kAltCS / 4; ++c) lds4[(wv * (kAltCS / 4) + c) * kAltTQ + q] = p[c];
        __syncthreads();
        if (inside2) {
            f32x4 s = lds4[c4s * kAltTQ + q2];
#pragma unroll
            for (int v = 1; v < kAltThreads / kAltTQ; ++v) s += lds4[(v * (kAltCS / 4) + c4s) * kAltTQ + q2];
            f32x4* dst = reinterpret_cast<f32x4*>(g1q + c0);
            *dst = *dst + s;
        }
    };

    if (staged) {
        // the points' gL and LDS pixel stay in registers for all slices.  A point off the map, or of a query whose window reads as
        // zero, has gL = 0 and the spare pixel kAltMaxFp (zero, never flushed): no branch in the loops
        int off[NP];
        float gl[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int k = wv + 4 * j, col = k % S, row = k / S, px = x0 + col, py = y0 + row;
            const bool in = valid && px >= 0 && px < w && py >= 0 && py < h;
            off[j] = in ? (py - mny) * F + (px - mnx) : kAltMaxFp;
            gl[j] = in ? point_grad(row, col) : 0.f;
        }
        constexpr bool kAhead = R <= 5;   // the next slice's loads in flight during this one's arithmetic, where the registers allow
        int gpix[kAltStageItems];
#pragma unroll
        for (int i = 0; i < kAltStageItems; ++i) {
            const int pix = (tid >> 2) + 64 * i, py = pix / F, px = pix - py * F;
            gpix[i] = (py < fh && px < fw) ? (mny + py) * w + mnx + px : -1;
        }
        f32x4 st[kAltStageItems];
        auto load_slice = [&](int c0) {
#pragma unroll
            for (int i = 0; i < kAltStageItems; ++i)
                if (gpix[i] >= 0) st[i] = *reinterpret_cast<const f32x4*>(f2b + (long)gpix[i] * a.Cp + c0 + 4 * c4s);
        };
        const int rowlen = fw * kAltCS;   // floats of one footprint row of a slice: contiguous in the level's gradient
        if (kAhead) load_slice(0);
        for (int c0 = 0; c0 < a.Cp; c0 += kAltCS) {
            if (!kAhead) load_slice(c0);
            __syncthreads();   // the previous slice's accumulator has been flushed
#pragma unroll
            for (int i = 0; i < kAltStageItems; ++i)
                if (gpix[i] >= 0) lds4[c4s * kAltAccPitch + (tid >> 2) + 64 * i] = st[i];
            if (tid < kAltCS / 4) lds4[tid * kAltAccPitch + kAltMaxFp] = f32x4{0.f, 0.f, 0.f, 0.f};
            __syncthreads();
            if (kAhead && c0 + kAltCS < a.Cp) load_slice(c0 + kAltCS);
            f32x4 av[kAltCS / 4], p[kAltCS / 4];
#pragma unroll
            for (int c = 0; c < kAltCS / 4; ++c) {
                av[c] = valid ? *reinterpret_cast<const f32x4*>(f1q + c0 + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f};
                p[c] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                // the LDS address is formed here, from an index the compiler cannot see through: hoisted out of the slice loop, the
                // points' byte addresses (two forms each) would double the registers the points hold
                int o = off[j];
                asm volatile("" : "+v"(o));
#pragma unroll
                for (int c = 0; c < kAltCS / 4; ++c) p[c] += gl[j] * lds4[c * kAltAccPitch + o];
                __builtin_amdgcn_sched_barrier(0);   // keep the reads of later points behind this one's: registers again
            }
            add_f1(p, c0);
            __syncthreads();   // the partial sums have been read: the buffer becomes the accumulator of dF2's slice
            for (int i = tid; i < kLds4; i += kAltThreads) lds4[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            __syncthreads();
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                int o = off[j];
                asm volatile("" : "+v"(o));
#pragma unroll
                for (int c = 0; c < kAltCS; ++c) atomicAdd(&lds[c * kAltAccPitch + o], gl[j] * av[c >> 2][c & 3]);
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();
            // flush: consecutive lanes -> consecutive floats of a footprint row (pixel-major, 16 channels each)
            float* dst = g2b + (long)(c0 / kAltCS) * slice_stride;
            int py = tid / rowlen, e = tid - py * rowlen;
            while (py < fh) {
                const float v = lds[(e & (kAltCS - 1)) * kAltAccPitch + py * F + (e >> 4)];
                if (v != 0.f) atomicAdd(dst + ((long)(mny + py) * w + mnx) * kAltCS + e, v);
                e += kAltThreads;
                while (e >= rowlen) {
                    e -= rowlen;
                    ++py;
                }
            }
        }
    } else {
        for (int c0 = 0; c0 < a.Cp; c0 += kAltCS) {
            f32x4 av[kAltCS / 4], p[kAltCS / 4];
#pragma unroll
            for (int c = 0; c < kAltCS / 4; ++c) {
                av[c] = valid ? *reinterpret_cast<const f32x4*>(f1q + c0 + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f};
                p[c] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            float* dst = g2b + (long)(c0 / kAltCS) * slice_stride;
#pragma unroll 1
            for (int k = wv; k < S * S; k += kAltThreads / kAltTQ) {   // rolled: this path is bound by its atomics
                const int col = k % S, row = k / S, px = x0 + col, py = y0 + row;
                if (!(valid && px >= 0 && px < w && py >= 0 && py < h)) continue;
                const float g = point_grad(row, col);
                const long pix = (long)py * w + px;
                const f32x4* src = reinterpret_cast<const f32x4*>(f2b + pix * a.Cp + c0);
#pragma unroll
                for (int c = 0; c < kAltCS / 4; ++c) p[c] += g * src[c];
#pragma unroll
                for (int c = 0; c < kAltCS; ++c) atomicAdd(dst + pix * kAltCS + c, g * av[c >> 2][c & 3]);
            }
            add_f1(p, c0);
        }
    }
}

template <int R>
int launch_alt_lookup_bwd(AltArgs a, AltGradArgs ga, hipStream_t stream) {
    void* args[] = {&a, &ga};
    return launch<corr_alt_lookup_bwd_kernel<R>>(a.nblocks, kAltThreads, 0, stream, "alo_corr_alt_lookup", args);
}

inline size_t alt_align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int alt_cpad(int C) { return (C + kAltCS - 1) / kAltCS * kAltCS; }

// the limits of alo_corr_alt.h; ALO_OK or an error with its message
int alt_check_sizes(int B, int C, int H, int W, int num_levels, const char* what) {
    ALO_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, ALO_ERR_INVALID_ARGUMENT, "%s: dimensions must be positive (B=%d C=%d H=%d W=%d)",
                what, B, C, H, W);
    ALO_REQUIRE(num_levels >= 1 && num_levels <= kAltMaxLevels, ALO_ERR_INVALID_ARGUMENT, "%s: num_levels must be in [1,%d], got %d",
                what, kAltMaxLevels, num_levels);
    ALO_REQUIRE(B <= 65535 && C <= 65536 && (long)H * W <= (1L << 26), ALO_ERR_UNSUPPORTED,
                "%s: size past the limits (B <= 65535, C <= 65536, H*W <= 2^26; got B=%d C=%d H=%d W=%d)", what, B, C, H, W);
    for (int l = 0; l < num_levels; ++l) {
        int h, w;
        alo_corr_level_shape(H, W, l, &h, &w);
        ALO_REQUIRE(h > 0 && w > 0, ALO_ERR_INVALID_ARGUMENT, "%s: pyramid level %d of a %dx%d grid is empty", what, l, H, W);
    }
    return ALO_OK;
}

}  // namespace
}  // namespace alo

using namespace alo;

namespace {
// num_levels as the entry points take it: the level count in the low byte, ALO_CORR_ALT_GRAD above it
inline bool alt_stray_bits(int num_levels) { return num_levels > 0 && (num_levels & ~(0xff | ALO_CORR_ALT_GRAD)) != 0; }
inline bool alt_grad_flag(int num_levels) { return num_levels > 0 && (num_levels & ALO_CORR_ALT_GRAD) != 0; }
}  // namespace

extern "C" size_t alo_corr_alt_workspace_bytes(int B, int C, int H, int W, int num_levels) {
    if (alt_stray_bits(num_levels)) return 0;
    const bool grad = alt_grad_flag(num_levels);
    if (grad) num_levels &= 0xff;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || num_levels < 1 || num_levels > kAltMaxLevels || B > 65535 || C > 65536 ||
        (long)H * W > (1L << 26))
        return 0;
    const size_t cp = (size_t)alt_cpad(C);
    const size_t plane = alt_align256((size_t)B * H * W * cp * sizeof(float));
    size_t total = plane;
    for (int l = 0; l < num_levels; ++l) {
        int h, w;
        alo_corr_level_shape(H, W, l, &h, &w);
        total += alt_align256((size_t)B * h * w * cp * sizeof(float));
    }
    // the gradient region: one grad_fmap1 plane per level, then every level's gradient (the sizes of the prepared parts)
    return grad ? total + (size_t)num_levels * plane + (total - plane) : total;
}

namespace {
// level pointers inside a prepared workspace; with g1 / g2 also those of the gradient region behind it
void alt_layout(void* ws, int B, int C, int H, int W, int num_levels, float** f1, float** f2, float** g1 = nullptr,
                float** g2 = nullptr) {
    const size_t cp = (size_t)alt_cpad(C);
    const size_t plane = alt_align256((size_t)B * H * W * cp * sizeof(float));
    unsigned char* p = static_cast<unsigned char*>(ws);
    *f1 = reinterpret_cast<float*>(p);
    p += plane;
    for (int pass = 0; pass < (g1 ? 2 : 1); ++pass) {
        for (int l = 0; pass == 1 && l < num_levels; ++l, p += plane) g1[l] = reinterpret_cast<float*>(p);
        for (int l = 0; l < num_levels; ++l) {
            int h, w;
            alo_corr_level_shape(H, W, l, &h, &w);
            (pass == 0 ? f2 : g2)[l] = reinterpret_cast<float*>(p);
            p += alt_align256((size_t)B * h * w * cp * sizeof(float));
        }
    }
}
}  // namespace

extern "C" int alo_corr_alt_prepare(const float* fmap1, const float* const* fmap2_levels, void* workspace, size_t workspace_bytes,
                                    int B, int C, int H, int W, int num_levels, void* stream_) {
    const char* what = "alo_corr_alt_prepare";
    ALO_REQUIRE(fmap1 && fmap2_levels, ALO_ERR_INVALID_ARGUMENT, "%s: null pointer argument", what);
    if (int rc = alt_check_sizes(B, C, H, W, num_levels, what)) return rc;
    for (int l = 0; l < num_levels; ++l) ALO_REQUIRE(fmap2_levels[l], ALO_ERR_INVALID_ARGUMENT, "%s: fmap2_levels[%d] is null", what, l);
    const size_t need = alo_corr_alt_workspace_bytes(B, C, H, W, num_levels);
    ALO_REQUIRE(workspace && workspace_bytes >= need && aligned16(workspace), ALO_ERR_INVALID_ARGUMENT,
                "%s: a 16-byte aligned workspace of %zu bytes is required, %zu given", what, need, workspace_bytes);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    float* f1 = nullptr;
    float* f2[kAltMaxLevels];
    alt_layout(workspace, B, C, H, W, num_levels, &f1, f2);
    const int Cp = alt_cpad(C);
    auto relayout = [&](const float* in, float* out, long n) -> int {
        const dim3 grid((unsigned)((n + 63) / 64), (unsigned)(Cp / kAltCS), (unsigned)B);
        void* args[] = {&in, &out, &C, const_cast<int*>(&Cp), &n};
        return launch<corr_alt_relayout_kernel>(grid, 256, 0, stream, what, args);
    };
    if (int rc = relayout(fmap1, f1, (long)H * W)) return rc;
    for (int l = 0; l < num_levels; ++l) {
        int h, w;
        alo_corr_level_shape(H, W, l, &h, &w);
        if (int rc = relayout(fmap2_levels[l], f2[l], (long)h * w)) return rc;
    }
    return ALO_OK;
}

extern "C" int alo_corr_alt_lookup(const void* workspace, size_t workspace_bytes, const float* coords, float* out, int B, int C,
                                   int H, int W, int radius, int num_levels, void* stream_) {
    const char* what = "alo_corr_alt_lookup";
    ALO_REQUIRE(workspace && coords && out, ALO_ERR_INVALID_ARGUMENT, "%s: null pointer argument", what);
    ALO_REQUIRE(!alt_stray_bits(num_levels), ALO_ERR_UNSUPPORTED,
                "%s: num_levels 0x%x has bits above the level count other than ALO_CORR_ALT_GRAD (0x%x)", what, (unsigned)num_levels,
                (unsigned)ALO_CORR_ALT_GRAD);
    const bool grad = alt_grad_flag(num_levels);
    const int flag = grad ? ALO_CORR_ALT_GRAD : 0;
    if (grad) num_levels &= 0xff;
    if (int rc = alt_check_sizes(B, C, H, W, num_levels, what)) return rc;
    ALO_REQUIRE(radius >= 0 && radius <= 7, ALO_ERR_UNSUPPORTED, "%s: radius must be in [0,7], got %d", what, radius);
    const size_t need = alo_corr_alt_workspace_bytes(B, C, H, W, num_levels | flag);
    ALO_REQUIRE(workspace_bytes >= need && aligned16(workspace), ALO_ERR_INVALID_ARGUMENT,
                "%s: a 16-byte aligned workspace of %zu bytes is required, %zu given", what, need, workspace_bytes);
    AltArgs a;
    float* f1 = nullptr;
    float* f2[kAltMaxLevels];
    AltGradArgs ga;
    alt_layout(const_cast<void*>(workspace), B, C, H, W, num_levels, &f1, f2, grad ? ga.g1 : nullptr, grad ? ga.g2 : nullptr);
    for (int l = num_levels; grad && l < kAltMaxLevels; ++l) ga.g1[l] = ga.g2[l] = nullptr;
    ga.B = B;
    a.f1 = f1;
    for (int l = 0; l < kAltMaxLevels; ++l) {
        a.f2[l] = l < num_levels ? f2[l] : nullptr;
        a.h[l] = a.w[l] = 1;
        if (l < num_levels) alo_corr_level_shape(H, W, l, &a.h[l], &a.w[l]);
    }
    a.coords = coords;
    a.out = out;
    a.H = H;
    a.W = W;
    a.Cp = alt_cpad(C);
    a.num_levels = num_levels;
    a.tiles_x = (W + kAltTile - 1) / kAltTile;
    a.tiles = a.tiles_x * ((H + kAltTile - 1) / kAltTile);
    const long nblocks = (long)a.tiles * num_levels * B;
    ALO_REQUIRE(nblocks < 0x7fffffffL, ALO_ERR_UNSUPPORTED, "%s: grid too large (%ld workgroups)", what, nblocks);
    a.nblocks = (unsigned)nblocks;
    a.scale = 1.0f / sqrtf((float)C);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (grad) {   // `out` is grad_out (read); the gradient region of the workspace is added to
        switch (radius) {
            case 0: return launch_alt_lookup_bwd<0>(a, ga, stream);
            case 1: return launch_alt_lookup_bwd<1>(a, ga, stream);
            case 2: return launch_alt_lookup_bwd<2>(a, ga, stream);
            case 3: return launch_alt_lookup_bwd<3>(a, ga, stream);
            case 4: return launch_alt_lookup_bwd<4>(a, ga, stream);
            case 5: return launch_alt_lookup_bwd<5>(a, ga, stream);
            case 6: return launch_alt_lookup_bwd<6>(a, ga, stream);
            default: return launch_alt_lookup_bwd<7>(a, ga, stream);
        }
    }
    switch (radius) {
        case 0: return launch_alt_lookup<0>(a, stream);
        case 1: return launch_alt_lookup<1>(a, stream);
        case 2: return launch_alt_lookup<2>(a, stream);
        case 3: return launch_alt_lookup<3>(a, stream);
        case 4: return launch_alt_lookup<4>(a, stream);
        case 5: return launch_alt_lookup<5>(a, stream);
        case 6: return launch_alt_lookup<6>(a, stream);
        default: return launch_alt_lookup<7>(a, stream);
    }
}
