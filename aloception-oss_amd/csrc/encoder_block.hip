// The row-local part of a Deformable-DETR encoder layer in one kernel (include/alo_encoder_block.h):
//
//   [ src  = LayerNorm1(attn_out Wo^T + bo + src) ]                    attention tail        (TAIL)
//     src' = LayerNorm2(relu(src W1^T + b1) W2^T + b2 + src)           feed-forward block
//   [ value = mask(src' Wv^T + bv) head-major,  offsets_logits = (src' + pos) Wq^T + bq ]    next layer's projections (PROJ)
//
// Run as separate launches (alo_linear_shortk, alo_add_layernorm, alo_ffn256, alo_add_layernorm, alo_value_proj_head_major,
// alo_linear_shortk) every arrow of that chain is a (rows, 256) bf16 tensor written by one streaming kernel and read back by the next:
// at 177784 rows about 900 MB of the 1500 MB a layer moves between two attention launches (counted from the shapes, not measured).  Here a workgroup owns 64 rows for the whole
// chain.  It is ffn256_kernel's frame (gemm.hip): 256 threads, two 64 x 256 bf16 LDS tiles A and B, persistent over the tiles, weights
// pre-packed in MFMA fragment order and streamed through two register buffers.  Each product reads A and stages its bf16 result in B;
// each LayerNorm reads B (+ its residual) one wave per row, a lane owning 4 consecutive columns as in add_layernorm_kernel, and leaves
// the normalised rows in A for the next product.  Rounding points, operand roles and summation orders are those of the kernels this
// stands in for, so the three outputs equal theirs bit for bit.
#include "mfma_tile.hpp"

#include "../../include/alo_encoder_block.h"

namespace alo {
namespace {

constexpr int kHeads = 8;          // value_hm is (batch, 8, S, 32)
constexpr int kQueryCols = 384;    // merged [sampling_offsets (256); attention_weights (128)]
constexpr int kRowsPerWave = kTileRows / 4;
constexpr int kTables = 256 * 7 + kQueryCols;   // fp32 tables next to b1: b2, bo, bv, bq, and the two LayerNorms' gamma / beta

struct EncBlockArgs {
    const bf16_t *attn, *wo, *bo, *g1, *be1;
    const bf16_t *src, *w1, *b1, *w2, *b2, *g2, *be2;
    bf16_t* out;
    const bf16_t* pos;
    const unsigned char* mask;
    const bf16_t *wv, *bv, *wq, *bq;
    bf16_t *value, *both;
    long M;
    int S, F, tiles;
    float eps1, eps2;
};

// LayerNorm of one 256-wide row spread over the wave, 4 consecutive columns per lane: add_layernorm_kernel's arithmetic
__device__ __forceinline__ void layernorm_row(const float (&v)[4], const f32x4& g, const f32x4& b, float eps, float (&y)[4]) {
    const float inv_c = 1.0f / 256.f;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s += v[i];
    const float mean = wave_sum(s) * inv_c;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const float d = v[i] - mean; q += d * d; }
    const float rstd = rsqrtf(wave_sum(q) * inv_c + eps);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = (v[i] - mean) * rstd * g[i] + b[i];
}

// accumulators start from the bias (linear_shortk_kernel): registers 4 q .. 4 q + 3 of column tile t = columns 32 t + 8 q + 4 kg ..
__device__ __forceinline__ void init_acc_bias(f32x16 (&acc)[2][2], const float* bias64, int kg) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 bb = *reinterpret_cast<const f32x4*>(bias64 + 32 * t + 8 * q + 4 * kg);
#pragma unroll
            for (int i = 0; i < 4; ++i) { acc[0][t][4 * q + i] = bb[i]; acc[1][t][4 * q + i] = bb[i]; }
        }
}

// An opaque copy of a weight pointer, taken once per tile: without it the address of every weight load of the three short products (a
// register pair each, the same for all tiles) is computed ahead of the tile loop and the pairs are spilled.
__device__ __forceinline__ const bf16_t* per_tile(const bf16_t* w) {
    asm volatile("" : "+v"(w));
    return w;
}

// The residual and pos rows a LayerNorm adds are wanted AFTER a product, in the one-wave-per-row layout; held in registers across the
// product (32 VGPRs next to 64 accumulators and 32 of weights) they pushed the kernel into scratch.  So they are loaded after the
// product, and only warmed before it: one dword per 128-byte line of this wave's 16 rows brings the lines into the L2 and costs one
// register; retire() is where that register is given up.
__device__ __forceinline__ unsigned warm_rows(const bf16_t* X, long first_row, long M, int lane) {
    long row = first_row + (lane >> 2);
    row = row < M ? row : M - 1;
    return *reinterpret_cast<const unsigned*>(X + row * 256 + (lane & 3) * 64);
}
__device__ __forceinline__ void retire(unsigned v) { asm volatile("" ::"v"(v)); }
// this wave's 16 rows, 4 consecutive columns per lane; rows past the end are read from the last row
__device__ __forceinline__ void load_rows(u32x2 (&v)[kRowsPerWave], const bf16_t* X, long first_row, long M, int lane) {
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) {
        long row = first_row + r;
        row = row < M ? row : M - 1;
        v[r] = *reinterpret_cast<const u32x2*>(X + row * 256 + 4 * lane);
    }
}

template <bool TAIL, bool PROJ>
__global__ void __launch_bounds__(256, 2)
encoder_block_kernel(const EncBlockArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const A = smem;                             // the tile every product reads
    unsigned char* const B = smem + kTileRows * kTileStride;   // hidden chunk / every product's bf16 result
    const int tid = threadIdx.x, lane = tid & 63;
    // the wave index as a scalar: row and weight-tile addresses then split into a scalar base and one per-lane offset, instead of a
    // register pair per row and per fragment
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nl = lane & 31, kg = lane >> 5;
    const int F = p.F;

    float* const b1s = reinterpret_cast<float*>(smem + 2 * kTileRows * kTileStride);
    float* const b2s = b1s + F;
    float* const bos = b2s + 256;
    float* const bvs = bos + 256;
    float* const bqs = bvs + 256;
    float* const g1s = bqs + kQueryCols;
    float* const e1s = g1s + 256;
    float* const g2s = e1s + 256;
    float* const e2s = g2s + 256;
    for (int i = tid; i < F; i += 256) b1s[i] = bf16_to_f32(p.b1[i].bits);
    b2s[tid] = bf16_to_f32(p.b2[tid].bits);
    g2s[tid] = bf16_to_f32(p.g2[tid].bits);
    e2s[tid] = bf16_to_f32(p.be2[tid].bits);
    if constexpr (TAIL) {
        bos[tid] = bf16_to_f32(p.bo[tid].bits);
        g1s[tid] = bf16_to_f32(p.g1[tid].bits);
        e1s[tid] = bf16_to_f32(p.be1[tid].bits);
    }
    if constexpr (PROJ) {
        bvs[tid] = bf16_to_f32(p.bv[tid].bits);
        for (int i = tid; i < kQueryCols; i += 256) bqs[i] = bf16_to_f32(p.bq[i].bits);
    }

    const int fs = F / 16;  // k steps per output-column tile of the packed W2
    // this lane's 16 bytes of the first fragment of this wave's first column tile (packed fragment = 64 lanes x 16 B contiguous)
    auto k256_frag = [&](const bf16_t* W, int col0) { return W + ((size_t)((col0 + 64 * wave) / 32) * 16 * 64 + lane) * 8; };  // tile stride 16 * 512
    auto w2_frag = [&](int r0) { return p.w2 + (((size_t)(2 * wave) * fs + r0 / 16) * 64 + lane) * 8; };                        // tile stride fs * 512
    constexpr size_t kStride256 = (size_t)16 * 512;

    for (int tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const long row0 = (long)tile * kTileRows;
        const int wrow = kRowsPerWave * wave;  // the 16 rows this wave normalises
        const bf16_t* const wo_f = TAIL ? per_tile(k256_frag(p.wo, 0)) : nullptr;
        const bf16_t* const wv_f = PROJ ? per_tile(k256_frag(p.wv, 0)) : nullptr;
        const bf16_t* const wq_f = PROJ ? per_tile(k256_frag(p.wq, 0)) : nullptr;  // columns 256 .. : 8 column tiles on
        u32x4 bufa[2][kTileKB], bufb[2][kTileKB];
        {
            u32x4 xv[8];
            fetch_tile256(xv, TAIL ? p.attn : p.src, row0, p.M, tid);
            park_tile256(A, xv, tid);
        }

        if constexpr (TAIL) {
            // ---- attention tail: A = LayerNorm1(attn_out Wo^T + bo + src); the residual rows are warmed before the product ----------
            const unsigned warm = warm_rows(p.src, row0 + wrow, p.M, lane);
            load_batch(bufa, wo_f, kStride256, 0);
            __syncthreads();
            f32x16 acc[2][2];
            init_acc_bias(acc, bos + 64 * wave, kg);
            mma_tile256(acc, A, bufa, bufb, wo_f, kStride256, k256_frag(p.w1, 0), kStride256, nl, kg);
            stage_tile256<false, false>(B, acc, nullptr, wave, nl, kg);
            __syncthreads();  // the projected rows are in B and nobody reads A any more
            retire(warm);
            u32x2 res[kRowsPerWave];
            load_rows(res, p.src, row0 + wrow, p.M, lane);
            const f32x4 g = *reinterpret_cast<const f32x4*>(g1s + 4 * lane), b = *reinterpret_cast<const f32x4*>(e1s + 4 * lane);
#pragma unroll
            for (int r = 0; r < kRowsPerWave; ++r) {
                float v[4], t[4], y[4];
                unpack4<bf16_t>(*reinterpret_cast<const u32x2*>(B + (wrow + r) * kTileStride + lane * 8), v);
                unpack4<bf16_t>(res[r], t);
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] += t[i];
                layernorm_row(v, g, b, p.eps1, y);
                *reinterpret_cast<u32x2*>(A + (wrow + r) * kTileStride + lane * 8) = pack4<bf16_t>(y);
            }
        } else {
            load_batch(bufa, k256_frag(p.w1, 0), kStride256, 0);
        }
        __syncthreads();  // the FFN's x tile is in A

        // ---- feed-forward block: ffn256_kernel's arithmetic, the hidden activation 256 units at a time through B -------------------
        {
            f32x16 acc2[2][2];
            zero_acc(acc2);
            for (int r0 = 0; r0 < F; r0 += 256) {
                f32x16 acc1[2][2];
                zero_acc(acc1);
                const bf16_t* w2p = w2_frag(r0);
                mma_tile256(acc1, A, bufa, bufb, k256_frag(p.w1, r0), kStride256, w2p, (size_t)fs * 512, nl, kg);
                stage_tile256<true, true>(B, acc1, b1s + r0, wave, nl, kg);
                __syncthreads();  // the whole 64 x 256 hidden chunk is in B
                const bf16_t* next = r0 + 256 < F ? k256_frag(p.w1, r0 + 256) : wv_f;
                mma_tile256(acc2, B, bufa, bufb, w2p, (size_t)fs * 512, next, kStride256, nl, kg);
                __syncthreads();  // everyone is done reading the chunk before it is overwritten
            }
            stage_tile256<true, false>(B, acc2, b2s, wave, nl, kg);
        }
        __syncthreads();

        // ---- src' = LayerNorm2(B + A) -> A and, in whole rows, to memory --------------------------------------------------------------
        {
            const f32x4 g = *reinterpret_cast<const f32x4*>(g2s + 4 * lane), b = *reinterpret_cast<const f32x4*>(e2s + 4 * lane);
#pragma unroll
            for (int r = 0; r < kRowsPerWave; ++r) {
                float v[4], t[4], y[4];
                unpack4<bf16_t>(*reinterpret_cast<const u32x2*>(B + (wrow + r) * kTileStride + lane * 8), v);
                unpack4<bf16_t>(*reinterpret_cast<const u32x2*>(A + (wrow + r) * kTileStride + lane * 8), t);
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] += t[i];
                layernorm_row(v, g, b, p.eps2, y);
                const u32x2 o = pack4<bf16_t>(y);
                *reinterpret_cast<u32x2*>(A + (wrow + r) * kTileStride + lane * 8) = o;
                const long row = row0 + wrow + r;
                if (row < p.M) *reinterpret_cast<u32x2*>(p.out + row * 256 + 4 * lane) = o;
            }
        }
        __syncthreads();  // src' is in A; B is free

        if constexpr (PROJ) {
            // ---- the next layer's value: mask(A Wv^T + bv), head-major; the pos rows are warmed before the product ------------------------
            const unsigned warm = warm_rows(p.pos, row0 + wrow, p.M, lane);
            f32x16 acc[2][2];
            init_acc_bias(acc, bvs + 64 * wave, kg);
            mma_tile256(acc, A, bufa, bufb, wv_f, kStride256, wq_f, kStride256, nl, kg);
            stage_tile256<false, false>(B, acc, nullptr, wave, nl, kg);
            __syncthreads();  // the value rows are in B and nobody reads A any more
            retire(warm);
            unsigned char masked[kTileRows / 16];  // first, so that the stores below wait for these bytes alone
#pragma unroll
            for (int pass = 0; pass < kTileRows / 16; ++pass) {
                long row = row0 + pass * 16 + (lane >> 2);
                row = row < p.M ? row : p.M - 1;
                masked[pass] = p.mask != nullptr ? p.mask[row] : (unsigned char)0;
            }
            u32x2 posr[kRowsPerWave];
            load_rows(posr, p.pos, row0 + wrow, p.M, lane);
            // the tile starts at token sp0 of batch item nb0: a 32-bit division per row instead of a 64-bit one
            const long nb0 = row0 / p.S;
            const int sp0 = (int)(row0 - nb0 * p.S);
            // per head (32 columns = 64 B per row): 4 lanes x 16 B per row, 16 consecutive rows = 1 KB per store instruction
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
#pragma unroll
                for (int pass = 0; pass < kTileRows / 16; ++pass) {
                    const int row = pass * 16 + (lane >> 2);
                    const long grow = row0 + row;
                    if (grow < p.M) {
                        u32x4 v = *reinterpret_cast<const u32x4*>(B + row * kTileStride + (64 * wave + 32 * hh) * 2 + (lane & 3) * 16);
                        if (masked[pass]) v = u32x4{0u, 0u, 0u, 0u};
                        const unsigned over = (unsigned)(sp0 + row) / (unsigned)p.S;
                        const long nb = nb0 + over, sp = sp0 + row - (long)over * p.S;
                        const int head = 2 * wave + hh;
                        *reinterpret_cast<u32x4*>(p.value + ((nb * kHeads + head) * p.S + sp) * 32 + (lane & 3) * 8) = v;
                    }
                }
            }
            // ---- the next layer's query, in place: A = bf16(A + pos), the sum taken on the rounded src' ---------------------------------
#pragma unroll
            for (int r = 0; r < kRowsPerWave; ++r) {
                float y[4], t[4];
                unpack4<bf16_t>(*reinterpret_cast<const u32x2*>(A + (wrow + r) * kTileStride + lane * 8), y);
                unpack4<bf16_t>(posr[r], t);
#pragma unroll
                for (int i = 0; i < 4; ++i) y[i] += t[i];
                *reinterpret_cast<u32x2*>(A + (wrow + r) * kTileStride + lane * 8) = pack4<bf16_t>(y);
            }
            __syncthreads();  // the query is in A; the value rows have left B

            // ---- offsets + logits: A Wq^T + bq over the merged 384 columns, 64 per wave: columns 0-255, then 256-383 (two waves) ------
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
                if (pass == 1 && wave >= 2) break;  // wave-uniform; no workgroup barrier below
                const int col0 = 256 * pass;
                init_acc_bias(acc, bqs + col0 + 64 * wave, kg);
                const bf16_t* const wq_p = wq_f + (size_t)pass * 8 * kStride256;
                const bf16_t* next = (pass == 0 && wave < 2) ? wq_f + 8 * kStride256 : nullptr;
                mma_tile256(acc, A, bufa, bufb, wq_p, kStride256, next, kStride256, nl, kg);
                wave_lds_fence();  // pass 1: the read-back of pass 0 is done
                stage_tile256<false, false>(B, acc, nullptr, wave, nl, kg);
                wave_lds_fence();
                // rows leave as whole 128-byte lines: 8 lanes x 16 B per row, 8 rows per store instruction
#pragma unroll
                for (int k = 0; k < kTileRows / 8; ++k) {
                    const int row = k * 8 + (lane >> 3);
                    const long grow = row0 + row;
                    const u32x4 v = *reinterpret_cast<const u32x4*>(B + row * kTileStride + (64 * wave) * 2 + (lane & 7) * 16);
                    if (grow < p.M) *reinterpret_cast<u32x4*>(p.both + grow * kQueryCols + col0 + 64 * wave + (lane & 7) * 8) = v;
                }
            }
            __syncthreads();  // A and B are rewritten by the next tile
        }
    }
}

template <bool TAIL, bool PROJ>
int launch_block(const EncBlockArgs& a, size_t lds, hipStream_t stream) {
    int dev = 0, cus = 0;  // persistent: two workgroups per CU
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
        return fail(ALO_ERR_LAUNCH, "alo_encoder_block: cannot read the device's compute unit count");
    const int gx = a.tiles < 2 * cus ? a.tiles : 2 * cus;
    void* args[] = {const_cast<EncBlockArgs*>(&a)};
    return launch<encoder_block_kernel<TAIL, PROJ>>(gx, 256, lds, stream, "alo_encoder_block", args);
}

// ---- the decoder's two row-local chains (ALO_BLOCK_NO_FFN, ALO_BLOCK_DECODER_NEXT of alo_encoder_block.h) ----------------------------
//
//   chain A (NEXT = false), between self-attention and the MSDA launch:
//       tgt1 = LayerNorm1(attn_out Wo^T + bo + tgt) -> out,   offsets_logits = (tgt1 + pos) Wq^T + bq over 384 columns
//   chain B (NEXT = true), between the MSDA launch and the next layer's self-attention:
//       tgt2 = LayerNorm1(attn_out Wo^T + bo + tgt1),  out = LayerNorm2(ffn(tgt2) + tgt2),
//       value = out Wv^T + bv ROW-major (rows, 256),   qk = (out + pos) Wq^T + bq over 512 columns
//
// The decoder forms have their OWN copy of encoder_block_kernel's loop instead of more template parameters on it: the encoder's four
// instantiations keep their device code instruction for instruction (tools/isa_diff.py), and the decoder's shape asks for another
// schedule.  A decoder has a few thousand rows (8 x 300): at 64 rows per workgroup 38 of 256 CUs have work, and a workgroup's time is
// its serial walk through the weights (1 MB and more in chain B), one L2 round trip per two k-steps.  So
//   * ROWS = 32 when the 64-row tiles would not fill the chip (the host decides): a wave then owns ONE 32-row MFMA tile of its 64
//     columns, twice as many CUs are busy and each carries half the matrix work.  The MFMA is the same v_mfma_f32_32x32x16_bf16 with
//     the accumulators started from the bias and k ascending, and a lane of it owns one row: a row's bits cannot depend on ROWS;
//   * the weights are prefetched KB = 8 k-steps deep at ROWS = 32 (two register buffers of half a 256-deep contraction each, 128
//     VGPRs) and 4 deep at ROWS = 64 (where the FFN holds 128 accumulators): one round trip per half contraction.  A whole
//     contraction per buffer (KB = 16, 256 + 234 registers) was slower: 34.5 against 31.9 us for chain B (docs/experiments.md);
//   * the barriers wait for LDS alone (lds_barrier): __syncthreads also waits for the global loads in flight, which here are the
//     prefetched weights of the NEXT product; for the same reason the weights come through global, not flat, loads (dec_load_batch);
//   * the residual and pos rows are parked in LDS with the tile itself (one exposed round trip per tile for all three) instead of
//     being warmed and loaded after a product: at one workgroup per CU the LDS is there (4 tiles of ROWS x 528 bytes).
// Rounding points, operand roles and summation orders are the encoder kernel's, i.e. those of alo_linear_shortk, alo_add_layernorm
// (with pos) and alo_ffn256.
struct DecBlockArgs {
    const bf16_t *attn, *wo, *bo, *g1, *be1;
    const bf16_t *res, *pos;
    const bf16_t *w1, *b1, *w2, *b2, *g2, *be2;
    const bf16_t *wv, *bv, *wq, *bq;
    bf16_t *out, *value, *both;
    long M;
    int F, tiles;
    float eps1, eps2;
};

// waits for this wave's LDS traffic only, then the workgroup barrier; the compiler keeps memory operations on their side of it
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <int ROWS>
__device__ __forceinline__ void fetch_rows256(u32x4 (&v)[ROWS / 8], const bf16_t* X, long row0, long M, int tid) {
#pragma unroll
    for (int j = 0; j < ROWS / 8; ++j) {
        const int p = tid + 256 * j;
        long row = row0 + (p >> 5);
        row = row < M ? row : M - 1;  // rows past the end are read from the last row and never stored
        v[j] = *reinterpret_cast<const u32x4*>(X + row * 256 + (p & 31) * 8);
    }
}
template <int ROWS>
__device__ __forceinline__ void park_rows256(unsigned char* lds, const u32x4 (&v)[ROWS / 8], int tid) {
#pragma unroll
    for (int j = 0; j < ROWS / 8; ++j) {
        const int p = tid + 256 * j;
        *reinterpret_cast<u32x4*>(lds + (p >> 5) * kTileStride + (p & 31) * 16) = v[j];
    }
}

template <int RT>
__device__ __forceinline__ void dec_init_bias(f32x16 (&acc)[RT][2], const float* bias64, int kg) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 bb = *reinterpret_cast<const f32x4*>(bias64 + 32 * t + 8 * q + 4 * kg);
#pragma unroll
            for (int a = 0; a < RT; ++a)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[a][t][4 * q + i] = bb[i];
        }
}

// load_batch (mfma_tile.hpp) through a pointer in the GLOBAL address space.  Behind per_tile's opaque copy the compiler no longer knows
// where a weight pointer points and emits flat loads; those count as LDS traffic as well, so every wait for an LDS read and every
// lds_barrier would also wait for the prefetched weights.
template <int KB>
__device__ __forceinline__ void dec_load_batch(u32x4 (&buf)[2][KB], const bf16_t* frag0, size_t tile_stride, int batch) {
    typedef const u32x4 __attribute__((address_space(1))) * global_u32x4;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < KB; ++j)
            buf[t][j] = *(global_u32x4)(uintptr_t)(frag0 + t * tile_stride + (size_t)(KB * batch + j) * 512);
    __builtin_amdgcn_sched_barrier(0);
}

// acc[row tile][column tile] += A (the LDS tile, k-steps KB * batch ..) x the batch's weight fragments
template <int RT, int KB>
__device__ __forceinline__ void dec_mma_batch(f32x16 (&acc)[RT][2], const unsigned char* a_lds, const u32x4 (&buf)[2][KB], int batch,
                                              int nl, int kg) {
#pragma unroll
    for (int j = 0; j < KB; ++j) {
        const int s = KB * batch + j;
        u32x4 af[RT];
#pragma unroll
        for (int a = 0; a < RT; ++a) af[a] = *reinterpret_cast<const u32x4*>(a_lds + (32 * a + nl) * kTileStride + (16 * s + 8 * kg) * 2);
#pragma unroll
        for (int a = 0; a < RT; ++a) {
            acc[a][0] = mfma_32x32x16<bf16_t>(buf[0][j], af[a], acc[a][0]);
            acc[a][1] = mfma_32x32x16<bf16_t>(buf[1][j], af[a], acc[a][1]);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
}
// One whole 256-deep contraction (mma_tile256 with KB k-steps per batch).  bufa already holds batch 0; on return it holds batch 0 of
// `next` when next != nullptr.
template <int RT, int KB>
__device__ __forceinline__ void dec_product(f32x16 (&acc)[RT][2], const unsigned char* a_lds, u32x4 (&bufa)[2][KB], u32x4 (&bufb)[2][KB],
                                            const bf16_t* w, size_t tile_stride, const bf16_t* next, size_t next_stride, int nl, int kg) {
    constexpr int kBatches = 16 / KB;
    static_assert(kBatches % 2 == 0, "the two buffers take turns inside a product");
#pragma unroll
    for (int bt = 0; bt < kBatches; bt += 2) {
        dec_load_batch(bufb, w, tile_stride, bt + 1);
        dec_mma_batch<RT, KB>(acc, a_lds, bufa, bt, nl, kg);
        if (bt + 2 < kBatches) dec_load_batch(bufa, w, tile_stride, bt + 2);
        else if (next != nullptr) dec_load_batch(bufa, next, next_stride, 0);
        dec_mma_batch<RT, KB>(acc, a_lds, bufb, bt + 1, nl, kg);
    }
}

// this wave's 64 staged columns of ROWS rows -> Y[(row0 + row) * ld + col ..] as whole 128-byte lines: 8 lanes x 16 B per row
template <int ROWS>
__device__ __forceinline__ void store_wave_cols(bf16_t* Y, int ld, int col, const unsigned char* B, int wave, long row0, long M, int lane) {
#pragma unroll
    for (int k = 0; k < ROWS / 8; ++k) {
        const int row = k * 8 + (lane >> 3);
        const long grow = row0 + row;
        const u32x4 v = *reinterpret_cast<const u32x4*>(B + row * kTileStride + (64 * wave) * 2 + (lane & 7) * 16);
        if (grow < M) *reinterpret_cast<u32x4*>(Y + grow * ld + col + (lane & 7) * 8) = v;
    }
}

template <int ROWS, bool NEXT>
__global__ void __launch_bounds__(256)
decoder_block_kernel(const DecBlockArgs p) {
    constexpr int RT = ROWS / 32;            // 32-row MFMA tiles per wave
    constexpr int KB = ROWS == 32 ? 8 : 4;   // k-steps per weight batch (16: a buffer would hold a whole product's weights)
    constexpr int kRpw = ROWS / 4;           // rows a wave normalises
    constexpr int kQc = NEXT ? 512 : kQueryCols;
    constexpr int kTile = ROWS * kTileStride;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const A = smem;              // the tile every product reads
    unsigned char* const B = smem + kTile;      // hidden chunk / every product's bf16 result
    unsigned char* const R = smem + 2 * kTile;  // LayerNorm1's residual rows
    unsigned char* const P = smem + 3 * kTile;  // pos rows
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nl = lane & 31, kg = lane >> 5;
    const int F = NEXT ? p.F : 0;

    float* const bos = reinterpret_cast<float*>(smem + 4 * kTile);
    float* const g1s = bos + 256;
    float* const e1s = g1s + 256;
    float* const bqs = e1s + 256;
    float* const bvs = bqs + kQc;   // NEXT only from here on
    float* const b2s = bvs + 256;
    float* const g2s = b2s + 256;
    float* const e2s = g2s + 256;
    float* const b1s = e2s + 256;
    bos[tid] = bf16_to_f32(p.bo[tid].bits);
    g1s[tid] = bf16_to_f32(p.g1[tid].bits);
    e1s[tid] = bf16_to_f32(p.be1[tid].bits);
    for (int i = tid; i < kQc; i += 256) bqs[i] = bf16_to_f32(p.bq[i].bits);
    if constexpr (NEXT) {
        bvs[tid] = bf16_to_f32(p.bv[tid].bits);
        b2s[tid] = bf16_to_f32(p.b2[tid].bits);
        g2s[tid] = bf16_to_f32(p.g2[tid].bits);
        e2s[tid] = bf16_to_f32(p.be2[tid].bits);
        for (int i = tid; i < F; i += 256) b1s[i] = bf16_to_f32(p.b1[i].bits);
    }

    const int fs = F / 16;
    auto k256_frag = [&](const bf16_t* W, int col0) { return W + ((size_t)((col0 + 64 * wave) / 32) * 16 * 64 + lane) * 8; };
    auto w2_frag = [&](int r0) { return p.w2 + (((size_t)(2 * wave) * fs + r0 / 16) * 64 + lane) * 8; };
    constexpr size_t kStride256 = (size_t)16 * 512;
    const int wrow = kRpw * wave;

    for (int tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
        const long row0 = (long)tile * ROWS;
        // opaque per-tile copies (per_tile above): otherwise every weight load's address pair is computed ahead of the tile loop
        const bf16_t* const wo_f = per_tile(k256_frag(p.wo, 0));
        const bf16_t* const wq_f = per_tile(k256_frag(p.wq, 0));
        u32x4 bufa[2][KB], bufb[2][KB];
        {
            u32x4 xa[ROWS / 8], xr[ROWS / 8], xp[ROWS / 8];
            fetch_rows256<ROWS>(xa, p.attn, row0, p.M, tid);
            fetch_rows256<ROWS>(xr, p.res, row0, p.M, tid);
            fetch_rows256<ROWS>(xp, p.pos, row0, p.M, tid);
            dec_load_batch(bufa, wo_f, kStride256, 0);
            park_rows256<ROWS>(A, xa, tid);
            park_rows256<ROWS>(R, xr, tid);
            park_rows256<ROWS>(P, xp, tid);
        }
        lds_barrier();  // the three tiles (and, first time round, the tables) are in LDS

        f32x16 acc[RT][2];
        // ---- B = attn_out Wo^T + bo ------------------------------------------------------------------------------------------------------
        dec_init_bias<RT>(acc, bos + 64 * wave, kg);
        dec_product<RT, KB>(acc, A, bufa, bufb, wo_f, kStride256, NEXT ? k256_frag(p.w1, 0) : wq_f, kStride256, nl, kg);
        stage_quads<bf16_t, false>(B, kTileStride, acc, nullptr, false, nl, 64 * wave, kg);
        lds_barrier();  // the projected rows are in B and nobody reads A any more

        // ---- A = LayerNorm1(B + R); chain A: that is `out`, and A = bf16(out + pos), the sum taken on the rounded value --------------
        {
            const f32x4 g = *reinterpret_cast<const f32x4*>(g1s + 4 * lane), b = *reinterpret_cast<const f32x4*>(e1s + 4 * lane);
#pragma unroll
            for (int r = 0; r < kRpw; ++r) {
                float v[4], t[4], y[4];
                unpack4<bf16_t>(*reinterpret_cast<const u32x2*>(B + (wrow + r) * kTileStride + lane * 8), v);
                unpack4<bf16_t>(*reinterpret_cast<const u32x2*>(R + (wrow + r) * kTileStride + lane * 8), t);
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] += t[i];
                layernorm_row(v, g, b, p.eps1, y);
                u32x2 o = pack4<bf16_t>(y);
                if constexpr (!NEXT) {
                    const long row = row0 + wrow + r;
                    if (row < p.M) *reinterpret_cast<u32x2*>(p.out + row * 256 + 4 * lane) = o;
                    unpack4<bf16_t>(o, y);
                    unpack4<bf16_t>(*reinterpret_cast<const u32x2*>(P + (wrow + r) * kTileStride + lane * 8), t);
#pragma unroll
                    for (int i = 0; i < 4; ++i) y[i] += t[i];
                    o = pack4<bf16_t>(y);
                }
                *reinterpret_cast<u32x2*>(A + (wrow + r) * kTileStride + lane * 8) = o;
            }
        }
        lds_barrier();  // chain A: the query is in A; chain B: the FFN's x tile

        if constexpr (NEXT) {
            // ---- feed-forward block: ffn256_kernel's arithmetic, the hidden activation 256 units at a time through B -------------------
            const bf16_t* const wv_f = per_tile(k256_frag(p.wv, 0));
            {
                f32x16 acc2[RT][2];
                zero_acc(acc2);
                for (int r0 = 0; r0 < F; r0 += 256) {
                    zero_acc(acc);
                    const bf16_t* w2p = w2_frag(r0);
                    dec_product<RT, KB>(acc, A, bufa, bufb, k256_frag(p.w1, r0), kStride256, w2p, (size_t)fs * 512, nl, kg);
                    stage_quads<bf16_t, true>(B, kTileStride, acc, b1s + r0, true, nl, 64 * wave, kg);
                    lds_barrier();  // the whole hidden chunk is in B
                    const bf16_t* next = r0 + 256 < F ? k256_frag(p.w1, r0 + 256) : wv_f;
                    dec_product<RT, KB>(acc2, B, bufa, bufb, w2p, (size_t)fs * 512, next, kStride256, nl, kg);
                    lds_barrier();  // everyone is done reading the chunk before it is overwritten
                }
                stage_quads<bf16_t, true>(B, kTileStride, acc2, b2s, false, nl, 64 * wave, kg);
            }
            lds_barrier();

            // ---- out = LayerNorm2(B + A) -> A and, in whole rows, to memory ------------------------------------------------------------
            {
                const f32x4 g = *reinterpret_cast<const f32x4*>(g2s + 4 * lane), b = *reinterpret_cast<const f32x4*>(e2s + 4 * lane);
#pragma unroll
                for (int r = 0; r < kRpw; ++r) {
                    float v[4], t[4], y[4];
                    unpack4<bf16_t>(*reinterpret_cast<const u32x2*>(B + (wrow + r) * kTileStride + lane * 8), v);
                    unpack4<bf16_t>(*reinterpret_cast<const u32x2*>(A + (wrow + r) * kTileStride + lane * 8), t);
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] += t[i];
                    layernorm_row(v, g, b, p.eps2, y);
                    const u32x2 o = pack4<bf16_t>(y);
                    *reinterpret_cast<u32x2*>(A + (wrow + r) * kTileStride + lane * 8) = o;
                    const long row = row0 + wrow + r;
                    if (row < p.M) *reinterpret_cast<u32x2*>(p.out + row * 256 + 4 * lane) = o;
                }
            }
            lds_barrier();  // out is in A; B is free

            // ---- the next layer's value, row-major: A Wv^T + bv; a wave stores the 64 columns it staged itself ------------------------
            dec_init_bias<RT>(acc, bvs + 64 * wave, kg);
            dec_product<RT, KB>(acc, A, bufa, bufb, wv_f, kStride256, wq_f, kStride256, nl, kg);
            stage_quads<bf16_t, false>(B, kTileStride, acc, nullptr, false, nl, 64 * wave, kg);
            ALO_WAVE_LDS_ORDER();
            store_wave_cols<ROWS>(p.value, 256, 64 * wave, B, wave, row0, p.M, lane);
            lds_barrier();  // nobody reads A any more
            // ---- the next layer's query, in place: A = bf16(A + pos), the sum taken on the rounded out ---------------------------------
#pragma unroll
            for (int r = 0; r < kRpw; ++r) {
                float y[4], t[4];
                unpack4<bf16_t>(*reinterpret_cast<const u32x2*>(A + (wrow + r) * kTileStride + lane * 8), y);
                unpack4<bf16_t>(*reinterpret_cast<const u32x2*>(P + (wrow + r) * kTileStride + lane * 8), t);
#pragma unroll
                for (int i = 0; i < 4; ++i) y[i] += t[i];
                *reinterpret_cast<u32x2*>(A + (wrow + r) * kTileStride + lane * 8) = pack4<bf16_t>(y);
            }
            lds_barrier();  // the query is in A
        }

        // ---- A Wq^T + bq, 64 columns per wave and pass: columns 0-255, then 256 .. kQc - 1 (chain A: 128 of them, two waves) -------------
        const bool again = NEXT || wave < 2;  // wave-uniform; no workgroup barrier below
        auto q_pass = [&](int pass) {
            const int col0 = 256 * pass;
            dec_init_bias<RT>(acc, bqs + col0 + 64 * wave, kg);
            const bf16_t* const wq_p = wq_f + (size_t)pass * 8 * kStride256;
            const bf16_t* next = (pass == 0 && again) ? wq_f + 8 * kStride256 : nullptr;
            dec_product<RT, KB>(acc, A, bufa, bufb, wq_p, kStride256, next, kStride256, nl, kg);
            ALO_WAVE_LDS_ORDER();  // the read-back of the value / of pass 0 comes first
            stage_quads<bf16_t, false>(B, kTileStride, acc, nullptr, false, nl, 64 * wave, kg);
            ALO_WAVE_LDS_ORDER();
            store_wave_cols<ROWS>(p.both, kQc, col0 + 64 * wave, B, wave, row0, p.M, lane);
        };
        q_pass(0);
        if (again) q_pass(1);
        lds_barrier();  // every tile of LDS is rewritten by the next tile
    }
}

// the LDS frame of decoder_block_kernel<rows, next>: its four tiles and the fp32 tables behind them
constexpr size_t decoder_block_lds(int rows, bool next, int F) {
    return 4 * (size_t)rows * kTileStride + (next ? (size_t)F + 256 * 7 + 512 : 256 * 3 + kQueryCols) * sizeof(float);
}

template <int ROWS, bool NEXT>
int launch_decoder_block(DecBlockArgs& a, int cus, hipStream_t stream) {
    a.tiles = (int)((a.M + ROWS - 1) / ROWS);
    const size_t lds = decoder_block_lds(ROWS, NEXT, a.F);
    ALO_REQUIRE(lds <= (size_t)kLdsLimit, ALO_ERR_UNSUPPORTED, "alo_encoder_block: hidden width %d needs %zu bytes of LDS", a.F, lds);
    const int gx = a.tiles < cus ? a.tiles : cus;  // persistent: one workgroup per CU (its four tiles take most of the LDS at 64 rows)
    void* args[] = {&a};
    return launch<decoder_block_kernel<ROWS, NEXT>>(gx, 256, lds, stream, "alo_encoder_block", args);
}

// the flagged forms of alo_encoder_block: every argument is checked here, by name, before anything is enqueued
int decoder_block(const void* attn_out, const void* wo_packed, const void* bo, const void* norm1_w, const void* norm1_b, const void* src,
                  const void* w1_packed, const void* b1, const void* w2_packed, const void* b2, const void* norm2_w, const void* norm2_b,
                  void* src_out, const void* pos, const void* padding_mask, const void* wv_packed, const void* bv, const void* wq_packed,
                  const void* bq, void* value_hm, void* offsets_logits, int batch, int S, int F, float eps1, float eps2, int dtype,
                  int flags, hipStream_t stream) {
    const char* what = "alo_encoder_block";
    constexpr int kChains = ALO_BLOCK_NO_FFN | ALO_BLOCK_DECODER_NEXT, kTiles = ALO_BLOCK_TILE_32 | ALO_BLOCK_TILE_64;
    ALO_REQUIRE(!(flags & ~(kChains | kTiles)), ALO_ERR_UNSUPPORTED,
                "%s: dtype carries 0x%x above its low byte: ALO_BLOCK_NO_FFN, ALO_BLOCK_DECODER_NEXT, ALO_BLOCK_TILE_32 / _64 or nothing", what,
                flags & ~(kChains | kTiles));
    ALO_REQUIRE((flags & kChains) != kChains, ALO_ERR_INVALID_ARGUMENT,
                "%s: dtype carries both ALO_BLOCK_NO_FFN and ALO_BLOCK_DECODER_NEXT: one chain per call", what);
    ALO_REQUIRE(flags & kChains, ALO_ERR_INVALID_ARGUMENT,
                "%s: dtype carries ALO_BLOCK_TILE_32 / _64 without ALO_BLOCK_NO_FFN or ALO_BLOCK_DECODER_NEXT", what);
    ALO_REQUIRE((flags & kTiles) != kTiles, ALO_ERR_INVALID_ARGUMENT,
                "%s: dtype carries both ALO_BLOCK_TILE_32 and ALO_BLOCK_TILE_64", what);
    const bool next = (flags & ALO_BLOCK_DECODER_NEXT) != 0;
    const char* flag = next ? "ALO_BLOCK_DECODER_NEXT" : "ALO_BLOCK_NO_FFN";
    ALO_REQUIRE(dtype == ALO_BF16, ALO_ERR_UNSUPPORTED, "%s: %s is bf16 only (dtype %d)", what, flag, dtype);
    const struct { const void* p; const char* name; bool wanted; } ptrs[] = {
        {attn_out, "attn_out", true}, {wo_packed, "wo_packed", true}, {bo, "bo", true}, {norm1_w, "norm1_w", true},
        {norm1_b, "norm1_b", true}, {src, "src", true}, {w1_packed, "w1_packed", next}, {b1, "b1", next}, {w2_packed, "w2_packed", next},
        {b2, "b2", next}, {norm2_w, "norm2_w", next}, {norm2_b, "norm2_b", next}, {src_out, "src_out", true}, {pos, "pos", true},
        {padding_mask, "padding_mask", false}, {wv_packed, "wv_packed", next}, {bv, "bv", next}, {wq_packed, "wq_packed", true},
        {bq, "bq", true}, {value_hm, "value_hm", next}, {offsets_logits, "offsets_logits", true}};
    for (const auto& a : ptrs) {
        ALO_REQUIRE(!a.wanted || a.p, ALO_ERR_INVALID_ARGUMENT, "%s: %s is NULL, %s needs it", what, a.name, flag);
        ALO_REQUIRE(a.wanted || !a.p, ALO_ERR_INVALID_ARGUMENT, "%s: %s must be NULL with %s", what, a.name, flag);
    }
    ALO_REQUIRE(batch > 0 && S > 0 && (!next || (F > 0 && F % 256 == 0)), ALO_ERR_INVALID_ARGUMENT,
                "%s: batch, S must be positive and the hidden width a positive multiple of 256 (batch=%d S=%d F=%d)", what, batch, S, F);
    ALO_REQUIRE(aligned16(attn_out, wo_packed, src, w1_packed, w2_packed, src_out, pos, wv_packed, wq_packed, value_hm, offsets_logits),
                ALO_ERR_INVALID_ARGUMENT, "%s: pointers must be 16-byte aligned", what);
    const size_t rows = (size_t)batch * S, qbytes = next ? 1024 : 2 * kQueryCols;
    const struct { const void* p; size_t bytes; bool out; } spans[] = {
        {attn_out, rows * 512, false}, {src, rows * 512, false}, {pos, rows * 512, false},
        {src_out, rows * 512, true}, {value_hm, rows * 512, true}, {offsets_logits, rows * qbytes, true}};
    for (const auto& o : spans)
        for (const auto& i : spans)
            ALO_REQUIRE(!o.out || &o == &i || !o.p || !i.p || (const char*)o.p + o.bytes <= (const char*)i.p ||
                            (const char*)i.p + i.bytes <= (const char*)o.p,
                        ALO_ERR_INVALID_ARGUMENT, "%s: an output overlaps an input or another output", what);
    DecBlockArgs a;
    a.attn = (const bf16_t*)attn_out; a.wo = (const bf16_t*)wo_packed; a.bo = (const bf16_t*)bo;
    a.g1 = (const bf16_t*)norm1_w; a.be1 = (const bf16_t*)norm1_b; a.res = (const bf16_t*)src; a.pos = (const bf16_t*)pos;
    a.w1 = (const bf16_t*)w1_packed; a.b1 = (const bf16_t*)b1; a.w2 = (const bf16_t*)w2_packed; a.b2 = (const bf16_t*)b2;
    a.g2 = (const bf16_t*)norm2_w; a.be2 = (const bf16_t*)norm2_b; a.wv = (const bf16_t*)wv_packed; a.bv = (const bf16_t*)bv;
    a.wq = (const bf16_t*)wq_packed; a.bq = (const bf16_t*)bq;
    a.out = (bf16_t*)src_out; a.value = (bf16_t*)value_hm; a.both = (bf16_t*)offsets_logits;
    a.M = (long)rows; a.F = next ? F : 0; a.tiles = 0; a.eps1 = eps1; a.eps2 = eps2;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
        return fail(ALO_ERR_LAUNCH, "%s: cannot read the device's compute unit count", what);
    // few rows: 32-row tiles while the 64-row ones would leave compute units without work; and whenever the 64-row frame does not
    // fit (chain B with a hidden width above 4864), since a row's bits do not depend on the height.  A forced height is taken as it
    // is and refused by launch_decoder_block when its frame does not fit.
    const bool rows32 = (flags & kTiles) ? (flags & ALO_BLOCK_TILE_32) != 0
                                         : (long)((rows + 63) / 64) < (long)cus || decoder_block_lds(64, next, a.F) > (size_t)kLdsLimit;
    if (next) return rows32 ? launch_decoder_block<32, true>(a, cus, stream) : launch_decoder_block<64, true>(a, cus, stream);
    return rows32 ? launch_decoder_block<32, false>(a, cus, stream) : launch_decoder_block<64, false>(a, cus, stream);
}

// ALO_BLOCK_ATTENTION (and ALO_BLOCK_PACKED_QK): dense attention on the entry point's pointers, checked by name; the kernel is
// attention.hip's
int attention_flagged(const void* attn_out, const void* wo_packed, const void* bo, const void* norm1_w, const void* norm1_b, const void* src,
                      const void* w1_packed, const void* b1, const void* w2_packed, const void* b2, const void* norm2_w,
                      const void* norm2_b, void* src_out, const void* pos, const void* padding_mask, const void* wv_packed, const void* bv,
                      const void* wq_packed, const void* bq, void* value_hm, void* offsets_logits, int batch, int S, int F, float eps1,
                      float eps2, int dtype, int flags, hipStream_t stream) {
    const char* what = "alo_encoder_block";
    constexpr int kAttn = ALO_BLOCK_ATTENTION | ALO_BLOCK_PACKED_QK;
    constexpr int kOthers = ALO_BLOCK_NO_FFN | ALO_BLOCK_DECODER_NEXT | ALO_BLOCK_TILE_32 | ALO_BLOCK_TILE_64;
    ALO_REQUIRE(!(flags & ~(kAttn | kOthers)), ALO_ERR_UNSUPPORTED,
                "%s: dtype carries 0x%x above its low byte: ALO_BLOCK_NO_FFN, ALO_BLOCK_DECODER_NEXT, ALO_BLOCK_TILE_32 / _64, "
                "ALO_BLOCK_ATTENTION (with ALO_BLOCK_PACKED_QK) or nothing", what, flags & ~(kAttn | kOthers));
    ALO_REQUIRE(flags & ALO_BLOCK_ATTENTION, ALO_ERR_INVALID_ARGUMENT, "%s: dtype carries ALO_BLOCK_PACKED_QK without ALO_BLOCK_ATTENTION",
                what);
    ALO_REQUIRE(!(flags & kOthers), ALO_ERR_INVALID_ARGUMENT,
                "%s: dtype carries ALO_BLOCK_ATTENTION together with a chain or tile flag (0x%x): attention is a call of its own", what,
                flags & kOthers);
    const bool packed = (flags & ALO_BLOCK_PACKED_QK) != 0;
    const char* flag = "ALO_BLOCK_ATTENTION";
    ALO_REQUIRE(dtype == ALO_BF16 || dtype == ALO_F16 || dtype == ALO_F32, ALO_ERR_UNSUPPORTED,
                "%s: %s takes ALO_BF16, ALO_F16 or ALO_F32 (dtype %d)", what, flag, dtype);
    const struct { const void* p; const char* name; bool wanted; } ptrs[] = {
        {attn_out, "attn_out", true}, {wo_packed, "wo_packed", false}, {bo, "bo", false}, {norm1_w, "norm1_w", false},
        {norm1_b, "norm1_b", false}, {src, "src", true}, {w1_packed, "w1_packed", false}, {b1, "b1", false}, {w2_packed, "w2_packed", false},
        {b2, "b2", false}, {norm2_w, "norm2_w", false}, {norm2_b, "norm2_b", false}, {src_out, "src_out", true}, {pos, "pos", true},
        {wv_packed, "wv_packed", false}, {bv, "bv", false}, {wq_packed, "wq_packed", false}, {bq, "bq", false},
        {value_hm, "value_hm", false}, {offsets_logits, "offsets_logits", false}};   // padding_mask: either way
    for (const auto& a : ptrs) {
        ALO_REQUIRE(!a.wanted || a.p, ALO_ERR_INVALID_ARGUMENT, "%s: %s is NULL, %s needs it", what, a.name, flag);
        ALO_REQUIRE(a.wanted || !a.p, ALO_ERR_INVALID_ARGUMENT, "%s: %s must be NULL with %s", what, a.name, flag);
    }
    ALO_REQUIRE(batch > 0 && S > 0 && F > 0, ALO_ERR_INVALID_ARGUMENT,
                "%s: batch, S (queries) and F (keys) must be positive (batch=%d S=%d F=%d)", what, batch, S, F);
    ALO_REQUIRE(eps1 > 0.f, ALO_ERR_INVALID_ARGUMENT, "%s: eps1 is the softmax scale with %s and must be positive (%g)", what, flag,
                (double)eps1);   // also refuses NaN
    ALO_REQUIRE(eps2 == 0.f, ALO_ERR_INVALID_ARGUMENT, "%s: eps2 must be 0 with %s (%g)", what, flag, (double)eps2);
    const size_t es = dtype == ALO_F32 ? 4 : 2, pitch = packed ? 512 : 256;
    ALO_REQUIRE(!packed || F == S, ALO_ERR_INVALID_ARGUMENT, "%s: ALO_BLOCK_PACKED_QK needs F == S (S=%d F=%d)", what, S, F);
    ALO_REQUIRE(!packed || (const char*)pos == (const char*)src + 256 * es, ALO_ERR_INVALID_ARGUMENT,
                "%s: ALO_BLOCK_PACKED_QK needs pos == src + 256 elements (the halves of one (rows, 512) matrix)", what);
    ALO_REQUIRE(aligned16(src, pos, attn_out, src_out), ALO_ERR_INVALID_ARGUMENT, "%s: pointers must be 16-byte aligned", what);
    // the bytes each operand spans: a packed q or k ends 256 elements into its last row
    const size_t qrows = (size_t)batch * S, krows = (size_t)batch * F;
    const size_t qbytes = ((qrows - 1) * pitch + 256) * es, kbytes = ((krows - 1) * pitch + 256) * es, vbytes = krows * 256 * es,
                 obytes = qrows * 256 * es;
    constexpr size_t kSlabLimit = (size_t)1 << 31;
    ALO_REQUIRE(qbytes < kSlabLimit && kbytes < kSlabLimit && vbytes < kSlabLimit && obytes < kSlabLimit, ALO_ERR_UNSUPPORTED,
                "%s: %s: q, k, v and out must each be below 2 GiB (batch=%d S=%d F=%d)", what, flag, batch, S, F);
    const struct { const void* p; size_t bytes; } ins[] = {{src, qbytes}, {pos, kbytes}, {attn_out, vbytes}, {padding_mask, krows}};
    for (const auto& i : ins)
        ALO_REQUIRE(!i.p || (const char*)src_out + obytes <= (const char*)i.p || (const char*)i.p + i.bytes <= (const char*)src_out,
                    ALO_ERR_INVALID_ARGUMENT, "%s: src_out (the attention output) overlaps an input", what);
    return attention_block(src, pos, attn_out, padding_mask, src_out, batch, S, F, (int)pitch, eps1, dtype, stream, what);
}

}  // namespace
}  // namespace alo

using namespace alo;

extern "C" int alo_encoder_block(const void* attn_out, const void* wo_packed, const void* bo, const void* norm1_w, const void* norm1_b,
                                 const void* src, const void* w1_packed, const void* b1, const void* w2_packed, const void* b2,
                                 const void* norm2_w, const void* norm2_b, void* src_out, const void* pos, const void* padding_mask,
                                 const void* wv_packed, const void* bv, const void* wq_packed, const void* bq, void* value_hm,
                                 void* offsets_logits, int batch, int S, int F, float eps1, float eps2, int dtype, void* stream) {
    const char* what = "alo_encoder_block";
    // ALO_BLOCK_* ride above the dtype's low byte (a negative dtype is no flagged one): dense attention, the decoder's chains
    if (dtype > 0 && (dtype & (ALO_BLOCK_ATTENTION | ALO_BLOCK_PACKED_QK)))
        return attention_flagged(attn_out, wo_packed, bo, norm1_w, norm1_b, src, w1_packed, b1, w2_packed, b2, norm2_w, norm2_b, src_out, pos,
                                 padding_mask, wv_packed, bv, wq_packed, bq, value_hm, offsets_logits, batch, S, F, eps1, eps2,
                                 dtype & 0xff, dtype & ~0xff, static_cast<hipStream_t>(stream));
    if (dtype > 0 && (dtype & ~0xff))
        return decoder_block(attn_out, wo_packed, bo, norm1_w, norm1_b, src, w1_packed, b1, w2_packed, b2, norm2_w, norm2_b, src_out, pos,
                             padding_mask, wv_packed, bv, wq_packed, bq, value_hm, offsets_logits, batch, S, F, eps1, eps2, dtype & 0xff,
                             dtype & ~0xff, static_cast<hipStream_t>(stream));
    ALO_REQUIRE(src && w1_packed && b1 && w2_packed && b2 && norm2_w && norm2_b && src_out, ALO_ERR_INVALID_ARGUMENT,
                "%s: null pointer argument", what);
    const bool tail = attn_out || wo_packed || bo || norm1_w || norm1_b;
    ALO_REQUIRE(!tail || (attn_out && wo_packed && bo && norm1_w && norm1_b), ALO_ERR_INVALID_ARGUMENT,
                "%s: null pointer argument (attn_out, wo_packed, bo, norm1_w and norm1_b go together)", what);
    const bool proj = pos || wv_packed || bv || wq_packed || bq || value_hm || offsets_logits;
    ALO_REQUIRE(!proj || (pos && wv_packed && bv && wq_packed && bq && value_hm && offsets_logits), ALO_ERR_INVALID_ARGUMENT,
                "%s: null pointer argument (pos, wv_packed, bv, wq_packed, bq, value_hm and offsets_logits go together)", what);
    ALO_REQUIRE(proj || !padding_mask, ALO_ERR_INVALID_ARGUMENT, "%s: padding_mask without the projections it applies to", what);
    ALO_REQUIRE(batch > 0 && S > 0 && F > 0 && F % 256 == 0, ALO_ERR_INVALID_ARGUMENT,
                "%s: batch, S must be positive and the hidden width a positive multiple of 256 (batch=%d S=%d F=%d)", what, batch, S, F);
    ALO_REQUIRE(dtype == ALO_BF16, ALO_ERR_UNSUPPORTED, "%s: bf16 only (dtype %d)", what, dtype);
    ALO_REQUIRE(aligned16(attn_out, wo_packed, src, w1_packed, w2_packed, src_out, pos, wv_packed, wq_packed, value_hm, offsets_logits),
                ALO_ERR_INVALID_ARGUMENT, "%s: pointers must be 16-byte aligned", what);
    // a tile's outputs are written while other tiles' inputs are still to be read: no output may overlap an input or another output
    const size_t rows = (size_t)batch * S;
    const struct { const void* p; size_t bytes; bool out; } spans[] = {
        {attn_out, rows * 512, false}, {src, rows * 512, false}, {pos, rows * 512, false}, {padding_mask, rows, false},
        {src_out, rows * 512, true}, {value_hm, rows * 512, true}, {offsets_logits, rows * 768, true}};
    for (const auto& o : spans)
        for (const auto& i : spans)
            ALO_REQUIRE(!o.out || &o == &i || !o.p || !i.p || (const char*)o.p + o.bytes <= (const char*)i.p ||
                            (const char*)i.p + i.bytes <= (const char*)o.p,
                        ALO_ERR_INVALID_ARGUMENT, "%s: an output overlaps an input or another output", what);
    EncBlockArgs a;
    a.attn = (const bf16_t*)attn_out; a.wo = (const bf16_t*)wo_packed; a.bo = (const bf16_t*)bo;
    a.g1 = (const bf16_t*)norm1_w; a.be1 = (const bf16_t*)norm1_b;
    a.src = (const bf16_t*)src; a.w1 = (const bf16_t*)w1_packed; a.b1 = (const bf16_t*)b1; a.w2 = (const bf16_t*)w2_packed;
    a.b2 = (const bf16_t*)b2; a.g2 = (const bf16_t*)norm2_w; a.be2 = (const bf16_t*)norm2_b;
    a.out = (bf16_t*)src_out; a.pos = (const bf16_t*)pos; a.mask = (const unsigned char*)padding_mask;
    a.wv = (const bf16_t*)wv_packed; a.bv = (const bf16_t*)bv; a.wq = (const bf16_t*)wq_packed; a.bq = (const bf16_t*)bq;
    a.value = (bf16_t*)value_hm; a.both = (bf16_t*)offsets_logits;
    a.M = (long)batch * S; a.S = S; a.F = F; a.tiles = (int)((a.M + kTileRows - 1) / kTileRows);
    a.eps1 = eps1; a.eps2 = eps2;
    const size_t lds = 2 * kTileRows * kTileStride + ((size_t)F + kTables) * sizeof(float);
    ALO_REQUIRE(lds <= (size_t)kLdsLimit, ALO_ERR_UNSUPPORTED, "%s: hidden width %d needs %zu bytes of LDS", what, F, lds);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (tail) return proj ? launch_block<true, true>(a, lds, st) : launch_block<true, false>(a, lds, st);
    return proj ? launch_block<false, true>(a, lds, st) : launch_block<false, false>(a, lds, st);
}
