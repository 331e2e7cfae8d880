// Dense multi-head attention with a key padding mask in one kernel (include/alo_encoder_block.h, ALO_BLOCK_ATTENTION):
//     out[b, i, 32 h + d] = sum_j softmax_j(q[b, i, h] . k[b, j, h] * scale + mask[b, j]) v[b, j, 32 h + d]      8 heads of 32 channels
// One wave owns 32 queries of one (batch, head) and walks the keys in tiles of 32 with the online softmax; a workgroup is 1, 2 or 4
// such waves on consecutive query blocks, sharing the K / V tiles in LDS (two buffers: the next tile's global loads are in flight
// during the current tile's math, one barrier per tile).
//   * first product swapped: S^T = K Q^T, so a lane holds 16 keys of ONE query (its accumulator column) and the lane 32 away the
//     other 16: the running max needs one exchange between the halves, the running sum and the rescale of O none at all (each half
//     keeps the sum over its own keys, the two are added once after the last tile).
//   * second product O^T += V^T P takes the converted accumulator as its B operand without leaving the registers; the k order of
//     a step is then row 16 s + 8 (j >> 2) + 4 h + (j & 3), and V^T's fragment is read in that order with the transposing LDS read
//     (16-bit).
//   * fp32 operands run both products on v_mfma_f64_16x16x4_f64, with the scores, the exponentials, the sums and the division in
//     fp64: the only rounding is the store's.  fp32 arithmetic cannot hold the result to an ulp of max |v| (a score of 100 alone is
//     rounded by 100 x 2^-24), which is what tests/test_attention_gpu.py asks of this flavour.
// Scores are scaled after the product (in fp32, in fp64 for fp32 operands), never the 16-bit operands.  A masked key, or one past F, gets the score -inf through a per-tile table in LDS;
// the K / V rows of keys past F are staged as zeros and never read from memory.  While every key so far is masked the running max
// stays -inf: exponents are then taken against 0, so p = exp(-inf) = 0 and the rescale factor exp(-inf) = 0, never exp(-inf + inf);
// only a row whose sum is 0 after the last tile is written as NaN (nn.MultiheadAttention's answer for a fully masked row).
#include "common.hpp"

namespace alo {
namespace {

constexpr int kQB = 32;        // queries per wave
constexpr int kKT = 32;        // keys per tile
constexpr int kHeadDim = 32;   // channels per head; 8 heads, row pitch of v and out 256 elements

struct AttnArgs {
    const unsigned char* q;
    const unsigned char* k;
    const unsigned char* v;
    const unsigned char* mask;
    unsigned char* out;
    int S, F, pitch;   // queries, keys, row pitch of q and k in elements (256, or 512 for the packed [q; k] matrix)
    int qgroups;       // workgroups per (batch, head)
    float scale;
};

typedef short v4i16_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4i16_t* lds_v4i16_ptr;

template <typename T, int NW>
__global__ void __launch_bounds__(64 * NW) attention_kernel(AttnArgs a) {
    constexpr bool kF32 = std::is_same<T, float>::value;
    constexpr int ES = sizeof(T);
    constexpr int kRowB = kHeadDim * ES;          // bytes of a head row: 64 or 128
    constexpr int kPadB = kRowB + 16;             // K rows and the output stage in LDS: 16 consecutive rows at one chunk hit 16 bank groups
    constexpr int kCPR = kRowB / 16;              // 16-byte chunks per row
    constexpr int kChunks = kKT * kCPR;           // per operand and tile
    constexpr int kPer = 2 * kChunks / (64 * NW); // K and V chunks a thread stages per tile
    static_assert(kPer >= 1 && kPer * 64 * NW == 2 * kChunks && kChunks % 64 == 0, "a wave stages chunks of one operand");
    constexpr int kKBytes = kKT * kPadB, kVBytes = kKT * kRowB, kBuf = kKBytes + kVBytes + kKT * 4;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * kBuf + NW * kQB * kPadB];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int qg = blockIdx.x % a.qgroups, bh = blockIdx.x / a.qgroups, head = bh & 7, b = bh >> 3;
    const int q0 = (qg * NW + wave) * kQB;
    const size_t qk_row = (size_t)a.pitch * ES, v_row = (size_t)256 * ES;
    const unsigned char* qb = a.q + ((size_t)b * a.S * a.pitch + head * kHeadDim) * ES;
    const unsigned char* kb = a.k + ((size_t)b * a.F * a.pitch + head * kHeadDim) * ES;
    const unsigned char* vb = a.v + ((size_t)b * a.F * 256 + head * kHeadDim) * ES;
    unsigned char* ob = a.out + ((size_t)b * a.S * 256 + head * kHeadDim) * ES;
    const unsigned char* mb = a.mask ? a.mask + (size_t)b * a.F : nullptr;
    const float ninf = -__builtin_huge_valf();

    // ---- staging: thread t takes chunks t, t + 64 NW, ..: the first kChunks are K's, the rest V's; thread t < 32 the key's mask ------
    u32x4 st[kPer];
    float st_bias = 0.f;
    auto fetch = [&](int tile) {
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int c = tid + i * 64 * NW, cc = c < kChunks ? c : c - kChunks;
            const int key = tile * kKT + cc / kCPR;
            const unsigned char* src = c < kChunks ? kb + (size_t)key * qk_row : vb + (size_t)key * v_row;
            st[i] = u32x4{0u, 0u, 0u, 0u};
            if (key < a.F) st[i] = *reinterpret_cast<const u32x4*>(src + (cc % kCPR) * 16);   // keys past F: zeros, no load
        }
        if (tid < kKT) {
            const int key = tile * kKT + tid;
            st_bias = ninf;
            if (key < a.F) st_bias = (mb && mb[key]) ? ninf : 0.f;
        }
    };
    auto stage = [&](int buf) {
        unsigned char* base = smem + buf * kBuf;
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int c = tid + i * 64 * NW, cc = c < kChunks ? c : c - kChunks;
            const int row = cc / kCPR, ch = cc % kCPR;
            unsigned char* dst = c < kChunks ? base + row * kPadB + ch * 16 : base + kKBytes + row * kRowB + ch * 16;
            *reinterpret_cast<u32x4*>(dst) = st[i];
        }
        if (tid < kKT) reinterpret_cast<float*>(base + kKBytes + kVBytes)[tid] = st_bias;
    };

    const int tiles = (a.F + kKT - 1) / kKT;
    unsigned char* Ob = smem + 2 * kBuf + wave * kQB * kPadB;
    // the wave's finished rows, out of its own LDS stage, as whole head rows; rows past S are not stored
    auto store_rows = [&]() {
        ALO_WAVE_LDS_ORDER();
#pragma unroll
        for (int i = 0; i < kQB * kCPR / 64; ++i) {
            const int c = lane + 64 * i, row = c / kCPR, ch = c % kCPR;
            const u32x4 val = *reinterpret_cast<const u32x4*>(Ob + row * kPadB + ch * 16);
            if (q0 + row < a.S) *reinterpret_cast<u32x4*>(ob + (size_t)(q0 + row) * v_row + ch * 16) = val;
        }
    };

    if constexpr (kF32) {
        // ---- fp32 operands, fp64 arithmetic: both products on v_mfma_f64_16x16x4_f64 (an fp32 element widens exactly), scores, exp,
        // sums and the division in fp64, one rounding to fp32 at the store.  The wave's 32 queries are two halves of 16 (qh); a tile's
        // 32 keys two blocks of 16 (ks).  Lane = (c16, g): S^T's block has key g + 4 i in register i and query c16 on the lane, so
        // register i IS the B operand of step i of O^T += V^T P (its k index is g on both operands); O^T's block (16 channels cb)
        // has channel g + 4 i in register i.  The k order of the first product: step e, lane group g -> channel 8 g + e.
        typedef double f64x4 __attribute__((ext_vector_type(4)));
        const int c16 = lane & 15, g = lane >> 4;
        const double dinf = -__builtin_huge_val(), scale = (double)a.scale;
        double qd[2][8];
#pragma unroll
        for (int qh = 0; qh < 2; ++qh) {
            const int row = q0 + 16 * qh + c16 < a.S ? q0 + 16 * qh + c16 : a.S - 1;   // clamped; its stores are suppressed
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const u32x4 x = *reinterpret_cast<const u32x4*>(qb + (size_t)row * qk_row + 32 * g + 16 * c);
                qd[qh][4 * c] = (double)__uint_as_float(x.x); qd[qh][4 * c + 1] = (double)__uint_as_float(x.y);
                qd[qh][4 * c + 2] = (double)__uint_as_float(x.z); qd[qh][4 * c + 3] = (double)__uint_as_float(x.w);
            }
        }
        f64x4 o[2][2];
        double m[2] = {dinf, dinf}, l[2] = {0.0, 0.0};   // running max of a query (all four groups agree), sum over this group's keys
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i >> 1][i & 1] = f64x4{0.0, 0.0, 0.0, 0.0};

        fetch(0);
        stage(0);
        __syncthreads();
        for (int t = 0; t < tiles; ++t) {
            if (t + 1 < tiles) fetch(t + 1);
            const unsigned char* Kb = smem + (t & 1) * kBuf;
            const unsigned char* Vb = Kb + kKBytes;
            const float* bias = reinterpret_cast<const float*>(Vb + kVBytes);
            f64x4 s[2][2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                s[0][ks] = s[1][ks] = f64x4{0.0, 0.0, 0.0, 0.0};
                const unsigned char* krow = Kb + (16 * ks + c16) * kPadB + 32 * g;
                const u32x4 k0 = *reinterpret_cast<const u32x4*>(krow), k1 = *reinterpret_cast<const u32x4*>(krow + 16);
                const unsigned kw[8] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const double kd = (double)__uint_as_float(kw[e]);
                    s[0][ks] = __builtin_amdgcn_mfma_f64_16x16x4f64(kd, qd[0][e], s[0][ks], 0, 0, 0);
                    s[1][ks] = __builtin_amdgcn_mfma_f64_16x16x4f64(kd, qd[1][e], s[1][ks], 0, 0, 0);
                }
            }
            double bz[2][4];   // 0 or -inf: masked keys and keys past F
#pragma unroll
            for (int i = 0; i < 8; ++i) bz[i >> 2][i & 3] = (double)bias[16 * (i >> 2) + g + 4 * (i & 3)];
#pragma unroll
            for (int qh = 0; qh < 2; ++qh) {
                double mx = dinf;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    s[qh][i >> 2][i & 3] = s[qh][i >> 2][i & 3] * scale + bz[i >> 2][i & 3];
                    mx = fmax(mx, s[qh][i >> 2][i & 3]);
                }
                mx = fmax(mx, __shfl_xor(mx, 16, 64));
                mx = fmax(mx, __shfl_xor(mx, 32, 64));
                const double m_new = fmax(m[qh], mx);
                const double m_ref = m_new == dinf ? 0.0 : m_new;   // every key so far masked: p = exp(-inf) = 0, alpha = exp(-inf) = 0
                const double alpha = exp(m[qh] - m_ref);
                m[qh] = m_new;
                double sum = 0.0;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    s[qh][i >> 2][i & 3] = exp(s[qh][i >> 2][i & 3] - m_ref);
                    sum += s[qh][i >> 2][i & 3];
                }
                l[qh] = l[qh] * alpha + sum;
                o[qh][0] *= alpha;
                o[qh][1] *= alpha;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {       // step: keys 16 ks + g + 4 j, ks = i >> 2, j = i & 3
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    const double vt = (double)*reinterpret_cast<const float*>(Vb + (16 * (i >> 2) + g + 4 * (i & 3)) * kRowB + (16 * cb + c16) * 4);
                    o[0][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(vt, s[0][i >> 2][i & 3], o[0][cb], 0, 0, 0);
                    o[1][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(vt, s[1][i >> 2][i & 3], o[1][cb], 0, 0, 0);
                }
            }
            if (t + 1 < tiles) stage((t + 1) & 1);
            __syncthreads();   // the other buffer is complete; nobody reads this one any more
        }
#pragma unroll
        for (int qh = 0; qh < 2; ++qh) {
            l[qh] += __shfl_xor(l[qh], 16, 64);
            l[qh] += __shfl_xor(l[qh], 32, 64);
#pragma unroll
            for (int i = 0; i < 8; ++i)     // channel 16 cb + g + 4 j of query 16 qh + c16; l == 0 (every key masked) writes NaN
                *reinterpret_cast<float*>(Ob + (16 * qh + c16) * kPadB + (16 * (i >> 2) + g + 4 * (i & 3)) * 4) =
                    l[qh] == 0.0 ? __builtin_nanf("") : (float)(o[qh][i >> 2][i & 3] / l[qh]);
        }
        store_rows();
    } else {
        // ---- the wave's Q fragments, for the whole key loop; rows past S are clamped (their stores are suppressed) ---------------------
        const int qrow = q0 + r < a.S ? q0 + r : a.S - 1;
        u32x4 qf[2];            // step s, lane half h: channels 16 s + 8 h .. + 7
#pragma unroll
        for (int s = 0; s < 2; ++s) qf[s] = *reinterpret_cast<const u32x4*>(qb + (size_t)qrow * qk_row + 32 * s + 16 * h);

        f32x16 o;
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = 0.f;
        float m = ninf, l = 0.f;   // running max of the query (both halves agree), running sum over this half's keys

        fetch(0);
        stage(0);
        __syncthreads();
        for (int t = 0; t < tiles; ++t) {
            if (t + 1 < tiles) fetch(t + 1);
            const unsigned char* Kb = smem + (t & 1) * kBuf;
            const unsigned char* Vb = Kb + kKBytes;
            const unsigned char* Bb = Vb + kVBytes;

            // S^T = K Q^T: row (register i) = key (i & 3) + 8 (i >> 2) + 4 h, column (lane) = query r
            f32x16 s;
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const u32x4 kf = *reinterpret_cast<const u32x4*>(Kb + r * kPadB + 32 * ks + 16 * h);
                s = mfma_32x32x16<T>(kf, qf[ks], s);
            }
            // scale in fp32, then the mask: -inf on masked keys and on keys past F
            float mx = ninf;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 bias = *reinterpret_cast<const f32x4*>(Bb + (8 * g + 4 * h) * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s[4 * g + e] = s[4 * g + e] * a.scale + bias[e];
                    mx = fmaxf(mx, s[4 * g + e]);
                }
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m, mx);
            const float m_ref = m_new == ninf ? 0.f : m_new;   // every key so far masked: p = exp(-inf - 0) = 0, alpha = exp(-inf - 0) = 0
            const float alpha = __expf(m - m_ref);
            m = m_new;
            float sum = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                s[i] = __expf(s[i] - m_ref);
                sum += s[i];
            }
            l = l * alpha + sum;
#pragma unroll
            for (int i = 0; i < 16; ++i) o[i] *= alpha;

            // O^T += V^T P: row = channel, column = query; P's fragment of k-step ks is registers 8 ks .. 8 ks + 7 as they stand
            {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const u32x4 pf = {pack2<T>(s[8 * ks], s[8 * ks + 1]), pack2<T>(s[8 * ks + 2], s[8 * ks + 3]),
                                      pack2<T>(s[8 * ks + 4], s[8 * ks + 5]), pack2<T>(s[8 * ks + 6], s[8 * ks + 7])};
                    // elements 4 u .. 4 u + 3 of V^T's fragment: keys 16 ks + 8 u + 4 h + (0..3) at channel r: the 4 x 16 block with first
                    // row 16 ks + 8 u + 4 h and first column 16 (r >> 4); lane 4 q + p of a 16-lane group addresses row q, columns 4 p .. 4 p + 3
                    const int li = lane & 15;
                    const unsigned char* blk = Vb + (16 * ks + 4 * h + (li >> 2)) * kRowB + 32 * (r >> 4) + 8 * (li & 3);
                    const v4i16_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16_ptr)(blk));
                    const v4i16_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16_ptr)(blk + 8 * kRowB));
                    union { v4i16_t v[2]; u32x4 u; } vf;
                    vf.v[0] = lo;
                    vf.v[1] = hi;
                    o = mfma_32x32x16<T>(vf.u, pf, o);
                }
            }
            if (t + 1 < tiles) stage((t + 1) & 1);
            __syncthreads();   // the other buffer is complete; nobody reads this one any more
        }

        // ---- out = O / l through the wave's own LDS rows, stored as whole head rows; l == 0 (every key masked) writes NaN ---------------
        l += __shfl_xor(l, 32, 64);
#pragma unroll
        for (int g = 0; g < 4; ++g) {   // registers 4 g .. 4 g + 3: channels 8 g + 4 h .. + 3 of query r
            float v4[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v4[e] = l == 0.f ? __builtin_nanf("") : o[4 * g + e] / l;
            unsigned char* dst = Ob + r * kPadB + (8 * g + 4 * h) * ES;
            *reinterpret_cast<u32x2*>(dst) = pack4<T>(v4);
        }
        store_rows();
    }
}

template <typename T, int NW>
int launch_attention(AttnArgs& a, int batch, int qblocks, hipStream_t stream, const char* what) {
    a.qgroups = (qblocks + NW - 1) / NW;
    void* args[] = {&a};
    return launch<attention_kernel<T, NW>>((unsigned)(batch * 8 * a.qgroups), 64 * NW, 0, stream, what, args);
}

template <typename T>
int attention_waves(AttnArgs& a, int batch, int cus, hipStream_t stream, const char* what) {
    // as many waves per workgroup (sharing each staged K / V tile) as still leave every compute unit a workgroup
    const int qblocks = (a.S + kQB - 1) / kQB;
    const long heads = (long)batch * 8;
    if (heads * ((qblocks + 3) / 4) >= cus) return launch_attention<T, 4>(a, batch, qblocks, stream, what);
    if (heads * ((qblocks + 1) / 2) >= cus) return launch_attention<T, 2>(a, batch, qblocks, stream, what);
    return launch_attention<T, 1>(a, batch, qblocks, stream, what);
}

}  // namespace

int attention_block(const void* q, const void* k, const void* v, const void* mask, void* out, int batch, int S, int F, int pitch,
                    float scale, int dtype, hipStream_t stream, const char* what) {
    ALO_REQUIRE((long)batch * 8 * ((S + kQB - 1) / kQB) < (1l << 31), ALO_ERR_UNSUPPORTED, "%s: batch %d x %d queries is too many workgroups",
                what, batch, S);
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
        return fail(ALO_ERR_LAUNCH, "%s: cannot read the device's compute unit count", what);
    AttnArgs a;
    a.q = (const unsigned char*)q; a.k = (const unsigned char*)k; a.v = (const unsigned char*)v;
    a.mask = (const unsigned char*)mask; a.out = (unsigned char*)out;
    a.S = S; a.F = F; a.pitch = pitch; a.qgroups = 0; a.scale = scale;
    if (dtype == ALO_F32) return attention_waves<float>(a, batch, cus, stream, what);
    return with_storage_type(dtype, [&](auto t) { return attention_waves<decltype(t)>(a, batch, cus, stream, what); });
}

}  // namespace alo
