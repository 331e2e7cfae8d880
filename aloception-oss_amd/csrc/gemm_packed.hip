// Y (M, N) = act(X (M, K) @ W (N, K)^T + bias [+ R]), bf16 (or, for alo_linear_packed, fp16) with fp32 accumulation, K a multiple of
// 256, N of 128 (dtype = ALO_F32 of either entry point: gemm_f32.hip): the backbone's 1x1
// convolutions with many input channels (512 / 1024 / 2048; alonet/detr/backbone.py:19-47 + torchvision Bottleneck.conv1 / conv3 /
// downsample) and the 1x1 input projections (alonet/deformable_detr/deformable_detr.py:75-84) over NHWC rows.
//
// linear_shortk_kernel keeps W in registers; at these K it cannot.  Here W streams instead — pre-packed in MFMA fragment order
// (alo_pack_mfma_b: one 1 KB line per fragment), two k-steps ahead of its use through two register buffers, as in ffn256_kernel —
// while X goes through LDS 256 (128) columns at a time, the next chunk being fetched into registers during the MFMAs of the
// current one.  A wave owns a 64 x 64 block of Y (2 x 2 MFMA tiles, computed transposed so a lane holds one row); a workgroup
// is 1 x 4 waves (64 rows x 256 columns) or, for N = 128, 2 x 2 (128 rows x 128 columns).
#include "mfma_tile.hpp"

namespace alo {
namespace {

constexpr int kOutStride = 64 * 2 + 16;   // LDS row stride of a wave's 64 x 64 output block

// storage type and waves along the columns of a launch as ONE template argument (ALO_RELU_RES takes a single leading argument)
template <typename T, int kWC>
struct Packed {
    using type = T;
    static constexpr int WC = kWC;
};

struct PackedDims {
    long M;
    int N, K;
    RowGather g;
};

// T: the 16-bit storage type (bf16_t / f16_t); the comments say bf16 for both
template <typename T, int WC, bool RELU, bool HAS_RES>
__global__ void __launch_bounds__(256, 2)
linear_packed_kernel(const T* __restrict__ X, const T* __restrict__ Wp, const T* __restrict__ bias, const T* __restrict__ R,
                     T* __restrict__ Y, const PackedDims dm) {
    constexpr int WR = 4 / WC;                 // waves along the rows
    constexpr int kRows = 64 * WR;             // rows of X per workgroup
    constexpr int KC = 256 / WR;               // columns of X staged at once
    constexpr int kStride = KC * 2 + 16;       // LDS row stride of the X chunk (+16 B: conflict-free fragment reads)
    constexpr int kPieces = KC / 8;            // 16-byte pieces per staged row
    constexpr int kLoads = kRows * kPieces / 256;   // = 8
    constexpr int KB = 2;                      // k-steps per weight batch
    constexpr int NB = KC / 16 / KB;           // batches per chunk
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const xs = smem;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nl = lane & 31, kg = lane >> 5;
    const int wr = wave / WC, wc = wave % WC;
    const long row0 = (long)blockIdx.x * kRows;
    const int col0 = blockIdx.y * (64 * WC) + wc * 64;   // this wave's 64 output columns (N % (64 WC) == 0)
    constexpr int kXBytes = kRows * kStride, kOBytes = 4 * 64 * kOutStride;
    float* const bias_s = reinterpret_cast<float*>(smem + (kXBytes > kOBytes ? kXBytes : kOBytes));   // [WC][64], behind both uses of the buffer
    unsigned char* const obuf = smem + wave * (64 * kOutStride);              // aliases the X chunk after the K loop

    bias_s[tid] = bias != nullptr ? ld(&bias[blockIdx.y * (64 * WC) + (tid & (64 * WC - 1))]) : 0.f;

    auto fetch = [&](int chunk, u32x4 (&r)[kLoads]) {
#pragma unroll
        for (int j = 0; j < kLoads; ++j) {
            const int p = tid + 256 * j;
            long row = row0 + p / kPieces;
            row = gather_row(dm.g, row < dm.M ? row : dm.M - 1);   // rows past the end are read from the last row and never stored
            r[j] = *reinterpret_cast<const u32x4*>(X + row * dm.K + chunk * KC + (p % kPieces) * 8);
        }
    };
    const int ksteps = dm.K / 16;
    const size_t tile_stride = (size_t)ksteps * 512;   // elements between packed column tiles
    const T* wfrag = Wp + (size_t)(col0 / 32) * tile_stride + lane * 8;
    f32x16 acc[2][2];   // [row tile][column tile]
    zero_acc(acc);
    const unsigned char* a_lds = xs + (64 * wr) * kStride;
    // mma_batch of mfma_tile.hpp with this kernel's stride; kept here (see there)
    auto mma_batch = [&](const u32x4 (&buf)[2][KB], int batch) {
        u32x4 af[2][KB];
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            const int s = KB * batch + j;
            af[0][j] = *reinterpret_cast<const u32x4*>(a_lds + nl * kStride + (16 * s + 8 * kg) * 2);
            af[1][j] = *reinterpret_cast<const u32x4*>(a_lds + (32 + nl) * kStride + (16 * s + 8 * kg) * 2);
        }
#pragma unroll
        for (int j = 0; j < KB; ++j)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    acc[a][t] = mfma_32x32x16<T>(buf[t][j], af[a][j], acc[a][t]);
        __builtin_amdgcn_sched_barrier(0);
    };

    const int nchunks = dm.K / KC;
    const int total_batches = nchunks * NB;
    u32x4 stage[kLoads];
    u32x4 bufa[2][KB], bufb[2][KB];
    fetch(0, stage);
    load_batch(bufa, wfrag, tile_stride, 0);
    for (int c = 0; c < nchunks; ++c) {
        park_tile<kPieces>(xs, kStride, stage, tid);
        __syncthreads();
        if (c + 1 < nchunks) fetch(c + 1, stage);   // in flight during this chunk's MFMAs
        const int gb = c * NB;
#pragma unroll
        for (int bt = 0; bt < NB; bt += 2) {
            load_batch(bufb, wfrag, tile_stride, gb + bt + 1);
            mma_batch(bufa, bt);
            if (gb + bt + 2 < total_batches) load_batch(bufa, wfrag, tile_stride, gb + bt + 2);
            mma_batch(bufb, bt + 1);
        }
        __syncthreads();   // everyone is done with the chunk (and, after the last one, with the LDS it sits in)
    }

    // ---- epilogue: + bias (-> ReLU) -> bf16 -> this wave's staging -> whole lines (+ residual -> ReLU) ----------------------------------
    stage_quads<T, true>(obuf, kOutStride, acc, bias_s + wc * 64, RELU && !HAS_RES, nl, 0, kg);
    wave_lds_fence();
    store_rows<T, RELU, HAS_RES>(Y, R, obuf, kOutStride, row0 + 64 * wr, dm.M, dm.N, col0, lane);
}

template <class Cfg, bool RELU, bool HAS_RES>
int launch_packed(const void* x, const void* w, const void* bias, const void* residual, void* y, const PackedDims& dm, hipStream_t stream) {
    constexpr int WC = Cfg::WC, WR = 4 / WC, kRows = 64 * WR, KC = 256 / WR;
    constexpr size_t xbytes = (size_t)kRows * (KC * 2 + 16), obytes = 4 * 64 * kOutStride;
    constexpr size_t lds = (xbytes > obytes ? xbytes : obytes) + 256 * sizeof(float);
    void* args[] = {&x, &w, &bias, &residual, &y, const_cast<PackedDims*>(&dm)};
    const dim3 grid((unsigned)((dm.M + kRows - 1) / kRows), (unsigned)(dm.N / (64 * WC)));
    return launch<linear_packed_kernel<typename Cfg::type, WC, RELU, HAS_RES>>(grid, 256, lds, stream, "alo_linear_packed", args);
}

template <typename T>
int dispatch_packed(const void* x, const void* w_packed, const void* bias, const void* residual, void* y, const PackedDims& dm,
                    int relu, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    using Wide = Packed<T, 4>;
    using Square = Packed<T, 2>;
    if (dm.N % 256 == 0) return ALO_RELU_RES(launch_packed, Wide, relu, residual, x, w_packed, bias, residual, y, dm, s);
    return ALO_RELU_RES(launch_packed, Square, relu, residual, x, w_packed, bias, residual, y, dm, s);
}

}  // namespace
}  // namespace alo

using namespace alo;

extern "C" int alo_linear_packed(const void* x, const void* w_packed, const void* bias, const void* residual, void* y, long M,
                                 int N, int K, int relu, int dtype, void* stream) {
    ALO_REQUIRE(dtype == ALO_BF16 || dtype == ALO_F16 || dtype == ALO_F32, ALO_ERR_UNSUPPORTED,
                "alo_linear_packed: bf16 / fp16, or fp32 with split weights, only (dtype %d)", dtype);
    ALO_REQUIRE(x && w_packed && y, ALO_ERR_INVALID_ARGUMENT, "alo_linear_packed: null pointer argument");
    ALO_REQUIRE(M > 0 && N > 0 && K > 0, ALO_ERR_INVALID_ARGUMENT, "alo_linear_packed: sizes must be positive");
    if (dtype == ALO_F32) {   // gemm_f32.hip: w_packed is the split layout of alo_hotpath.h
        ALO_REQUIRE(K % 64 == 0 && N % 64 == 0, ALO_ERR_UNSUPPORTED, "alo_linear_packed: fp32 needs K and N to be multiples of 64 (K=%d N=%d)", K, N);
        ALO_REQUIRE(aligned16(x, w_packed, y, residual), ALO_ERR_INVALID_ARGUMENT, "alo_linear_packed: pointers must be 16-byte aligned");
        ALO_REQUIRE((M + 63) / 64 < (1L << 28), ALO_ERR_UNSUPPORTED, "alo_linear_packed: too many rows");
        return linear_f32(x, w_packed, bias, residual, y, M, N, K, relu, row_gather(), static_cast<hipStream_t>(stream), "alo_linear_packed");
    }
    ALO_REQUIRE(K % 256 == 0 && N % 128 == 0, ALO_ERR_UNSUPPORTED,
                "alo_linear_packed: K must be a multiple of 256 and N of 128 (K=%d N=%d)", K, N);
    ALO_REQUIRE(aligned16(x, w_packed, y, residual), ALO_ERR_INVALID_ARGUMENT, "alo_linear_packed: pointers must be 16-byte aligned");
    ALO_REQUIRE((M + 63) / 64 < (1L << 31), ALO_ERR_UNSUPPORTED, "alo_linear_packed: too many rows");
    PackedDims dm;
    dm.M = M; dm.N = N; dm.K = K; dm.g = row_gather();
    return with_storage_type(dtype, [&](auto t) { return dispatch_packed<decltype(t)>(x, w_packed, bias, residual, y, dm, relu, stream); });
}

extern "C" int alo_conv1x1_nhwc(const void* x, const void* weight, int weight_is_packed, const void* bias, const void* residual,
                                void* y, int N, int H, int W, int Cin, int Cout, int stride, int relu, int dtype, void* stream) {
    ALO_REQUIRE(x && weight && y, ALO_ERR_INVALID_ARGUMENT, "alo_conv1x1_nhwc: null pointer argument");
    ALO_REQUIRE(N > 0 && H > 0 && W > 0 && stride >= 1, ALO_ERR_INVALID_ARGUMENT, "alo_conv1x1_nhwc: N, H, W, stride must be positive");
    ALO_REQUIRE(dtype == ALO_BF16 || dtype == ALO_F32, ALO_ERR_UNSUPPORTED,
                "alo_conv1x1_nhwc: bf16 only, or fp32 with split packed weights (dtype %d)", dtype);
    ALO_REQUIRE(aligned16(x, weight, y, residual), ALO_ERR_INVALID_ARGUMENT, "alo_conv1x1_nhwc: pointers must be 16-byte aligned");
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const long M = (long)N * Ho * Wo;
    ALO_REQUIRE((long)H * W < (1L << 30), ALO_ERR_UNSUPPORTED, "alo_conv1x1_nhwc: map too large");
    if (weight_is_packed & ALO_CONV1X1_CHAIN) {   // conv1x1_chain.hip: conv3 (+ downsample) (+ the next conv1) of a layer1 bottleneck
        const bool down = (weight_is_packed & ALO_CONV1X1_CHAIN_DOWN) != 0;
        const int n2 = weight_is_packed & ~(ALO_CONV1X1_CHAIN | ALO_CONV1X1_CHAIN_DOWN);
        const bool l1 = Cin == 64 && Cout == 256 && stride == 1 && (n2 == 0 || n2 == 64 || n2 == 128);
        // conv1x1_chain_l2.hip: a layer2 bottleneck, whose downsample convolution (256 input channels) may carry the stage's stride
        const bool l2 = Cin == 128 && Cout == 512 && (stride == 1 || (stride == 2 && down)) && (n2 == 0 || n2 == 128);
        ALO_REQUIRE(dtype == ALO_BF16 && relu && (l1 || l2), ALO_ERR_UNSUPPORTED,
                    "alo_conv1x1_nhwc: a chain buffer needs bf16, Cin = 64, Cout = 256, stride 1, relu and a next width of 0, 64 or 128, "
                    "or Cin = 128, Cout = 512, stride 1 (2 with _DOWN) and a next width of 0 or 128 "
                    "(dtype %d Cin=%d Cout=%d stride=%d relu=%d next=%d)", dtype, Cin, Cout, stride, relu, n2);
        ALO_REQUIRE(residual && !bias, ALO_ERR_INVALID_ARGUMENT,
                    "alo_conv1x1_nhwc: a chain buffer carries its biases (bias must be NULL) and needs the identity, or the downsample "
                    "convolution's input, in residual");
        ALO_REQUIRE((M + 63) / 64 < (1L << 31), ALO_ERR_UNSUPPORTED, "alo_conv1x1_nhwc: too many output pixels");
        // a tile's outputs are written while other tiles' inputs are still to be read: y-then-z may overlap neither input
        const size_t rows = (size_t)M;
        // (with _DOWN at Cin = 128 the second input is x0's whole (N, H, W, 256) map)
        const size_t other = !down ? rows * 2 * (size_t)Cout : l1 ? rows * 128 : (size_t)N * H * W * 512;
        const struct { const void* p; size_t bytes; } out = {y, rows * 2 * ((size_t)Cout + (size_t)n2)},
                                                      ins[] = {{x, rows * 2 * (size_t)Cin}, {residual, other}};
        for (const auto& i : ins)
            ALO_REQUIRE((const char*)out.p + out.bytes <= (const char*)i.p || (const char*)i.p + i.bytes <= (const char*)out.p,
                        ALO_ERR_INVALID_ARGUMENT, "alo_conv1x1_nhwc: the output of a chain overlaps an input");
        if (l1) return conv1x1_chain(x, weight, residual, y, M, down, n2, static_cast<hipStream_t>(stream));
        return conv1x1_chain_l2(x, weight, residual, y, M, down, n2, row_gather(stride, Ho, Wo, H, W), static_cast<hipStream_t>(stream));
    }
    const RowGather gather = row_gather(stride, Ho, Wo, H, W);
    if (dtype == ALO_F32) {   // gemm_f32.hip behind the same row addressing
        ALO_REQUIRE(weight_is_packed, ALO_ERR_UNSUPPORTED, "alo_conv1x1_nhwc: fp32 takes the split packed weight only (weight_is_packed = 1)");
        ALO_REQUIRE(Cin > 0 && Cout > 0 && Cin % 64 == 0 && Cout % 64 == 0, ALO_ERR_UNSUPPORTED,
                    "alo_conv1x1_nhwc: fp32 needs Cin and Cout to be multiples of 64 (Cin=%d Cout=%d)", Cin, Cout);
        ALO_REQUIRE((M + 63) / 64 < (1L << 28), ALO_ERR_UNSUPPORTED, "alo_conv1x1_nhwc: too many output pixels");
        return linear_f32(x, weight, bias, residual, y, M, Cout, Cin, relu, gather, static_cast<hipStream_t>(stream), "alo_conv1x1_nhwc");
    }
    if (!weight_is_packed) {
        ALO_REQUIRE(Cout % 64 == 0, ALO_ERR_UNSUPPORTED, "alo_conv1x1_nhwc: Cout must be a multiple of 64 (got %d)", Cout);
        return linear_shortk_gather(x, weight, bias, residual, y, M, Cout, Cin, relu, gather, static_cast<hipStream_t>(stream));
    }
    ALO_REQUIRE(Cin % 256 == 0 && Cout % 128 == 0, ALO_ERR_UNSUPPORTED,
                "alo_conv1x1_nhwc: packed weights need Cin %% 256 == 0 and Cout %% 128 == 0 (Cin=%d Cout=%d)", Cin, Cout);
    PackedDims dm;
    dm.M = M; dm.N = Cout; dm.K = Cin; dm.g = gather;
    return dispatch_packed<bf16_t>(x, weight, bias, residual, y, dm, relu, stream);
}
