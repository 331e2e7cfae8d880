// Shared helpers for the gfx950 kernels: error reporting, the launch path, buffer-resource loads, element conversion, MFMA operands.
// What the GEMM-shaped kernels share around the MFMA (tiles, epilogues, weight streaming) is in mfma_tile.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdarg>
#include <cstdio>
#include <type_traits>

#include "../../include/alo_hotpath.h"

namespace alo {

// ---- host side: thread-local error string -------------------------------------------------------------------------
char* error_buffer();  // api.hip
inline int fail(alo_status_t code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(error_buffer(), 512, fmt, ap);
    va_end(ap);
    return (int)code;
}
#define ALO_REQUIRE(cond, code, ...) \
    do {                             \
        if (!(cond)) return ::alo::fail(code, __VA_ARGS__); \
    } while (0)

// Whether every pointer is on a 16-byte boundary (a null pointer is).
template <typename... P>
inline bool aligned16(const P*... p) {
    return ((... | (uintptr_t)p) & 15) == 0;
}

// The one launch path of the library.  A launch that asks for more than 48 KiB of dynamic LDS raises the kernel's limit to the whole
// LDS first, once per (kernel, device): a function attribute is per device, so a process-wide flag would leave the second GPU of a
// single-process multi-GPU job at the 48/64 KB default.  `done` is one atomic bit mask per kernel (this instantiation's own; up to 64
// devices); the attribute call itself is idempotent, so a race only repeats it.  The attribute call, the launch and hipGetLastError
// all report through `what`.
constexpr int kLdsLimit = 160 * 1024;
template <auto kernel>
int launch(dim3 grid, dim3 block, size_t lds, hipStream_t stream, const char* what, void** args) {
    ALO_REQUIRE(lds <= (size_t)kLdsLimit, ALO_ERR_UNSUPPORTED, "%s: %zu bytes of dynamic LDS, the limit is %d", what, lds, kLdsLimit);
    const void* fn = reinterpret_cast<const void*>(kernel);
    hipError_t e = hipSuccess;
    if (lds > 48 * 1024) {
        static unsigned long long done = 0;
        int dev = 0;
        e = hipGetDevice(&dev);
        const unsigned long long bit = 1ull << (dev & 63);
        if (e == hipSuccess && !(__atomic_load_n(&done, __ATOMIC_ACQUIRE) & bit)) {
            e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsLimit);
            if (e == hipSuccess) __atomic_fetch_or(&done, bit, __ATOMIC_RELEASE);
        }
    }
    if (e == hipSuccess) e = hipLaunchKernel(fn, grid, block, args, lds, stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return fail(ALO_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return ALO_OK;
}

constexpr int kNumXcd = 8;  // MI355X: 8 XCDs, block b is dispatched to XCD b % 8 (speed only, never correctness)

// Remap a launch-order block id so that each XCD (private 4 MiB L2) receives one CONTIGUOUS range of logical work
// items instead of every 8th one.  Bijective for any grid size.
__device__ __forceinline__ unsigned xcd_contiguous_block(unsigned bid, unsigned nblocks) {
    const unsigned q = nblocks / kNumXcd, r = nblocks % kNumXcd;
    const unsigned xcd = bid % kNumXcd, k = bid / kNumXcd;
    const unsigned start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return start + k;
}

// Persistent workgroups over `ntiles` tiles, one CONTIGUOUS eighth of the tiles per XCD: XCD x (workgroup ids = x mod 8) walks tiles
// [x * per_xcd, (x + 1) * per_xcd), so neighbouring tiles meet in the same L2.  A workgroup takes tiles first, first + step, .. below
// end; xcd_grid is the matching grid size.
static_assert(kNumXcd == 8, "the tile ranges below shift by 3");
struct TileRange { int first, end, step; };
__device__ __forceinline__ TileRange xcd_tile_range(int ntiles) {
    const int per_xcd = (ntiles + 7) >> 3, xcd = blockIdx.x & 7;
    const int end = (xcd + 1) * per_xcd < ntiles ? (xcd + 1) * per_xcd : ntiles;
    return {(int)(xcd * per_xcd + (blockIdx.x >> 3)), end, (int)(gridDim.x >> 3)};
}
inline unsigned xcd_grid(int ntiles, int max_per_xcd) {
    const int per_xcd = (ntiles + 7) / 8;
    return 8u * (unsigned)(per_xcd < max_per_xcd ? per_xcd : max_per_xcd);
}

// msda_bwd_wide.hip: the 16x16-block backward.  msda_wide_plan is pure host logic: whether the path takes a launch (fp32 / bf16 values,
// D = 32 or 64, Lq == S, a host copy of the shapes its block table can describe; the caller vouches for L = P = 4 and 16-byte aligned
// pointers), filling `wp` when it does.  WidePlan is that file's WideDims, the kernel's by-value argument, opaque here: WideDims stays
// in its anonymous namespace because the kernels' names carry it.  A field added there needs `words` resized (a static_assert says so).
struct WidePlan {
    int words[31];
};
bool msda_wide_plan(int N, int S, int M, int D, int Lq, int value_dtype, const int32_t* host_shapes, WidePlan* wp);
int msda_wide_launch(const void* value, const int32_t* shapes, const int32_t* lstart, const void* loc, const void* attn,
                     const void* grad_out, void* grad_value, void* grad_loc, void* grad_attn, const WidePlan& wp, int D,
                     int value_dtype, hipStream_t stream);

// Strided 1x1 convolution over an NHWC map read as a GEMM: row r of X' = pixel (n, s * yo, s * xo) of X; s <= 1: X' = X.
struct RowGather {
    int s, Wo, HoWo, W, HW;
};
inline RowGather row_gather(int stride = 1, int Ho = 1, int Wo = 1, int H = 1, int W = 1) { return {stride, Wo, Ho * Wo, W, H * W}; }

// gemm.hip: linear_shortk_kernel over gathered rows, the resident-weight flavour of alo_conv1x1_nhwc (gemm_packed.hip).
int linear_shortk_gather(const void* x, const void* weight, const void* bias, const void* residual, void* y, long M, int N, int K,
                         int relu, const RowGather& gather, hipStream_t stream);

// conv1x1_chain.hip: alo_conv1x1_nhwc with a chain buffer on checked arguments (w_chain and the y-then-z output: alo_hotpath.h);
// res_or_x0 is the (M, 256) identity, or with `down` the (M, 64) input of the downsample convolution; n2 = 0, 64 or 128.
int conv1x1_chain(const void* mid, const void* w_chain, const void* res_or_x0, void* y, long M, bool down, int n2, hipStream_t stream);
// conv1x1_chain_l2.hip: the same at layer2's widths, mid (M, 128) -> y (M, 512); res_or_x0 is the (M, 512) identity, or with `down` the
// (N, H, W, 256) map whose pixels `gather` picks as the downsample convolution's input rows; n2 = 0 or 128.
int conv1x1_chain_l2(const void* mid, const void* w_chain, const void* res_or_x0, void* y, long M, bool down, int n2, const RowGather& gather,
                     hipStream_t stream);

// conv_f32.hip: the fp32 flavour of alo_conv3x3_nhwc on checked arguments (w_split and image_mag: alo_hotpath.h); image_mag holds N words.
int conv3x3_f32(const void* x, const void* w_split, const void* bias, void* y, void* image_mag, int N, int H, int W, int Cin, int Cout,
                int stride, int dilation, int relu, hipStream_t stream);   // dilation 2 (ALO_CONV_DILATION_2): stride 1, padding 2
// the five-tap flavours behind ALO_CONV_TAPS_1X5 (vertical = 0) / ALO_CONV_TAPS_5X1 (vertical = 1): stride 1, w_split of the (Cout, 5 Cin) matrix
int conv_taps_f32(const void* x, const void* w_split, const void* bias, void* y, void* image_mag, int N, int H, int W, int Cin, int Cout,
                  int vertical, int relu, hipStream_t stream);

// gemm_f32.hip: the fp32 flavour of alo_linear_packed / alo_conv1x1_nhwc on checked arguments (w_split: alo_hotpath.h); `what` names the
// entry point in a launch error.
int linear_f32(const void* x, const void* w_split, const void* bias, const void* residual, void* y, long M, int N, int K, int relu,
               const RowGather& gather, hipStream_t stream, const char* what);

// ffn_f32.hip: the fp32 flavour of alo_ffn256 on checked arguments (w1_split, w2_split: alo_hotpath.h); refuses an F whose tiles and
// tables do not fit in LDS with ALO_ERR_UNSUPPORTED.
int ffn_f32(const void* x, const void* w1_split, const void* b1, const void* w2_split, const void* b2, void* y, long M, int F,
            hipStream_t stream, const char* what);

// stem_f32.hip: the fp32 flavour of alo_stem_conv_pool on checked arguments (w_split: alo_hotpath.h); refuses a batch with 2^30 tiles or more.
int stem_conv_pool_f32(const void* x, const void* w_split, const void* bias, void* y, int N, int H, int W, long stride_n, long stride_c,
                       long stride_h, long stride_w, hipStream_t stream);

// instancenorm_f32.hip: the fp32 flavour of alo_groupnorm_rows_act on checked arguments (groups == C, no affine; alo_hotpath.h); the
// workspace is the bf16 call's: a triple per 256-row chunk and channel.
int instancenorm_f32(const void* x, void* y, void* workspace, int B, int HW, int C, float eps, long y_batch_stride, int relu,
                     hipStream_t stream, const char* what);

// upsample_flow.hip: the fp32 flavour of alo_upsample_add_nhwc on checked arguments (planar flow and mask: alo_hotpath.h); mask NULL is
// the bilinear mode; refuses a map whose mask planes of one image reach 4 GiB.
int upsample_flow_f32(const void* flow, const void* mask, void* out, int BQ, int C, int h, int w, hipStream_t stream, const char* what);
// its convex mode's backward (ALO_UPSAMPLE_GRAD) on checked arguments: x_low = flow then grad_up, out = grad_mask then taps (alo_hotpath.h)
int upsample_flow_grad_f32(const void* flow_and_grad, const void* mask, void* out, int BQ, int C, int h, int w, hipStream_t stream,
                           const char* what);

// attention.hip: ALO_BLOCK_ATTENTION of alo_encoder_block on checked arguments (alo_encoder_block.h): q (batch, S, .) and k (batch, F, .)
// with a row pitch of `pitch` elements (256, or 512 for the two halves of a packed [q; k] matrix), v (batch, F, 256), mask (batch, F)
// or NULL, out (batch, S, 256); dtype ALO_BF16, ALO_F16 or ALO_F32.
int attention_block(const void* q, const void* k, const void* v, const void* mask, void* out, int batch, int S, int F, int pitch,
                    float scale, int dtype, hipStream_t stream, const char* what);

// relu x residual -> the four instantiations of a launcher template: ALO_RELU_RES(fn, first, relu, residual, args...) calls
// fn<first, relu != 0, residual != nullptr>(args...)
#define ALO_RELU_RES(fn, first, relu, residual, ...)                                                                          \
    ((residual) ? ((relu) ? fn<first, true, true>(__VA_ARGS__) : fn<first, false, true>(__VA_ARGS__))                          \
                : ((relu) ? fn<first, true, false>(__VA_ARGS__) : fn<first, false, false>(__VA_ARGS__)))

// ---- device side ---------------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

struct bf16_t {
    uint16_t bits;
};

// ReLU with torch's semantics: NaN is kept (fmaxf(NaN, 0) is 0 under IEEE maxNum) and -0 becomes +0 (the stem max-pools bf16
// bit patterns as uint16, where 0x8000 would beat every positive value)
__device__ __forceinline__ float relu_keep_nan(float v) { return (v > 0.f || v != v) ? v : 0.f; }

__device__ __forceinline__ float bf16_to_f32(uint16_t b) { return __uint_as_float(((unsigned)b) << 16); }
// fp32 -> bf16, round to nearest even: gfx950 converts in hardware (v_cvt_pk_bf16_f32, two values per instruction)
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
    const __bf16 b = static_cast<__bf16>(f);
    return __builtin_bit_cast(uint16_t, b);
}
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {  // lo in bits 0-15
    typedef __bf16 bf16x2_hw __attribute__((ext_vector_type(2)));
    typedef float f32x2_hw __attribute__((ext_vector_type(2)));
    const bf16x2_hw r = __builtin_convertvector(f32x2_hw{lo, hi}, bf16x2_hw);
    return __builtin_bit_cast(unsigned, r);
}

// fp16 storage (IEEE binary16): 11 significant bits, 5-bit exponent.  Both conversions are single hardware instructions;
// fp32 -> fp16 rounds to nearest even (v_cvt_f16_f32 / v_cvt_pk_f16_f32), never toward zero (v_cvt_pkrtz_f16_f32).
struct f16_t {
    uint16_t bits;
};
__device__ __forceinline__ float f16_to_f32(uint16_t b) { return (float)__builtin_bit_cast(_Float16, b); }
__device__ __forceinline__ uint16_t f32_to_f16(float f) {
    const _Float16 h = static_cast<_Float16>(f);
    return __builtin_bit_cast(uint16_t, h);
}
__device__ __forceinline__ unsigned pack_f16x2(float lo, float hi) {  // lo in bits 0-15
    typedef _Float16 f16x2_hw __attribute__((ext_vector_type(2)));
    typedef float f32x2_hw __attribute__((ext_vector_type(2)));
    const f16x2_hw r = __builtin_convertvector(f32x2_hw{lo, hi}, f16x2_hw);
    return __builtin_bit_cast(unsigned, r);
}
// the two 16-bit elements of one register, widened (lo = bits 0-15), and their packed store, by storage type
template <typename T>
__device__ __forceinline__ void unpack2(unsigned w, float& lo, float& hi) {
    if constexpr (std::is_same<T, f16_t>::value) {
        lo = f16_to_f32((uint16_t)(w & 0xffffu));
        hi = f16_to_f32((uint16_t)(w >> 16));
    } else {
        lo = __uint_as_float(w << 16);
        hi = __uint_as_float(w & 0xffff0000u);
    }
}
template <typename T>
__device__ __forceinline__ unsigned pack2(float lo, float hi) {
    if constexpr (std::is_same<T, f16_t>::value) return pack_f16x2(lo, hi);
    else return pack_bf16x2(lo, hi);
}
// four consecutive elements = one 8-byte access
template <typename T>
__device__ __forceinline__ void unpack4(const u32x2& x, float (&v)[4]) {
    unpack2<T>(x.x, v[0], v[1]);
    unpack2<T>(x.y, v[2], v[3]);
}
template <typename T>
__device__ __forceinline__ u32x2 pack4(const float (&v)[4]) { return u32x2{pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3])}; }

// Host side: f(bf16_t{}) or f(f16_t{}) for a dtype the caller has checked to be ALO_BF16 or ALO_F16 (f: a generic lambda, decltype(t))
template <typename F>
inline int with_storage_type(int dtype, F&& f) {
    return dtype == ALO_F16 ? f(f16_t{}) : f(bf16_t{});
}

// the bf16 MFMA's operand type over the four registers a 16-byte load fills
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
__device__ __forceinline__ bf16x8_t as_bf16x8(const u32x4& v) {
    union { u32x4 u; bf16x8_t b; } x;
    x.u = v;
    return x.b;
}

// the fp16 MFMA's operand type, and the 32x32x16 MFMA of storage type T (same operand layout for both: 8 consecutive k per lane)
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
__device__ __forceinline__ f16x8_t as_f16x8(const u32x4& v) {
    union { u32x4 u; f16x8_t h; } x;
    x.u = v;
    return x.h;
}
template <typename T>
__device__ __forceinline__ f32x16 mfma_32x32x16(const u32x4& a, const u32x4& b, const f32x16& c) {
    if constexpr (std::is_same<T, f16_t>::value) return __builtin_amdgcn_mfma_f32_32x32x16_f16(as_f16x8(a), as_f16x8(b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a), as_bf16x8(b), c, 0, 0, 0);
}

// GEMM epilogue on 8 outputs of storage type T (bf16 / fp16): + identity (same coordinates as y), then the activation, re-packed to T
template <typename T, bool RELU>
__device__ __forceinline__ u32x4 add_residual_x8(const u32x4& v, const u32x4& rv) {
    const unsigned a4[4] = {v.x, v.y, v.z, v.w}, r4[4] = {rv.x, rv.y, rv.z, rv.w};
    unsigned o4[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float alo, ahi, rlo, rhi;
        unpack2<T>(a4[i], alo, ahi);
        unpack2<T>(r4[i], rlo, rhi);
        float lo = alo + rlo, hi = ahi + rhi;
        if (RELU) { lo = relu_keep_nan(lo); hi = relu_keep_nan(hi); }
        o4[i] = pack2<T>(lo, hi);
    }
    return u32x4{o4[0], o4[1], o4[2], o4[3]};
}

// row of the GEMM -> row of the NHWC input it reads (identity unless the 1x1 convolution is strided)
__device__ __forceinline__ long gather_row(const RowGather& g, long row) {
    if (g.s <= 1) return row;
    const long n = row / g.HoWo;
    const int rem = (int)(row - n * g.HoWo);
    const int yo = rem / g.Wo, xo = rem - yo * g.Wo;
    return n * g.HW + (long)(yo * g.s) * g.W + xo * g.s;
}

// A raw (stride-0) buffer resource over [base, base + bytes).  Loads whose byte offset falls outside return 0 and
// touch no memory: the hardware's bounds check is how out-of-map bilinear corners get their zero padding.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
constexpr unsigned kOutOfRange = 0xC0000000u;  // byte offset guaranteed past any slab (slabs are < 3 GiB)

// Load VEC elements of storage type T at byte offset `off` (raw registers), widen them to the compute type CT later:
// keeping the two steps apart lets a kernel put a whole batch of loads in flight before the first conversion.
template <typename T, typename CT, int VEC>
struct Loader;

template <>
struct Loader<float, float, 4> {
    using raw_t = u32x4;
    static __device__ __forceinline__ raw_t load(__amdgpu_buffer_rsrc_t r, unsigned off) {
        return __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
    }
    static __device__ __forceinline__ void widen(const raw_t& x, float (&v)[4]) {
        v[0] = __uint_as_float(x.x); v[1] = __uint_as_float(x.y); v[2] = __uint_as_float(x.z); v[3] = __uint_as_float(x.w);
    }
};
template <>
struct Loader<float, float, 1> {
    using raw_t = unsigned;
    static __device__ __forceinline__ raw_t load(__amdgpu_buffer_rsrc_t r, unsigned off) {
        return __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0);
    }
    static __device__ __forceinline__ void widen(const raw_t& x, float (&v)[1]) { v[0] = __uint_as_float(x); }
};
template <>
struct Loader<double, double, 2> {
    using raw_t = u32x4;
    static __device__ __forceinline__ raw_t load(__amdgpu_buffer_rsrc_t r, unsigned off) {
        return __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
    }
    static __device__ __forceinline__ void widen(const raw_t& x, double (&v)[2]) {
        v[0] = __hiloint2double((int)x.y, (int)x.x);
        v[1] = __hiloint2double((int)x.w, (int)x.z);
    }
};
template <>
struct Loader<double, double, 1> {
    using raw_t = u32x2;
    static __device__ __forceinline__ raw_t load(__amdgpu_buffer_rsrc_t r, unsigned off) {
        return __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0);
    }
    static __device__ __forceinline__ void widen(const raw_t& x, double (&v)[1]) {
        v[0] = __hiloint2double((int)x.y, (int)x.x);
    }
};
template <>
struct Loader<bf16_t, float, 8> {
    using raw_t = u32x4;
    static __device__ __forceinline__ raw_t load(__amdgpu_buffer_rsrc_t r, unsigned off) {
        return __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
    }
    static __device__ __forceinline__ void widen(const raw_t& x, float (&v)[8]) {
        const unsigned w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = __uint_as_float(w[i] << 16);
            v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
        }
    }
};
template <>
struct Loader<bf16_t, float, 1> {
    using raw_t = unsigned short;
    static __device__ __forceinline__ raw_t load(__amdgpu_buffer_rsrc_t r, unsigned off) {
        return __builtin_amdgcn_raw_buffer_load_b16(r, off, 0, 0);
    }
    static __device__ __forceinline__ void widen(const raw_t& x, float (&v)[1]) { v[0] = bf16_to_f32(x); }
};

template <>
struct Loader<f16_t, float, 8> {
    using raw_t = u32x4;
    static __device__ __forceinline__ raw_t load(__amdgpu_buffer_rsrc_t r, unsigned off) {
        return __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
    }
    static __device__ __forceinline__ void widen(const raw_t& x, float (&v)[8]) {
        const unsigned w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) unpack2<f16_t>(w[i], v[2 * i], v[2 * i + 1]);
    }
};
template <>
struct Loader<f16_t, float, 1> {
    using raw_t = unsigned short;
    static __device__ __forceinline__ raw_t load(__amdgpu_buffer_rsrc_t r, unsigned off) {
        return __builtin_amdgcn_raw_buffer_load_b16(r, off, 0, 0);
    }
    static __device__ __forceinline__ void widen(const raw_t& x, float (&v)[1]) { v[0] = f16_to_f32(x); }
};

// Scalar global load/store with widening / narrowing (sampling locations, attention weights, outputs).
__device__ __forceinline__ float ld(const float* p) { return *p; }
__device__ __forceinline__ double ld(const double* p) { return *p; }
__device__ __forceinline__ float ld(const bf16_t* p) { return bf16_to_f32(p->bits); }
__device__ __forceinline__ float ld(const f16_t* p) { return f16_to_f32(p->bits); }
__device__ __forceinline__ void st(float* p, float v) { *p = v; }
__device__ __forceinline__ void st(double* p, double v) { *p = v; }
__device__ __forceinline__ void st(bf16_t* p, float v) { p->bits = f32_to_bf16(v); }
__device__ __forceinline__ void st(f16_t* p, float v) { p->bits = f32_to_f16(v); }

// Store VEC consecutive outputs (16-byte vector store when VEC * sizeof(T) == 16).
template <typename T, typename CT, int VEC>
__device__ __forceinline__ void store_vec(T* p, const CT (&v)[VEC]) {
    if constexpr (sizeof(T) == 4 && VEC == 4) {
        *reinterpret_cast<f32x4*>(p) = f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    } else if constexpr (sizeof(T) == 8 && VEC == 2) {
        *reinterpret_cast<double2*>(p) = double2{(double)v[0], (double)v[1]};
    } else if constexpr (sizeof(T) == 2 && VEC == 8) {
        u32x4 o;
        o.x = pack2<T>(v[0], v[1]);
        o.y = pack2<T>(v[2], v[3]);
        o.z = pack2<T>(v[4], v[5]);
        o.w = pack2<T>(v[6], v[7]);
        *reinterpret_cast<u32x4*>(p) = o;
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) st(p + i, v[i]);
    }
}

// A wave hands LDS data from some of its lanes to others.  LDS operations of one wave execute in order, so nothing has to be waited
// for: the compiler alone must not move the reads above the writes.  The fence builtins at "wavefront" scope (wave_lds_fence of
// mfma_tile.hpp) are NOT that: they lower to s_waitcnt vmcnt(0) lgkmcnt(0), which also waits for the wave's outstanding global traffic.
#define ALO_WAVE_LDS_ORDER() do { asm volatile("" ::: "memory"); __builtin_amdgcn_wave_barrier(); asm volatile("" ::: "memory"); } while (0)

// Sum over the 64 lanes of a wave, every lane gets it (the LayerNorm kernels: one wave per row).
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

}  // namespace alo
