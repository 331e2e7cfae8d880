// EXPERIMENT: which shape should the backward of RAFT's convex up-sampling (csrc/upsample_flow.hip, upsample_flow_grad_kernel) have?
// `taps` needs a sum over the eight sub-rows i of a coarse pixel, and two shapes deliver it without atomics:
//
//   lds   the library's kernel (this file includes csrc/upsample_flow.hip and launches it): a workgroup is 8 sub-rows x 64 pixels,
//         a thread owns one (pixel, sub-row), the partial sums meet in LDS
//   loop  the variant below: a thread owns a whole coarse pixel, walks its eight sub-rows and keeps the 9 C tap sums in registers;
//         no LDS, no barrier, one eighth of the threads
//
// C = 2.  Both run at (4, 2, 90, 160) (4 pairs of 1280 x 720: 57.6k coarse pixels) and (6, 2, 46, 62) (a 368 x 496 crop at batch 6:
// 17k), alternating for 3 rounds of 20 launches in one process, each launch between its own pair of events; the launches of a round
// walk over 4 sets of mask / grad_mask buffers, so none is found in the Infinity Cache.  Per shape and variant one JSON line: median
// round, min and max of the rounds, and max |difference| of grad_mask and taps against the library's kernel.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o upsample_grad_shapes upsample_grad_shapes.hip && ./upsample_grad_shapes
// Not part of the library; nothing imports this.
#include "../../aloception-oss_amd/csrc/upsample_flow.hip"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

namespace alo {
char* error_buffer() {
    static thread_local char buf[512];
    return buf;
}

namespace {

// one thread per coarse pixel, 64 threads per workgroup (the most workgroups a map can give)
__global__ void __launch_bounds__(64)
upsample_flow_grad_loop_kernel(const float* __restrict__ flow, const float* __restrict__ grad_up, const float* __restrict__ mask,
                               float* __restrict__ grad_mask, float* __restrict__ taps, const UpFlowDims dm) {
    constexpr int NC = 2;
    const unsigned b = blockIdx.x;
    const int chunk = b % dm.chunks;
    const long n = b / dm.chunks;
    const int p = chunk * 64 + threadIdx.x;
    if (p >= dm.hw) return;
    const int y = p / dm.w, x = p - y * dm.w;
    const __amdgpu_buffer_rsrc_t mask_r = make_rsrc(mask + n * 576 * dm.hw, 576u * (unsigned)dm.hw * 4u);
    const __amdgpu_buffer_rsrc_t gmask_r = make_rsrc(grad_mask + n * 576 * dm.hw, 576u * (unsigned)dm.hw * 4u);
    const __amdgpu_buffer_rsrc_t flow_r = make_rsrc(flow + n * dm.C * dm.hw, (unsigned)(dm.C * dm.hw) * 4u);
    float v[NC][9], acc[NC][9];
    load_neighbours<NC>(flow_r, dm, 0, y, x, v);
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[c][k] = 0.f;
    for (int i = 0; i < 8; ++i) {
        const float* const grow = grad_up + ((n * dm.C * 8 * dm.h + 8 * y + i) * (8L * dm.w) + 8 * x);
        float e[9][8], g[NC][8];
#pragma unroll
        for (int k = 0; k < 9; ++k)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                e[k][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(mask_r, (unsigned)p * 4u, (int)((unsigned)(k * 64 + i * 8 + j) * (unsigned)dm.hw * 4u), 0));
        load_grad_rows<NC>(grow, dm, g);
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
            float t[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                e[k][j] *= rs;
                t[k] = fmaf(g[1][j], v[1][k], g[0][j] * v[0][k]);
            }
            float st = e[0][j] * t[0];
#pragma unroll
            for (int k = 1; k < 9; ++k) st = fmaf(e[k][j], t[k], st);
#pragma unroll
            for (int k = 0; k < 9; ++k)
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(e[k][j] * (t[k] - st)), gmask_r, (unsigned)p * 4u,
                                                      (int)((unsigned)(k * 64 + i * 8 + j) * (unsigned)dm.hw * 4u), 0);
        }
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                float a = e[k][0] * g[c][0];
#pragma unroll
                for (int j = 1; j < 8; ++j) a = fmaf(e[k][j], g[c][j], a);
                acc[c][k] += 8.f * a;
            }
    }
    float* const timg = taps + n * 9 * dm.C * dm.hw;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int k = 0; k < 9; ++k) timg[(long)(c * 9 + k) * dm.hw + p] = acc[c][k];
}

#define CK(x)                                                                            \
    do {                                                                                 \
        hipError_t e_ = (x);                                                             \
        if (e_ != hipSuccess) {                                                          \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_));   \
            exit(1);                                                                     \
        }                                                                                \
    } while (0)

struct Case {
    int BQ, C, h, w;
    long hw, nflow, start, nmask, ntaps;
    float* in;                       // flow, then grad_up
    float* mask[4];
    float* out[4];                   // grad_mask, then taps
};

int run_lds(const Case& c, int s) { return upsample_flow_grad_f32(c.in, c.mask[s], c.out[s], c.BQ, c.C, c.h, c.w, nullptr, "lds"); }

int run_loop(const Case& c, int s) {
    UpFlowDims dm;
    dm.C = c.C; dm.h = c.h; dm.w = c.w; dm.hw = (int)c.hw; dm.chunks = (int)((c.hw + 63) / 64);
    const float* flow = c.in;
    const float* grad_up = c.in + c.start;
    const float* mask = c.mask[s];
    float* grad_mask = c.out[s];
    float* taps = grad_mask + c.nmask;
    void* args[6] = {&flow, &grad_up, &mask, &grad_mask, &taps, &dm};
    return launch<upsample_flow_grad_loop_kernel>((unsigned)(dm.chunks * c.BQ), 64, 0, nullptr, "loop", args);
}

float round_ms(int (*run)(const Case&, int), const Case& c, int launches) {
    std::vector<hipEvent_t> ev(launches + 1);
    for (auto& e : ev) CK(hipEventCreate(&e));
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(ev[0], nullptr));
    for (int l = 0; l < launches; ++l) {
        if (run(c, l % 4) != 0) {
            fprintf(stderr, "%s\n", error_buffer());
            exit(1);
        }
        CK(hipEventRecord(ev[l + 1], nullptr));
    }
    CK(hipDeviceSynchronize());
    std::vector<float> ms(launches);
    for (int l = 0; l < launches; ++l) CK(hipEventElapsedTime(&ms[l], ev[l], ev[l + 1]));
    for (auto& e : ev) CK(hipEventDestroy(e));
    std::sort(ms.begin(), ms.end());
    return ms[launches / 2];
}

void one_case(int BQ, int h, int w) {
    Case c;
    c.BQ = BQ; c.C = 2; c.h = h; c.w = w;
    c.hw = (long)h * w; c.nflow = (long)BQ * c.C * c.hw; c.start = (c.nflow + 3) / 4 * 4;
    c.nmask = (long)BQ * 576 * c.hw; c.ntaps = (long)BQ * 9 * c.C * c.hw;
    const long nin = c.start + 64 * c.nflow, nout = c.nmask + c.ntaps;
    std::vector<float> host(std::max(nin, c.nmask));
    unsigned state = 12345u;
    auto next = [&]() { state = state * 1664525u + 1013904223u; return ((state >> 8) & 0xFFFF) / 65536.f * 2.f - 1.f; };
    for (long i = 0; i < nin; ++i) host[i] = 4.f * next();
    CK(hipMalloc(&c.in, nin * 4));
    CK(hipMemcpy(c.in, host.data(), nin * 4, hipMemcpyHostToDevice));
    for (int s = 0; s < 4; ++s) {
        for (long i = 0; i < c.nmask; ++i) host[i] = 6.f * next();
        CK(hipMalloc(&c.mask[s], c.nmask * 4));
        CK(hipMemcpy(c.mask[s], host.data(), c.nmask * 4, hipMemcpyHostToDevice));
        CK(hipMalloc(&c.out[s], nout * 4));
    }
    // agreement on buffer set 0
    std::vector<float> a(nout), b(nout);
    if (run_lds(c, 0) != 0) { fprintf(stderr, "%s\n", error_buffer()); exit(1); }
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(a.data(), c.out[0], nout * 4, hipMemcpyDeviceToHost));
    CK(hipMemset(c.out[0], 0xFF, nout * 4));
    if (run_loop(c, 0) != 0) { fprintf(stderr, "%s\n", error_buffer()); exit(1); }
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(b.data(), c.out[0], nout * 4, hipMemcpyDeviceToHost));
    double dmask = 0, dtaps = 0;
    for (long i = 0; i < nout; ++i) {
        const double d = std::fabs((double)a[i] - (double)b[i]);
        if (!(d == d)) { dmask = dtaps = NAN; break; }
        (i < c.nmask ? dmask : dtaps) = std::max(i < c.nmask ? dmask : dtaps, d);
    }
    for (int s = 0; s < 4; ++s) { run_lds(c, s); run_loop(c, s); }
    float ms[2][3];
    for (int r = 0; r < 3; ++r) {
        ms[0][r] = round_ms(run_lds, c, 20);
        ms[1][r] = round_ms(run_loop, c, 20);
    }
    const char* names[2] = {"lds", "loop"};
    for (int v = 0; v < 2; ++v) {
        std::sort(ms[v], ms[v] + 3);
        printf("{\"shape\": [%d, 2, %d, %d], \"variant\": \"%s\", \"ms\": %.4f, \"min_ms\": %.4f, \"max_ms\": %.4f, "
               "\"bytes\": %ld, \"max_diff_grad_mask\": %.3g, \"max_diff_taps\": %.3g}\n",
               BQ, h, w, names[v], ms[v][1], ms[v][0], ms[v][2], 4 * (nin + c.nmask + nout), dmask, dtaps);
    }
    fflush(stdout);
    CK(hipFree(c.in));
    for (int s = 0; s < 4; ++s) { CK(hipFree(c.mask[s])); CK(hipFree(c.out[s])); }
}

}  // namespace
}  // namespace alo

int main() {
    alo::one_case(4, 90, 160);
    alo::one_case(6, 46, 62);
    return 0;
}
