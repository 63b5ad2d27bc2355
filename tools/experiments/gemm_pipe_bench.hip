// Stand-alone timing harness for the LDS-tiled GEMM kernels of the product (includes csrc/fr_gemm.hip itself): Model-C FC1 / FC2 / FC3
// shapes at batch 4096, random bf16 / e4m3 operands, HIP events over back-to-back launches after a warm-up.
// The kernel is the one the product picks for the shape at chain width 1.
//   ./gemm_pipe_bench <prec: 1 bf16 | 2 fp8> [K N M]
#include "../../gpu-fpga-recommendation-system_amd/csrc/fr_gemm.hip"

#include <cstdarg>
#include <cstdio>
#include <vector>
void fr_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}

static char g_kernel[128];
void fr_note_kernel(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_kernel, sizeof g_kernel, fmt, ap);
    va_end(ap);
}
const char *fr_noted_kernel() { return g_kernel; }

int main(int argc, char **argv) {
    const int prec = argc > 1 ? atoi(argv[1]) : 1;
    const int K = argc > 2 ? atoi(argv[2]) : 3968, N = argc > 3 ? atoi(argv[3]) : 2048, M = argc > 4 ? atoi(argv[4]) : 4096;
    const int per16 = prec == 1 ? 8 : 16;               // k per 16-byte element
    const int KE = prec == 1 ? K / 8 : (K + 63) / 64 * 4;
    std::vector<uint32_t> hw((size_t)KE * N * 4), hx((size_t)KE * M * 4);
    uint32_t st = 12345u;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return st; };
    for (auto &v : hw) v = prec == 1 ? ((rnd() & 0x807F807Fu) | 0x3E003E00u) : (rnd() & 0xB7B7B7B7u);   // moderate magnitudes, random signs / mantissas
    for (auto &v : hx) v = prec == 1 ? ((rnd() & 0x807F807Fu) | 0x3E803E80u) : (rnd() & 0xB7B7B7B7u);
    void *dw, *dx, *dy;
    (void)hipMalloc(&dw, hw.size() * 4);
    (void)hipMalloc(&dx, hx.size() * 4);
    (void)hipMalloc(&dy, (size_t)N * M * 2);
    (void)hipMemcpy(dw, hw.data(), hw.size() * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(dx, hx.data(), hx.size() * 4, hipMemcpyHostToDevice);
    hipStream_t s;
    (void)hipStreamCreate(&s);
    if (!frk_fc_lp_gemm_ok(prec, K, N, M)) { printf("shape not served by the GEMM kernels\n"); return 1; }
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    for (int i = 0; i < 3000; i++) frk_fc_lp_gemm(prec, dw, dx, dy, K, N, M, 0, 0, 0, 1, false, s);   // ~0.2 s of load first: the clock ramps
    (void)hipStreamSynchronize(s);
    for (int w = 0; w < 3; w++) {
        const int reps = 500;
        (void)hipEventRecord(e0, s);
        for (int i = 0; i < reps; i++) frk_fc_lp_gemm(prec, dw, dx, dy, K, N, M, 0, 0, 0, 1, false, s);
        (void)hipEventRecord(e1, s);
        (void)hipEventSynchronize(e1);
        float ms;
        (void)hipEventElapsedTime(&ms, e0, e1);
        const double us = 1e3 * ms / reps, flops = 2.0 * K * N * M;
        printf("prec %d %dx%dx%d (%d k/elem) %s: %.2f us  %.3f PFLOP/s\n", prec, K, N, M, per16, fr_noted_kernel(), us, flops / (us * 1e-6) / 1e15);
    }
    return 0;
}
