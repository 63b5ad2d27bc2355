// Device-side helpers shared by the kernel translation units of libfleetrec (gfx950 only): vector typedefs of the MFMA
// builtins, the launch-error macro, bf16 / e4m3 packing, 16-byte buffer loads.
#pragma once
#include <atomic>
#include <cstdlib>
#include <mutex>

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include "fr_internal.h"

// Two builds of the FC-chain kernel files (fr_fused.hip, fr_pipeline.hip, fr_gemm.hip).  libfleetrec.so: the kernels as they always were, without a line
// of epilogue code (FR_HAS_EPI 0: every epilogue argument folds to {NULL, 0} at compile time); a launch of a context WITH an epilogue is forwarded to
// the companion.  -DFR_EPI_FORMS -> libfleetrec_epi.so: the same bodies under names of their own (fr_epi_* / fc_epi_*), which apply the epilogues.
#ifdef FR_EPI_FORMS
#define FR_HAS_EPI 1
extern thread_local char fr_epi_noted[96];   // the companion's fr_note_kernel writes here (fr_fused.hip)
extern thread_local int fr_epi_hip_error;    // ... and its KCHECK keeps the launch error it consumed here, for the export to return
// what an export of the companion returns for a launcher's status: 0, the kept hipError_t, or hipErrorInvalidValue (a shape without an instantiation)
static inline int fr_epi_status(int rc) { return rc == 0 ? 0 : (fr_epi_hip_error ? fr_epi_hip_error : (int)hipErrorInvalidValue); }
#else
#define FR_HAS_EPI 0
#endif

#ifdef FR_EPI_FORMS
#define FR_KEEP_HIP_ERROR(e) (fr_epi_hip_error = (int)(e))
#else
#define FR_KEEP_HIP_ERROR(e) ((void)0)
#endif
#define KCHECK()                                                                          \
    do {                                                                                  \
        hipError_t e_ = hipGetLastError();                                                \
        if (e_ != hipSuccess) {                                                           \
            FR_KEEP_HIP_ERROR(e_);                                                        \
            fr_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
            return FR_ERR_HIP;                                                            \
        }                                                                                 \
    } while (0)

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE attribute of a kernel: raise it once per (instantiation, device),
// safely from concurrent driver threads.  One FrLdsAttrOnce lives next to each launcher (function-local static).
struct FrLdsAttrOnce {
    std::mutex m;
    std::atomic<unsigned long long> done[4] = {};  // one bit per device ordinal (256 devices)
};
template <class Kernel>
static inline int fr_allow_full_lds(Kernel kernel, FrLdsAttrOnce &once) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 256) FR_FAIL(FR_ERR_HIP, "hipGetDevice failed");
    const unsigned long long bit = 1ull << (dev & 63);
    if (once.done[dev >> 6].load(std::memory_order_acquire) & bit) return FR_OK;
    std::lock_guard<std::mutex> g(once.m);
    if (once.done[dev >> 6].load(std::memory_order_relaxed) & bit) return FR_OK;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
        FR_FAIL(FR_ERR_HIP, "hipFuncSetAttribute(max dynamic LDS) failed on device %d", dev);
    once.done[dev >> 6].fetch_or(bit, std::memory_order_release);
    return FR_OK;
}

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    const __bf16 a = (__bf16)lo, b = (__bf16)hi;  // v_cvt_pk_bf16_f32: round-to-nearest-even, NaN stays NaN
    return (uint32_t)__builtin_bit_cast(unsigned short, a) | ((uint32_t)__builtin_bit_cast(unsigned short, b) << 16);
}

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t pack_fp8x4(float a, float b, float c, float d, float scale) {
    const float lim = 448.0f;  // largest finite e4m3fn: values beyond it saturate (v_cvt_pk_fp8_f32 alone would return NaN above 448)
    // compares, not fminf / fmaxf: a NaN fails both and stays a NaN (the conversion keeps it), as in the fp32 and bf16 chains --
    // fminf(fmaxf(NaN, -448), 448) would quietly turn a corrupt table value into -448
    auto sat = [lim](float x) { x = x > lim ? lim : x; return x < -lim ? -lim : x; };
    a = sat(a * scale);
    b = sat(b * scale);
    c = sat(c * scale);
    d = sat(d * scale);
    int v = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    v = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, v, true);
    return (uint32_t)v;
}
__device__ __forceinline__ uint32_t pack_fp8_word(const uint4 &v, float scale) {
    return pack_fp8x4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w), scale);
}

// ---- per-layer epilogue (FrEpi, fr_internal.h) ------------------------------------------------------------------------------------------
// ReLU as the contract states it: v > 0 ? v : +0.0f.  The compare is written so that a NaN fails it and is kept (v_max_f32 alone would drop
// it); -0 and negatives become +0.
__device__ __forceinline__ float fr_relu(float v) { return v <= 0.0f ? 0.0f : v; }
// Four consecutive outputs n .. n + 3 of a layer, as every MFMA accumulator layout here holds them (registers 4i .. 4i + 3 of a 32 x 32 tile:
// n = n_tile + 8i + 4 (lane / 32) + c; of a 16 x 16 tile: n = n_tile + 4 (lane / 16) + c): the lane's n = n_uni + STRIDE * sel with n_uni
// wave-uniform (n_uni % 4 == 0) and sel = 0 .. NSEL - 1 the lane's half / quarter of the wave.  The NSEL aligned 16-byte bias fragments are read
// through the SCALAR cache (constant address space: nothing writes a bias while a kernel runs) and the lane picks its own with v_cndmask: no vector
// register is held across the read, which is what the fused kernels, full of accumulators, cannot spare.  Both branches are wave-uniform;
// without an epilogue nothing is added at all (-0 stays -0).
template <int NSEL = 2, int STRIDE = 4>
__device__ __forceinline__ void fr_epi4(float &a, float &b, float &c, float &d, const FrEpi &e, int n_uni, int sel) {
    typedef float cf4 __attribute__((ext_vector_type(4)));
    typedef const cf4 __attribute__((address_space(4))) *cf4_ptr;
    if (e.bias) {
        const cf4_ptr bp = (cf4_ptr)(uintptr_t)(e.bias + __builtin_amdgcn_readfirstlane(n_uni));
        cf4 b4 = bp[0];
#pragma unroll
        for (int s = 1; s < NSEL; s++) {
            const cf4 o = bp[s * STRIDE / 4];
            b4.x = sel == s ? o.x : b4.x;
            b4.y = sel == s ? o.y : b4.y;
            b4.z = sel == s ? o.z : b4.z;
            b4.w = sel == s ? o.w : b4.w;
        }
        a += b4.x;
        b += b4.y;
        c += b4.z;
        d += b4.w;
    }
    if (e.relu) {
        a = fr_relu(a);
        b = fr_relu(b);
        c = fr_relu(c);
        d = fr_relu(d);
    }
}

// The branch-free form of the fused kernels' epilogue forms (fr_fused.hip): the bias pointer is always there (a vector of -0.0f stands for "no
// bias": v + (-0.0f) == v for every v, -0 and NaN included) and ReLU is `v <= lo ? +0 : v` with lo = +0 (on) or NaN (off: nothing compares <= NaN).
template <int NSEL = 2, int STRIDE = 4>
__device__ __forceinline__ void fr_epi4_always(float &a, float &b, float &c, float &d, const float *bias, float lo, int n_uni, int sel) {
    typedef float cf4 __attribute__((ext_vector_type(4)));
    typedef const cf4 __attribute__((address_space(4))) *cf4_ptr;
    const cf4_ptr bp = (cf4_ptr)(uintptr_t)(bias + __builtin_amdgcn_readfirstlane(n_uni));
    cf4 b4 = bp[0];
#pragma unroll
    for (int s = 1; s < NSEL; s++) {
        const cf4 o = bp[s * STRIDE / 4];
        b4.x = sel == s ? o.x : b4.x;
        b4.y = sel == s ? o.y : b4.y;
        b4.z = sel == s ? o.z : b4.z;
        b4.w = sel == s ? o.w : b4.w;
    }
    a += b4.x;
    b += b4.y;
    c += b4.z;
    d += b4.w;
    a = a <= lo ? 0.0f : a;
    b = b <= lo ? 0.0f : b;
    c = c <= lo ? 0.0f : c;
    d = d <= lo ? 0.0f : d;
}

typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 bload4u(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
    const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0);
    return make_uint4(v.x, v.y, v.z, v.w);
}
// 16 bytes per lane through a buffer resource: per-lane byte offset in a VGPR, wave-uniform byte offset in an SGPR
__device__ __forceinline__ float4 bload4(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
    const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
