// What the three bf16 image scans have in common beyond fr_retrieve_select.h: retrieve_lp_scan_kernel (fr_retrieve_lp.hip), retrieve_probe_lp_scan_kernel
// (fr_retrieve_probe_lp.hip) and retrieve_filter_scan_kernel (fr_retrieve_filter.hip).  Device code only; every function is inlined into its kernel, so
// nothing here appears in a code object under a name of its own.
//
// A piece lives here only if, with it, every kernel of every retrieval code object keeps the instruction sequence and the register, LDS and scratch
// counts it had with the piece written out in its kernel.  The B operand's load, the MFMA steps and the operand masks pass; the zero-sign fix, the
// threshold test and append, and the A operand's build do not in any form tried, and stay one copy per kernel: DESIGN.md section 3.1f has each
// piece's figures.
//
// The sign of a zero score.  Query columns >= dim, query slots without a query and the image's pads make products of -0 x +0 = -0, the identity of the
// addition, and accumulators start at -0, so that a score whose every product is -0 is -0, as the CPU twin's ascending sum from -0 gives it.  The bf16
// MFMA does not keep that sign (measured: it returns +0 where every term is -0).  Each scan therefore sets the sign of a ZERO score behind its MFMAs,
// from the zero and sign bit masks of the two operands (lp_masks: a query's sit in LDS from the start, a row's are made from the B registers when a wave
// meets a zero score and exchanged between the half-waves): -0 exactly when every product is -0 -- one operand zero, the signs different --, +0
// otherwise.  Zero scores that are looked at are rare: one wave-uniform branch.
#pragma once
#include "fr_device.h"
#include "fr_retrieve_select.h"

constexpr int LP_MAX_STEPS = FR_RETRIEVE_MAX_DIM / FR_RETRIEVE_IMAGE_STEP;   // 8

static __device__ __forceinline__ uint4 lp_pack8(const float4 &lo, const float4 &hi) {
    return make_uint4(pack_bf16x2(lo.x, lo.y), pack_bf16x2(lo.z, lo.w), pack_bf16x2(hi.x, hi.y), pack_bf16x2(hi.z, hi.w));
}

// of the first `steps` operand words of a lane (8 bf16 each): bit 8 s + j of z = element j of word s is a zero, of sg = its sign bit
static __device__ __forceinline__ void lp_masks(const uint4 (&w)[LP_MAX_STEPS], int steps, u64 &z, u64 &sg) {
    z = 0ull, sg = 0ull;
#pragma unroll
    for (int s = 0; s < LP_MAX_STEPS; s++) {
        if (s < steps) {
            const uint32_t d[4] = {w[s].x, w[s].y, w[s].z, w[s].w};
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const uint32_t e = (d[j >> 1] >> (16 * (j & 1))) & 0xffffu;
                z |= (u64)((e & 0x7fffu) == 0u) << (8 * s + j);
                sg |= (u64)(e >> 15) << (8 * s + j);
            }
        }
    }
}

// the B operand of image tile min(tile, t_last): one 16-byte load per (lane, step), 1 KB contiguous per wave and step, straight into the MFMA's register
// order -- no LDS, no transpose.  (A tile past t_last, the scan's last, loads t_last: its scores are never looked at.)
static __device__ __forceinline__ void lp_load(uint4 (&b)[LP_MAX_STEPS], const uint4 *image, int64_t tile, int64_t t_last, int steps, int lane) {
    int steps_l = steps;
    asm volatile("" : "+s"(steps_l));   // compared inside the loop, not hoisted into eight lane masks held for the whole kernel
    const uint4 *p = image + (size_t)(tile < t_last ? tile : t_last) * (size_t)steps * 64 + (size_t)lane;
#pragma unroll
    for (int s = 0; s < LP_MAX_STEPS; s++)
        if (s < steps_l) b[s] = p[s * 64];
}

// the 32 x 32 scores of a query tile against an image tile, in the fp32 scan's accumulator layout; accumulators start at -0
static __device__ __forceinline__ f32x16 lp_scores(const uint4 (&a)[LP_MAX_STEPS], const uint4 (&b)[LP_MAX_STEPS], int steps) {
    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; v++) acc[v] = -0.0f;
    int steps_l = steps;
    asm volatile("" : "+s"(steps_l));   // (as in lp_load)
#pragma unroll
    for (int s = 0; s < LP_MAX_STEPS; s++)
        if (s < steps_l) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[s]), __builtin_bit_cast(bf16x8, b[s]), acc, 0, 0, 0);
    return acc;
}
