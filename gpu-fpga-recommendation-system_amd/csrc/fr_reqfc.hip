// Factored FC1 of request-form batches (fr_worker_push_requests_factored_device / fr_worker_submit_requests_factored, fleetrec_serving.h)
// -> libfleetrec_reqfc.so, the seventh COMPANION code object of libfleetrec.so, built and linked as libfleetrec_request.so is.  It calls nothing of
// libfleetrec.so: each of its two launchers returns 0 or a hipError_t value.
//
// FC1 is linear in its input and a request's shared columns are the same for all of its candidates:
//     W1 x = W1[:, S] x_S(request) + W1[:, C] x_C(candidate)
// reqfc_user_kernel computes U[r][n] = sum_{k in S} W1[n][k] x[r][k] once per REQUEST, reqfc_cand_kernel computes V[b][n] = sum_{k in C} W1[n][k] x[b][k]
// per item, adds U[owner(b)], applies FC1's epilogue, rounds for the chain and stores R1 where stage 2 of the stage pipeline reads it.
//
// Operands are the stage pipeline's: feature-major 16-byte elements, E[row][column] with `row` = 4 k of fp32 (q4) or 8 k of bf16 (q8), so one
// 16-byte load per lane is four v_mfma_f32_32x32x2_f32 operands or one v_mfma_f32_32x32x16_bf16 operand (lane half hk = lane / 32 carries element
// row 2 g + hk of k-group g on both operands).  K_S and K_C are whatever the split leaves: a k-group whose second element row lies past the
// operand is loaded as zeros by the lanes of that half (0 x 0 adds +0 to a sum that started at +0: nothing changes).
//
// reqfc_user_kernel<PREC>: a skinny GEMM (M = n_req, often 1 .. 64), bound by the stream of W1_S, not by the MFMAs.  A workgroup of 4 waves owns
// ONE 32-request x 32-output accumulator tile and one of `nparts` <= 4 ranges of the k-groups; its waves take a quarter of that range each, so the
// weight stream of a tile is spread over 4 x nparts waves (Model-C: 32 n-tiles x 4 parts = 128 workgroups, 512 waves, each streaming 1 / 16 of a
// 32-output column block).  The four accumulators meet in LDS (16 KiB) and are summed in wave order; a part's tile goes to ITS partial buffer
// U_p[r][n] (request-major, [round_up(n_req, 32)][H1] fp32) as 16-byte stores of the four consecutive n a lane holds per accumulator group.  No
// atomics: the candidate kernel sums the partials in ascending p.
//
// reqfc_cand_kernel<PREC>: a workgroup of 4 waves owns 32 ITEMS x 128 outputs: every wave one 32 x 32 MFMA tile over the WHOLE K_C, both operands
// straight from L2 into registers as the stage-1 body does (the four waves load the same X_C elements: the second to fourth hit the CU's vector
// cache; W1_C is H1 x K_C x 4 bytes at most -- 1.8 MiB for Model-C -- and stays in every XCD's L2).  No K split and no LDS reduce here: with half of
// the columns on the request side the K loop is 14 .. 55 k-groups, and what a split-K tile would add (7 more LDS round trips per tile) is what the
// stage-1 body pays to fill the chip at batch 256 with a K twice as long.  LDS holds only the tile's 32 owners (128 bytes): thread t < 32 finds the
// owner of item m0 + t ONCE -- the last r with off[r] <= i by binary search, clamped into [0, n_req): request_expand_kernel's rule -- so a tile's
// owners are a contiguous range of requests and the U rows it reads are neighbours.  After the K loop lane (hk, lm) holds, per accumulator group i,
// outputs n = n0 + 8 i + 4 hk + (0 .. 3) of item m0 + lm: it loads U_0 .. U_{nparts-1}[owner][n .. n + 3] (16 bytes each), sums them in ascending
// p, adds the sum to its accumulators (s = fl(V + U)), applies FrEpi (launch-uniform branches; {NULL, 0} adds nothing: -0 stays -0), rounds (bf16:
// RNE, once) and stores the element of R1's [n / E][ldm][n % E] image, pad items [batch, ldm) included (their X_C columns are zeros).
// The pair checks on off ride along as in request_expand_kernel (system-scope atomicOr on the error path only).
// Bounds, for ANY content of off: owner is in [0, n_req) by the clamp, so U is read inside [0, round_up(n_req, 32) x H1) of every partial; X_C and
// R1 are addressed by m0 + lm < ldm and element rows below `rows` / H1 / E; off is read inside [0, n_req].
// Registers / LDS (tools/kernel_resources.py): see DESIGN.md section 3.1c-2.
#include <hip/hip_runtime.h>

#include "fr_device.h"

constexpr int RQ_THREADS = 256, RQ_WAVES = 4;

template <int PREC>
__device__ __forceinline__ void reqfc_mfma(f32x16 &acc, const uint4 &a, const uint4 &b) {
    if constexpr (PREC == 0) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
    } else {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
    }
}

// k-groups [g_begin, g_end) of a 32 x 32 tile: group g multiplies element rows 2 g + hk of both operands (A, B: the lane's column of element row 0).
// The groups that lie whole inside the operand run four at a time with their eight loads issued first; the last group of an odd row count reads
// zeros in the half-wave whose row is past the end.
template <int PREC>
__device__ __forceinline__ void reqfc_k_loop(f32x16 &acc, const uint4 *__restrict__ A, const uint4 *__restrict__ B, int g_begin, int g_end, int hk, int rows, size_t lda, size_t ldb) {
    const int whole = rows / 2, g_whole = g_end < whole ? g_end : whole;
    int k = g_begin;
    for (; k + 4 <= g_whole; k += 4) {
        uint4 a[4], b[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const size_t row = (size_t)(2 * (k + j) + hk);
            a[j] = A[row * lda], b[j] = B[row * ldb];
        }
#pragma unroll
        for (int j = 0; j < 4; j++) reqfc_mfma<PREC>(acc, a[j], b[j]);
    }
    for (; k < g_end; k++) {
        const int row = 2 * k + hk;
        uint4 a = make_uint4(0u, 0u, 0u, 0u), b = make_uint4(0u, 0u, 0u, 0u);
        if (row < rows) a = A[(size_t)row * lda], b = B[(size_t)row * ldb];
        reqfc_mfma<PREC>(acc, a, b);
    }
}

template <int PREC>
__global__ __launch_bounds__(RQ_THREADS) void reqfc_user_kernel(const FrReqfcUserArgs g) {
    __shared__ float red[RQ_WAVES * 16 * 64];   // 16 KiB
    const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int hk = lane >> 5, lm = lane & 31;
    const int tiles_n = g.H1 / 32, tiles = tiles_n * (g.ldr / 32);
    const int part = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - part * tiles;   // part < nparts: the grid is tiles x nparts
    const int n0 = (tile % tiles_n) * 32, r0 = (tile / tiles_n) * 32;
    // the part's range of k-groups, then this wave's quarter of it
    const int groups = (g.rows + 1) / 2, per_part = (groups + g.nparts - 1) / g.nparts;
    const int p_begin = part * per_part, p_end = p_begin + per_part < groups ? p_begin + per_part : groups;
    const int per_wave = (per_part + RQ_WAVES - 1) / RQ_WAVES;
    const int g_begin = p_begin + wave * per_wave, g_end = g_begin + per_wave < p_end ? g_begin + per_wave : p_end;
    const uint4 *A = static_cast<const uint4 *>(g.w) + n0 + lm, *B = static_cast<const uint4 *>(g.x) + r0 + lm;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0.0f;
    reqfc_k_loop<PREC>(acc, A, B, g_begin, g_end, hk, g.rows, (size_t)g.H1, (size_t)g.ldr);
#pragma unroll
    for (int r = 0; r < 16; r++) red[(wave * 16 + r) * 64 + lane] = acc[r];
    __syncthreads();
    // thread (i, l): accumulator group i of lane l, summed over the waves in wave order -> outputs n0 + 8 i + 4 (l / 32) + (0 .. 3) of request r0 + l % 32
    const int i = (int)threadIdx.x >> 6, l = (int)threadIdx.x & 63;
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        float s = red[(4 * i + c) * 64 + l];
#pragma unroll
        for (int w = 1; w < RQ_WAVES; w++) s += red[(w * 16 + 4 * i + c) * 64 + l];
        v[c] = s;
    }
    float *U = g.u + (size_t)part * (size_t)g.ldr * (size_t)g.H1;
    *reinterpret_cast<float4 *>(U + (size_t)(r0 + (l & 31)) * (size_t)g.H1 + (size_t)(n0 + 8 * i + 4 * (l >> 5))) = make_float4(v[0], v[1], v[2], v[3]);
}

template <int PREC>
__global__ __launch_bounds__(RQ_THREADS) void reqfc_cand_kernel(const FrReqfcCandArgs g) {
    __shared__ int s_owner[32];
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hk = lane >> 5, lm = lane & 31;
    const int tiles_n = g.H1 / 32, n_groups = (tiles_n + RQ_WAVES - 1) / RQ_WAVES;
    const int m0 = ((int)blockIdx.x / n_groups) * 32;                    // < ldm: the grid is (ldm / 32) x n_groups
    const int n_tile = ((int)blockIdx.x % n_groups) * RQ_WAVES + wave;   // may lie past the layer in the last group of an H1 that is no multiple of 128
    if (g.off) {
        bool bad = false;
        const size_t step = (size_t)gridDim.x * (size_t)RQ_THREADS;
        for (size_t j = (size_t)blockIdx.x * (size_t)RQ_THREADS + (size_t)tid; j < (size_t)g.n_req; j += step) bad |= g.off[j] > g.off[j + 1];
        if (blockIdx.x == 0 && tid == 0) bad |= g.off[0] != 0 || g.off[g.n_req] != g.batch;
        if (bad) atomicOr_system(g.err_flag, 1);   // pinned host word; error path only
    }
    if (tid < 32) {
        const int i = m0 + tid;   // a pad item (i >= batch) takes the last request: its column of X_C is zeros and nothing reads its R1
        int r;
        if (g.off) {   // lo = how many of off[0 .. n_req) are <= i, were the array sorted; any array leaves lo in [0, n_req]
            int lo = 0, hi = g.n_req;
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if (g.off[mid] <= i) lo = mid + 1;
                else hi = mid;
            }
            r = lo - 1;
        } else {
            r = i / (g.batch / g.n_req);   // (the host refused batch % n_req != 0: n_req <= batch)
        }
        s_owner[tid] = r < 0 ? 0 : (r >= g.n_req ? g.n_req - 1 : r);
    }
    __syncthreads();
    if (n_tile >= tiles_n) return;   // wave-uniform, behind the workgroup's only barrier
    const int n0 = n_tile * 32;
    const uint4 *A = static_cast<const uint4 *>(g.w) + n0 + lm, *B = static_cast<const uint4 *>(g.x) + m0 + lm;
    const int groups = (g.rows + 1) / 2;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0.0f;
    reqfc_k_loop<PREC>(acc, A, B, 0, groups, hk, g.rows, (size_t)g.H1, (size_t)g.ldm);
    const size_t u_part = (size_t)g.ldr * (size_t)g.H1;
    const float *Urow = g.u + (size_t)s_owner[lm] * (size_t)g.H1 + (size_t)(n0 + 4 * hk);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        float4 u = *reinterpret_cast<const float4 *>(Urow + 8 * i);
        for (int p = 1; p < g.nparts; p++) {   // the partials of the K_S sum, in ascending order
            const float4 q = *reinterpret_cast<const float4 *>(Urow + (size_t)p * u_part + 8 * i);
            u.x += q.x, u.y += q.y, u.z += q.z, u.w += q.w;
        }
        float v0 = acc[4 * i] + u.x, v1 = acc[4 * i + 1] + u.y, v2 = acc[4 * i + 2] + u.z, v3 = acc[4 * i + 3] + u.w;
        fr_epi4(v0, v1, v2, v3, g.epi, n0 + 8 * i, hk);   // n = n0 + 8 i + 4 hk + c
        if constexpr (PREC == 0) {   // q4 element (n / 4, m)
            reinterpret_cast<float4 *>(g.r1)[(size_t)((n0 >> 2) + 2 * i + hk) * (size_t)g.ldm + (size_t)(m0 + lm)] = make_float4(v0, v1, v2, v3);
        } else {                     // half hk of q8 element (n / 8, m): ONE rounding to bf16
            reinterpret_cast<uint2 *>(g.r1)[((size_t)((n0 >> 3) + i) * (size_t)g.ldm + (size_t)(m0 + lm)) * 2 + (size_t)hk] = make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
        }
    }
}

extern "C" __attribute__((visibility("default"))) int fr_reqfc_user_launch(const FrReqfcUserArgs *args, void *stream) {
    const FrReqfcUserArgs g = *args;
    const dim3 grid((unsigned)((g.H1 / 32) * (g.ldr / 32) * g.nparts)), block(RQ_THREADS);
    if (g.precision == FR_FC_BF16) reqfc_user_kernel<1><<<grid, block, 0, (hipStream_t)stream>>>(g);
    else reqfc_user_kernel<0><<<grid, block, 0, (hipStream_t)stream>>>(g);
    return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("default"))) int fr_reqfc_cand_launch(const FrReqfcCandArgs *args, void *stream) {
    const FrReqfcCandArgs g = *args;
    const dim3 grid((unsigned)((g.ldm / 32) * ((g.H1 / 32 + RQ_WAVES - 1) / RQ_WAVES))), block(RQ_THREADS);
    if (g.precision == FR_FC_BF16) reqfc_cand_kernel<1><<<grid, block, 0, (hipStream_t)stream>>>(g);
    else reqfc_cand_kernel<0><<<grid, block, 0, (hipStream_t)stream>>>(g);
    return (int)hipGetLastError();
}
