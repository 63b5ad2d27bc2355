// Top-K inner-product retrieval over a table window (fr_worker_retrieve_device / fr_worker_retrieve, fleetrec_serving.h) -> libfleetrec_retrieve.so,
// the eighth COMPANION code object of libfleetrec.so, built and linked as libfleetrec_rank.so is.  It calls nothing of libfleetrec.so: its one
// launcher returns 0 or a hipError_t value.  DESIGN.md section 3.1e has the reasoning and the measurements.
//
// The score matrix [n_q][n_rows] is never stored: a workgroup scores 32 queries x 128 rows per ROUND in MFMA accumulators, and only a composite
// that beats its query's current k-th best leaves the registers.
//
// retrieve_scan_kernel<KP, NT>: workgroup (chunk, query tile) = 4 waves, 32 queries, one chunk of the window.
//   A operand: lane (n, h) = (lane % 32, lane / 32) holds the 16-byte words h, h + 2, h + 4, ... of query q0 + n for the whole chunk (NT float4).
//   B operand: in round r wave w takes rows c_begin + 32 (4 r + w) + n: lane (n, h) loads the SAME words of its table row straight from HBM, so MFMA
//     step 4 t + e multiplies columns 8 t + e (h = 0) and 8 t + 4 + e (h = 1) of both: the k order is a permutation, the same for every row, and no
//     transpose through LDS is needed.  The loads of round r + 1 are issued before the MFMAs of round r.  A dim with an odd word count leaves the
//     h = 1 lanes of the last t without a word: they feed -0 x +0.  Accumulators start at -0 as well (the identity of the addition), so a row
//     whose products are all -0 scores -0, as the ascending sum of the CPU back-end does.
//   Selection: lane (n, h) ends a round with the scores of queries 8 (v / 4) + 4 h + v % 4, v < 16, for ITS row.  Each becomes the composite
//     (fr_rank_key << 32) | (0xffffffff - (row - row0)) of fr_rank.hip -- all distinct, none 0 -- and is appended (LDS atomic counter) to the query's
//     buffer only when it beats thr[q], the query's k-th composite so far (0 until k rows were seen).  Buffer of a query: BUF u64 = kp leaders,
//     descending, then the append area; kp = pow2_ceil(k).  A round appends at most 128 composites per query, the vote behind every round
//     (__syncthreads_or: uniform over the workgroup) starts a reduction as soon as one counter has passed S = BUF - kp - 128, so a counter never
//     passes BUF - kp: nothing is dropped and nothing is written past a buffer, whatever the order of the rows.
//   Reduction: wave w takes queries w, w + 4, ...: the bitonic leader reduction of fr_rank.hip (runs of kp sorted in alternating directions, pairs
//     of runs halved by max until one run is left) over the next power of two of what the buffer holds, by the 64 lanes of ONE wave -- DS
//     instructions of a wave execute in order, so the steps are fenced for the compiler only and no workgroup barrier is spent on them.
//   KP = 64: BUF = 256 (64 KB of LDS, two workgroups per CU); KP = 256: BUF = 512 (128 KB, one).  NT = 4 serves dim <= 32, NT = 16 dim <= 128.
//   End of chunk: the k leaders of every query go to the planes as (score bits, row); entries behind the chunk's rows are (NaN, -1).
// fr_rank_launch (the host code calls it between the two steps) ranks the n_chunks * k partial scores of every query as one segment: lists are in
//   chunk order = row order and equal scores inside a list are in row order, so its "lower position first" is "lower row first"; pads can only sit
//   at the end of the last list (chunk >= 1024 >= k) and carry the lowest key.
// retrieve_rows_kernel: position -> (row, score bits); a pad or no position -> (-1, -inf).
// Bounds: table rows are read inside [c_begin, c_end) of the window only, words below dim / 4; queries below n_q; the planes at
//   ((q * n_chunks + chunk) * k + j), j < k; the outputs at q * k + j.  A NaN score is delivered as the quiet NaN 0x7fc00000.
#include <hip/hip_runtime.h>

#include "fr_internal.h"
#include "fr_retrieve_select.h"

template <int KP, int NT>
__global__ __launch_bounds__(RT_THREADS, KP <= 64 && NT <= 4 ? 2 : 1) void retrieve_scan_kernel(const FrRetrieveArgs g) {
    constexpr int BUF = KP <= 64 ? 256 : 512;
    __shared__ u64 buf[FR_RETRIEVE_QTILE * BUF];
    __shared__ u64 thr[FR_RETRIEVE_QTILE];
    __shared__ int cnt[FR_RETRIEVE_QTILE];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, h = lane >> 5;
    const int dim = g.dim, W = dim >> 2, nt = (W + 1) >> 1;
    const int k = g.k, kp = pow2_ceil(k), S = BUF - kp - FR_RETRIEVE_ROUND;
    const int q0 = (int)blockIdx.y * FR_RETRIEVE_QTILE, chunk = (int)blockIdx.x;
    const int64_t c_begin = g.row0 + (int64_t)chunk * g.chunk;
    const int64_t w_end = g.row0 + g.n_rows;
    const int64_t c_end = c_begin + g.chunk < w_end ? c_begin + g.chunk : w_end;

    for (int i = tid; i < FR_RETRIEVE_QTILE * BUF; i += RT_THREADS) buf[i] = 0ull;
    if (tid < FR_RETRIEVE_QTILE) thr[tid] = 0ull, cnt[tid] = 0;

    float4 a[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) {
        a[t] = make_float4(-0.0f, -0.0f, -0.0f, -0.0f);
        if (t < nt && h + 2 * t < W && q0 + n < g.n_q) {
            const float *p = g.queries + (size_t)(q0 + n) * (size_t)dim + 4 * (h + 2 * t);
            a[t] = make_float4(p[0], p[1], p[2], p[3]);
        }
    }
    // rows past the chunk load the chunk's last row (their scores are never looked at), a word past the row loads the row's last word and counts as +0
    auto load = [&](float4(&b)[NT], int64_t row) {
        int nt_l = nt, W_l = W;
        asm volatile("" : "+s"(nt_l), "+s"(W_l));   // compared inside the loop: hoisted out of it, every comparison below holds a lane mask in two SGPRs for the whole kernel
        const float4 *p = reinterpret_cast<const float4 *>(g.table + (size_t)(row < c_end ? row : c_end - 1) * (size_t)dim);
#pragma unroll
        for (int t = 0; t < NT; t++) {
            if (t < nt_l) {
                const int w = h + 2 * t;
                const float4 x = p[w < W_l ? w : W_l - 1];
                b[t] = w < W_l ? x : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
    };
    // through a lambda: with scan_reduce called at its two places directly, two VGPRs of wave_ce_step's loop trade names in this kernel and in
    // retrieve_probe_scan_kernel (32 instructions each, no count changes); the bf16 scans call it directly
    auto reduce = [&]() { scan_reduce<BUF>(buf, thr, cnt, k, kp, lane, wave); };
    __syncthreads();

    const int rounds = (int)((c_end - c_begin + FR_RETRIEVE_ROUND - 1) / FR_RETRIEVE_ROUND);
    float4 b[NT], nb[NT];
    load(nb, c_begin + 32 * wave + n);
    for (int r = 0; r < rounds; r++) {
        const int64_t row = c_begin + (int64_t)(RT_WAVES * r + wave) * 32 + n;
#pragma unroll
        for (int t = 0; t < NT; t++) b[t] = nb[t];
        if (r + 1 < rounds) load(nb, row + FR_RETRIEVE_ROUND);
        f32x16 acc;
#pragma unroll
        for (int v = 0; v < 16; v++) acc[v] = -0.0f;
        int nt_l = nt;
        asm volatile("" : "+s"(nt_l));   // (as in load)
#pragma unroll
        for (int t = 0; t < NT; t++) {
            if (t < nt_l) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t].x, b[t].x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t].y, b[t].y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t].z, b[t].z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t].w, b[t].w, acc, 0, 0, 0);
            }
        }
        // the common case leaves nothing to append: the 16 comparisons become one bit mask, and one branch skips the appends
        int over = 0;
        const u64 low = (u64)(0xffffffffu - (uint32_t)(row - g.row0));
        uint32_t key[16], pass = 0u;
#pragma unroll
        for (int v = 0; v < 16; v++) {
            const int qi = 8 * (v >> 2) + 4 * h + (v & 3);
            key[v] = fr_rank_key(__float_as_uint(acc[v]));
            pass |= ((((u64)key[v] << 32) | low) > thr[qi] ? 1u : 0u) << v;
        }
        if (row >= c_end) pass = 0u;
        if (pass) {
#pragma unroll
            for (int v = 0; v < 16; v++) {
                const int qi = 8 * (v >> 2) + 4 * h + (v & 3);
                if ((pass >> v & 1u) && q0 + qi < g.n_q) {
                    const int slot = atomicAdd(&cnt[qi], 1);
                    if (kp + slot < BUF) buf[qi * BUF + kp + slot] = ((u64)key[v] << 32) | low;   // (always: a counter starts a round at S or less)
                    over |= slot >= S;
                }
            }
        }
        if (__syncthreads_or(over)) {
            reduce();
            __syncthreads();
        }
    }
    reduce();
    __syncthreads();

    for (int e = tid; e < FR_RETRIEVE_QTILE * k; e += RT_THREADS) {
        const int qi = e / k, j = e - qi * k, q = q0 + qi;
        if (q >= g.n_q) break;
        const u64 c = buf[qi * BUF + j];
        const size_t o = ((size_t)q * (size_t)g.n_chunks + (size_t)chunk) * (size_t)k + (size_t)j;
        g.part_scores[o] = __uint_as_float(c ? retrieve_bits((uint32_t)(c >> 32)) : FR_RETRIEVE_PAD_BITS);
        g.part_rows[o] = c ? (int32_t)(g.row0 + (int64_t)(0xffffffffu - (uint32_t)c)) : -1;
    }
    if (chunk == 0 && tid < FR_RETRIEVE_QTILE && q0 + tid < g.n_q) {
        const int q = q0 + tid, per = g.n_chunks * k;
        g.seg_off[q] = q * per;
        if (q == g.n_q - 1) g.seg_off[g.n_q] = g.n_q * per;
    }
}

__global__ __launch_bounds__(RT_THREADS) void retrieve_rows_kernel(const FrRetrieveArgs g) {
    const int64_t e = (int64_t)blockIdx.x * RT_THREADS + (int64_t)threadIdx.x;
    if (e >= (int64_t)g.n_q * g.k) return;
    const int q = (int)(e / g.k), per = g.n_chunks * g.k;
    const int pos = g.top_pos[e];
    int32_t row = -1;
    uint32_t bits = 0xff800000u;
    if (pos >= 0 && pos < per) {
        const size_t o = (size_t)q * (size_t)per + (size_t)pos;
        row = g.part_rows[o];
        if (row >= 0) bits = __float_as_uint(g.part_scores[o]);
    }
    g.top_rows[e] = row;
    if (g.top_scores) g.top_scores[e] = __uint_as_float(bits);
}

extern "C" __attribute__((visibility("default"))) int fr_retrieve_launch(const FrRetrieveArgs *args, int step, void *stream) {
    const FrRetrieveArgs g = *args;
    hipStream_t s = (hipStream_t)stream;
    if (step == 1) {
        const int64_t n = (int64_t)g.n_q * g.k;
        retrieve_rows_kernel<<<dim3((unsigned)((n + RT_THREADS - 1) / RT_THREADS)), dim3(RT_THREADS), 0, s>>>(g);
        return (int)hipGetLastError();
    }
    const dim3 grid((unsigned)g.n_chunks, (unsigned)((g.n_q + FR_RETRIEVE_QTILE - 1) / FR_RETRIEVE_QTILE));
    const bool wide = g.dim > 32, deep = g.k > 64;
    if (!wide && !deep) retrieve_scan_kernel<64, 4><<<grid, dim3(RT_THREADS), 0, s>>>(g);
    else if (!wide) retrieve_scan_kernel<256, 4><<<grid, dim3(RT_THREADS), 0, s>>>(g);
    else if (!deep) retrieve_scan_kernel<64, 16><<<grid, dim3(RT_THREADS), 0, s>>>(g);
    else retrieve_scan_kernel<256, 16><<<grid, dim3(RT_THREADS), 0, s>>>(g);
    return (int)hipGetLastError();
}
