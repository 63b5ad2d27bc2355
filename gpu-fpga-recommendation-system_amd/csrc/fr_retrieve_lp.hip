// bf16 retrieval over a fragment-major table image (fr_ctx_set_retrieve_image, fr_worker_retrieve_image_device / fr_worker_retrieve_image,
// fleetrec_serving.h) -> libfleetrec_retrieve_lp.so, the ninth COMPANION code object of libfleetrec.so, built and linked as libfleetrec_retrieve.so is.  It
// calls nothing of libfleetrec.so: each of its two launchers returns 0 or a hipError_t value.  DESIGN.md section 3.1f has the reasoning.
//
// The image (fr_internal.h states the layout): tile T (rows 32 T .. 32 T + 31 by ABSOLUTE row), step s (columns 16 s .. 16 s + 15) is one 1024-byte block
// in which lane (n, h) = (lane % 32, lane / 32) owns the 16 bytes (T * steps + s) * 64 + lane: the B operand of v_mfma_f32_32x32x16_bf16 as it sits in
// registers.  Pads (columns >= dim, rows >= the table's rows) are +0.
//
// retrieve_lp_image_kernel: one thread per 16-byte image word, threads in ROW-major order (thread i: row i / (2 steps), word i % (2 steps)), so the 32-byte
//   reads of neighbouring threads are neighbours in the fp32 table; a row's words go to 2 steps different blocks, the 32 rows of a tile fill them.  Range arm:
//   tiles [tile0, tile0 + n_tiles) whole, pads included.  List arm: the words of the listed rows, an id outside [0, rows) does nothing; a row listed
//   twice is converted twice from the same fp32 words.  The arm is chosen once, around the body.
//
// retrieve_lp_scan_kernel<KP>: workgroup (chunk, query tile) = 4 waves, 32 queries.  Chunks start at A = row0 & ~31, a tile boundary, and are multiples of
//   128 rows, so every chunk begins on a tile of the image; rows of the first tile below row0 are masked exactly as rows at and past the window's end are.
//   A operand: lane (n, h) converts columns 16 s + 8 h .. + 7 of query q0 + n from the caller's fp32 to bf16 (RNE) once: steps x 4 VGPRs.  Query
//     columns >= dim (and queries >= n_q) are bf16 -0, and the sign of a ZERO score is set behind the MFMAs: fr_retrieve_lp_scan.h has the reasoning.
//   B operand: in round r wave w takes tile (c_begin / 32) + 4 r + w (lp_load).  The loads of round r + 1 are issued before the MFMAs of round r.
//   Selection: the accumulator layout is the fp32 kernel's (lane (n, h): queries 8 (v / 4) + 4 h + v % 4 of ITS row), and so is everything behind it --
//     composites, one mask and one branch per round, the __syncthreads_or vote, the one-wave leader reductions of fr_retrieve_select.h, BUF = kp + S + 128.
//   Shared with the probed and the filtered image scan (fr_retrieve_lp_scan.h, fr_retrieve_select.h): the operand masks, the B load, the MFMA steps and
//     the tile's leader reduction.  The A operand's build, the zero-sign fix and the threshold test with its appends are written out in each of the three:
//     as functions they changed this kernel's code (DESIGN.md section 3.1f has the figures).
//   KP = 64: BUF = 256 (64 KB of LDS, two workgroups per CU at every dim); KP = 256: BUF = 512 (128 KB, one).  dim is a run-time bound over steps <= 8.
//   The planes and the segment offsets are written in the fp32 scan's format: the ranking and retrieve_rows_kernel follow unchanged.
// Bounds: the image is read at tiles [c_begin / 32, (c_end - 1) / 32] <= tiles - 1, steps below `steps`; queries below n_q and columns below dim; the
//   planes at ((q * n_chunks + chunk) * k + j), j < k.  The image kernel reads table rows below `rows`, columns below dim, and writes words of tiles
//   below ceil(rows / 32).
#include <hip/hip_runtime.h>

#include "fr_retrieve_lp_scan.h"

__global__ __launch_bounds__(RT_THREADS) void retrieve_lp_image_kernel(const FrRetrieveImageArgs g) {
    const int steps = fr_retrieve_image_steps(g.dim), wpr = 2 * steps;
    const int64_t i = (int64_t)blockIdx.x * RT_THREADS + (int64_t)threadIdx.x;
    const int64_t e = i / wpr;
    const int j = (int)(i - e * wpr), s = j >> 1, h = j & 1;
    int64_t row;
    if (g.ids) {
        if (e >= (int64_t)g.n) return;
        row = (int64_t)g.ids[e];
        if (row < 0 || row >= g.rows) return;
    } else {
        if (e >= g.n_tiles * FR_RETRIEVE_IMAGE_TILE) return;
        row = g.tile0 * FR_RETRIEVE_IMAGE_TILE + e;
    }
    const int c0 = FR_RETRIEVE_IMAGE_STEP * s + 8 * h;
    float4 lo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hi = lo;
    if (row < g.rows) {
        const float4 *p = reinterpret_cast<const float4 *>(g.table + (size_t)row * (size_t)g.dim + c0);
        if (c0 < g.dim) lo = p[0];
        if (c0 + 4 < g.dim) hi = p[1];
    }
    g.image[((size_t)(row >> 5) * (size_t)steps + (size_t)s) * 64 + (size_t)(32 * h + (int)(row & 31))] = lp_pack8(lo, hi);
}

template <int KP>
__global__ __launch_bounds__(RT_THREADS, KP <= 64 ? 2 : 1) void retrieve_lp_scan_kernel(const FrRetrieveLpArgs ga) {
    constexpr int BUF = KP <= 64 ? 256 : 512;
    __shared__ u64 buf[FR_RETRIEVE_QTILE * BUF];
    __shared__ u64 thr[FR_RETRIEVE_QTILE];
    __shared__ int cnt[FR_RETRIEVE_QTILE];
    __shared__ u64 qmask[FR_RETRIEVE_QTILE][2][2];   // [query][half h][zero, sign]: bit 8 s + j = column 16 s + 8 h + j of the query as bf16
    const FrRetrieveArgs &g = ga.r;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, h = lane >> 5;
    const int dim = g.dim, steps = fr_retrieve_image_steps(dim);
    const int k = g.k, kp = pow2_ceil(k), S = BUF - kp - FR_RETRIEVE_ROUND;
    const int q0 = (int)blockIdx.y * FR_RETRIEVE_QTILE, chunk = (int)blockIdx.x;
    const int64_t c_begin = (g.row0 & ~(int64_t)(FR_RETRIEVE_IMAGE_TILE - 1)) + (int64_t)chunk * g.chunk;   // a tile boundary; <= row0 in chunk 0 only
    const int64_t w_end = g.row0 + g.n_rows;
    const int64_t c_end = c_begin + g.chunk < w_end ? c_begin + g.chunk : w_end;                            // > c_begin, > row0
    const int64_t t_begin = c_begin >> 5, t_last = (c_end - 1) >> 5;                                        // t_last < ga.tiles: c_end <= the table's rows

    for (int i = tid; i < FR_RETRIEVE_QTILE * BUF; i += RT_THREADS) buf[i] = 0ull;
    if (tid < FR_RETRIEVE_QTILE) thr[tid] = 0ull, cnt[tid] = 0;

    uint4 a[LP_MAX_STEPS];
    {
        const bool live = q0 + n < g.n_q;
        const float *qp = g.queries + (size_t)(live ? q0 + n : 0) * (size_t)dim;
#pragma unroll
        for (int s = 0; s < LP_MAX_STEPS; s++) {
            float x[8];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int c = FR_RETRIEVE_IMAGE_STEP * s + 8 * h + j;
                x[j] = live && c < dim ? qp[c] : -0.0f;
            }
            a[s] = lp_pack8(make_float4(x[0], x[1], x[2], x[3]), make_float4(x[4], x[5], x[6], x[7]));
        }
        u64 z, sg;
        lp_masks(a, LP_MAX_STEPS, z, sg);
        if (wave == 0) qmask[n][h][0] = z, qmask[n][h][1] = sg;
    }
    uint32_t live_v = 0u;   // bit v: the lane's accumulator v belongs to a query below n_q
#pragma unroll
    for (int v = 0; v < 16; v++) live_v |= (q0 + 8 * (v >> 2) + 4 * h + (v & 3) < g.n_q ? 1u : 0u) << v;
    __syncthreads();

    const int rounds = (int)((c_end - c_begin + FR_RETRIEVE_ROUND - 1) / FR_RETRIEVE_ROUND);
    uint4 b[LP_MAX_STEPS], nb[LP_MAX_STEPS];
    lp_load(nb, ga.image, t_begin + wave, t_last, steps, lane);
    for (int r = 0; r < rounds; r++) {
        const int64_t tile = t_begin + (int64_t)(RT_WAVES * r + wave);
        const int64_t row = tile * FR_RETRIEVE_IMAGE_TILE + n;
#pragma unroll
        for (int s = 0; s < LP_MAX_STEPS; s++) b[s] = nb[s];
        if (r + 1 < rounds) lp_load(nb, ga.image, tile + RT_WAVES, t_last, steps, lane);
        f32x16 acc = lp_scores(a, b, steps);
        // the sign of a zero score is set here, not taken from the MFMA (fr_retrieve_lp_scan.h has the reasoning).  The scores of the query tile's slots
        // past n_q, all -0, are not looked at: one wave-uniform branch, rarely taken.
        bool zero = false;
        uint32_t live_l = live_v;
        asm volatile("" : "+v"(live_l));   // (kept one register: its 16 bit tests are not hoisted into 16 lane masks)
#pragma unroll
        for (int v = 0; v < 16; v++) zero |= (live_l >> v & 1u) && (__float_as_uint(acc[v]) & 0x7fffffffu) == 0u;
        if (__builtin_amdgcn_ballot_w64(zero) != 0ull) {
            u64 rz[2], rs[2];   // [half]
            int steps_z = steps;
            asm volatile("" : "+s"(steps_z));   // (as in lp_load)
            lp_masks(b, steps_z, rz[h], rs[h]);
            rz[1 - h] = __shfl_xor(rz[h], 32), rs[1 - h] = __shfl_xor(rs[h], 32);
            const u64 valid = steps >= LP_MAX_STEPS ? ~0ull : (1ull << (8 * steps)) - 1ull;   // (steps past the table's: the query's -0 against no operand at all)
#pragma unroll
            for (int v = 0; v < 16; v++) {
                if ((__float_as_uint(acc[v]) & 0x7fffffffu) == 0u) {
                    const int qi = 8 * (v >> 2) + 4 * h + (v & 3);
                    const u64 m0 = (rz[0] | qmask[qi][0][0]) & (rs[0] ^ qmask[qi][0][1]), m1 = (rz[1] | qmask[qi][1][0]) & (rs[1] ^ qmask[qi][1][1]);
                    acc[v] = (m0 & m1 & valid) == valid ? -0.0f : 0.0f;
                }
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
        if (row < g.row0 || row >= c_end) pass = 0u;
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
            scan_reduce<BUF>(buf, thr, cnt, k, kp, lane, wave);
            __syncthreads();
        }
    }
    scan_reduce<BUF>(buf, thr, cnt, k, kp, lane, wave);
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

extern "C" __attribute__((visibility("default"))) int fr_retrieve_lp_image_launch(const FrRetrieveImageArgs *args, void *stream) {
    const FrRetrieveImageArgs g = *args;
    const int64_t words = (g.ids ? (int64_t)g.n : g.n_tiles * FR_RETRIEVE_IMAGE_TILE) * 2 * fr_retrieve_image_steps(g.dim);
    if (words <= 0) return 0;
    retrieve_lp_image_kernel<<<dim3((unsigned)((words + RT_THREADS - 1) / RT_THREADS)), dim3(RT_THREADS), 0, (hipStream_t)stream>>>(g);
    return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("default"))) int fr_retrieve_lp_scan_launch(const FrRetrieveLpArgs *args, void *stream) {
    const FrRetrieveLpArgs g = *args;
    const dim3 grid((unsigned)g.r.n_chunks, (unsigned)((g.r.n_q + FR_RETRIEVE_QTILE - 1) / FR_RETRIEVE_QTILE));
    if (g.r.k <= 64) retrieve_lp_scan_kernel<64><<<grid, dim3(RT_THREADS), 0, (hipStream_t)stream>>>(g);
    else retrieve_lp_scan_kernel<256><<<grid, dim3(RT_THREADS), 0, (hipStream_t)stream>>>(g);
    return (int)hipGetLastError();
}
