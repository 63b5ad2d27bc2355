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
//     columns >= dim (and queries >= n_q) are bf16 -0: against the image's +0 pads the product is -0, the identity of the addition, and accumulators start
//     at -0.  The bf16 MFMA does not keep the sign of such a sum (measured: it returns +0 where every term is -0), so the sign of a ZERO score is set
//     behind the MFMAs from the operands' zero and sign bit masks (a query's masks sit in LDS, a row's are made from the B registers when a wave meets a
//     zero score): -0 exactly when every product is -0, as the CPU twin's ascending sum from -0 gives it.
//   B operand: in round r wave w takes tile (c_begin / 32) + 4 r + w: one 16-byte load per (lane, step), 1 KB contiguous per wave and step, straight into
//     the MFMA's register order -- no LDS, no transpose.  The loads of round r + 1 are issued before the MFMAs of round r.  A tile past the chunk's last
//     loads the chunk's last tile (its scores are never looked at).
//   Selection: the accumulator layout is the fp32 kernel's (lane (n, h): queries 8 (v / 4) + 4 h + v % 4 of ITS row), and so is everything behind it --
//     composites, one mask and one branch per round, the __syncthreads_or vote, the one-wave leader reductions of fr_retrieve_select.h, BUF = kp + S + 128.
//     The round's body is written here a second time: moved into a shared function it changed the registers of retrieve_scan_kernel.
//   KP = 64: BUF = 256 (64 KB of LDS, two workgroups per CU at every dim); KP = 256: BUF = 512 (128 KB, one).  dim is a run-time bound over steps <= 8.
//   The planes and the segment offsets are written in the fp32 scan's format: the ranking and retrieve_rows_kernel follow unchanged.
// Bounds: the image is read at tiles [c_begin / 32, (c_end - 1) / 32] <= tiles - 1, steps below `steps`; queries below n_q and columns below dim; the
//   planes at ((q * n_chunks + chunk) * k + j), j < k.  The image kernel reads table rows below `rows`, columns below dim, and writes words of tiles
//   below ceil(rows / 32).
#include <hip/hip_runtime.h>

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
    auto load = [&](uint4(&b)[LP_MAX_STEPS], int64_t tile) {
        int steps_l = steps;
        asm volatile("" : "+s"(steps_l));   // compared inside the loop, not hoisted into eight lane masks held for the whole kernel
        const uint4 *p = ga.image + (size_t)(tile < t_last ? tile : t_last) * (size_t)steps * 64 + (size_t)lane;
#pragma unroll
        for (int s = 0; s < LP_MAX_STEPS; s++)
            if (s < steps_l) b[s] = p[s * 64];
    };
    auto reduce = [&]() {
        for (int qi = wave; qi < FR_RETRIEVE_QTILE; qi += RT_WAVES) {
            const int c = __builtin_amdgcn_readfirstlane(cnt[qi]);
            if (c == 0) continue;
            u64 *bq = buf + qi * BUF;
            const int m = pow2_ceil(kp + c);   // <= BUF: c <= BUF - kp
            for (int i = kp + c + lane; i < m; i += 64) bq[i] = 0ull;
            wave_sync();
            wave_leaders(bq, m, kp, lane);
            if (lane == 0) thr[qi] = bq[k - 1], cnt[qi] = 0;
        }
    };
    uint32_t live_v = 0u;   // bit v: the lane's accumulator v belongs to a query below n_q
#pragma unroll
    for (int v = 0; v < 16; v++) live_v |= (q0 + 8 * (v >> 2) + 4 * h + (v & 3) < g.n_q ? 1u : 0u) << v;
    __syncthreads();

    const int rounds = (int)((c_end - c_begin + FR_RETRIEVE_ROUND - 1) / FR_RETRIEVE_ROUND);
    uint4 b[LP_MAX_STEPS], nb[LP_MAX_STEPS];
    load(nb, t_begin + wave);
    for (int r = 0; r < rounds; r++) {
        const int64_t tile = t_begin + (int64_t)(RT_WAVES * r + wave);
        const int64_t row = tile * FR_RETRIEVE_IMAGE_TILE + n;
#pragma unroll
        for (int s = 0; s < LP_MAX_STEPS; s++) b[s] = nb[s];
        if (r + 1 < rounds) load(nb, tile + RT_WAVES);
        f32x16 acc;
#pragma unroll
        for (int v = 0; v < 16; v++) acc[v] = -0.0f;
        int steps_l = steps;
        asm volatile("" : "+s"(steps_l));   // (as in load)
#pragma unroll
        for (int s = 0; s < LP_MAX_STEPS; s++)
            if (s < steps_l) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[s]), __builtin_bit_cast(bf16x8, b[s]), acc, 0, 0, 0);
        // The sign of a zero score is set here, not taken from the MFMA (it returns +0 for a sum whose terms are all -0): s = -0 + products is -0 exactly
        // when every product is -0 -- one operand zero, the signs different --, +0 otherwise.  Zero scores are rare (those of the
        // query tile's slots past n_q, all -0, are not looked at): one wave-uniform branch.
        bool zero = false;
        uint32_t live_l = live_v;
        asm volatile("" : "+v"(live_l));   // (kept one register: its 16 bit tests are not hoisted into 16 lane masks)
#pragma unroll
        for (int v = 0; v < 16; v++) zero |= (live_l >> v & 1u) && (__float_as_uint(acc[v]) & 0x7fffffffu) == 0u;
        if (__builtin_amdgcn_ballot_w64(zero) != 0ull) {
            u64 rz[2], rs[2];   // [half]
            int steps_z = steps;
            asm volatile("" : "+s"(steps_z));   // (as in load)
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
