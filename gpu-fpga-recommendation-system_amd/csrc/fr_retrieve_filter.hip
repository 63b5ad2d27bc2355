// Filtered bf16 retrieval over the table image (fr_ctx_set_retrieve_filter, fr_*_retrieve_filter_rows, fr_worker_retrieve_image_filtered_device /
// fr_worker_retrieve_image_filtered, fleetrec_serving.h) -> libfleetrec_retrieve_filter.so, the twelfth COMPANION code object of libfleetrec.so, built and
// linked as libfleetrec_retrieve_lp.so is.  It calls nothing of libfleetrec.so: each of its three launchers returns 0 or a hipError_t value.  DESIGN.md
// section 3.1i has the reasoning.
//
// The mask: one bit per row, word T for the rows of image tile T (32 T .. 32 T + 31), bit n for row 32 T + n; bits past the table's rows are clear.
//
// retrieve_filter_mask_kernel: range arm (ids == NULL): one thread per word, written whole -- all ones, the bits at and past `rows` clear in the last word.
//   List arm: one thread per listed id, atomicOr (live) / atomicAnd (dead) on the row's word; an id outside [0, rows) does nothing.  One `live` value per
//   launch and idempotent bit operations: the words do not depend on how the atomics interleave.
//
// retrieve_filter_scan_kernel<KP>: retrieve_lp_scan_kernel (fr_retrieve_lp.hip) -- the work split, both operands, the MFMA steps, the zero-sign fix, the
//   composites, BUF = kp + S + 128, the vote and the one-wave leader reductions are its own.  The operand masks, the B load, the MFMA steps and the
//   tile's leader reduction are the shared functions of fr_retrieve_lp_scan.h and fr_retrieve_select.h; the A operand's build, the zero-sign fix and the
//   threshold test with its appends are written out here as they are there, for the reason given there -- with the two filters folded into the SELECTION:
//   Mask: wave w of round r scans image tile t; its mask word mask[t] is one wave-uniform load (one address, one 4-byte request) issued with the round's
//     B loads, one round ahead.
//     Lane (n, h) tests bit n, and the test joins the row-valid condition: a dead row costs what a row outside the window costs -- nothing is appended, no
//     threshold moves.
//   Exclusions: the query tile's lists sit in LDS (32 x n_excl int32 rounded up to whole 16-byte words, 8 KB; a slot past n_q or n_excl holds -1).  They
//     are read only for a composite that has already beaten its query's threshold, inside the branch the steady state skips: a pass over THAT query's
//     entries, four per read.  An excluded row is never appended, so it never raises a threshold.
//   Output: ONE plane of u64 composites [n_q][n_chunks][k], (fr_rank_key(score bits) << 32) | (0xffffffff - (row - row0)), per chunk descending; an entry
//     without a row is the pad composite 0, strictly below every real one (a real NaN's has key 0 and a low word >= 0x80000000).  The low word is
//     window-relative, so a query's composites are distinct across chunks and comparable as they are.
//   KP = 64: BUF = 256, 64 KB + 8 KB + 1.4 KB of LDS, two workgroups per CU; KP = 256: BUF = 512, 128 KB + 8 KB + 1.4 KB, one.
//
// retrieve_filter_merge_kernel<KP>: the k largest of a stretch of one query's composites, descending.  Workgroup (query, part) = 4 waves; the part's
//   stretch [part * stretch, + stretch) of the query's n composites is cut into four contiguous quarters, one per wave.  A wave streams its quarter through
//   its own LDS tile (TILE = 256 / 512 composites for KP = 64 / 256: the kp leaders so far + TILE - kp new ones, wave_leaders of fr_retrieve_select.h),
//   then wave 0 folds the four waves' leaders.  Composites of one query are distinct (pads excepted, which are all 0), so the k largest and their order are
//   a function of the composite SET: no cut, no wave count and no arrival order shows in the result.  final == 0: the leaders go to dst [n_q][parts][k]
//   as composites, for a second launch with one part per query; final != 0: they are mapped to (row0 + 0xffffffff - low word, the score bits the key
//   stands for -- a NaN as 0x7fc00000) and composite 0 to (-1, -inf).
// Bounds: the scan reads the image and the mask at tiles <= (c_end - 1) / 32 < ceil(rows / 32), queries below n_q, exclude below n_q * n_excl, and writes
//   comp at ((q * n_chunks + chunk) * k + j), j < k.  The merge reads src at q * n + [0, n) and writes dst at (q * parts + part) * k + j or the outputs at
//   q * k + j.  The mask kernel touches words below ceil(rows / 32) and ids below n.
#include <hip/hip_runtime.h>

#include "fr_retrieve_lp_scan.h"

__global__ __launch_bounds__(RT_THREADS) void retrieve_filter_mask_kernel(const FrRetrieveFilterMaskArgs g) {
    const int64_t i = (int64_t)blockIdx.x * RT_THREADS + (int64_t)threadIdx.x;
    if (g.ids) {
        if (i >= g.n) return;
        const int64_t row = (int64_t)g.ids[i];
        if (row < 0 || row >= g.rows) return;
        const uint32_t bit = 1u << (uint32_t)(row & 31);
        if (g.live) atomicOr(g.mask + (row >> 5), bit);
        else atomicAnd(g.mask + (row >> 5), ~bit);
    } else {
        if (i >= (g.rows + 31) / 32) return;
        const int64_t left = g.rows - 32 * i;   // >= 1
        g.mask[i] = left >= 32 ? 0xffffffffu : (1u << (uint32_t)left) - 1u;
    }
}

template <int KP>
__global__ __launch_bounds__(RT_THREADS, KP <= 64 ? 2 : 1) void retrieve_filter_scan_kernel(const FrRetrieveFilterArgs ga) {
    constexpr int BUF = KP <= 64 ? 256 : 512;
    __shared__ u64 buf[FR_RETRIEVE_QTILE * BUF];
    __shared__ u64 thr[FR_RETRIEVE_QTILE];
    __shared__ int cnt[FR_RETRIEVE_QTILE];
    __shared__ u64 qmask[FR_RETRIEVE_QTILE][2][2];   // [query][half h][zero, sign]: bit 8 s + j = column 16 s + 8 h + j of the query as bf16
    __shared__ int4 excl[FR_RETRIEVE_QTILE * FR_RETRIEVE_MAX_EXCLUDE / 4];   // [query][nx4] int32: a query's list, padded with -1 to whole 16-byte words
    const FrRetrieveArgs &g = ga.lp.r;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, h = lane >> 5;
    const int dim = g.dim, steps = fr_retrieve_image_steps(dim), n_excl = ga.n_excl, nx4 = (n_excl + 3) & ~3;
    const int k = g.k, kp = pow2_ceil(k), S = BUF - kp - FR_RETRIEVE_ROUND;
    const int q0 = (int)blockIdx.y * FR_RETRIEVE_QTILE, chunk = (int)blockIdx.x;
    const int64_t c_begin = (g.row0 & ~(int64_t)(FR_RETRIEVE_IMAGE_TILE - 1)) + (int64_t)chunk * g.chunk;   // a tile boundary; <= row0 in chunk 0 only
    const int64_t w_end = g.row0 + g.n_rows;
    const int64_t c_end = c_begin + g.chunk < w_end ? c_begin + g.chunk : w_end;                            // > c_begin, > row0
    const int64_t t_begin = c_begin >> 5, t_last = (c_end - 1) >> 5;                                        // t_last < ga.lp.tiles: c_end <= the table's rows

    for (int i = tid; i < FR_RETRIEVE_QTILE * BUF; i += RT_THREADS) buf[i] = 0ull;
    if (tid < FR_RETRIEVE_QTILE) thr[tid] = 0ull, cnt[tid] = 0;
    for (int i = tid; i < FR_RETRIEVE_QTILE * nx4; i += RT_THREADS) {
        const int q = q0 + i / nx4, j = i % nx4;
        reinterpret_cast<int32_t *>(excl)[i] = q < g.n_q && j < n_excl ? ga.exclude[(size_t)q * (size_t)n_excl + (size_t)j] : -1;
    }

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
    // the B words of a tile and, with them, the tile's mask word: the tile number is the same in every lane, so the word is one scalar load
    auto load = [&](uint4(&b)[LP_MAX_STEPS], uint32_t &word, int64_t tile) {
        lp_load(b, ga.lp.image, tile, t_last, steps, lane);
        word = ga.mask[tile < t_last ? tile : t_last];   // one address per wave: a single 4-byte request (kept in a VGPR: the scan has no scalar register to spare)
    };
    uint32_t live_v = 0u;   // bit v: the lane's accumulator v belongs to a query below n_q
#pragma unroll
    for (int v = 0; v < 16; v++) live_v |= (q0 + 8 * (v >> 2) + 4 * h + (v & 3) < g.n_q ? 1u : 0u) << v;
    __syncthreads();

    const int rounds = (int)((c_end - c_begin + FR_RETRIEVE_ROUND - 1) / FR_RETRIEVE_ROUND);
    uint4 b[LP_MAX_STEPS], nb[LP_MAX_STEPS];
    uint32_t word, nword;
    load(nb, nword, t_begin + wave);
    for (int r = 0; r < rounds; r++) {
        const int64_t tile = t_begin + (int64_t)(RT_WAVES * r + wave);
        const int64_t row = tile * FR_RETRIEVE_IMAGE_TILE + n;
#pragma unroll
        for (int s = 0; s < LP_MAX_STEPS; s++) b[s] = nb[s];
        word = nword;
        if (r + 1 < rounds) load(nb, nword, tile + RT_WAVES);
        f32x16 acc = lp_scores(a, b, steps);
        // the sign of a zero score is set here, not taken from the MFMA (fr_retrieve_lp_scan.h has the reasoning): one wave-uniform branch
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
        pass &= live_l;   // (a slot past n_q keeps threshold 0 and would pass in every round: it must not reach the look at the lists)
        if (row < g.row0 || row >= c_end || !(word >> n & 1u)) pass = 0u;   // outside the window, or not an item: the same cost
        if (pass) {
            // only a lane with a composite that beat its threshold comes here, and it looks at the list of THAT query alone: for every set bit of pass
            // (mostly one) a pass over the query's entries, four per LDS read.  (One loop over the bits, not one per accumulator: the scan has no scalar
            // registers for 16 loop masks.)
            if (nx4) {
                for (uint32_t left = pass; left; left &= left - 1u) {
                    const int v = __ffs(left) - 1;
                    const int4 *e = excl + (8 * (v >> 2) + 4 * h + (v & 3)) * (nx4 >> 2);
                    bool named = false;
                    for (int j = 0; j < (nx4 >> 2); j++) {
                        const int4 x = e[j];
                        named |= x.x == (int32_t)row || x.y == (int32_t)row || x.z == (int32_t)row || x.w == (int32_t)row;
                    }
                    if (named) pass &= ~(1u << v);
                }
            }
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
        ga.comp[((size_t)q * (size_t)g.n_chunks + (size_t)chunk) * (size_t)k + (size_t)j] = buf[qi * BUF + j];
    }
}

template <int KP>
__global__ __launch_bounds__(RT_THREADS) void retrieve_filter_merge_kernel(const FrRetrieveMergeArgs g) {
    constexpr int TILE = KP <= 64 ? 256 : 512;
    __shared__ u64 tile[RT_WAVES][TILE];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = g.k, kp = pow2_ceil(k), q = (int)blockIdx.x, part = (int)blockIdx.y;
    const int64_t p_begin = (int64_t)part * g.stretch, p_end = p_begin + g.stretch < g.n ? p_begin + g.stretch : g.n;
    const int64_t quarter = (p_end - p_begin + RT_WAVES - 1) / RT_WAVES;
    const int64_t w_begin = p_begin + wave * quarter < p_end ? p_begin + wave * quarter : p_end, w_end = w_begin + quarter < p_end ? w_begin + quarter : p_end;
    const u64 *src = g.src + (size_t)q * (size_t)g.n;
    u64 *b = tile[wave];
    for (int i = lane; i < kp; i += 64) b[i] = 0ull;
    for (int64_t pos = w_begin; pos < w_end; pos += TILE - kp) {
        const int c = (int)(w_end - pos < TILE - kp ? w_end - pos : TILE - kp);
        const int m = pow2_ceil(kp + c);   // <= TILE
        for (int i = lane; i < m - kp; i += 64) b[kp + i] = i < c ? src[pos + i] : 0ull;
        wave_sync();
        wave_leaders(b, m, kp, lane);
    }
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < RT_WAVES; w++) {   // 2 kp <= TILE
        for (int i = lane; i < kp; i += 64) b[kp + i] = tile[w][i];
        wave_sync();
        wave_leaders(b, 2 * kp, kp, lane);
    }
    for (int j = lane; j < k; j += 64) {
        const u64 c = b[j];
        if (!g.final) {
            g.dst[((size_t)q * (size_t)gridDim.y + (size_t)part) * (size_t)k + (size_t)j] = c;
            continue;
        }
        const size_t o = (size_t)q * (size_t)k + (size_t)j;
        g.top_rows[o] = c ? (int32_t)(g.row0 + (int64_t)(0xffffffffu - (uint32_t)c)) : -1;
        if (g.top_scores) g.top_scores[o] = __uint_as_float(c ? retrieve_bits((uint32_t)(c >> 32)) : 0xff800000u);
    }
}

extern "C" __attribute__((visibility("default"))) int fr_retrieve_filter_mask_launch(const FrRetrieveFilterMaskArgs *args, void *stream) {
    const FrRetrieveFilterMaskArgs g = *args;
    const int64_t threads = g.ids ? g.n : (g.rows + 31) / 32;
    if (threads <= 0) return 0;
    retrieve_filter_mask_kernel<<<dim3((unsigned)((threads + RT_THREADS - 1) / RT_THREADS)), dim3(RT_THREADS), 0, (hipStream_t)stream>>>(g);
    return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("default"))) int fr_retrieve_filter_scan_launch(const FrRetrieveFilterArgs *args, void *stream) {
    const FrRetrieveFilterArgs g = *args;
    const dim3 grid((unsigned)g.lp.r.n_chunks, (unsigned)((g.lp.r.n_q + FR_RETRIEVE_QTILE - 1) / FR_RETRIEVE_QTILE));
    if (g.lp.r.k <= 64) retrieve_filter_scan_kernel<64><<<grid, dim3(RT_THREADS), 0, (hipStream_t)stream>>>(g);
    else retrieve_filter_scan_kernel<256><<<grid, dim3(RT_THREADS), 0, (hipStream_t)stream>>>(g);
    return (int)hipGetLastError();
}

// one launch: grid (n_q, ceil(n / stretch)) -- n_q may be 65536, the parts are few
extern "C" __attribute__((visibility("default"))) int fr_retrieve_filter_merge_launch(const FrRetrieveMergeArgs *args, void *stream) {
    const FrRetrieveMergeArgs g = *args;
    const dim3 grid((unsigned)g.n_q, (unsigned)((g.n + g.stretch - 1) / g.stretch));
    if (g.k <= 64) retrieve_filter_merge_kernel<64><<<grid, dim3(RT_THREADS), 0, (hipStream_t)stream>>>(g);
    else retrieve_filter_merge_kernel<256><<<grid, dim3(RT_THREADS), 0, (hipStream_t)stream>>>(g);
    return (int)hipGetLastError();
}
