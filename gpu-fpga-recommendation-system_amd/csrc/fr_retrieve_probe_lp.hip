// Probed (IVF) bf16 retrieval over the table image (fr_worker_retrieve_probed_image_device / fr_worker_retrieve_probed_image, fleetrec_serving.h) ->
// libfleetrec_retrieve_probe_lp.so, the eleventh COMPANION code object of libfleetrec.so, built and linked as libfleetrec_retrieve.so is.  It calls
// nothing of libfleetrec.so: its one launcher returns 0 or a hipError_t value.  DESIGN.md section 3.1h has the reasoning; fr_internal.h names the arrays.
//
// The candidates are the probed scan's, the scores the image scan's.  The grouping (probe_sort_kernel, probe_group_scan_kernel,
// probe_group_scatter_kernel of the tenth companion) runs unchanged in front of this kernel, and the ranking and retrieve_rows_kernel behind it.
//
// retrieve_probe_lp_scan_kernel<KP>: workgroup (tile, part) = 4 waves, the 32 (query, list) pairs of one tile of pairs against part `part` of their list,
//   the rows [c_begin, c_end) = [lb + part * g.part, min(+ g.part, le)).  Parts are cut in ROWS from the list's first row, exactly as in
//   retrieve_probe_scan_kernel: probe_sort_kernel counted min(k, rows of the part) plane entries for every part, and a part moved onto tile boundaries
//   would hold another number of rows.
//   B operand: the image is tiled by ABSOLUTE row and a part begins and ends anywhere, so the workgroup scans the image tiles t_begin = c_begin >> 5 ..
//     t_last = (c_end - 1) >> 5.  In round r wave w takes tile t_begin + 4 r + w (lp_load of fr_retrieve_lp_scan.h); the loads of round r + 1 are issued
//     before the MFMAs of round r.  A row passes the mask only when c_begin <= row < c_end: a boundary tile that two lists, or two parts of one list,
//     share is read by both workgroups, and each masks the other's rows.
//   A operand: lane (n, h) fetches the query of pair first + n through the pair array and converts columns 16 s + 8 h .. + 7 to bf16 (RNE) once.  Lanes
//     without a pair and columns >= dim hold bf16 -0.
//   Sign of a zero score: set behind the MFMAs from the operands' masks (fr_retrieve_lp_scan.h has the reasoning).  One wave-uniform branch, taken only
//     when a lane holds a zero score of a LIVE pair in a row of the part.
//   Selection: everything behind the MFMAs is retrieve_probe_scan_kernel's -- composites (low word: 0xffffffff - ABSOLUTE row), one mask and one branch,
//     the LDS append buffers, the __syncthreads_or vote behind every round, the one-wave leader reductions of fr_retrieve_select.h, and the part's
//     min(k, rows) leaders at plane entries slot_base[pair] + part * k + j.
//   Shared with the two other image scans: the operand masks, the B load, the MFMA steps and the tile's leader reduction.  The zero-sign fix and the
//     threshold test with its appends are written out here as in retrieve_lp_scan_kernel, for the reason given there.
//   Buffers: a part spans at most one tile more than g.part / 32, so it may take one round more than the fp32 probed scan -- but a round is still 4 tiles
//     of 32 rows and appends at most 128 composites per pair.  BUF = kp + S + 128, the vote after every round and the overflow argument of section 3.1e
//     therefore hold unchanged: a counter starts a round at S or less and ends it at S + 128 or less.
//   KP = 64: BUF = 256 (65.5 KB of LDS with the masks, two workgroups per CU at every dim); KP = 256: BUF = 512 (one).  dim is a run-time bound over
//     steps <= 8.
// Bounds: the image is read at tiles [t_begin, t_last] only, and t_last <= tiles - 1 because c_end <= the rows the image was built of (c_end is clipped
//   to 32 * tiles once more here); steps below `steps`; offsets at list and list + 1 of a list the scatter named; pairs below the pair total; queries
//   below n_q and columns below dim; the planes inside the query's stretch, as in retrieve_probe_scan_kernel.
#include <hip/hip_runtime.h>

#include "fr_retrieve_lp_scan.h"

template <int KP>
__global__ __launch_bounds__(RT_THREADS, KP <= 64 ? 2 : 1) void retrieve_probe_lp_scan_kernel(const FrRetrieveProbeLpArgs ga) {
    constexpr int BUF = KP <= 64 ? 256 : 512;
    __shared__ u64 buf[FR_RETRIEVE_QTILE * BUF];
    __shared__ u64 thr[FR_RETRIEVE_QTILE];
    __shared__ int cnt[FR_RETRIEVE_QTILE];
    __shared__ int pair_of[FR_RETRIEVE_QTILE];
    __shared__ u64 qmask[FR_RETRIEVE_QTILE][2][2];   // [pair][half h][zero, sign]: bit 8 s + j = column 16 s + 8 h + j of the pair's query as bf16
    const FrRetrieveProbeArgs &g = ga.p;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, h = lane >> 5;
    const int tile = (int)blockIdx.x, part = (int)blockIdx.y;
    const u64 totals = g.list_first[g.n_lists];
    if (tile >= (int)(uint32_t)totals || tile >= g.tiles_cap) return;   // (uniform)
    const int list = g.tile_list[tile];
    if ((unsigned)list >= (unsigned)g.n_lists) return;   // (never: the scatter named the list of every tile below the total)
    const u64 lf = g.list_first[list];
    const int first = (int)(lf >> 32) + 32 * (tile - (int)(uint32_t)lf);
    const int list_pairs = (int)(g.list_first[list + 1] >> 32) - first;
    const int n_pairs = list_pairs < FR_RETRIEVE_QTILE ? list_pairs : FR_RETRIEVE_QTILE;
    const int64_t lb = g.offsets[list], le = g.offsets[list + 1];
    const int64_t c_begin = lb + (int64_t)part * g.part;
    int64_t c_end = c_begin + g.part < le ? c_begin + g.part : le;
    if (c_end > ga.tiles * FR_RETRIEVE_IMAGE_TILE) c_end = ga.tiles * FR_RETRIEVE_IMAGE_TILE;   // (never: the partition lies inside the table the image was built of)
    if (c_begin >= c_end || n_pairs < 1) return;   // the list ends before this part: it has no entries in the planes (uniform)
    const int64_t t_begin = c_begin >> 5, t_last = (c_end - 1) >> 5;   // 0 <= t_begin <= t_last < ga.tiles

    const int dim = g.dim, steps = fr_retrieve_image_steps(dim);
    const int k = g.k, kp = pow2_ceil(k), S = BUF - kp - FR_RETRIEVE_ROUND;
    for (int i = tid; i < FR_RETRIEVE_QTILE * BUF; i += RT_THREADS) buf[i] = 0ull;
    if (tid < FR_RETRIEVE_QTILE) thr[tid] = 0ull, cnt[tid] = 0, pair_of[tid] = tid < n_pairs ? g.pairs[first + tid] : -1;

    uint4 a[LP_MAX_STEPS];
    {
        const int my_pair = n < n_pairs ? g.pairs[first + n] : -1;
        const float4 *qp = reinterpret_cast<const float4 *>(g.queries + (size_t)(my_pair >= 0 ? my_pair / g.n_probe : 0) * (size_t)dim);
#pragma unroll
        for (int s = 0; s < LP_MAX_STEPS; s++) {
            const int c0 = FR_RETRIEVE_IMAGE_STEP * s + 8 * h;   // (dim is a multiple of 4: a float4 lies below dim whole or not at all)
            float4 lo = make_float4(-0.0f, -0.0f, -0.0f, -0.0f), hi = lo;
            if (my_pair >= 0 && c0 < dim) lo = qp[c0 >> 2];
            if (my_pair >= 0 && c0 + 4 < dim) hi = qp[(c0 >> 2) + 1];
            // (spelled out: through lp_pack8 the eight conversions keep their registers' count but change their order once lp_load is shared)
            a[s] = make_uint4(pack_bf16x2(lo.x, lo.y), pack_bf16x2(lo.z, lo.w), pack_bf16x2(hi.x, hi.y), pack_bf16x2(hi.z, hi.w));
        }
        u64 z, sg;
        lp_masks(a, LP_MAX_STEPS, z, sg);
        if (wave == 0) qmask[n][h][0] = z, qmask[n][h][1] = sg;
    }
    uint32_t live_v = 0u;   // bit v: the lane's accumulator v belongs to a pair of the tile
#pragma unroll
    for (int v = 0; v < 16; v++) live_v |= (8 * (v >> 2) + 4 * h + (v & 3) < n_pairs ? 1u : 0u) << v;
    __syncthreads();

    const int rounds = (int)((t_last - t_begin + RT_WAVES) / RT_WAVES);   // <= g.part / 128 + 1
    uint4 b[LP_MAX_STEPS], nb[LP_MAX_STEPS];
    lp_load(nb, ga.image, t_begin + wave, t_last, steps, lane);
    for (int r = 0; r < rounds; r++) {
        const int64_t t = t_begin + (int64_t)(RT_WAVES * r + wave);
        const int64_t row = t * FR_RETRIEVE_IMAGE_TILE + n;
        const bool inside = row >= c_begin && row < c_end;   // (a tile past t_last: row >= 32 (t_last + 1) >= c_end)
#pragma unroll
        for (int s = 0; s < LP_MAX_STEPS; s++) b[s] = nb[s];
        if (r + 1 < rounds) lp_load(nb, ga.image, t + RT_WAVES, t_last, steps, lane);
        f32x16 acc = lp_scores(a, b, steps);
        // the sign of a zero score is set here, not taken from the MFMA (fr_retrieve_lp_scan.h has the reasoning).  Only the scores that are looked at
        // count: a live pair and a row of the part (the +0 pad rows of the table's last tile and a neighbouring list's rows in a boundary tile never
        // take the branch).
        bool zero = false;
        uint32_t live_l = inside ? live_v : 0u;
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
        const u64 low = (u64)(0xffffffffu - (uint32_t)row);   // by ABSOLUTE row (< 2^31: never 0)
        uint32_t key[16], pass = 0u;
#pragma unroll
        for (int v = 0; v < 16; v++) {
            const int qi = 8 * (v >> 2) + 4 * h + (v & 3);
            key[v] = fr_rank_key(__float_as_uint(acc[v]));
            pass |= ((((u64)key[v] << 32) | low) > thr[qi] ? 1u : 0u) << v;
        }
        if (!inside) pass = 0u;
        if (pass) {
#pragma unroll
            for (int v = 0; v < 16; v++) {
                const int qi = 8 * (v >> 2) + 4 * h + (v & 3);
                if ((pass >> v & 1u) && qi < n_pairs) {
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

    const int64_t part_rows = c_end - c_begin;
    const int ent = part_rows < k ? (int)part_rows : k;   // what probe_sort_kernel counted for this part
    for (int e = tid; e < n_pairs * ent; e += RT_THREADS) {
        const int qi = e / ent, j = e - qi * ent;
        const u64 c = buf[qi * BUF + j];   // (never 0: the part has at least `ent` rows)
        const size_t o = (size_t)g.slot_base[pair_of[qi]] + (size_t)part * (size_t)k + (size_t)j;
        g.part_scores[o] = __uint_as_float(c ? retrieve_bits((uint32_t)(c >> 32)) : FR_RETRIEVE_PAD_BITS);
        g.part_rows[o] = c ? (int32_t)(0xffffffffu - (uint32_t)c) : -1;
    }
}

extern "C" __attribute__((visibility("default"))) int fr_retrieve_probe_lp_scan_launch(const FrRetrieveProbeLpArgs *args, void *stream) {
    const FrRetrieveProbeLpArgs g = *args;
    const dim3 grid((unsigned)g.p.tiles_cap, (unsigned)g.p.split);
    if (g.p.k <= 64) retrieve_probe_lp_scan_kernel<64><<<grid, dim3(RT_THREADS), 0, (hipStream_t)stream>>>(g);
    else retrieve_probe_lp_scan_kernel<256><<<grid, dim3(RT_THREADS), 0, (hipStream_t)stream>>>(g);
    return (int)hipGetLastError();
}
