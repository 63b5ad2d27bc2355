// Probed (IVF) top-K retrieval (fr_ctx_set_retrieve_lists, fr_worker_retrieve_probed_device / fr_worker_retrieve_probed, fleetrec_serving.h) ->
// libfleetrec_retrieve_probe.so, the tenth COMPANION code object of libfleetrec.so, built and linked as libfleetrec_retrieve.so is.  It calls nothing of
// libfleetrec.so: each launcher returns 0 or a hipError_t value.  DESIGN.md section 3.1g has the reasoning; fr_internal.h names the arrays.
//
// Every query scans its own lists, and queries that probe the same list share its tiles: the (query, list) pairs are grouped by list on the device, 32
// pairs of one list are the A operand of one workgroup, and the list's rows stream past them exactly as a chunk does in retrieve_scan_kernel.
//
// probe_sort_kernel, one wave per query: the probe row into LDS (an id outside [0, n_lists) becomes "none", an id >= n_lists raises the error flag), a
//   bitonic sort ascending over pow2_ceil(n_probe) <= 256, then one pass that keeps an id once and drops the lists without rows.  Slot j of the query is
//   its j-th smallest list: offsets ascend, so the slots are in row order.  Per live slot: + 1 on the list's pair counter, and the plane index of its
//   first entry -- the exclusive prefix, over the query's slots, of the entries a list of that length fills (k per full part, min(k, rows) of the last).
//   The query's entries are therefore COMPACT in (slot, part) order; the wave pads the rest of the query's stretch with (NaN, -1) and writes the
//   segment offsets.  Why compact: a pad and a real NaN score share the lowest rank key, and the ranking orders equal keys by position -- a pad in the
//   middle of a stretch would come before a real NaN row of a later list (and could push it out of the k).  With every pad behind every real entry the
//   stretch has the shape section 3.1e relied on: real rows first, a real NaN before the pads.
// probe_group_scan_kernel, ONE workgroup: the exclusive prefix of (pairs, tiles) over the list counters, both sums in one 64-bit word, 4096 lists a pass.
// probe_group_scatter_kernel, one thread per (query, slot): the pair goes to place first + (atomicSub(counter) - 1) of its list, which also leaves every
//   counter at 0 for the next call; the pair that opens a tile names the tile's list in tile_list.  The order of the pairs inside a list is whatever
//   the atomics gave.  It decides only WHICH workgroup and lane scores a (query, row) -- the score of a pair of vectors does not depend on the MFMA
//   column it sits in, and the selection keeps exactly the k largest composites, which are all distinct -- so a query's result is a function of its
//   candidate set alone.
// retrieve_probe_scan_kernel<KP, NT>: workgroup (tile, part) = 4 waves; a tile past the total leaves at once.  The tile's list is ONE load of tile_list
//   (the scatter wrote it; a search of the tile prefix would be ~20 dependent loads in front of every workgroup).  A operand: lane (n, h) holds the
//   words of the query of pair first + n, fetched through the pair array; lanes without a pair hold -0.  B operand, MFMA steps, column order, composites
//   (low word: 0xffffffff - ABSOLUTE row), the mask and branch, the LDS append buffers, the vote behind every 128-row round and the one-wave leader
//   reductions are retrieve_scan_kernel's, so the score of (query, row) has the bits fr_worker_retrieve_device gives that pair.  The tile's leader
//   reduction is scan_reduce of fr_retrieve_select.h; the rest of the round body is a second copy on purpose: the exact kernel's registers changed when
//   it was moved into a shared header.
//   End of part: the min(k, rows of the part) leaders of every pair go to plane entries slot_base[pair] + part * k + j.
// Bounds: probe below n_q * n_probe; offsets at valid ids l and l + 1 only; table rows inside [lb + part * g.part, min(+ g.part, le)) of a list the
//   offsets name; pairs below the pair total, tile_list below tiles_cap; the planes inside the query's stretch (the prefix of a stretch's entries is
//   <= n_probe * split * k by construction: a list is clipped to split parts).
#include <hip/hip_runtime.h>

#include "fr_internal.h"
#include "fr_retrieve_select.h"

constexpr int PROBE_NONE = 0x7fffffff;

__global__ __launch_bounds__(RT_THREADS) void probe_clear_kernel(int *list_cnt, int n) {
    const int i = (int)blockIdx.x * RT_THREADS + (int)threadIdx.x;
    if (i < n) list_cnt[i] = 0;
}

__global__ __launch_bounds__(RT_THREADS) void probe_sort_kernel(const FrRetrieveProbeArgs g) {
    __shared__ int ids[RT_WAVES][FR_RETRIEVE_MAX_PROBE];
    __shared__ int live_id[RT_WAVES][FR_RETRIEVE_MAX_PROBE];
    __shared__ int live_ent[RT_WAVES][FR_RETRIEVE_MAX_PROBE];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, q = (int)blockIdx.x * RT_WAVES + wave;
    if (q >= g.n_q) return;   // (a whole wave: nothing below is a workgroup barrier)
    int *s = ids[wave], *lid = live_id[wave], *lent = live_ent[wave];
    const int np = g.n_probe, m = pow2_ceil(np), k = g.k;
    int bad = 0;
    for (int i = lane; i < m; i += 64) {
        int id = i < np ? g.probe[(size_t)q * (size_t)np + (size_t)i] : -1;
        if (id >= g.n_lists) id = -1, bad = 1;
        s[i] = id < 0 ? PROBE_NONE : id;
    }
    if (__any(bad) && lane == 0) atomicOr_system(g.err_flag, 1);   // pinned host word; error path only
    wave_sync();
    for (int size = 2; size <= m; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int p = lane; p < (m >> 1); p += 64) {
                const int i = 2 * p - (p & (stride - 1));
                const int x = s[i], y = s[i + stride];
                if ((x > y) == ((i & size) == 0)) s[i] = y, s[i + stride] = x;
            }
            wave_sync();
        }
    // once each, lists without rows dropped; what is left moves to the front in order
    int n_live = 0;
    for (int c = 0; c < m; c += 64) {
        const int i = c + lane, v = i < m ? s[i] : PROBE_NONE;
        bool live = v != PROBE_NONE && (i == 0 || s[i - 1] != v);
        int ent = 0;
        if (live) {
            int64_t len = g.offsets[v + 1] - g.offsets[v];
            if (len > g.part * g.split) len = g.part * g.split;   // (never: the host sized the parts by the longest list)
            const int64_t rem = len % g.part;
            ent = (int)(len / g.part) * k + (rem < k ? (int)rem : k);
            live = len > 0;
        }
        const u64 vote = __ballot(live);
        if (live) {
            const int j = n_live + __popcll(vote & ((1ull << lane) - 1ull));
            lid[j] = v, lent[j] = ent;
        }
        n_live += __popcll(vote);
    }
    wave_sync();
    const int stride_q = np * g.split * k, base_q = q * stride_q;   // n_q * stride_q <= 2^24
    int total = 0;
    for (int c = 0; c < np; c += 64) {
        const int j = c + lane, ent = j < n_live ? lent[j] : 0;
        int x = ent;
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (j < np) {
            const size_t e = (size_t)q * (size_t)np + (size_t)j;
            g.slots[e] = j < n_live ? lid[j] : -1;
            g.slot_base[e] = base_q + total + x - ent;
            if (j < n_live) atomicAdd(&g.list_cnt[lid[j]], 1);
        }
        total += __shfl(x, 63);
    }
    for (int i = total + lane; i < stride_q; i += 64) {
        g.part_scores[(size_t)base_q + (size_t)i] = __uint_as_float(FR_RETRIEVE_PAD_BITS);
        g.part_rows[(size_t)base_q + (size_t)i] = -1;
    }
    if (lane == 0) {
        g.seg_off[q] = base_q;
        if (q == g.n_q - 1) g.seg_off[g.n_q] = g.n_q * stride_q;
    }
}

__global__ __launch_bounds__(FR_RETRIEVE_PROBE_SCAN_THREADS) void probe_group_scan_kernel(const FrRetrieveProbeArgs g) {
    constexpr int T = FR_RETRIEVE_PROBE_SCAN_THREADS;
    __shared__ u64 sh[T];
    const int tid = (int)threadIdx.x;
    u64 carry = 0ull;   // the same in every thread
    for (int base = 0; base < g.n_lists; base += 4 * T) {
        const int i0 = base + 4 * tid;
        u64 v[4], t = 0ull;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const u64 c = i0 + j < g.n_lists ? (u64)g.list_cnt[i0 + j] : 0ull;
            v[j] = (c << 32) | ((c + 31ull) >> 5);
            t += v[j];
        }
        sh[tid] = t;
        __syncthreads();
        for (int d = 1; d < T; d <<= 1) {
            const u64 x = tid >= d ? sh[tid - d] : 0ull;
            __syncthreads();
            sh[tid] += x;
            __syncthreads();
        }
        u64 ex = carry + sh[tid] - t;
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (i0 + j < g.n_lists) g.list_first[i0 + j] = ex, ex += v[j];
        carry += sh[T - 1];
        __syncthreads();
    }
    if (tid == 0) g.list_first[g.n_lists] = carry;
}

__global__ __launch_bounds__(RT_THREADS) void probe_group_scatter_kernel(const FrRetrieveProbeArgs g) {
    const int64_t e = (int64_t)blockIdx.x * RT_THREADS + (int64_t)threadIdx.x;
    if (e >= (int64_t)g.n_q * g.n_probe) return;
    const int l = g.slots[e];
    if (l < 0) return;
    const int at = atomicSub(&g.list_cnt[l], 1) - 1;   // 0 .. count - 1, each once
    const u64 f = g.list_first[l];
    const int64_t at_pair = (int64_t)(f >> 32) + at;
    if (at < 0 || at_pair >= (int64_t)g.n_q * g.n_probe) return;   // (never: the counters were 0 before the sort)
    g.pairs[at_pair] = (int32_t)e;
    const int64_t tile = (int64_t)(uint32_t)f + (at >> 5);
    if ((at & 31) == 0 && tile < g.tiles_cap) g.tile_list[tile] = l;
}

template <int KP, int NT>
__global__ __launch_bounds__(RT_THREADS, KP <= 64 && NT <= 4 ? 2 : 1) void retrieve_probe_scan_kernel(const FrRetrieveProbeArgs g) {
    constexpr int BUF = KP <= 64 ? 256 : 512;
    __shared__ u64 buf[FR_RETRIEVE_QTILE * BUF];
    __shared__ u64 thr[FR_RETRIEVE_QTILE];
    __shared__ int cnt[FR_RETRIEVE_QTILE];
    __shared__ int pair_of[FR_RETRIEVE_QTILE];
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
    const int64_t c_end = c_begin + g.part < le ? c_begin + g.part : le;
    if (c_begin >= c_end || n_pairs < 1) return;   // the list ends before this part: it has no entries in the planes (uniform)

    const int dim = g.dim, W = dim >> 2, nt = (W + 1) >> 1;
    const int k = g.k, kp = pow2_ceil(k), S = BUF - kp - FR_RETRIEVE_ROUND;
    for (int i = tid; i < FR_RETRIEVE_QTILE * BUF; i += RT_THREADS) buf[i] = 0ull;
    if (tid < FR_RETRIEVE_QTILE) thr[tid] = 0ull, cnt[tid] = 0, pair_of[tid] = tid < n_pairs ? g.pairs[first + tid] : -1;

    float4 a[NT];
    const int my_pair = n < n_pairs ? g.pairs[first + n] : -1;
#pragma unroll
    for (int t = 0; t < NT; t++) {
        a[t] = make_float4(-0.0f, -0.0f, -0.0f, -0.0f);
        if (t < nt && h + 2 * t < W && my_pair >= 0) {
            const float *p = g.queries + (size_t)(my_pair / g.n_probe) * (size_t)dim + 4 * (h + 2 * t);
            a[t] = make_float4(p[0], p[1], p[2], p[3]);
        }
    }
    // rows past the part load the part's last row (their scores are never looked at), a word past the row loads the row's last word and counts as +0
    auto load = [&](float4(&b)[NT], int64_t row) {
        int nt_l = nt, W_l = W;
        asm volatile("" : "+s"(nt_l), "+s"(W_l));   // (as in retrieve_scan_kernel: keeps the loop's comparisons out of SGPR pairs)
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
    auto reduce = [&]() { scan_reduce<BUF>(buf, thr, cnt, k, kp, lane, wave); };   // (a lambda for the reason given in retrieve_scan_kernel)
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
        const u64 low = (u64)(0xffffffffu - (uint32_t)row);   // by ABSOLUTE row (< 2^31: never 0)
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
                if ((pass >> v & 1u) && qi < n_pairs) {
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

extern "C" __attribute__((visibility("default"))) int fr_retrieve_probe_clear_launch(int *list_cnt, int n, void *stream) {
    probe_clear_kernel<<<dim3((unsigned)((n + RT_THREADS - 1) / RT_THREADS)), dim3(RT_THREADS), 0, (hipStream_t)stream>>>(list_cnt, n);
    return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("default"))) int fr_retrieve_probe_sort_launch(const FrRetrieveProbeArgs *args, void *stream) {
    probe_sort_kernel<<<dim3((unsigned)((args->n_q + RT_WAVES - 1) / RT_WAVES)), dim3(RT_THREADS), 0, (hipStream_t)stream>>>(*args);
    return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("default"))) int fr_retrieve_probe_group_launch(const FrRetrieveProbeArgs *args, void *stream) {
    probe_group_scan_kernel<<<dim3(1), dim3(FR_RETRIEVE_PROBE_SCAN_THREADS), 0, (hipStream_t)stream>>>(*args);
    return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("default"))) int fr_retrieve_probe_scatter_launch(const FrRetrieveProbeArgs *args, void *stream) {
    const int64_t n = (int64_t)args->n_q * args->n_probe;
    probe_group_scatter_kernel<<<dim3((unsigned)((n + RT_THREADS - 1) / RT_THREADS)), dim3(RT_THREADS), 0, (hipStream_t)stream>>>(*args);
    return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("default"))) int fr_retrieve_probe_scan_launch(const FrRetrieveProbeArgs *args, void *stream) {
    const FrRetrieveProbeArgs g = *args;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)g.tiles_cap, (unsigned)g.split);
    const bool wide = g.dim > 32, deep = g.k > 64;
    if (!wide && !deep) retrieve_probe_scan_kernel<64, 4><<<grid, dim3(RT_THREADS), 0, s>>>(g);
    else if (!wide) retrieve_probe_scan_kernel<256, 4><<<grid, dim3(RT_THREADS), 0, s>>>(g);
    else if (!deep) retrieve_probe_scan_kernel<64, 16><<<grid, dim3(RT_THREADS), 0, s>>>(g);
    else retrieve_probe_scan_kernel<256, 16><<<grid, dim3(RT_THREADS), 0, s>>>(g);
    return (int)hipGetLastError();
}
