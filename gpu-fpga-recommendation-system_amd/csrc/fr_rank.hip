// Segmented top-K ranking of scores (fr_worker_topk_device / fr_worker_topk, fleetrec_serving.h) -> libfleetrec_rank.so, the COMPANION code object
// of libfleetrec.so: the kernel list of libfleetrec.so is pinned name for name (tests/golden/libfleetrec_kernel_names.txt), so these kernels live in
// a shared object of their own that libfleetrec.so links against ($ORIGIN rpath).  The companion calls nothing of libfleetrec.so: its one launcher
// returns a hipError_t value and the entry points (fr_api.cpp) turn it into a status and a text.
//
// What is ranked is a 64-bit COMPOSITE per score: (key << 32) | (0xffffffff - position inside the segment), key = the contract's total order on the
// score's bits (fr_rank_key, fr_internal.h).  Composites of one segment are all distinct and none is 0 (positions stay below 2^24), so a plain
// descending sort gives the one answer, and 0 pads every tile and every candidate list.  The score itself is read again through the winning
// position: a NaN's payload is not in its key.
//
// rank_segments_kernel<T>: one workgroup of T threads per segment, a tile of 16 T composites in LDS (T = 256: 4096 composites, 32 KB; T = 64: one
//   wave, 1024 composites, 8 KB -- the form for many short segments).  A bitonic network over the next power of two of what the tile holds sorts
//   runs of kp = pow2_ceil(k); pairs of runs are then halved to their kp leaders until one run is left (tile_leaders).  A segment longer than the
//   tile streams through it: the kp leaders stay at the tile's head, the next 16 T - kp scores fill the rest, the tile is reduced again.  A segment
//   of more than FR_RANK_PART (16384) scores is not ranked here: the workgroup reserves ceil(len / 16384) UNITS in the worker's scratch (one
//   atomic add) and writes one unit record per part.
// rank_parts_kernel: one workgroup per unit streams its part of at most 16384 scores and leaves its k leading composites in the unit's candidate list.
// rank_merge_kernel: level l (stride 16^l): the first unit of every group of 16 lists sorts them (16 x 256 = one tile) into its own list -- or, when
//   the group is the whole segment, into the outputs.  ceil(log16(ceil(n / 16384))) levels, at most 3: a lone segment of 2^24 scores is ranked by
//   1024 workgroups, then 64, 4 and 1.
// Bounds: a segment is ranked only when 0 <= off[s] <= off[s + 1] <= n, and every score load is scores[off[s] + i] with i < off[s + 1] - off[s]; a
// malformed segment raises the worker's index-range word and is ranked as empty.  The unit records are read back only below u_cap and name segments
// the first kernel validated; every kernel validates them again.
#include <hip/hip_runtime.h>

#include "fr_internal.h"

typedef unsigned long long u64;

static __device__ __forceinline__ u64 rank_composite(uint32_t bits, uint32_t pos) { return ((u64)fr_rank_key(bits) << 32) | (u64)(0xffffffffu - pos); }

static __device__ __forceinline__ int pow2_ceil(int v) {
    int m = 2;
    while (m < v) m <<= 1;
    return m;
}

// One compare-exchange step of a bitonic network over lds[0 .. 2 * half): pair p < half is (i, i + stride), i = 2p - (p & (stride - 1)); the pair
// ends descending where (i & dirmask) == 0, ascending elsewhere.  half <= 8 T.  All loads of the step are issued before its first store (the pairs
// of a step are disjoint), both stores are unconditional; ends behind a barrier.
template <int T>
static __device__ __forceinline__ void ce_step(u64 *lds, int half, int stride, int dirmask, int tid) {
    u64 a[8], b[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int p = tid + r * T;
        if (p < half) {
            const int i = 2 * p - (p & (stride - 1));
            a[r] = lds[i];
            b[r] = lds[i + stride];
        }
    }
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int p = tid + r * T;
        if (p < half) {
            const int i = 2 * p - (p & (stride - 1));
            const bool sw = (a[r] < b[r]) == ((i & dirmask) == 0);
            lds[i] = sw ? b[r] : a[r];
            lds[i + stride] = sw ? a[r] : b[r];
        }
    }
    __syncthreads();
}

// The kp = pow2_ceil(k) leaders of lds[0 .. m), m a power of two <= 16 T, descending in lds[0 .. min(m, kp)); -> min(m, kp).  m <= kp: the whole
// bitonic sort.  Otherwise the network runs only up to runs of kp (run c descending for even c, ascending for odd c); then, until one run is
// left, every pair of runs (descending X, ascending Y) is replaced by max(X[t], Y[t]) -- the first step of their bitonic merge, whose upper
// half holds the pair's kp largest as a bitonic run -- packed into half the tile, and the log2(kp) remaining merge steps sort the runs in
// alternating directions again.  The work halves with every round.
template <int T>
static __device__ __forceinline__ int tile_leaders(u64 *lds, int m, int kp, int tid) {
    const int top = m < kp ? m : kp;
    for (int size = 2; size <= top; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) ce_step<T>(lds, m >> 1, stride, size, tid);
    while (m > kp) {
        const int half = m >> 1;
        u64 v[8];
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int p = tid + r * T;
            if (p < half) {
                const int x = 2 * p - (p & (kp - 1));   // element t = p % kp of run 2 (p / kp); its partner run starts kp further
                const u64 a = lds[x], b = lds[x + kp];
                v[r] = a > b ? a : b;
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int p = tid + r * T;
            if (p < half) lds[p] = v[r];
        }
        __syncthreads();
        m = half;
        for (int stride = kp >> 1; stride > 0; stride >>= 1) ce_step<T>(lds, m >> 1, stride, kp, tid);
    }
    return top;
}

// Streams `count` composites load(0 .. count) through the tile and leaves the leaders, descending, in lds[0 .. returned m) (0-padded): the caller
// reads entry j < k as (j < m ? lds[j] : 0).  `count` and k are uniform over the workgroup.  A stream longer than the tile keeps its kp leaders
// at the tile's head (run 0, descending, as the network wants it) and fills the rest with the next 16 T - kp composites.
template <int T, class Load>
static __device__ __forceinline__ int rank_stream(u64 *lds, int count, int k, int tid, Load load) {
    constexpr int TILE = 16 * T;
    const int kp = pow2_ceil(k);
    int done = count < TILE ? count : TILE;
    int m = pow2_ceil(done);
    for (int i = tid; i < m; i += T) lds[i] = i < done ? load(i) : 0ull;
    __syncthreads();
    int lead = tile_leaders<T>(lds, m, kp, tid);
    while (done < count) {   // (count > TILE: the first tile was full, lead == kp)
        const int c = (count - done) < (TILE - kp) ? (count - done) : (TILE - kp);
        m = pow2_ceil(kp + c);
        for (int i = kp + tid; i < m; i += T) lds[i] = i < kp + c ? load(done + i - kp) : 0ull;
        __syncthreads();
        lead = tile_leaders<T>(lds, m, kp, tid);
        done += c;
    }
    return lead;
}

// the outputs of segment s from the sorted tile: position, and the score read again through it (a + pos < a + len <= n)
template <int T>
static __device__ __forceinline__ void rank_emit(const u64 *lds, int m, const FrRankArgs &g, int s, int a, int tid) {
    for (int j = tid; j < g.k; j += T) {
        const u64 c = j < m ? lds[j] : 0ull;
        const size_t o = (size_t)s * (size_t)g.k + (size_t)j;
        if (c == 0ull) {
            g.top_idx[o] = -1;
            if (g.top_scores) g.top_scores[o] = __uint_as_float(0xff800000u);
        } else {
            const uint32_t pos = 0xffffffffu - (uint32_t)c;
            g.top_idx[o] = (int32_t)pos;
            if (g.top_scores) g.top_scores[o] = g.scores[(size_t)a + pos];
        }
    }
}

// [a, b) of segment s, or false when it is malformed (uniform over the workgroup)
static __device__ __forceinline__ bool rank_bounds(const FrRankArgs &g, int s, int &a, int &b) {
    a = 0, b = g.n;
    if (g.off) {
        a = g.off[s];
        b = g.off[s + 1];
    }
    return a >= 0 && b >= a && b <= g.n;
}

template <int T>
__global__ __launch_bounds__(T) void rank_segments_kernel(const FrRankArgs g) {
    __shared__ u64 lds[16 * T];
    __shared__ int s_base;
    const int tid = (int)threadIdx.x, s = (int)blockIdx.x;
    int a, b;
    if (!rank_bounds(g, s, a, b)) {
        if (tid == 0) atomicOr_system(g.err_flag, 1);   // pinned host word; error path only
        b = a = 0;
    }
    const int len = b - a;
    if (len > FR_RANK_PART && g.hdr) {
        const int parts = (len + FR_RANK_PART - 1) / FR_RANK_PART;
        if (tid == 0) s_base = atomicAdd(g.hdr, parts);
        __syncthreads();
        const int base = s_base;
        if (base >= 0 && base <= g.u_cap - parts) {   // (overlapping segments, possible only beside malformed ones, can outgrow the units: ranked here then)
            for (int p = tid; p < parts; p += T) g.unitmap[base + p] = make_int4(s, p, parts, 0);
            return;
        }
    }
    const float *sc = g.scores + a;
    const int m = rank_stream<T>(lds, len, g.k, tid, [&](int i) { return rank_composite(__float_as_uint(sc[i]), (uint32_t)i); });
    rank_emit<T>(lds, m, g, s, a, tid);
}

// the unit's record, checked again: false = not a unit of this call
static __device__ __forceinline__ bool rank_unit(const FrRankArgs &g, int u, int &s, int &p, int &parts, int &a, int &b) {
    const int4 e = g.unitmap[u];
    s = e.x, p = e.y, parts = e.z;
    if (s < 0 || s >= g.n_seg || p < 0 || parts < 2 || p >= parts || u - p < 0 || u - p + parts > g.u_cap) return false;
    if (!rank_bounds(g, s, a, b)) return false;
    return (b - a + FR_RANK_PART - 1) / FR_RANK_PART == parts;
}

__global__ __launch_bounds__(256) void rank_parts_kernel(const FrRankArgs g) {
    __shared__ u64 lds[4096];
    const int tid = (int)threadIdx.x, u = (int)blockIdx.x;
    int s, p, parts, a, b;
    if (!rank_unit(g, u, s, p, parts, a, b)) return;
    const int first = p * FR_RANK_PART;
    const int count = (b - a - first) < FR_RANK_PART ? (b - a - first) : FR_RANK_PART;
    const float *sc = g.scores + a + first;
    const int m = rank_stream<256>(lds, count, g.k, tid, [&](int i) { return rank_composite(__float_as_uint(sc[i]), (uint32_t)(first + i)); });
    u64 *out = g.cand + (size_t)u * (size_t)g.k;
    for (int j = tid; j < g.k; j += 256) out[j] = j < m ? lds[j] : 0ull;
}

__global__ __launch_bounds__(256) void rank_merge_kernel(const FrRankArgs g, int stride) {
    __shared__ u64 lds[4096];
    const int tid = (int)threadIdx.x, u = (int)blockIdx.x;
    int s, p, parts, a, b;
    if (!rank_unit(g, u, s, p, parts, a, b)) return;
    if (p % (stride * FR_RANK_FAN) != 0 || parts <= stride) return;   // not the head of a group / finished at an earlier level
    int lists = (parts - p + stride - 1) / stride;
    if (lists > FR_RANK_FAN) lists = FR_RANK_FAN;
    const int k = g.k;
    const u64 *in = g.cand + (size_t)u * (size_t)k;
    const size_t step = (size_t)stride * (size_t)k;
    // lists * k <= 16 * 256: one tile, no streaming -- every list is in LDS before the head's own list is written again
    const int m = rank_stream<256>(lds, lists * k, k, tid, [&](int i) { return in[(size_t)(i / k) * step + (size_t)(i % k)]; });
    if (parts <= stride * FR_RANK_FAN) {
        rank_emit<256>(lds, m, g, s, a, tid);
    } else {
        u64 *out = g.cand + (size_t)u * (size_t)k;
        for (int j = tid; j < k; j += 256) out[j] = j < m ? lds[j] : 0ull;
    }
}

extern "C" __attribute__((visibility("default"))) int fr_rank_launch(const FrRankArgs *args, int wave_form, void *stream) {
    const FrRankArgs g = *args;
    hipStream_t s = (hipStream_t)stream;
    if (g.hdr) {   // the unit counter and the unit records of this call: zero / "no unit" (s = -1)
        hipError_t e = hipMemsetAsync(g.hdr, 0, FR_RANK_HDR_BYTES, s);
        if (e == hipSuccess) e = hipMemsetAsync(g.unitmap, 0xff, (size_t)g.u_cap * sizeof(int4), s);
        if (e != hipSuccess) return (int)e;
    }
    if (wave_form) rank_segments_kernel<64><<<dim3((unsigned)g.n_seg), dim3(64), 0, s>>>(g);
    else rank_segments_kernel<256><<<dim3((unsigned)g.n_seg), dim3(256), 0, s>>>(g);
    if (g.hdr) {
        rank_parts_kernel<<<dim3((unsigned)g.u_cap), dim3(256), 0, s>>>(g);
        const int max_parts = (g.n + FR_RANK_PART - 1) / FR_RANK_PART;
        for (int stride = 1; stride < max_parts; stride *= FR_RANK_FAN) rank_merge_kernel<<<dim3((unsigned)g.u_cap), dim3(256), 0, s>>>(g, stride);
    }
    return (int)hipGetLastError();
}
