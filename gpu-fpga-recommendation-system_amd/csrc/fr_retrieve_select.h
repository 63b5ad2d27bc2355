// The selection networks of the retrieval scans, shared by all five of them (fr_retrieve.hip, fr_retrieve_lp.hip, fr_retrieve_probe.hip,
// fr_retrieve_probe_lp.hip, fr_retrieve_filter.hip): the one-wave bitonic leader reduction over a query's buffer, the reduction of a whole query tile
// and the key -> score bits mapping.  fr_retrieve.hip's head comment has the reasoning.  Device code only; every function is inlined into its kernel, so
// nothing here appears in a code object under a name of its own.  What the bf16 scans share beyond this is in fr_retrieve_lp_scan.h.
#pragma once
#include <hip/hip_runtime.h>

#include "fr_internal.h"

typedef unsigned long long u64;
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int RT_THREADS = 256, RT_WAVES = 4;

static __device__ __forceinline__ int pow2_ceil(int v) {
    int m = 2;
    while (m < v) m <<= 1;
    return m;
}

// between two steps of a wave's own LDS network: the hardware keeps a wave's DS instructions in order, the compiler must too
static __device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one compare-exchange step over b[0 .. 2 * half) (ce_step of fr_rank.hip, by one wave): pair p is (i, i + stride), i = 2p - (p & (stride - 1)),
// descending where (i & dirmask) == 0
static __device__ __forceinline__ void wave_ce_step(u64 *b, int half, int stride, int dirmask, int lane) {
    for (int p = lane; p < half; p += 64) {
        const int i = 2 * p - (p & (stride - 1));
        const u64 x = b[i], y = b[i + stride];
        if ((x < y) == ((i & dirmask) == 0)) b[i] = y, b[i + stride] = x;
    }
    wave_sync();
}

// the kp leaders of b[0 .. m), descending in b[0 .. kp); m a power of two, kp < m <= 512 (tile_leaders of fr_rank.hip, by one wave)
static __device__ __forceinline__ void wave_leaders(u64 *b, int m, int kp, int lane) {
    for (int size = 2; size <= kp; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) wave_ce_step(b, m >> 1, stride, size, lane);
    while (m > kp) {
        const int half = m >> 1;   // <= 256: four per lane
        u64 v[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int p = lane + 64 * r;
            if (p < half) {
                const int x = 2 * p - (p & (kp - 1));
                const u64 c = b[x], d = b[x + kp];
                v[r] = c > d ? c : d;
            }
        }
        wave_sync();
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int p = lane + 64 * r;
            if (p < half) b[p] = v[r];
        }
        wave_sync();
        m = half;
        for (int stride = kp >> 1; stride > 0; stride >>= 1) wave_ce_step(b, m >> 1, stride, kp, lane);
    }
}

// the leader reduction of a scan's query tile: wave w takes queries w, w + 4, ...; a query with appended composites gets its kp leaders back in
// buf[qi * BUF .. + kp), its k-th as the new threshold and an empty append area
template <int BUF>
static __device__ __forceinline__ void scan_reduce(u64 *buf, u64 *thr, int *cnt, int k, int kp, int lane, int wave) {
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
}

// the score bits a key stands for (every NaN: the quiet NaN)
static __device__ __forceinline__ uint32_t retrieve_bits(uint32_t key) { return key == 0u ? FR_RETRIEVE_PAD_BITS : ((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key); }
