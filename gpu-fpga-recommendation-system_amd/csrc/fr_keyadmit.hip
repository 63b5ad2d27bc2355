// Row pools: admitting ids (fr_ctx_set_row_pool / fr_*_admit_keys, and fr_*_erase_keys on a column with a pool; fleetrec_serving.h) ->
// libfleetrec_admit.so, the sixth COMPANION code object of libfleetrec.so, built and linked as the other five are (the kernel lists of libfleetrec.so,
// libfleetrec_keys.so and libfleetrec_keymaint.so are pinned name for name; every kernel here carries keyadmit_ in front).  It calls nothing of
// libfleetrec.so: its four launchers return a hipError_t value.  Slot layout, mix64, the probe rule and the pool record (FrKeyPool: one bit per pool
// row, set = taken, and ONE signed counter of free rows) are fr_keys.h's, shared with the CPU back-end.
//
// keyadmit_admit_kernel: one thread per key.  The occurrences of a key inside the call first elect ONE of them in the call's own table (a 64-bit
//   atomicCAS on a table of >= 2 n slots the host pre-filled; the others leave the table slot's index in rows_out for keyadmit_settle_kernel): so a key
//   listed 301 times takes one row and one place in the key count, not 301 of each for a moment.  The elected lane probes as key_put_kernel does; a live
//   key is done.  Otherwise it takes a row -- one from the counter (a counter found at zero or below is given back and reported), then a clear bit found
//   by a scan that starts at a hash of the key (a few hashed hops, then word after word) and claims with atomicOr: the bit is ours only if the
//   returned word had it clear --, claims a slot under the put's rules when the key is absent (the place in n_keys reserved before the 64-bit CAS, given back when the key turns out to be there), and
//   decides the row with ONE 32-bit atomicCAS on the slot's row word, miss_row -> r: empty slots are pre-filled with miss_row and dead ones hold it, so
//   of any number of lanes admitting the key (other workers' included) exactly one CAS succeeds; a loser reports the row the CAS returned and gives its
//   own bit and count back.  No lane waits for another.  The row comes before the slot so that a key that finds no row stays absent.
// keyadmit_settle_kernel: one thread per key; an entry <= -2 names the table slot of the elected occurrence, whose row it takes.
// keyadmit_release_kernel: one thread per key.  fr_key_find, then atomicExch(row, miss_row); a returned row inside the pool range has its bit cleared
//   with atomicAnd, and the counter is incremented only if the returned word had the bit set: a key listed twice, or a row the pool never handed out,
//   releases nothing.  A key of -1 raises FR_KEYS_ERR_ERASE_EMPTY.
// keyadmit_mark_kernel: one pass over the slots in the shape of keymap_walk_kernel (16-byte slot loads, 1 KiB per wave-instruction, a thread's loads
//   all issued before its first compare): the bit of every live key's row inside the range is set, the newly set bits are counted per wave (ballot +
//   popcount) and leave the counter with ONE atomic per wave.  The host clears the bitmap (but for the pad bits) and sets the counter to n_rows first.
// Every decision rests on the value an atomic returned; the scans read with relaxed agent-scope atomic loads.  Every loop has a trip count bounded by
// the slot count, the word count of the bitmap or the table of the call, whatever the memory holds.  No kernel needs scratch or LDS.
#include <hip/hip_runtime.h>

#include "fr_internal.h"

static __device__ __forceinline__ void pool_give(const FrKeyPool &p, int32_t row) {
    const uint32_t o = (uint32_t)(row - p.first_row), bit = 1u << (o & 31u);
    if (atomicAnd(p.bits + (o >> 5), ~bit) & bit) atomicAdd(p.free_rows, 1);
}

// -> a row of the pool, now taken, or -1: no free row (or, beside racing erases, none found within two turns of the bitmap).
// The scan: FR_KEYADMIT_HOPS words at positions drawn from the key's hash (a walk from word to NEXT word clusters as linear probing does: with 99 % of
// a 4 M-row pool taken, runs of full words made the slowest lanes of a 65 536-key call walk hundreds of words), then, for the bound, word after word
// for two turns of the bitmap.
constexpr uint32_t FR_KEYADMIT_HOPS = 32;
static __device__ int32_t pool_take(const FrKeyPool &p, uint64_t z) {
    if (atomicSub(p.free_rows, 1) <= 0) {
        atomicAdd(p.free_rows, 1);
        return -1;
    }
    const uint32_t words = fr_key_pool_words(p.n_rows);
    uint32_t w = (uint32_t)(z >> 32) % words;
    for (uint32_t left = 2u * words + FR_KEYADMIT_HOPS; left; left--) {
        uint32_t v = __hip_atomic_load(p.bits + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int tries = 0; tries < 32 && v != ~0u; tries++) {   // (a word has 32 bits: every failed claim found one more of them taken)
            const uint32_t b = (uint32_t)__ffs((int)~v) - 1u, bit = 1u << b;
            v = atomicOr(p.bits + w, bit);
            if (!(v & bit)) return p.first_row + (int32_t)(w * 32u + b);   // (a pad bit is never clear: w * 32 + b < n_rows)
        }
        if (left > 2u * words) {   // still hopping
            z = z * 6364136223846793005ull + 1442695040888963407ull;
            w = (uint32_t)(z >> 33) % words;
        } else if (++w == words) {
            w = 0;
        }
    }
    atomicAdd(p.free_rows, 1);
    return -1;
}

// the admit of ONE key (not -1) -> what rows_out reports; *bad: the FR_KEYS_ERR_* bit of a key that was not applied
static __device__ int32_t admit_one(const FrKeyAdmitArgs &g, int64_t k, int *bad) {
    const uint64_t z = fr_mix64((uint64_t)k ^ g.col.seed);
    uint64_t h = z & (uint64_t)g.col.mask;
    uint64_t left = (uint64_t)g.col.mask + 1;   // at most `slots` probes, the claim below included
    bool found = false;
    for (; left; left--) {
        const unsigned long long cur = __hip_atomic_load(reinterpret_cast<unsigned long long *>(&g.col.slots[h].key), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == (unsigned long long)k) found = true;
        if (found || cur == (unsigned long long)FR_KEYS_EMPTY_KEY) break;
        h = (h + 1) & (uint64_t)g.col.mask;
    }
    if (found) {
        const int32_t row = __hip_atomic_load(&g.col.slots[h].row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (row != g.col.miss_row) return row;   // live: nothing is written
    }
    const int32_t r = pool_take(g.pool, z);
    if (r < 0) {
        *bad = FR_KEYS_ERR_NO_FREE_ROW;
        return FR_KEYS_NO_ROW;
    }
    if (!found) {   // absent: a slot under the put's rules, from the empty slot the probe stopped at
        bool reserved = false;
        for (; left; left--) {
            unsigned long long *kp = reinterpret_cast<unsigned long long *>(&g.col.slots[h].key);
            unsigned long long cur = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == (unsigned long long)FR_KEYS_EMPTY_KEY) {
                if (!reserved) {
                    if (atomicAdd(g.n_keys, 1u) >= g.max_keys) {   // the map is full: nothing is claimed, the row goes back
                        atomicSub(g.n_keys, 1u);
                        break;
                    }
                    reserved = true;
                }
                cur = atomicCAS(kp, (unsigned long long)FR_KEYS_EMPTY_KEY, (unsigned long long)k);
                if (cur == (unsigned long long)FR_KEYS_EMPTY_KEY) {   // claimed: the reservation is this key's place in the count
                    reserved = false, found = true;
                    break;
                }
            }
            if (cur == (unsigned long long)k) {   // another worker's admit or put claimed it meanwhile
                found = true;
                break;
            }
            h = (h + 1) & (uint64_t)g.col.mask;
        }
        if (reserved) atomicSub(g.n_keys, 1u);
        if (!found) {
            pool_give(g.pool, r);
            *bad = FR_KEYS_ERR_FULL;
            return FR_KEYS_NO_ROW;
        }
    }
    const int32_t prev = atomicCAS(&g.col.slots[h].row, g.col.miss_row, r);
    if (prev == g.col.miss_row) return r;
    pool_give(g.pool, r);   // somebody gave the key a row meanwhile: theirs
    return prev;
}

__global__ __launch_bounds__(256) void keyadmit_admit_kernel(const FrKeyAdmitArgs g) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= g.n) return;
    const int64_t k = g.keys[i];
    if (k == FR_KEYS_EMPTY_KEY) {
        atomicOr_system(g.err_flag, FR_KEYS_ERR_EMPTY_KEY | FR_KEYS_ERR_ADMIT);   // pinned host word; error path only
        g.rows_out[i] = -1;
        return;
    }
    // the election among the occurrences of k in this call
    uint32_t t = (uint32_t)fr_mix64((uint64_t)k + 0x9e3779b97f4a7c15ull) & g.tab_mask;
    bool elected = false, other = false;
    for (uint64_t left = (uint64_t)g.tab_mask + 1; left; left--) {   // (the table holds >= 2 n slots: an empty one is always found)
        unsigned long long *kp = reinterpret_cast<unsigned long long *>(&g.tab[t].key);
        unsigned long long cur = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == (unsigned long long)FR_KEYS_EMPTY_KEY) {
            cur = atomicCAS(kp, (unsigned long long)FR_KEYS_EMPTY_KEY, (unsigned long long)k);
            elected = cur == (unsigned long long)FR_KEYS_EMPTY_KEY;
        }
        other = cur == (unsigned long long)k;
        if (elected || other) break;
        t = (t + 1u) & g.tab_mask;
    }
    if (other) {
        g.rows_out[i] = -2 - (int32_t)t;   // (t <= tab_mask < 2^31 - 2) settled by the next launch
        return;
    }
    int bad = 0;
    const int32_t row = admit_one(g, k, &bad);   // (a table without room, which the host rules out, would admit every occurrence: still one row per key)
    if (elected) g.tab[t].row = row;
    g.rows_out[i] = row;
    if (bad) atomicOr_system(g.err_flag, bad | FR_KEYS_ERR_ADMIT);
}

__global__ __launch_bounds__(256) void keyadmit_settle_kernel(const FrKeyAdmitArgs g) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= g.n) return;
    const int32_t v = g.rows_out[i];
    if (v > -2) return;
    const uint32_t t = (uint32_t)(-2 - v);
    if (t <= g.tab_mask) g.rows_out[i] = g.tab[t].row;
}

__global__ __launch_bounds__(256) void keyadmit_release_kernel(const FrKeyReleaseArgs g) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= g.n) return;
    const int64_t k = g.keys[i];
    if (k == FR_KEYS_EMPTY_KEY) {
        atomicOr_system(g.err_flag, FR_KEYS_ERR_ERASE_EMPTY);
        return;
    }
    const int64_t at = fr_key_find(g.col, k);
    if (at < 0) return;
    const int32_t was = atomicExch(&g.col.slots[at].row, g.col.miss_row);
    if (was != g.col.miss_row && fr_key_pool_holds(g.pool, was)) pool_give(g.pool, was);
}

__global__ __launch_bounds__(256) void keyadmit_mark_kernel(const FrKeyMarkArgs g) {
    constexpr int PT = FR_KEYADMIT_PER_THREAD;
    constexpr unsigned CHUNK = 256u * PT;
    const uint64_t n = (uint64_t)g.col.mask + 1;
    const uint64_t step = (uint64_t)gridDim.x * CHUNK;
    const unsigned tid = threadIdx.x;
    unsigned taken = 0;   // the wave's (uniform); at most n_rows
    for (uint64_t base = (uint64_t)blockIdx.x * CHUNK; base < n; base += step) {   // (uniform: the whole workgroup stays in the loop)
        FrKeySlot s[PT];
#pragma unroll
        for (int j = 0; j < PT; j++) {   // every load is issued before the first compare
            const uint64_t i = base + (uint64_t)j * 256u + tid;
            s[j] = FrKeySlot{FR_KEYS_EMPTY_KEY, g.col.miss_row, 0};
            if (i < n) s[j] = fr_key_load_slot(g.col.slots + i);
        }
#pragma unroll
        for (int j = 0; j < PT; j++) {
            bool fresh = false;
            if (fr_key_slot_live(s[j], g.col.miss_row) && fr_key_pool_holds(g.pool, s[j].row)) {
                const uint32_t o = (uint32_t)(s[j].row - g.pool.first_row), bit = 1u << (o & 31u);
                fresh = !(atomicOr(g.pool.bits + (o >> 5), bit) & bit);   // (two live keys may share a row put by hand: it is taken once)
            }
            taken += (unsigned)__popcll(__ballot(fresh));
        }
    }
    if ((tid & 63u) == 0 && taken) atomicSub(g.pool.free_rows, (int)taken);
}

extern "C" __attribute__((visibility("default"))) int fr_keyadmit_admit_launch(const FrKeyAdmitArgs *args, void *stream) {
    const FrKeyAdmitArgs g = *args;
    keyadmit_admit_kernel<<<dim3((unsigned)((g.n + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(g);
    return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("default"))) int fr_keyadmit_settle_launch(const FrKeyAdmitArgs *args, void *stream) {
    const FrKeyAdmitArgs g = *args;
    keyadmit_settle_kernel<<<dim3((unsigned)((g.n + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(g);
    return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("default"))) int fr_keyadmit_release_launch(const FrKeyReleaseArgs *args, void *stream) {
    const FrKeyReleaseArgs g = *args;
    keyadmit_release_kernel<<<dim3((unsigned)((g.n + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(g);
    return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("default"))) int fr_keyadmit_mark_launch(const FrKeyMarkArgs *args, void *stream) {
    const FrKeyMarkArgs g = *args;
    const uint64_t slots = (uint64_t)g.col.mask + 1, chunk = 256u * FR_KEYADMIT_PER_THREAD;
    const uint64_t chunks = (slots + chunk - 1) / chunk, cap = (uint64_t)(g.max_blocks > 0 ? g.max_blocks : 1);
    keyadmit_mark_kernel<<<dim3((unsigned)(chunks < cap ? chunks : cap)), dim3(256), 0, (hipStream_t)stream>>>(g);
    return (int)hipGetLastError();
}
