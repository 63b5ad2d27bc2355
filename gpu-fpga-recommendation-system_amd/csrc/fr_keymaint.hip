// The life cycle of a key map (fr_*_erase_keys / fr_ctx_key_space_stats / fr_ctx_export_keys / fr_ctx_rebuild_key_space, fleetrec_serving.h) ->
// libfleetrec_keymaint.so, the fifth COMPANION code object of libfleetrec.so, built and linked as the other four are (the kernel lists of libfleetrec.so
// and of libfleetrec_keys.so are pinned name for name; every kernel here carries keymap_ in front).  It calls nothing of libfleetrec.so: its two
// launchers return a hipError_t value.  Slot layout, mix64, the probe rule, the dead / live predicates and the displacement are fr_keys.h's, shared
// with the CPU back-end.  A new map is filled by fr_key_fill_launch (libfleetrec_keys.so).
//
// keymap_erase_kernel: one thread per key.  fr_key_find walks from the home slot (at most `slots` probes whatever the memory holds); on a match ONE plain
//   4-byte store writes the column's miss_row into the slot's row.  The key stays, so every probe chain stays whole and neither key_resolve_kernel nor
//   key_put_kernel has anything to learn; an absent key writes nothing.  A key of -1 raises FR_KEYS_ERR_ERASE_EMPTY (pinned host word; error path only).
// keymap_walk_kernel<SINK>: one pass over the slots of a map.  A workgroup takes a chunk of 256 x FR_KEYMAINT_PER_THREAD consecutive slots, thread t the
//   slots t, t + 256, ... of it: every wave-instruction loads 1 KiB of contiguous slots (one 16-byte load per lane), and a thread's loads are all issued
//   before its first compare.  The workgroups stride over the chunks (the grid is capped by max_blocks).  A whole wave stays in the loop -- a slot past
//   the map reads as empty -- so ballots and shuffles see 64 lanes.
//     COUNT   occupied and live through ballot + popcount, the displacements summed per lane and then across the wave; ONE atomic add per wave and
//             quantity when the wave leaves the loop, none for a quantity that stayed zero.
//     EXPORT  per chunk a wave reserves the places of its live pairs with ONE returning atomic add (lane 0; the sum of its ballots' popcounts) and
//             every live lane writes at its prefix -- only where the position is below cap.  counts[0] ends as the live pairs of the map.
//     REHASH  every live lane inserts its pair into the new map: home slot under the new seed and mask, a 64-bit atomicCAS claims an empty slot, the row
//             is stored second.  Every decision rests on the value the CAS returned.  The keys of a map are distinct, so there is no duplicate to
//             handle and no place to reserve; the loop is bounded by the new map's slot count.  The inserted pairs are counted once per wave.
// No kernel here needs scratch.
#include <hip/hip_runtime.h>

#include "fr_internal.h"

__global__ __launch_bounds__(256) void keymap_erase_kernel(const FrKeyEraseArgs g) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= g.n) return;
    const int64_t k = g.keys[i];
    if (k == FR_KEYS_EMPTY_KEY) {
        atomicOr_system(g.err_flag, FR_KEYS_ERR_ERASE_EMPTY);
        return;
    }
    const int64_t at = fr_key_find(g.col, k);
    if (at >= 0) g.col.slots[at].row = g.col.miss_row;
}

static __device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, d), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), d);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

template <int SINK> __global__ __launch_bounds__(256) void keymap_walk_kernel(const FrKeyWalkArgs g) {
    constexpr int PT = FR_KEYMAINT_PER_THREAD;
    constexpr unsigned CHUNK = 256u * PT;
    const uint64_t n = (uint64_t)g.col.mask + 1;
    const uint64_t step = (uint64_t)gridDim.x * CHUNK;
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long occupied = 0, live = 0, psum = 0;   // occupied, live: the wave's (uniform); psum: the lane's
    for (uint64_t base = (uint64_t)blockIdx.x * CHUNK; base < n; base += step) {   // (uniform: the whole workgroup stays in the loop)
        FrKeySlot s[PT];
#pragma unroll
        for (int j = 0; j < PT; j++) {   // every load is issued before the first compare
            const uint64_t i = base + (uint64_t)j * 256u + tid;
            s[j] = FrKeySlot{FR_KEYS_EMPTY_KEY, g.col.miss_row, 0};
            if (i < n) s[j] = fr_key_load_slot(g.col.slots + i);
        }
        if (SINK == FR_KEYWALK_COUNT) {
#pragma unroll
            for (int j = 0; j < PT; j++) {
                const bool o = fr_key_slot_occupied(s[j]);
                occupied += (unsigned long long)__popcll(__ballot(o));
                live += (unsigned long long)__popcll(__ballot(fr_key_slot_live(s[j], g.col.miss_row)));
                if (o) psum += fr_key_displacement(g.col, s[j].key, base + (uint64_t)j * 256u + tid);
            }
        } else if (SINK == FR_KEYWALK_EXPORT) {
            unsigned long long b[PT];
            unsigned total = 0;
#pragma unroll
            for (int j = 0; j < PT; j++) {
                b[j] = __ballot(fr_key_slot_live(s[j], g.col.miss_row));
                total += (unsigned)__popcll(b[j]);
            }
            if (total) {   // (uniform in the wave)
                unsigned long long first = 0;
                if (lane == 0) first = atomicAdd(g.counts, (unsigned long long)total);
                const unsigned lo = (unsigned)__shfl((int)(unsigned)first, 0), hi = (unsigned)__shfl((int)(unsigned)(first >> 32), 0);
                uint64_t pos = ((uint64_t)hi << 32) | lo;
#pragma unroll
                for (int j = 0; j < PT; j++) {
                    const uint64_t mine = pos + (uint64_t)__popcll(b[j] & below);
                    if (((b[j] >> lane) & 1ull) && mine < g.cap) g.out_keys[mine] = s[j].key, g.out_rows[mine] = s[j].row;
                    pos += (uint64_t)__popcll(b[j]);
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < PT; j++) {
                bool placed = false;
                if (fr_key_slot_live(s[j], g.col.miss_row)) {
                    const int64_t k = s[j].key;
                    uint64_t h = fr_key_home(g.dst, k);
                    for (uint64_t left = (uint64_t)g.dst.mask + 1; left; left--) {   // at most the new map's slots
                        unsigned long long *kp = reinterpret_cast<unsigned long long *>(&g.dst.slots[h].key);
                        unsigned long long cur = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (cur == (unsigned long long)FR_KEYS_EMPTY_KEY) cur = atomicCAS(kp, (unsigned long long)FR_KEYS_EMPTY_KEY, (unsigned long long)k);
                        if (cur == (unsigned long long)FR_KEYS_EMPTY_KEY) {   // claimed (a stale load can only show a taken slot empty: the CAS then returns its key)
                            placed = true;
                            break;
                        }
                        h = (h + 1) & (uint64_t)g.dst.mask;
                    }
                    if (placed) g.dst.slots[h].row = s[j].row;   // the row second
                }
                live += (unsigned long long)__popcll(__ballot(placed));
            }
        }
    }
    if (SINK == FR_KEYWALK_COUNT) {
        psum = wave_sum(psum);
        if (lane == 0) {
            if (occupied) atomicAdd(g.counts + 0, occupied);
            if (live) atomicAdd(g.counts + 1, live);
            if (psum) atomicAdd(g.counts + 2, psum);
        }
    } else if (SINK == FR_KEYWALK_REHASH) {
        if (lane == 0 && live) atomicAdd(g.counts + 0, live);
    }
}

extern "C" __attribute__((visibility("default"))) int fr_keymap_erase_launch(const FrKeyEraseArgs *args, void *stream) {
    const FrKeyEraseArgs g = *args;
    keymap_erase_kernel<<<dim3((unsigned)((g.n + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(g);
    return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("default"))) int fr_keymap_walk_launch(const FrKeyWalkArgs *args, void *stream) {
    const FrKeyWalkArgs g = *args;
    const uint64_t slots = (uint64_t)g.col.mask + 1, chunk = 256u * FR_KEYMAINT_PER_THREAD;
    const uint64_t chunks = (slots + chunk - 1) / chunk, cap = (uint64_t)(g.max_blocks > 0 ? g.max_blocks : 1);
    const dim3 grid((unsigned)(chunks < cap ? chunks : cap));
    if (g.sink == FR_KEYWALK_COUNT) keymap_walk_kernel<FR_KEYWALK_COUNT><<<grid, dim3(256), 0, (hipStream_t)stream>>>(g);
    else if (g.sink == FR_KEYWALK_EXPORT) keymap_walk_kernel<FR_KEYWALK_EXPORT><<<grid, dim3(256), 0, (hipStream_t)stream>>>(g);
    else if (g.sink == FR_KEYWALK_REHASH) keymap_walk_kernel<FR_KEYWALK_REHASH><<<grid, dim3(256), 0, (hipStream_t)stream>>>(g);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}
