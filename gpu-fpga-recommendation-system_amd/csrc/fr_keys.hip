// Keyed lookups (fr_ctx_set_key_space / fr_*_put_keys / fr_worker_resolve_keys_device, fleetrec_serving.h) -> libfleetrec_keys.so, the third COMPANION
// code object of libfleetrec.so, built and linked as libfleetrec_rank.so and libfleetrec_request.so are (the kernel list of libfleetrec.so is pinned
// name for name; every kernel here carries key_ in front).  It calls nothing of libfleetrec.so: its three launchers return a hipError_t value.  Slot
// layout, mix64 and the probe rule are fr_keys.h's, shared with the CPU back-end.
//
// key_resolve_kernel: int64 keys [total] (total = n_rows x W, 8-byte aligned only) -> int32 rows [total]; word e belongs to index column wcol[e % W].
//   Lanes run along consecutive key words: a workgroup takes a chunk of 256 x FR_KEY_PER_THREAD consecutive words, thread t the words t, t + 256, ...
//   of it, so every wave-instruction loads 512 contiguous bytes of keys and stores 256 contiguous bytes of rows whatever W is.  The word inside the row
//   advances by (256 % W) per key and by (grid step % W) per chunk: one division per thread in front of the loop, none inside.
//   The word -> column table (uint16, up to FR_KEYS_LDS_WORDS words; a longer row reads it in place) and
//   the per-column records (32 bytes each, at most FR_KEYS_LDS_COLS of them) are staged in LDS once per workgroup -- consecutive lanes read
//   consecutive columns -- and the workgroups stride over the chunks, so that the staging is paid once per ~3 chunks per CU at the large shapes.
//   A MAPPED lookup is a dependent read that misses every cache when the map is large (MI355X guide, "Indexed rows": a lone dependent read pays the
//   whole HBM-miss latency): a thread first loads its FR_KEY_PER_THREAD keys, then issues the first probe (ONE 16-byte slot load) of every one of
//   them, and only then compares; linear probing keeps a second probe in the same 128-byte line seven times out of eight.
//   Misses: one atomic add per wave and chunk (ballot + popcount over the wave's lanes), none when the wave had no miss.
// key_put_kernel: one thread per (key, row) pair.  A 64-bit atomicCAS claims an empty slot for the key, a plain store then writes the row: a resolve
//   in flight on another stream sees the key with the row the slot was pre-filled with (the column's miss_row) or with the new row, nothing else.
//   A place in the column's key count is reserved BEFORE a slot is claimed and given back when the key turns out to be there already (a
//   duplicate inside the call, or a claim that lost its race to the same key); a put that finds the count at max_keys claims nothing.
//   The decisions rest on the values the CAS returns, never on what a plain load showed: slots are never released, so a stale load can only show a
//   slot empty that is taken by now, and the CAS on it then returns the key that took it.
// key_fill_kernel: every slot <- {FR_KEY_EMPTY, miss_row, 0}, one 16-byte store per slot.
// Every loop has a trip count bounded by the slot count or by the words of the call, whatever the memory holds.
#include <hip/hip_runtime.h>

#include "fr_internal.h"

template <bool LDS> __global__ __launch_bounds__(256) void key_resolve_kernel(const FrKeyResolveArgs g) {
    __shared__ __attribute__((aligned(16))) FrKeyCol s_cols[LDS ? FR_KEYS_LDS_COLS : 1];   // (staged with 16-byte stores)
    __shared__ uint16_t s_wcol[FR_KEYS_LDS_WORDS];
    const int tid = (int)threadIdx.x;
    const bool w_lds = g.W <= FR_KEYS_LDS_WORDS;   // (uniform) the word -> column table fits: one global round trip less in front of every first probe
    if (w_lds)
        for (int i = tid; i < g.W; i += 256) s_wcol[i] = g.wcol[i];
    if (LDS) {
        const uint4 *src = reinterpret_cast<const uint4 *>(g.cols);
        uint4 *dst = reinterpret_cast<uint4 *>(s_cols);
        for (int i = tid; i < 2 * g.n_cols; i += 256) dst[i] = src[i];   // n_cols <= FR_KEYS_LDS_COLS (the launcher picks the form)
    }
    __syncthreads();
    const FrKeyCol *cols = LDS ? s_cols : g.cols;
    constexpr unsigned CHUNK = 256u * FR_KEY_PER_THREAD;
    const unsigned W = (unsigned)g.W;
    const unsigned w256 = 256u % W;
    const uint64_t step = (uint64_t)gridDim.x * CHUNK;
    const unsigned w_step = (unsigned)(step % W);
    uint64_t e0 = (uint64_t)blockIdx.x * CHUNK + (uint64_t)tid;
    unsigned word0 = (unsigned)(e0 % W);
    for (; e0 - (uint64_t)tid < g.total; e0 += step) {   // (the chunk's first word is inside: the whole wave stays in the loop)
        int64_t k[FR_KEY_PER_THREAD];
        unsigned col[FR_KEY_PER_THREAD];
        int32_t row[FR_KEY_PER_THREAD];
        uint64_t h[FR_KEY_PER_THREAD];
        FrKeySlot s[FR_KEY_PER_THREAD];
        bool probe[FR_KEY_PER_THREAD];
        unsigned word = word0;
#pragma unroll
        for (int j = 0; j < FR_KEY_PER_THREAD; j++) {
            const uint64_t e = e0 + (uint64_t)j * 256u;
            const bool in = e < g.total;
            k[j] = in ? g.keys[e] : FR_KEYS_EMPTY_KEY;
            col[j] = in ? (unsigned)(w_lds ? s_wcol[word] : g.wcol[word]) : 0u;
            word += w256;
            if (word >= W) word -= W;
        }
#pragma unroll
        for (int j = 0; j < FR_KEY_PER_THREAD; j++) {   // every first probe is issued before the first compare
            const FrKeyCol &c = cols[col[j]];
            probe[j] = !fr_key_direct(c, k[j], &row[j]);
            h[j] = 0;
            s[j] = FrKeySlot{FR_KEYS_EMPTY_KEY, 0, 0};
            if (probe[j]) {
                h[j] = fr_key_home(c, k[j]);
                s[j] = fr_key_load_slot(c.slots + h[j]);
            }
        }
        unsigned misses = 0;
#pragma unroll
        for (int j = 0; j < FR_KEY_PER_THREAD; j++) {
            bool miss = false;
            if (probe[j]) row[j] = fr_key_probe(cols[col[j]], k[j], h[j], s[j], &miss);
            misses += (unsigned)__popcll(__ballot(miss));
            const uint64_t e = e0 + (uint64_t)j * 256u;
            if (e < g.total) g.out[e] = row[j];
        }
        if (misses && (tid & 63) == 0) atomicAdd(g.misses, (unsigned long long)misses);
        word0 += w_step;
        if (word0 >= W) word0 -= W;
    }
}

__global__ __launch_bounds__(256) void key_put_kernel(const FrKeyPutArgs g) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= g.n) return;
    const int64_t k = g.keys[i];
    const int32_t r = g.rows[i];
    if (k == FR_KEYS_EMPTY_KEY) {
        atomicOr_system(g.err_flag, FR_KEYS_ERR_EMPTY_KEY);   // pinned host word; error path only
        return;
    }
    if (!fr_key_row_legal(g.col.range, g.col.miss_row, r)) {
        atomicOr_system(g.err_flag, FR_KEYS_ERR_ROW);
        return;
    }
    uint64_t h = fr_key_home(g.col, k);
    bool reserved = false, found = false;
    for (uint64_t left = (uint64_t)g.col.mask + 1; left; left--) {   // at most `slots` probes
        unsigned long long *kp = reinterpret_cast<unsigned long long *>(&g.col.slots[h].key);
        unsigned long long cur = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == (unsigned long long)FR_KEYS_EMPTY_KEY) {
            if (!reserved) {
                if (atomicAdd(g.n_keys, 1u) >= g.max_keys) {   // the map is full: nothing is claimed
                    atomicSub(g.n_keys, 1u);
                    atomicOr_system(g.err_flag, FR_KEYS_ERR_FULL);
                    return;
                }
                reserved = true;
            }
            cur = atomicCAS(kp, (unsigned long long)FR_KEYS_EMPTY_KEY, (unsigned long long)k);
            if (cur == (unsigned long long)FR_KEYS_EMPTY_KEY) {   // claimed: the reservation is this key's place in the count
                reserved = false, found = true;
                break;
            }
        }
        if (cur == (unsigned long long)k) {
            found = true;
            break;
        }
        h = (h + 1) & (uint64_t)g.col.mask;
    }
    if (reserved) atomicSub(g.n_keys, 1u);   // the key was there already (or, in a corrupt map, no slot was)
    if (found) g.col.slots[h].row = r;       // the row second: until it lands the slot reads as the pre-filled miss_row (or the key's old row)
    else atomicOr_system(g.err_flag, FR_KEYS_ERR_FULL);
}

__global__ __launch_bounds__(256) void key_fill_kernel(const FrKeyFillArgs g) {
    const int4 v = make_int4(-1, -1, g.miss_row, 0);
    int4 *dst = reinterpret_cast<int4 *>(g.slots);
    const uint64_t step = (uint64_t)gridDim.x * 256u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < g.n; i += step) dst[i] = v;
}

extern "C" __attribute__((visibility("default"))) int fr_key_resolve_launch(const FrKeyResolveArgs *args, void *stream) {
    const FrKeyResolveArgs g = *args;
    const uint64_t chunks = (g.total + 256u * FR_KEY_PER_THREAD - 1) / (256u * FR_KEY_PER_THREAD);
    const uint64_t cap = (uint64_t)(g.max_blocks > 0 ? g.max_blocks : 1);
    const dim3 grid((unsigned)(chunks < cap ? chunks : cap));
    if (g.n_cols <= FR_KEYS_LDS_COLS) key_resolve_kernel<true><<<grid, dim3(256), 0, (hipStream_t)stream>>>(g);
    else key_resolve_kernel<false><<<grid, dim3(256), 0, (hipStream_t)stream>>>(g);
    return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("default"))) int fr_key_put_launch(const FrKeyPutArgs *args, void *stream) {
    const FrKeyPutArgs g = *args;
    key_put_kernel<<<dim3((unsigned)((g.n + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(g);
    return (int)hipGetLastError();
}

extern "C" __attribute__((visibility("default"))) int fr_key_fill_launch(const FrKeyFillArgs *args, void *stream) {
    const FrKeyFillArgs g = *args;
    const uint64_t blocks = (g.n + 255) / 256;
    key_fill_kernel<<<dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream>>>(g);
    return (int)hipGetLastError();
}
