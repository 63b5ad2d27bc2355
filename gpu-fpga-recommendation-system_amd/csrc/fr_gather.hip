// gather_pack kernels: the record-producing gather (fr_worker_gather_only, BLOCKED layout, sharded slices).
#include "fr_device.h"

// ---------------------------------------------------------------------------------------------------
// gather_pack: HBM-bound, no MFMA.
//
// One thread owns one 16-byte word position of the record (its FrWordDesc stays in registers) and
// walks ITEMS items: index load -> 16-byte row-word load -> 16-byte record store.  Consecutive lanes
// own consecutive record words, so record stores are fully coalesced (1 KiB per wave-instruction)
// and a dim-d row is read by d/4 adjacent lanes as one contiguous d*4-byte segment.
// All ITEMS index loads are issued before the row loads, and all row loads before the stores, so a
// wave keeps ITEMS x 1 KiB of gathers in flight.
// ---------------------------------------------------------------------------------------------------
// TP = what a record word is stored as: 0 fp32 (16 bytes, a bit copy), 1 bf16 (8 bytes, RNE), 2 e4m3 (4 bytes, x scale, saturated).
// The low-precision forms are the sharded mode's slice TRANSPORT formats: half / a quarter of the all-gather bytes, and exactly the
// values the bf16 / fp8 chain would have made of the fp32 slice on arrival.
// AUX = the cache-policy bits of a buffer store (gfx950: 1 sc0, 2 nt, 16 sc1; 16 = write-through): only the fp32 record stores of
// gather_pack_xcd_kernel use it, through a resource over `out` (the launcher keeps AUX = 0 when the records exceed 4 GiB)
template <int TP, int AUX = 0>
__device__ __forceinline__ void store_word(void *out, size_t word, const uint4 &v, float scale) {
    if constexpr (TP == 0 && AUX != 0) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(out, 0, 0xffffffffu, 0x00020000);
        u32x4_t q;
        q.x = v.x, q.y = v.y, q.z = v.z, q.w = v.w;
        __builtin_amdgcn_raw_buffer_store_b128(q, rs, (unsigned)(word * 16), 0, AUX);
    } else if constexpr (TP == 0) {
        reinterpret_cast<uint4 *>(out)[word] = v;
    } else if constexpr (TP == 1) {
        reinterpret_cast<uint2 *>(out)[word] = make_uint2(pack_bf16x2(__uint_as_float(v.x), __uint_as_float(v.y)), pack_bf16x2(__uint_as_float(v.z), __uint_as_float(v.w)));
    } else {
        reinterpret_cast<uint32_t *>(out)[word] = pack_fp8_word(v, scale);
    }
}

template <int ITEMS, int TP>
__global__ void __launch_bounds__(256) gather_pack_kernel(const FrWordDesc *__restrict__ words, int n_words,
                                                          const int32_t *__restrict__ idx, int idx_stride,
                                                          const float *__restrict__ dense, void *__restrict__ out,
                                                          int batch, int *__restrict__ err_flag, float scale) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    const uint4 d0 = reinterpret_cast<const uint4 *>(words)[2 * w];
    const uint4 d1 = reinterpret_cast<const uint4 *>(words)[2 * w + 1];
    const uint64_t src = ((uint64_t)d0.y << 32) | d0.x;
    const uint32_t stride = d0.z, idx_col = d0.w;
    const uint32_t rows = d1.x, dst_off = d1.y, dst_stride = d1.z, dst_blk = d1.w;
    const bool is_dense = (idx_col & FR_DESC_DENSE) != 0;
    const char *base = is_dense ? reinterpret_cast<const char *>(dense) + src : reinterpret_cast<const char *>(src);
    const int b0 = blockIdx.y * ITEMS;

    uint32_t id[ITEMS];
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        const int b = b0 + i;
        id[i] = 0;
        if (b < batch) id[i] = is_dense ? (uint32_t)b : (uint32_t)idx[(size_t)b * idx_stride + idx_col];
    }
    bool bad = false;
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        if (!is_dense && id[i] >= rows) {  // reference: silent out-of-bounds read (embedding_47_krnl.cpp:927-933)
            bad = true;
            id[i] = 0;
        }
    }
    uint4 v[ITEMS];
#pragma unroll
    for (int i = 0; i < ITEMS; i++) v[i] = *reinterpret_cast<const uint4 *>(base + (uint64_t)id[i] * stride);
    const size_t blk = (size_t)dst_blk * (size_t)batch + dst_off;
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        const int b = b0 + i;
        if (b < batch) store_word<TP>(out, blk + (size_t)b * dst_stride, v[i], scale);
    }
    if (bad) atomicOr_system(err_flag, 1);  // pinned host word; error path only
}

// XCD-partitioned form for wide records and large batches: workgroup b serves XCD group b % 8 (workgroups are dealt
// round-robin over the 8 XCDs; a speed assumption only), and each group owns a fixed contiguous run of the record words for
// ALL items (FrGatherGroups: cut on source-row boundaries, so no table row / bank row is fetched by two XCDs).  Every table is then
// touched from ONE XCD only, so the 8 x 4 MiB L2s cache 8 different table sets instead of 8 copies of the same hottest 4 MiB --
// rows served by L2 cost ~5 cycles/CU instead of ~12 from the fabric (profiles/archive/r01_experiments.md, ta_cost2).
template <int ITEMS, int TP, int AUX = 0>
__global__ void __launch_bounds__(256) gather_pack_xcd_kernel(const FrWordDesc *__restrict__ words, const FrGatherGroups groups,
                                                              const int32_t *__restrict__ idx, int idx_stride,
                                                              const float *__restrict__ dense, void *__restrict__ out,
                                                              int batch, int *__restrict__ err_flag, float scale, int n_chunks) {
    const int group = blockIdx.x & 7;
    const int w0 = groups.start[group];
    if ((int)threadIdx.x >= groups.start[group + 1] - w0) return;
    const int w = w0 + threadIdx.x;
    const uint4 d0 = reinterpret_cast<const uint4 *>(words)[2 * w];
    const uint4 d1 = reinterpret_cast<const uint4 *>(words)[2 * w + 1];
    const uint64_t src = ((uint64_t)d0.y << 32) | d0.x;
    const uint32_t stride = d0.z, idx_col = d0.w;
    const uint32_t rows = d1.x, dst_off = d1.y, dst_stride = d1.z, dst_blk = d1.w;
    const bool is_dense = (idx_col & FR_DESC_DENSE) != 0;
    const char *base = is_dense ? reinterpret_cast<const char *>(dense) + src : reinterpret_cast<const char *>(src);
    const size_t blk = (size_t)dst_blk * (size_t)batch + dst_off;
    bool bad = false;
    // a thread keeps its descriptor and walks chunks of ITEMS items: chunk = blockIdx.x / 8, stepping by the grid's chunk count
    for (int chunk = blockIdx.x >> 3; chunk < n_chunks; chunk += gridDim.x >> 3) {
        const int b0 = chunk * ITEMS;
        uint32_t id[ITEMS];
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            const int b = b0 + i;
            id[i] = 0;
            if (b < batch) id[i] = is_dense ? (uint32_t)b : (uint32_t)idx[(size_t)b * idx_stride + idx_col];
        }
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            if (!is_dense && id[i] >= rows) {
                bad = true;
                id[i] = 0;
            }
        }
        uint4 v[ITEMS];
#pragma unroll
        for (int i = 0; i < ITEMS; i++) v[i] = *reinterpret_cast<const uint4 *>(base + (uint64_t)id[i] * stride);
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            const int b = b0 + i;
            if (b < batch) store_word<TP, AUX>(out, blk + (size_t)b * dst_stride, v[i], scale);
        }
    }
    if (bad) atomicOr_system(err_flag, 1);
}

// Software-pipelined form of gather_pack_xcd_kernel: a workgroup keeps its descriptors and walks NSTEP chunks of ITEMS items
// (chunks j, j + cs, j + 2 cs, ... of its XCD group) with the index loads TWO chunks ahead and the row loads ONE chunk ahead of the
// record stores.  A chunk's dependent chain (descriptor -> index -> row -> store) is then paid once per workgroup of NSTEP chunks, and
// every wave mixes loads and stores from its first stored chunk on (the one-chunk-per-workgroup form starts with a read-only phase
// of every resident workgroup at once).  Straight-line code (NSTEP is a template parameter), so every s_waitcnt is a counted one;
// items past the batch cost no branch: their index loads and record stores go through buffer resources whose bounds drop them.
// Needs batch * idx_stride * 4 and the record bytes below 4000 MiB (the launcher falls back to gather_pack_xcd_kernel otherwise).
// LEAD: one index load per RUN of adjacent lanes that share an index column (a bank row of a bank-interleaved context is 7-16 record
// words, a table row 1-8): only the run's first lane loads (the others are masked off the instruction), everybody takes the value
// from that lane through ds_bpermute -- the texture path sees an eighth to a half of the index lanes.
template <int ITEMS, int NSTEP, int TP, int AUX, bool LEAD>
__global__ void __launch_bounds__(256) gather_pack_stream_kernel(const FrWordDesc *__restrict__ words, const FrGatherGroups groups,
                                                                 const int32_t *__restrict__ idx, int idx_stride,
                                                                 const float *__restrict__ dense, void *__restrict__ out,
                                                                 int batch, int *__restrict__ err_flag, float scale, unsigned out_bytes) {
    const int group = blockIdx.x & 7;
    const int w0 = groups.start[group];
    if ((int)threadIdx.x >= groups.start[group + 1] - w0) return;
    const int w = w0 + threadIdx.x;
    const uint4 d0 = reinterpret_cast<const uint4 *>(words)[2 * w];
    const uint4 d1 = reinterpret_cast<const uint4 *>(words)[2 * w + 1];
    const uint64_t src = ((uint64_t)d0.y << 32) | d0.x;
    const uint32_t stride = d0.z, idx_col = d0.w;
    const uint32_t rows = d1.x, dst_off = d1.y, dst_stride = d1.z, dst_blk = d1.w;
    const bool is_dense = (idx_col & FR_DESC_DENSE) != 0;
    const uint64_t base = (is_dense ? (uint64_t)reinterpret_cast<uintptr_t>(dense) : 0ull) + src;
    constexpr unsigned ESZ = TP == 0 ? 16u : TP == 1 ? 8u : 4u;   // bytes a record word is stored as
    const unsigned blk = (dst_blk * (unsigned)batch + dst_off) * ESZ;
    const unsigned ostride = dst_stride * ESZ;
    const __amdgpu_buffer_rsrc_t rs_idx = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t *>(idx), 0, (unsigned)batch * (unsigned)idx_stride * 4u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(out, 0, out_bytes, 0x00020000);
    const unsigned icol = is_dense ? 0u : idx_col * 4u;
    bool bad = false;
    const int cs = gridDim.x >> 3, c0 = blockIdx.x >> 3;
    uint32_t id[NSTEP][ITEMS];
    uint4 v[NSTEP][ITEMS];
    // run leaders (LEAD): lane l leads when it is the wave's first lane or its index column differs from lane l - 1's
    bool leader = true;
    int lead_byte = 0;   // 4 x the lane that holds this lane's index value
    if constexpr (LEAD) {
        const int lane = threadIdx.x & 63;
        const unsigned prev = (unsigned)__shfl_up((int)idx_col, 1);
        leader = lane == 0 || prev != idx_col;
        const unsigned long long lm = __ballot(leader);
        lead_byte = 4 * (63 - __builtin_clzll(lm & ((2ull << lane) - 1ull)));
    }
    auto load_idx = [&](int st) {
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            const unsigned b = (unsigned)(c0 + st * cs) * ITEMS + i;
            // an item past the batch reads past the resource: 0, no branch (dense words do not use the value)
            if constexpr (LEAD) {
                id[st][i] = 0;
                if (leader) id[st][i] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs_idx, b * (unsigned)idx_stride * 4u + icol, 0, 0);
            } else {
                id[st][i] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs_idx, b * (unsigned)idx_stride * 4u + icol, 0, 0);
            }
        }
    };
    auto load_rows = [&](int st) {
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            const unsigned b = (unsigned)(c0 + st * cs) * ITEMS + i;
            uint32_t r = id[st][i];
            if constexpr (LEAD) r = (uint32_t)__builtin_amdgcn_ds_bpermute(lead_byte, (int)r);   // the run leader's value
            const bool oob = !is_dense & (r >= rows);  // reference: silent out-of-bounds read (embedding_47_krnl.cpp:927-933)
            bad |= oob;
            r = oob ? 0u : r;
            r = is_dense ? (b < (unsigned)batch ? b : 0u) : r;
            typedef const u32x4_t __attribute__((address_space(1))) * gptr_t;   // a global_load (not a flat one: no lgkmcnt, no aperture check)
            const u32x4_t q = *(gptr_t)(base + (uint64_t)r * stride);
            v[st][i] = make_uint4(q.x, q.y, q.z, q.w);
        }
    };
    auto store_rows = [&](int st) {
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            const unsigned b = (unsigned)(c0 + st * cs) * ITEMS + i;
            const unsigned off = b < (unsigned)batch ? blk + b * ostride : out_bytes;   // past the batch: offset == num_records, dropped by the resource's bounds (no 32-bit wrap)
            const uint4 &q = v[st][i];
            if constexpr (TP == 0) {
                u32x4_t x;
                x.x = q.x, x.y = q.y, x.z = q.z, x.w = q.w;
                __builtin_amdgcn_raw_buffer_store_b128(x, rs_out, off, 0, AUX);
            } else if constexpr (TP == 1) {
                typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
                u32x2_t x;
                x.x = pack_bf16x2(__uint_as_float(q.x), __uint_as_float(q.y)), x.y = pack_bf16x2(__uint_as_float(q.z), __uint_as_float(q.w));
                __builtin_amdgcn_raw_buffer_store_b64(x, rs_out, off, 0, AUX);
            } else {
                __builtin_amdgcn_raw_buffer_store_b32(pack_fp8_word(q, scale), rs_out, off, 0, AUX);
            }
        }
    };
    load_idx(0);
    if constexpr (NSTEP > 1) load_idx(1);
    load_rows(0);
#pragma unroll
    for (int st = 0; st < NSTEP; st++) {
        if (st + 2 < NSTEP) load_idx(st + 2);
        if (st + 1 < NSTEP) load_rows(st + 1);
        store_rows(st);
    }
    if (bad) atomicOr_system(err_flag, 1);
}

// stream_form: 0 = the one-chunk-per-workgroup kernel (gather_pack_xcd_kernel; also what records or index buffers of >= 4000 MiB take),
// n > 0 = gather_pack_stream_kernel with n chunks per workgroup (the product launches 2)
template <int ITEMS, int TP>
static int gather_launch_xcd(const FrWordDesc *words, const FrGatherGroups &groups, const int32_t *idx, int idx_stride, const float *dense, void *out, int batch,
                             int *err_flag, float scale, hipStream_t s, int n_words, int out_words, int stream_form) {
    const size_t n_rec_bytes = (size_t)out_words * 16;
    const int bx = ((groups.max_words + 63) / 64) * 64;
    const int n_chunks = (batch + ITEMS - 1) / ITEMS;
    const int per_wg_knob = FR_KNOB("GATHER_LOOP", 1);  // experiment knob: chunks a workgroup of the one-chunk form walks
    const int per_wg = per_wg_knob > 0 ? per_wg_knob : 1;
    dim3 grid(8 * ((n_chunks + per_wg - 1) / per_wg));
    (void)n_rec_bytes;
    if constexpr (ITEMS == 4 || ITEMS == 2) {
        // default: the software-pipelined form, 2 chunks per workgroup, write-through record stores while the records fit the Infinity
        // Cache with room to spare (profiles/archive/r02_gather_stream_sweep.txt: Model-C batch 4096 per-bank 25.2 -> 22.0 us; beyond ~200 MB of
        // records write-back stores are as fast or 1-2 % faster).  Experiments build only: FR_GATHER_STREAM = chunks per workgroup,
        // FR_GATHER_STORE = 0 write-back / 16 write-through, both read per launch.
        const int nstep = FR_KNOB("GATHER_STREAM", stream_form);
        const size_t esz = TP == 0 ? 16 : TP == 1 ? 8 : 4;
        const size_t out_bytes = (size_t)batch * (size_t)out_words * esz, idx_bytes = (size_t)batch * (size_t)idx_stride * 4;
        if (nstep > 0 && out_bytes < ((size_t)4000 << 20) && idx_bytes < ((size_t)4000 << 20)) {  // 32-bit resource offsets, with room for the chunk past the batch
            const int st_knob = FR_KNOB("GATHER_STORE", -1);
            const bool wt = st_knob >= 0 ? st_knob == 16 : out_bytes <= ((size_t)200 << 20);
            const bool lead = FR_KNOB("GATHER_LEAD", 0) != 0;   // experiments build: one index load per run of lanes sharing an index column (slower: 22.3 -> 22.9 us)
#ifdef FR_EXPERIMENTS   /* the LEAD instantiations exist in the experiments build only (measured slower: profiles/archive/r03_experiments.md) */
#define FR_G_LEAD(NS)                                                                                                                       \
            if (wt) gather_pack_stream_kernel<ITEMS, NS, TP, 16, true><<<g2, dim3(bx), 0, s>>>(words, groups, idx, idx_stride, dense, out, batch, err_flag, scale, (unsigned)out_bytes); \
            else gather_pack_stream_kernel<ITEMS, NS, TP, 0, true><<<g2, dim3(bx), 0, s>>>(words, groups, idx, idx_stride, dense, out, batch, err_flag, scale, (unsigned)out_bytes);
#else
#define FR_G_LEAD(NS)
#endif
#define FR_G_STREAM(NS)                                                                                                                     \
    case NS: {                                                                                                                              \
        dim3 g2(8 * ((n_chunks + NS - 1) / NS));                                                                                            \
        if (lead) {                                                                                                                         \
            FR_G_LEAD(NS)                                                                                                                   \
        } else {                                                                                                                            \
            if (wt) gather_pack_stream_kernel<ITEMS, NS, TP, 16, false><<<g2, dim3(bx), 0, s>>>(words, groups, idx, idx_stride, dense, out, batch, err_flag, scale, (unsigned)out_bytes); \
            else gather_pack_stream_kernel<ITEMS, NS, TP, 0, false><<<g2, dim3(bx), 0, s>>>(words, groups, idx, idx_stride, dense, out, batch, err_flag, scale, (unsigned)out_bytes);    \
        }                                                                                                                                   \
        KCHECK();                                                                                                                           \
        fr_note_kernel("gather_pack_stream_kernel<%d, %d, %d, %d, %s>", ITEMS, NS, TP, wt ? 16 : 0, lead ? "true" : "false");               \
        return FR_OK;                                                                                                                       \
    }
            switch (nstep) {
                FR_G_STREAM(2)
#ifdef FR_EXPERIMENTS
                FR_G_STREAM(1)
                FR_G_STREAM(4)
                FR_G_STREAM(8)
#endif
                default: break;
            }
#undef FR_G_STREAM
#undef FR_G_LEAD
        }
    }
#ifdef FR_EXPERIMENTS
    if constexpr (ITEMS == 4 && TP == 0) {
        const int st = FR_KNOB("GATHER_STORE", 0);  // experiment knob: cache policy of the record stores (0 plain, 16 sc1, 2 nt) of the one-chunk form
        if (st && (size_t)batch * (size_t)n_rec_bytes < ((size_t)1 << 32)) {
#define FR_G_ST(A) case A: gather_pack_xcd_kernel<4, 0, A><<<grid, dim3(bx), 0, s>>>(words, groups, idx, idx_stride, dense, out, batch, err_flag, scale, n_chunks); KCHECK(); return FR_OK;
            switch (st) {
                FR_G_ST(16)
                FR_G_ST(2)
                default: break;
            }
#undef FR_G_ST
        }
    }
#endif
    gather_pack_xcd_kernel<ITEMS, TP><<<grid, dim3(bx), 0, s>>>(words, groups, idx, idx_stride, dense, out, batch, err_flag, scale, n_chunks);
    KCHECK();
    fr_note_kernel("gather_pack_xcd_kernel<%d, %d, 0>", ITEMS, TP);   // the symbol's three arguments (AUX = 0), as rocprofv3 prints it
    return FR_OK;
}

template <int TP>
static int gather_launch(const FrWordDesc *words, int n_words, const FrGatherGroups &planned, const int32_t *idx, int idx_stride, const float *dense, void *out, int batch, int *err_flag,
                         float scale, hipStream_t s, int out_words, int stream_form) {
    // experiments build only (tools/experiments/gather_sweep.py), read per launch: FR_GATHER_XCD = 0 / 1 forces the kernel form,
    // FR_GATHER_ITEMS = items per thread of the XCD-partitioned form, FR_GATHER_UNIFORM_GROUPS = n_words / 8 words per XCD group
    const int force = FR_KNOB("GATHER_XCD", -1);
    const bool xcd = force >= 0 ? force != 0 : (n_words >= 512 && batch >= 1024);
    if (xcd) {
        FrGatherGroups groups = planned;
        if (groups.max_words <= 0 || FR_KNOB("GATHER_UNIFORM_GROUPS", 0)) {  // no plan (or the experiment knob): n_words / 8 each
            const int wpg = (n_words + 7) / 8;
            for (int g = 0; g <= 8; g++) groups.start[g] = g * wpg < n_words ? g * wpg : n_words;
            groups.max_words = wpg;
        }
        if (groups.max_words <= 256) {
            switch (FR_KNOB("GATHER_ITEMS", 4)) {  // 4 items per thread: fastest in the r02 sweep (profiles/archive/r02_gather_sweep.txt)
#ifdef FR_EXPERIMENTS
                case 1: return gather_launch_xcd<1, TP>(words, groups, idx, idx_stride, dense, out, batch, err_flag, scale, s, n_words, out_words, stream_form);
                case 2: return gather_launch_xcd<2, TP>(words, groups, idx, idx_stride, dense, out, batch, err_flag, scale, s, n_words, out_words, stream_form);
                case 8: return gather_launch_xcd<8, TP>(words, groups, idx, idx_stride, dense, out, batch, err_flag, scale, s, n_words, out_words, stream_form);
                case 16: return gather_launch_xcd<16, TP>(words, groups, idx, idx_stride, dense, out, batch, err_flag, scale, s, n_words, out_words, stream_form);
#endif
                default: return gather_launch_xcd<4, TP>(words, groups, idx, idx_stride, dense, out, batch, err_flag, scale, s, n_words, out_words, stream_form);
            }
        }
    }
    // block width: whole waves, at most 256 lanes
    int bx = n_words >= 256 ? 256 : ((n_words + 63) / 64) * 64;
    dim3 block(bx);
    if (batch >= 2048) {
        constexpr int ITEMS = 8;
        dim3 grid((n_words + bx - 1) / bx, (batch + ITEMS - 1) / ITEMS);
        gather_pack_kernel<ITEMS, TP><<<grid, block, 0, s>>>(words, n_words, idx, idx_stride, dense, out, batch, err_flag, scale);
        fr_note_kernel("gather_pack_kernel<%d, %d>", ITEMS, TP);
    } else {
        constexpr int ITEMS = 4;
        dim3 grid((n_words + bx - 1) / bx, (batch + ITEMS - 1) / ITEMS);
        gather_pack_kernel<ITEMS, TP><<<grid, block, 0, s>>>(words, n_words, idx, idx_stride, dense, out, batch, err_flag, scale);
        fr_note_kernel("gather_pack_kernel<%d, %d>", ITEMS, TP);
    }
    KCHECK();
    return FR_OK;
}

// transport: FR_FC_FP32 (fp32 records, the reference's wire format), FR_FC_BF16 or FR_FC_FP8 (slice transport of the sharded mode)
int frk_gather(const FrWordDesc *words, int n_words, const FrGatherGroups &groups, const int32_t *idx, int idx_stride, const float *dense, void *out, int batch, int *err_flag,
               int transport, int e_x, hipStream_t s, int out_words, bool one_chunk) {
    // out_words = 16-byte words per item of the DESTINATION (the record, or a shard's padded slice: >= n_words): the bounds of the
    // software-pipelined kernel's store resource.  one_chunk: the FR_GATHER_WORD_MAJOR_ONE_CHUNK variant (gather_pack_xcd_kernel).
    if (n_words <= 0 || batch <= 0) return FR_OK;
    if (out_words < n_words) out_words = n_words;
    const int stream_form = one_chunk ? 0 : 2;
    if (transport == FR_FC_BF16) return gather_launch<1>(words, n_words, groups, idx, idx_stride, dense, out, batch, err_flag, 1.0f, s, out_words, stream_form);
    if (transport == FR_FC_FP8) return gather_launch<2>(words, n_words, groups, idx, idx_stride, dense, out, batch, err_flag, ldexpf(1.0f, e_x), s, out_words, stream_form);
    return gather_launch<0>(words, n_words, groups, idx, idx_stride, dense, out, batch, err_flag, 1.0f, s, out_words, stream_form);
}

// ---------------------------------------------------------------------------------------------------
// gather_pooled_kernel: the multi-hot (pooled) form of gather_pack -- fr_worker_gather_pooled.
//
// Word-major like the kernels above: a thread owns one 16-byte record word (FrWordDesc + FrPoolDesc in registers), consecutive lanes own
// consecutive words, so record stores stay coalesced.  The word's bag is `hots` consecutive int32 slots of the item's pooled index row
// (idx[b][first .. first + hots)); the record word is the fp32 sum of the bag's row words under the contract of fleetrec_serving.h: the
// FIRST non-empty slot's word is taken as a bit copy, every further non-empty slot's word is added to it, one v_add_f32 per lane, in
// ascending slot order (the accumulator is a select between "take" and "add": no FMA, no tree); slot -1 is empty, an all-empty bag
// gives +0.0f.  A DENSE word is a bag of one: the item's own dense row.
// Per chunk of ITEMS items the bag is walked in windows of WIN slots: the window's index slots are loaded first (WIDE: as 16-byte
// loads -- every bag starts and ends on a multiple of 4 slots and the row length is one), then all ITEMS x WIN row words are issued back
// to back, then they are folded in slot order: a wave keeps ITEMS x WIN x 1 KiB of gathers in flight.  Lanes of a wave sit on different
// columns and may have different `hots`: slots past a lane's bag are masked off the loads (exec mask), a lane whose bag is exhausted
// idles through the wave's remaining windows.  Items past the batch cost no branch: their index loads and record stores go through
// buffer resources whose bounds drop them (both buffers below 4000 MiB: the launcher checks).  XCD grouping as in gather_pack_xcd_kernel
// (workgroup b serves group b % n_groups and chunk b / n_groups; n_groups = 8, or 1 for records too narrow for a plan); blockIdx.y walks
// a group wider than one workgroup.
// ---------------------------------------------------------------------------------------------------
// The fold has three forms (fleetrec_serving.h).  SUM: as above.  MEAN (bit FR_POOL_DESC_MEAN of the word's `hots`): the SUM fold, then ONE IEEE fp32
// division by the bag's count of non-empty slots, under a per-lane predicate (count >= 2: a bag of one stays a bit copy, an empty one +0.0f;
// DENSE words never carry the bit).  WEIGHTED (weights != NULL: float [batch][pool_cols], a slot's weight sits where the slot sits): the
// window's weights are loaded exactly as its slots are (the same offsets through a resource of their own, 16-byte loads in the WIDE form,
// masked past the lane's bag), every row word is multiplied by its weight -- one v_mul_f32 per lane, rounded on its own: contraction is off
// in this body, the product and the add that follows are never an FMA -- and the FIRST non-empty slot's product starts the accumulator
// (not a bit copy).  An empty slot's weight is dropped by the same select that drops its word; DENSE words are copied unweighted.
// `weights` and `any_mean` (a column of the context is MEAN) are uniform over the launch: the kernel branches on them once, around the whole
// body, so the unweighted SUM window loop holds no trace of weights, counts or quotients.  A kernel's register count is that of its larger arm, and it decides the occupancy of both: the weighted arm
// therefore runs the chunk in two passes of half as many row words in flight (gather_pooled_kernel below) and takes its weights in units of
// at most 4 slots, one unit ahead of the fold, so that it stays inside the unweighted arm's registers (no spill, no scratch in either).
// The OFFSETS form (CSR = true; offsets != NULL at the launch): the bags are not a padded rectangle but indices[offsets[b * n_icols + c] ..
// offsets[b * n_icols + c + 1]), weights parallel to indices, nnz entries in all; the word's FrPoolDesc then holds its index COLUMN in `first` and the
// column's CAP in `hots`.  Per item the thread loads its bag's two offsets through a resource bounded at (batch * n_icols + 1) * 4 bytes (an item
// past the batch is sent past the bounds and reads 0, 0: an empty bag), checks them (start < 0, end < start, end > nnz, longer than the cap: the
// error flag, and the bag is taken as empty, so a malformed bag issues no slot load at all), and walks windows up to the LONGEST bag among its
// items; the slot and weight loads go at (start + slot) * 4 through resources bounded at nnz * 4 bytes, masked by the bag's own length.  Rows,
// the clamp of a bad row to 0 and the fold are the code of the padded form, so the bits are those of the same bags padded with -1.  Only
// 4-byte alignment is given: the form has no 16-byte index loads (the WIDE instantiations compile it out), and it always runs in the half
// passes of the MEAN / weighted arms, with its offsets and lengths in the registers the other half's row words would have taken.
template <int ITEMS, int WIN, bool WIDE, bool WEIGHTED, bool COUNT, bool CSR = false, int OPND = 0>
__device__ __forceinline__ void gather_pooled_body(const FrWordDesc *__restrict__ words, const FrPoolDesc *__restrict__ pool, int w, unsigned b0,
                                                   const int32_t *__restrict__ idx, const float *__restrict__ weights, int pool_cols,
                                                   const float *__restrict__ dense, void *__restrict__ out, int batch, int *__restrict__ err_flag,
                                                   unsigned out_bytes, const FrPoolDest &dst, const int32_t *__restrict__ offsets = nullptr, int n_icols = 0, unsigned nnz = 0u) {
#pragma clang fp contract(off)
    static_assert(!WIDE || WIN % 4 == 0, "16-byte index loads need whole groups of 4 slots");
    static_assert(!(CSR && WIDE), "the offsets form has no 16-byte index loads");
    const uint4 d0 = reinterpret_cast<const uint4 *>(words)[2 * w];
    const uint4 d1 = reinterpret_cast<const uint4 *>(words)[2 * w + 1];
    const uint2 pd = reinterpret_cast<const uint2 *>(pool)[w];
    const uint64_t src = ((uint64_t)d0.y << 32) | d0.x;
    const uint32_t stride = d0.z;
    const bool is_dense = (d0.w & FR_DESC_DENSE) != 0;
    const uint32_t rows = d1.x, dst_off = d1.y, dst_stride = d1.z, dst_blk = d1.w;
    const uint32_t first = pd.x, hots = pd.y & ~FR_POOL_DESC_MEAN;
    const bool mean = COUNT && (pd.y & FR_POOL_DESC_MEAN) != 0;
    const uint64_t base = (is_dense ? (uint64_t)reinterpret_cast<uintptr_t>(dense) : 0ull) + src;
    // where the word goes: the item's fp32 record, or (OPND) the chain's feature-major stage-1 operand -- element (w >> sh, b) of 16 bytes, the
    // word's 16 >> sh bytes at (w & mask) inside it; both are `blk + b * ostride`.  The operand's zeros (pad k-rows, chunks of pad items) are stored by
    // gather_pooled_operand_zeros before the fold, so that the fold keeps two scalars more than the record arm (dst.ldm, dst.code)
    constexpr unsigned sh = OPND ? (unsigned)OPND - 1u : 0u;   // OPND = the operand's form (FrPoolDest), fixed per arm
    // FR_PD_ROWS (forms 2 / 3, uniform over the launch): the item-major low-precision slice of a shard -- item b's row of dst.ldm words of 16 >> sh bytes,
    // the word at its dst_off inside the row; only the batch's items are stored
    // Decided in vector registers by a mask, not by a scalar branch or select: the folds leave no scalar register for the choice.  With a k-row
    // stride of ONE item the feature-major formula below is dst_off * (16 >> sh), the word's place in the row.
    unsigned rmask = 0u;   // all ones in the item-major form
    if constexpr (OPND >= 2) {
        rmask = (unsigned)dst.code;
        asm volatile("" : "+v"(rmask));
        rmask = 0u - ((rmask >> 11) & 1u);
        static_assert(FR_PD_ROWS == 1u << 11, "the shift above");
    }
    unsigned ldmv = dst.ldm;
    if constexpr (OPND >= 2) asm volatile("" : "+v"(ldmv));
    const unsigned kstride = OPND >= 2 ? (ldmv & ~rmask) | (1u & rmask) : dst.ldm;
    const unsigned blk = OPND ? ((dst_off >> sh) * kstride) * 16u + (dst_off & ((1u << sh) - 1u)) * (16u >> sh) : (dst_blk * (unsigned)batch + dst_off) * 16u;
    const unsigned ostride = OPND >= 2 ? (16u & ~rmask) | ((ldmv << (4u - sh)) & rmask) : OPND ? 16u : dst_stride * 16u;
    unsigned lim = OPND >= 2 ? (ldmv & ~rmask) | ((unsigned)batch & rmask) : OPND ? dst.ldm : (unsigned)batch;   // items the stores cover: the operand's pad items [batch, ldm) are stored as zeros
    float scale = OPND == 3 ? __builtin_ldexpf(1.0f, dst.code >> FR_PD_EX_SHIFT) : 1.0f;   // 2^e_x, exact
    // OPND: both in vector registers from here on (the half passes leave some; the fold's masks leave no scalar one)
    if constexpr (OPND != 0) asm volatile("" : "+v"(lim));
    if constexpr (OPND == 3) asm volatile("" : "+v"(scale));
    const unsigned irow = (unsigned)pool_cols * 4u;
    const unsigned idx_bytes = CSR ? nnz * 4u : (unsigned)batch * irow;   // CSR: the flat entries (the launcher keeps nnz * 4 below 4000 MiB)
    const __amdgpu_buffer_rsrc_t rs_idx = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t *>(idx), 0, idx_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(out, 0, out_bytes, 0x00020000);
    // the weights' resource has the index rows' shape and bounds (WEIGHTED only; the unweighted body never touches it)
    const __amdgpu_buffer_rsrc_t rs_wt = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(weights), 0, WEIGHTED ? idx_bytes : 0u, 0x00020000);
    typedef const u32x4_t __attribute__((address_space(1))) * gptr_t;   // a global_load (not a flat one)
    // one folded word of item b out, in the destination's type: a bit copy, two pack_bf16x2 or pack_fp8_word (the rounding of store_word)
    auto store_out = [&](unsigned b, unsigned o, uint32_t ax, uint32_t ay, uint32_t az, uint32_t aw) __attribute__((always_inline)) {
        const unsigned off = b < lim ? o + b * ostride : out_bytes;   // past the batch (the operand: past ldm): dropped by the resource's bounds
        if constexpr (sh == 0u) {
            u32x4_t x;
            x.x = ax, x.y = ay, x.z = az, x.w = aw;
            __builtin_amdgcn_raw_buffer_store_b128(x, rs_out, off, 0, 0);
        } else if constexpr (sh == 1u) {
            typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
            u32x2_t x;
            x.x = pack_bf16x2(__uint_as_float(ax), __uint_as_float(ay)), x.y = pack_bf16x2(__uint_as_float(az), __uint_as_float(aw));
            __builtin_amdgcn_raw_buffer_store_b64(x, rs_out, off, 0, 0);
        } else {
            __builtin_amdgcn_raw_buffer_store_b32(pack_fp8x4(__uint_as_float(ax), __uint_as_float(ay), __uint_as_float(az), __uint_as_float(aw), scale), rs_out, off, 0, 0);
        }
    };
    bool bad = false;
    uint32_t badv = 0u;   // WEIGHTED: `bad` as a vector register
    uint4 acc[ITEMS];
    bool have[ITEMS];
    uint32_t cnt[(ITEMS + 3) / 4];   // COUNT: the MEAN divisors -- non-empty slots folded so far, one byte per item (a bag has at most 64 slots)
#pragma unroll
    for (int i = 0; i < ITEMS; i++) acc[i] = make_uint4(0u, 0u, 0u, 0u), have[i] = false;
#pragma unroll
    for (int i = 0; i < (ITEMS + 3) / 4; i++) cnt[i] = 0u;
    // CSR: where each item's bag starts (in entries) and how long it is; `bound` = the longest of them (the padded form: the word's hots)
    uint32_t st[CSR ? ITEMS : 1], ln[CSR ? ITEMS : 1];
    uint32_t bound = hots;
    if constexpr (CSR) {
        const unsigned off_bytes = ((unsigned)batch * (unsigned)n_icols + 1u) * 4u;
        const __amdgpu_buffer_rsrc_t rs_off = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t *>(offsets), 0, off_bytes, 0x00020000);
        bound = is_dense ? 1u : 0u;   // a DENSE word is a bag of one and has no offsets
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            const unsigned b = b0 + i;
            st[i] = 0u, ln[i] = 0u;
            if (!is_dense) {
                // an item past the batch goes to the resource's end: both loads are dropped by its bounds and give 0
                const unsigned ooff = b < (unsigned)batch ? (b * (unsigned)n_icols + first) * 4u : off_bytes;
                const int32_t s0 = (int32_t)__builtin_amdgcn_raw_buffer_load_b32(rs_off, ooff, 0, 0);
                const int32_t s1 = (int32_t)__builtin_amdgcn_raw_buffer_load_b32(rs_off, ooff + 4u, 0, 0);
                // 0 <= s0 <= s1 <= nnz and s1 - s0 <= cap, in unsigned compares (a negative value is a huge one)
                const bool mal = ((uint32_t)s0 > (uint32_t)s1) | ((uint32_t)s1 > nnz) | ((uint32_t)s1 - (uint32_t)s0 > hots);
                badv |= mal ? 1u : 0u;
                st[i] = (uint32_t)s0;
                ln[i] = mal ? 0u : (uint32_t)s1 - (uint32_t)s0;
                bound = ln[i] > bound ? ln[i] : bound;
            }
        }
    }
    for (uint32_t j0 = 0; j0 < bound; j0 += WIN) {
        // the window's slots: -1 (empty) past the bag; an item past the batch reads past the resource: 0 (row 0; its store is dropped)
        int32_t sl[ITEMS][WIN];
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            const unsigned ioff = CSR ? (st[i] + j0) * 4u : (b0 + i) * irow + (first + j0) * 4u;
            const uint32_t fill = CSR ? ln[i] : hots;   // slots of this item's bag
            if constexpr (WIDE) {
#pragma unroll
                for (int q = 0; q < WIN / 4; q++) {
                    u32x4_t v4 = {~0u, ~0u, ~0u, ~0u};
                    if (!is_dense && j0 + 4 * q < hots) v4 = __builtin_amdgcn_raw_buffer_load_b128(rs_idx, ioff + 16u * q, 0, 0);
                    sl[i][4 * q] = (int32_t)v4.x, sl[i][4 * q + 1] = (int32_t)v4.y, sl[i][4 * q + 2] = (int32_t)v4.z, sl[i][4 * q + 3] = (int32_t)v4.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < WIN; j++) {
                    sl[i][j] = -1;
                    if (!is_dense && j0 + j < fill) sl[i][j] = (int32_t)__builtin_amdgcn_raw_buffer_load_b32(rs_idx, ioff + 4u * j, 0, 0);
                }
            }
        }
        // all row words of the window, back to back
        uint4 v[ITEMS][WIN];
        bool on[ITEMS][WIN];
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            const unsigned b = b0 + i;
#pragma unroll
            for (int j = 0; j < WIN; j++) {
                uint32_t r = (uint32_t)sl[i][j];
                on[i][j] = is_dense ? (j0 + j == 0) : (r != 0xFFFFFFFFu);
                const bool oob = !is_dense & on[i][j] & (r >= rows);  // reference: silent out-of-bounds read (embedding_47_krnl.cpp:927-933)
                if constexpr (WEIGHTED) {   // the flag goes to a vector register at once: kept as masks until the window's end, the 16 comparisons
                    badv |= oob ? 1u : 0u;  // cost 32 scalar registers that the weighted fold (a fourth resource) does not have
                    asm volatile("" : "+v"(badv));
                } else {
                    bad |= oob;
                }
                r = oob ? 0u : r;
                r = is_dense ? (b < (unsigned)batch ? b : 0u) : r;
                v[i][j] = make_uint4(0u, 0u, 0u, 0u);
                if (on[i][j]) {
                    const u32x4_t q = *(gptr_t)(base + (uint64_t)r * stride);
                    v[i][j] = make_uint4(q.x, q.y, q.z, q.w);
                }
            }
        }
        // WEIGHTED: the window's weights, loaded as its slots were -- the same offsets and masks through a resource of their own, 16-byte loads
        // in the WIDE form, an item past the batch reads past the resource -- but in units of G slots, each issued one unit ahead of its fold
        // (the first behind the row loads): the weights then sit in registers the folded row words have left, not next to a full window
        constexpr int G = WIN < 4 ? WIN : 4, UPI = WIN / G;   // slots per unit, units per item
        uint32_t wt[WEIGHTED ? ITEMS : 1][WEIGHTED ? WIN : 1];
        // the slots left in the lane's bag, through an empty asm: the masks are then compared afresh at each load instead of being kept
        // from the index loads across the row-load phase (scalar registers the weighted fold does not have)
        uint32_t left = is_dense ? 0u : hots - j0;
        if constexpr (WEIGHTED) asm volatile("" : "+v"(left));
        auto load_weights = [&](int u) {
            const int i = u / UPI, g = u % UPI;
            const unsigned woff = (CSR ? (st[i] + j0) * 4u : (b0 + i) * irow + (first + j0) * 4u) + 4u * G * g;
            if constexpr (CSR) left = ln[i] > j0 ? ln[i] - j0 : 0u;   // this item's own bag (0 for a DENSE word)
            if constexpr (WIDE) {
                u32x4_t w4 = {0u, 0u, 0u, 0u};
                if (4u * g < left) w4 = __builtin_amdgcn_raw_buffer_load_b128(rs_wt, woff, 0, 0);
                wt[i][4 * g] = w4.x, wt[i][4 * g + 1] = w4.y, wt[i][4 * g + 2] = w4.z, wt[i][4 * g + 3] = w4.w;
            } else {
#pragma unroll
                for (int k = 0; k < G; k++) {
                    wt[i][G * g + k] = 0u;
                    if ((unsigned)(G * g + k) < left) wt[i][G * g + k] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs_wt, woff + 4u * k, 0, 0);
                }
            }
        };
        if constexpr (WEIGHTED) load_weights(0);
        // fold in slot order: take the first non-empty word as it is (WEIGHTED: its product), add every further one
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
#pragma unroll
            for (int j = 0; j < WIN; j++) {
                if constexpr (WEIGHTED)
                    if (j % G == 0 && i * UPI + j / G + 1 < ITEMS * UPI) load_weights(i * UPI + j / G + 1);
                const uint4 a = acc[i];
                uint4 x = v[i][j];
                const bool o = on[i][j];
                if constexpr (WEIGHTED) {   // w * x, rounded to fp32 before the add sees it; a DENSE word stays the bit copy it is
                    const float wj = __uint_as_float(wt[i][j]);
                    const uint32_t px = __float_as_uint(wj * __uint_as_float(x.x)), py = __float_as_uint(wj * __uint_as_float(x.y));
                    const uint32_t pz = __float_as_uint(wj * __uint_as_float(x.z)), pw = __float_as_uint(wj * __uint_as_float(x.w));
                    x.x = is_dense ? x.x : px, x.y = is_dense ? x.y : py, x.z = is_dense ? x.z : pz, x.w = is_dense ? x.w : pw;
                }
                uint4 sum;
                sum.x = __float_as_uint(__uint_as_float(a.x) + __uint_as_float(x.x));
                sum.y = __float_as_uint(__uint_as_float(a.y) + __uint_as_float(x.y));
                sum.z = __float_as_uint(__uint_as_float(a.z) + __uint_as_float(x.z));
                sum.w = __float_as_uint(__uint_as_float(a.w) + __uint_as_float(x.w));
                const uint4 nxt = have[i] ? sum : x;
                acc[i] = o ? nxt : a;
                have[i] |= o;
                if constexpr (COUNT) cnt[i / 4] += o ? 1u << (8 * (i % 4)) : 0u;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        const unsigned b = b0 + i;
        if constexpr (COUNT) {   // (never with weights: they are legal on all-SUM contexts only, the C-ABI refuses the mix)
            const uint32_t n_i = (cnt[i / 4] >> (8 * (i % 4))) & 0xFFu;
            if (mean && n_i > 1u) {   // MEAN: one correctly rounded division per lane; the count converts exactly (<= 64)
                const float n = (float)n_i;
                acc[i].x = __float_as_uint(__uint_as_float(acc[i].x) / n);
                acc[i].y = __float_as_uint(__uint_as_float(acc[i].y) / n);
                acc[i].z = __float_as_uint(__uint_as_float(acc[i].z) / n);
                acc[i].w = __float_as_uint(__uint_as_float(acc[i].w) / n);
            }
        }
        const bool pad = OPND && b >= (unsigned)batch;   // a pad item of the operand (its lookups read row 0): zeros
        store_out(b, blk, pad ? 0u : acc[i].x, pad ? 0u : acc[i].y, pad ? 0u : acc[i].z, pad ? 0u : acc[i].w);
    }
    if (bad || badv) atomicOr_system(err_flag, 1);  // pinned host word; error path only
}

// The zeros of the operand form (FrPoolDest), stored by the word threads before their fold: the pad words behind the record in the operand's
// k-rows (the last FR_PD_PAD words of FrPoolDest::code: e4m3 rows are 64 k long), dealt over the n_words word threads, for every item of the chunk below
// ldm -- and, for a chunk of pad items only (b0 >= batch, uniform over the workgroup), the thread's own word too: -> true, the thread is done.
template <int ITEMS>
__device__ __forceinline__ bool gather_pooled_operand_zeros(const FrWordDesc *__restrict__ words, int w, unsigned n_words, unsigned b0, void *__restrict__ out, int batch,
                                                            unsigned out_bytes, const FrPoolDest &dst) {
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(out, 0, out_bytes, 0x00020000);
    const unsigned sh = ((unsigned)dst.code & FR_PD_FORM_MASK) - 1u, esz = 16u >> sh;
    auto zeros = [&](unsigned word) __attribute__((always_inline)) {
        const unsigned o = ((word >> sh) * dst.ldm) * 16u + (word & ((1u << sh) - 1u)) * esz;
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            const unsigned b = b0 + i, off = b < dst.ldm ? o + b * 16u : out_bytes;   // past ldm: dropped by the resource's bounds
            if (sh == 0u) {
                const u32x4_t z = {0u, 0u, 0u, 0u};
                __builtin_amdgcn_raw_buffer_store_b128(z, rs_out, off, 0, 0);
            } else if (sh == 1u) {
                typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
                const u32x2_t z = {0u, 0u};
                __builtin_amdgcn_raw_buffer_store_b64(z, rs_out, off, 0, 0);
            } else {
                __builtin_amdgcn_raw_buffer_store_b32(0u, rs_out, off, 0, 0);
            }
        }
    };
    const unsigned pad_hi = (out_bytes / (dst.ldm * 16u)) << sh, n_pad = ((unsigned)dst.code >> FR_PD_PAD_SHIFT) & FR_PD_PAD_MASK;
    for (unsigned p = pad_hi - n_pad + (unsigned)w; p < pad_hi; p += n_words) zeros(p);
    if (b0 < (unsigned)batch) return false;
    zeros(words[w].dst_off);
    return true;
}

// The folds of gather_pooled_kernel once more, for the operand form F (FrPoolDest: 1 fp32, 2 bf16, 3 e4m3).  All of them run in the half passes of
// the MEAN / weighted / offsets arms -- the SUM fold too -- so that the operand's scalars fit the registers of the record arms.
// The half passes of the MEAN / weighted / offsets arms and of every operand arm: half the items, or half the window for one item
template <int ITEMS, int WIN>
struct PooledHalf {
    static constexpr int HI = ITEMS >= 2 ? ITEMS / 2 : 1, HW = ITEMS >= 2 ? WIN : (WIN >= 8 ? WIN / 2 : WIN);
    static constexpr unsigned NH = ITEMS >= 2 ? 2u : 1u;
};

template <int ITEMS, int WIN, bool WIDE, int F>
__device__ __forceinline__ void gather_pooled_operand_arms(const FrWordDesc *__restrict__ words, const FrPoolDesc *__restrict__ pool, int wd, unsigned b0,
                                                           const int32_t *__restrict__ idx, const float *__restrict__ weights, int pool_cols,
                                                           const float *__restrict__ dense, void *__restrict__ out, int batch, int *__restrict__ err_flag,
                                                           unsigned out_bytes, const int32_t *__restrict__ offsets, int n_icols, unsigned nnz, const FrPoolDest &dst) {
    constexpr int HI = PooledHalf<ITEMS, WIN>::HI, HW = PooledHalf<ITEMS, WIN>::HW;
    constexpr unsigned NH = PooledHalf<ITEMS, WIN>::NH;
    // which fold: decided by the launcher (FrPoolDest::code), one scalar to branch on instead of the record arms' three
    const unsigned fold = ((unsigned)dst.code >> FR_PD_FOLD_SHIFT) & FR_PD_FOLD_MASK;
    if (fold == FR_PD_FOLD_CSR_WEIGHTED) {
        if constexpr (!WIDE)
            for (unsigned h = 0; h < NH; h++)
                gather_pooled_body<HI, HW, false, true, false, true, F>(words, pool, wd, b0 + h * HI, idx, weights, pool_cols, dense, out, batch, err_flag, out_bytes, dst, offsets, n_icols, nnz);
    } else if (fold == FR_PD_FOLD_CSR) {
        if constexpr (!WIDE)
            for (unsigned h = 0; h < NH; h++)
                gather_pooled_body<HI, HW, false, false, true, true, F>(words, pool, wd, b0 + h * HI, idx, nullptr, pool_cols, dense, out, batch, err_flag, out_bytes, dst, offsets, n_icols, nnz);
    } else if (fold == FR_PD_FOLD_WEIGHTED) {
        for (unsigned h = 0; h < NH; h++)
            gather_pooled_body<HI, HW, WIDE, true, false, false, F>(words, pool, wd, b0 + h * HI, idx, weights, pool_cols, dense, out, batch, err_flag, out_bytes, dst);
    } else if (fold == FR_PD_FOLD_MEAN) {
        for (unsigned h = 0; h < NH; h++)
            gather_pooled_body<HI, HW, WIDE, false, true, false, F>(words, pool, wd, b0 + h * HI, idx, nullptr, pool_cols, dense, out, batch, err_flag, out_bytes, dst);
    } else {
        for (unsigned h = 0; h < NH; h++)
            gather_pooled_body<HI, HW, WIDE, false, false, false, F>(words, pool, wd, b0 + h * HI, idx, nullptr, pool_cols, dense, out, batch, err_flag, out_bytes, dst);
    }
}

// Which operand forms (bit F of the result: FrPoolDest form F) an instantiation carries arms for.  Six product shapes carry all three.  <4, 2, false>
// and <2, 4, false>, whose record folds sit at 76 and 74 of the 78 scalar registers that 8 waves leave, carry the fp32 arms only: with the bf16 or the
// e4m3 arms next to them (<2, 4, false> holds fp32 or bf16, not both; <4, 2, false> fp32 alone) the compiler carries the dispatch in scalar registers
// the folds have no room for, and spills.  A pooled push of those shapes on a bf16 / fp8 chain writes records and converts them (fr_api.cpp).
// Experiment shapes: none.
constexpr unsigned pooled_operand_forms(int items, int win, bool wide) {
    if ((items == 2 && win == 2) || (items == 2 && win == 4 && wide) || (items == 2 && win == 8) || (items == 1 && win == 16)) return 0xEu;
    if ((items == 4 && win == 2) || (items == 2 && win == 4)) return 0x2u;
    return 0u;
}
// Waves per SIMD the register allocation must leave room for (ITEMS x WIN = 8 row words in flight: 8 waves, 64 registers; 16: 5 waves, 96
// registers): what the shapes had with the plain SUM fold alone, so that no later arm costs that fold a wave.  Experiment shapes: no floor.
constexpr int pooled_min_waves(int items, int win) { return items * win <= 8 ? 8 : items * win == 16 ? 5 : 1; }

template <int ITEMS, int WIN, bool WIDE>
__global__ void __launch_bounds__(256, pooled_min_waves(ITEMS, WIN)) gather_pooled_kernel(const FrWordDesc *__restrict__ words, const FrPoolDesc *__restrict__ pool, const FrGatherGroups groups,
                                                            int n_groups, const int32_t *__restrict__ idx, const float *__restrict__ weights, int pool_cols,
                                                            const float *__restrict__ dense, void *__restrict__ out, int batch, int *__restrict__ err_flag,
                                                            unsigned out_bytes, int any_mean, const int32_t *__restrict__ offsets, int n_icols, unsigned nnz, const FrPoolDest dst) {
    const int group = blockIdx.x & (n_groups - 1);
    const int w0 = groups.start[group];
    const int t = blockIdx.y * blockDim.x + threadIdx.x;
    if (t >= groups.start[group + 1] - w0) return;
    const unsigned b0 = (blockIdx.x / (unsigned)n_groups) * ITEMS;   // the workgroup's chunk of ITEMS items
    bool csr = false;   // uniform over the launch, like `weights` and `any_mean`; the 16-byte-index instantiations hold no offsets arm
    if constexpr (!WIDE) csr = offsets != nullptr;
    constexpr int HI = PooledHalf<ITEMS, WIN>::HI, HW = PooledHalf<ITEMS, WIN>::HW;
    constexpr unsigned NH = PooledHalf<ITEMS, WIN>::NH;
    const int wd = w0 + t;
    constexpr unsigned FORMS = pooled_operand_forms(ITEMS, WIN, WIDE);
    if (FORMS != 0u && __builtin_expect(dst.ldm != 0u, false)) {
        // the operand-store arms (FrPoolDest; uniform over the launch): every fold once more per operand type, its words stored straight into the
        // chain's stage-1 operand.  The operand's zeros come first, while the fold's registers are still free; a chunk of pad items only (uniform
        // over the workgroup) has no fold.  (The launcher sends no form here that the instantiation has no arm for.)
        if constexpr (FORMS != 0u) {
            // (the item-major slice form, FR_PD_ROWS, stores no zeros and needs no test here: its code names no pad word and its grid ends with the
            // batch, so the call below stores nothing and returns false)
            if (gather_pooled_operand_zeros<ITEMS>(words, wd, (unsigned)groups.start[n_groups], b0, out, batch, out_bytes, dst)) return;
            const unsigned form = (unsigned)dst.code & FR_PD_FORM_MASK;
            if constexpr ((FORMS & 2u) != 0u)
                if (form == 1u) gather_pooled_operand_arms<ITEMS, WIN, WIDE, 1>(words, pool, wd, b0, idx, weights, pool_cols, dense, out, batch, err_flag, out_bytes, offsets, n_icols, nnz, dst);
            if constexpr ((FORMS & 4u) != 0u)
                if (form == 2u) gather_pooled_operand_arms<ITEMS, WIN, WIDE, 2>(words, pool, wd, b0, idx, weights, pool_cols, dense, out, batch, err_flag, out_bytes, offsets, n_icols, nnz, dst);
            if constexpr ((FORMS & 8u) != 0u)
                if (form == 3u) gather_pooled_operand_arms<ITEMS, WIN, WIDE, 3>(words, pool, wd, b0, idx, weights, pool_cols, dense, out, batch, err_flag, out_bytes, offsets, n_icols, nnz, dst);
        }
    } else if (__builtin_expect(csr, false)) {   // (out of the padded arms' way)
        // the offsets form (`pool` is then the context's second descriptor array: column and cap per word): two arms, the weighted fold and
        // the counting fold (which is the SUM fold on a word without the MEAN bit), both in the half passes of the arms below
        if constexpr (!WIDE) {
            if (weights) {
                for (unsigned h = 0; h < NH; h++)
                    gather_pooled_body<HI, HW, false, true, false, true>(words, pool, wd, b0 + h * HI, idx, weights, pool_cols, dense, out, batch, err_flag, out_bytes, dst, offsets, n_icols, nnz);
            } else {
                for (unsigned h = 0; h < NH; h++)
                    gather_pooled_body<HI, HW, false, false, true, true>(words, pool, wd, b0 + h * HI, idx, nullptr, pool_cols, dense, out, batch, err_flag, out_bytes, dst, offsets, n_icols, nnz);
            }
        }
    } else if (weights) {
        // the weighted fold keeps half as many row words in flight per pass (half the items, or half the window for one item), so that
        // its weights and products fit the registers the unweighted fold needs anyway: the kernel's register count, hence the unweighted
        // path's occupancy, is the unweighted fold's
        for (unsigned h = 0; h < NH; h++)
            gather_pooled_body<HI, HW, WIDE, true, false>(words, pool, wd, b0 + h * HI, idx, weights, pool_cols, dense, out, batch, err_flag, out_bytes, dst);
    } else if (any_mean) {
        // a context with a MEAN column: the fold that also counts each bag and divides, in half passes like the weighted fold and for the
        // same reason (its count and quotients cost the 4-item form 72 registers against 64: a wave less per SIMD for every SUM context)
        for (unsigned h = 0; h < NH; h++)
            gather_pooled_body<HI, HW, WIDE, false, true>(words, pool, wd, b0 + h * HI, idx, nullptr, pool_cols, dense, out, batch, err_flag, out_bytes, dst);
    } else {   // every column SUM, no weights: the fold as it was before there were modes
        gather_pooled_body<ITEMS, WIN, WIDE, false, false>(words, pool, wd, b0, idx, nullptr, pool_cols, dense, out, batch, err_flag, out_bytes, dst);
    }
}

// what frk_gather_pooled has worked out for the launch, whatever the instantiation
struct PooledLaunch {
    FrGatherGroups groups;
    int n_groups;
    unsigned out_bytes;
    FrPoolDest dst;
};

template <int ITEMS, int WIN, bool WIDE>
static int gather_pooled_launch(const FrPooledPlan &p, const FrPooledBatch &b, const FrPooledOut &o, const PooledLaunch &l, hipStream_t s) {
    const bool feature_major = l.dst.ldm && !((unsigned)l.dst.code & FR_PD_ROWS);
    const int n_chunks = ((feature_major ? (int)l.dst.ldm : b.batch) + ITEMS - 1) / ITEMS;   // the operand form covers the pad items [batch, ldm) too
    const int bx = l.groups.max_words >= 256 ? 256 : ((l.groups.max_words + 63) / 64) * 64;
    dim3 grid(l.n_groups * n_chunks, (l.groups.max_words + bx - 1) / bx);
    // (the padded form: offsets NULL, n_icols and nnz 0 -- the only form the 16-byte-index instantiations are launched for)
    gather_pooled_kernel<ITEMS, WIN, WIDE><<<grid, dim3(bx), 0, s>>>(p.words, p.pool, l.groups, l.n_groups, b.idx, b.weights, p.pool_cols, b.dense, o.ptr, b.batch, p.err_flag, l.out_bytes,
                                                                   p.any_mean ? 1 : 0, b.offsets, p.n_icols, (unsigned)b.nnz, l.dst);
    KCHECK();
    fr_note_kernel("gather_pooled_kernel<%d, %d, %s>", ITEMS, WIN, WIDE ? "true" : "false");
    return FR_OK;
}

// The batch, the destination and the context's part: fr_internal.h.  A RECORDS destination holds p.out_words 16-byte words per item; an OPERAND (SEMANTIC
// records only: a word's place is its dst_off) is Xq[K/4][ldm], Xh[K/8][ldm] or Xf[KE][ldm] in 16-byte elements, p.out_words = K / 4 record words, written
// whole, pad items and pad k-rows as zeros.  p.max_hots picks the window; the offsets form always takes the narrow instantiation (4-byte alignment only).
int frk_gather_pooled(const FrPooledPlan &p, const FrPooledBatch &b, const FrPooledOut &o, hipStream_t s) {
    const int n_words = p.n_words, batch = b.batch;
    if (n_words <= 0 || batch <= 0) return FR_OK;
    const int out_words = p.out_words < n_words ? n_words : p.out_words;
    const int operand = o.kind == FrPooledOut::RECORDS ? 0 : 1 + o.precision;   // FrPoolDest's form: 1 fp32, 2 bf16, 3 e4m3
    const bool item_major = o.kind == FrPooledOut::LP_SLICE;
    PooledLaunch l{};
    size_t out_bytes = (size_t)batch * (size_t)out_words * 16;
    if (operand) {
        const unsigned fold = b.offsets ? (b.weights ? FR_PD_FOLD_CSR_WEIGHTED : FR_PD_FOLD_CSR) : b.weights ? FR_PD_FOLD_WEIGHTED : p.any_mean ? FR_PD_FOLD_MEAN : FR_PD_FOLD_SUM;
        unsigned n_pad = 0;
        if (item_major) {
            // the item-major low-precision slice (FR_PD_ROWS): [batch][out_words] words of 8 (bf16) or 4 (e4m3) bytes; fp32 slices are the record arm's layout already
            if (operand != 2 && operand != 3) FR_FAIL(FR_ERR_INVALID, "pooled gather: no item-major form %d", operand);
            l.dst.ldm = (unsigned)out_words;
            out_bytes = (size_t)batch * (size_t)out_words * (16u >> (operand - 1));   // the resource ends with the batch: the chunk past it is dropped
        } else {
            if (o.ldm < batch || o.ldm % 32) FR_FAIL(FR_ERR_INVALID, "pooled gather: operand of %d items for a batch of %d", o.ldm, batch);
            if (operand < 1 || operand > 3) FR_FAIL(FR_ERR_INVALID, "pooled gather: no operand form %d", operand);
            l.dst.ldm = (unsigned)o.ldm;
            const unsigned per_row = 1u << (operand - 1);   // record words per 16-byte element
            const size_t k_rows = operand == 3 ? ((size_t)out_words * 4 + 63) / 64 * 4 : ((size_t)out_words + per_row - 1) / per_row;
            n_pad = (unsigned)(k_rows * per_row - (size_t)out_words);   // at most 15
            static_assert(15u <= FR_PD_PAD_MASK, "an e4m3 row pads at most 15 words");
            out_bytes = k_rows * (size_t)o.ldm * 16;
        }
        if (p.e_x < -126 || p.e_x > 127) FR_FAIL(FR_ERR_INVALID, "pooled gather: X exponent %d", p.e_x);   // (behind the form's own checks, as ever)
        l.dst.code = operand | (int)(item_major ? FR_PD_ROWS : n_pad << FR_PD_PAD_SHIFT) | (int)(fold << FR_PD_FOLD_SHIFT) | (int)((unsigned)(operand == 3 ? p.e_x : 0) << FR_PD_EX_SHIFT);   // (arithmetic shift in the kernel: the exponent's sign survives)
    }
    const size_t idx_bytes = b.offsets ? (size_t)b.nnz * 4 : (size_t)batch * (size_t)p.pool_cols * 4;
    const size_t off_bytes = b.offsets ? ((size_t)batch * (size_t)p.n_icols + 1) * 4 : 0;
    // 32-bit resource offsets, with room for the chunk past the batch (the offsets form's three sizes are refused by the C-ABI, for both back-ends, before it gets here)
    if (out_bytes >= ((size_t)4000 << 20) || idx_bytes >= ((size_t)4000 << 20) || off_bytes >= ((size_t)4000 << 20))
        FR_FAIL(FR_ERR_INVALID, "pooled gather: the batch's index rows%s (%zu bytes) or records (%zu bytes) reach 4000 MiB", b.weights ? " / weights" : "", idx_bytes, out_bytes);
    l.out_bytes = (unsigned)out_bytes;
    l.groups = *p.groups;
    l.n_groups = 8;
    if (l.groups.max_words <= 0) {   // no XCD plan (a narrow record): one group, whole workgroups along the words
        l.n_groups = 1;
        l.groups.start[0] = 0;
        for (int g = 1; g <= 8; g++) l.groups.start[g] = n_words;
        l.groups.max_words = n_words;
    }
    const bool wide = p.wide && !b.offsets && ((reinterpret_cast<uintptr_t>(b.idx) | reinterpret_cast<uintptr_t>(b.weights)) & 15) == 0;   // 16-byte loads of both arrays
    // window x items per thread by the longest bag, from the sweep on the MI355X (profiles/pooled_gather_window_sweep.md: Model-C batch 4096, every
    // window x items pair at hots 1 .. 16): the longest window that a bag fills wins by 1-5 %, with as few items per thread as keep 16 row words
    // in flight; a one-slot window is 20 % slower than a two-slot one at hots = 1 and is not built.  FR_POOL_WIN / FR_POOL_ITEMS: experiments build only
    int win = p.max_hots >= 16 ? 16 : p.max_hots >= 8 ? 8 : p.max_hots >= 4 ? 4 : 2;
    int items = win >= 16 ? 1 : p.max_hots >= 2 ? 2 : 4;
    win = FR_KNOB("POOL_WIN", win);
    items = FR_KNOB("POOL_ITEMS", items);
    if (item_major && !((pooled_operand_forms(items, win, win % 4 == 0 && wide) >> operand) & 1u)) {
        // <4, 2, false> and <2, 4, false> carry no bf16 / e4m3 arm: the slice takes the neighbouring shape that does -- any shape folds any bag with the
        // same bits (a longest bag of 1: a window of 2 x 2 items; of 4 .. 7 in the narrow form: a window of 8 x 2 items)
        if (items == 4 && win == 2) items = 2;
        else if (items == 2 && win == 4) win = 8;
    }
#define FR_GP(I, W)                                                                                                                 \
    if (items == I && win == W) {                                                                                                   \
        if (l.dst.ldm && !((pooled_operand_forms(I, W, W % 4 == 0 && wide) >> operand) & 1u)) return FR_POOL_NO_OPERAND_ARM;        \
        if constexpr (W % 4 == 0)                                                                                                   \
            if (wide) return gather_pooled_launch<I, W, true>(p, b, o, l, s);                                                       \
        return gather_pooled_launch<I, W, false>(p, b, o, l, s);                                                                    \
    }
    FR_GP(4, 2)
    FR_GP(2, 2)
    FR_GP(2, 4)
    FR_GP(2, 8)
    FR_GP(1, 16)
#ifdef FR_EXPERIMENTS
    FR_GP(1, 1) FR_GP(2, 1) FR_GP(4, 1) FR_GP(8, 1)
    FR_GP(1, 2) FR_GP(8, 2)
    FR_GP(1, 4) FR_GP(4, 4) FR_GP(8, 4)
    FR_GP(1, 8) FR_GP(4, 8)
    FR_GP(2, 16)
#endif
#undef FR_GP
    FR_FAIL(FR_ERR_INVALID, "pooled gather: no kernel for %d items x a window of %d slots", items, win);
}

// ---------------------------------------------------------------------------------------------------
// gather_tile_kernel<DEDUP>: the item-tile form of the record-producing gather -- LDS-staged row packing, with (DEDUP) or without a
// wave-level merge of duplicate lookups (north_star: "LDS-staged row packing and wavefront ballot/shuffle for index dedup").
//
// A 256-thread workgroup owns 64 items x one chunk of <= 64 consecutive record words.  A wave-instruction ("pass") covers 64 / w items
// x the w 16-byte words of one source row each, so every row is one contiguous request of w adjacent lanes and a wave sees up to 64
// lookups of the SAME table at once -- which is what makes duplicates visible to it (in gather_pack_kernel a wave holds one item's
// words of many tables: no two lanes ever want the same row).  DEDUP: the lanes of a pass agree on one leader per distinct index
// through a 128-slot LDS hash of the index (last writer wins; a slot collision between different indices only costs a missed
// merge, never a wrong row: the leader's index is compared through a shuffle), only leaders load, the others take the leader's
// registers by ds_bpermute (__shfl); __ballot counts the merged lookups when a counter is supplied.
// All index loads of the wave's passes are issued first, then all row loads, then the rows go to the LDS tile; after one barrier the
// tile leaves as whole 1 KiB record pieces per item (fully coalesced, like gather_pack_kernel's stores).
// ---------------------------------------------------------------------------------------------------
constexpr int FR_TILE_LD = FR_TILE_WORDS + 1;     // LDS tile row stride in 16-byte words (+1: conflict-free column writes)
constexpr int FR_TILE_MAXP = FR_TILE_WORDS / 4;   // passes per wave: a chunk has <= 64 passes, dealt round-robin to 4 waves

template <bool DEDUP>
__global__ void __launch_bounds__(256) gather_tile_kernel(const FrPassDesc *__restrict__ passes, const FrChunkDesc *__restrict__ chunks, int n_chunks,
                                                          int chunks_per_group, const int32_t *__restrict__ idx, int idx_stride,
                                                          const float *__restrict__ dense, uint4 *__restrict__ out, int out_stride_words, int batch,
                                                          int *__restrict__ err_flag, unsigned long long *__restrict__ dup_counter) {
    __shared__ uint4 tile[FR_TILE_ITEMS * FR_TILE_LD];
    __shared__ uint32_t hash_slots[4][128];
    // workgroup b serves XCD group b % 8 (round-robin dealing; a speed assumption only): a chunk, hence a table, is always fetched by
    // the same XCD, so the 8 L2s cache 8 different table sets (as gather_pack_xcd_kernel does)
    const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
    const int chunk = (j % chunks_per_group) * 8 + x;
    const int item_tile = j / chunks_per_group;
    if (chunk >= n_chunks) return;
    const FrChunkDesc ch = chunks[chunk];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: descriptors load through SMEM
    const int m0 = item_tile * FR_TILE_ITEMS;

    uint32_t id[FR_TILE_MAXP];
    uint4 v[FR_TILE_MAXP];
    bool bad = false;
    // phase 1: index loads of every pass of this wave
#pragma unroll
    for (int q = 0; q < FR_TILE_MAXP; q++) {
        const int p = ch.pass_begin + 4 * q + wave;
        id[q] = 0;
        if (p < ch.pass_end) {
            const FrPassDesc d = passes[p];
            const int m = m0 + d.item0 + (lane >> d.log2_words);
            const bool is_dense = (d.idx_col & FR_DESC_DENSE) != 0;
            if (m < batch) id[q] = is_dense ? (uint32_t)m : (uint32_t)idx[(size_t)m * idx_stride + d.idx_col];
        }
    }
    // phase 2: (dedup,) row loads
    uint32_t src_lane[FR_TILE_MAXP];
    unsigned merged = 0;
#pragma unroll
    for (int q = 0; q < FR_TILE_MAXP; q++) {
        const int p = ch.pass_begin + 4 * q + wave;
        src_lane[q] = (uint32_t)lane;
        if (p < ch.pass_end) {
            const FrPassDesc d = passes[p];
            const bool is_dense = (d.idx_col & FR_DESC_DENSE) != 0;
            const uint32_t word = (uint32_t)lane & ((1u << d.log2_words) - 1u);
            if (!is_dense && id[q] >= d.rows) {  // reference: silent out-of-bounds read (embedding_47_krnl.cpp:927-933)
                bad = true;
                id[q] = 0;
            }
            bool dup = false;
            if (DEDUP && !is_dense) {
                const uint32_t slot = (uint32_t)lane >> d.log2_words;
                const uint32_t h = (id[q] * 0x9E3779B1u) >> 25;
                // same-wave LDS accesses execute in order: the read sees this pass's last writer.  volatile: without it hipcc forwards
                // the lane's own store to its load and no lane ever finds a leader
                volatile uint32_t *slots = hash_slots[wave];
                slots[h] = slot;
                __builtin_amdgcn_wave_barrier();
                const uint32_t winner = slots[h];
                const uint32_t wid = (uint32_t)__shfl((int)id[q], (int)(winner << d.log2_words));
                dup = wid == id[q] && winner != slot;
                if (dup) src_lane[q] = (winner << d.log2_words) + word;
                if (dup_counter) merged += (unsigned)__popcll(__ballot(dup && word == 0));
            }
            const char *base = is_dense ? reinterpret_cast<const char *>(dense) + d.src : reinterpret_cast<const char *>(d.src);
            if (!dup) v[q] = *reinterpret_cast<const uint4 *>(base + (uint64_t)id[q] * d.stride + 16u * word);
        }
    }
    // phase 3: duplicates take their leader's registers; rows -> LDS tile
#pragma unroll
    for (int q = 0; q < FR_TILE_MAXP; q++) {
        const int p = ch.pass_begin + 4 * q + wave;
        if (p < ch.pass_end) {
            const FrPassDesc d = passes[p];
            uint4 r = v[q];
            if (DEDUP) {
                r.x = (uint32_t)__shfl((int)v[q].x, (int)src_lane[q]);
                r.y = (uint32_t)__shfl((int)v[q].y, (int)src_lane[q]);
                r.z = (uint32_t)__shfl((int)v[q].z, (int)src_lane[q]);
                r.w = (uint32_t)__shfl((int)v[q].w, (int)src_lane[q]);
            }
            const uint32_t word = (uint32_t)lane & ((1u << d.log2_words) - 1u);
            tile[(d.item0 + (lane >> d.log2_words)) * FR_TILE_LD + d.tile_word + word] = r;
        }
    }
    __syncthreads();
    // phase 4: whole record pieces out, 16 items per wave
#pragma unroll 4
    for (int i = 0; i < FR_TILE_ITEMS / 4; i++) {
        const int it = wave * (FR_TILE_ITEMS / 4) + i, m = m0 + it;
        if (m < batch && lane < ch.n_words) out[(size_t)m * out_stride_words + ch.word0 + lane] = tile[it * FR_TILE_LD + lane];
    }
    if (bad) atomicOr_system(err_flag, 1);
    if (DEDUP && dup_counter && lane == 0 && merged) atomicAdd(dup_counter, (unsigned long long)merged);
}

int frk_gather_tile(const FrPassDesc *passes, const FrChunkDesc *chunks, int n_chunks, const int32_t *idx, int idx_stride, const float *dense, void *out,
                    int out_stride_words, int batch, int *err_flag, bool dedup, unsigned long long *dup_counter, hipStream_t s) {
    if (n_chunks <= 0 || batch <= 0) return FR_OK;
    const int cpg = (n_chunks + 7) / 8;
    const int tiles = (batch + FR_TILE_ITEMS - 1) / FR_TILE_ITEMS;
    dim3 grid(8 * cpg * tiles);
    if (dedup)
        gather_tile_kernel<true><<<grid, dim3(256), 0, s>>>(passes, chunks, n_chunks, cpg, idx, idx_stride, dense, reinterpret_cast<uint4 *>(out), out_stride_words, batch,
                                                           err_flag, dup_counter);
    else
        gather_tile_kernel<false><<<grid, dim3(256), 0, s>>>(passes, chunks, n_chunks, cpg, idx, idx_stride, dense, reinterpret_cast<uint4 *>(out), out_stride_words, batch,
                                                            err_flag, nullptr);
    KCHECK();
    fr_note_kernel("gather_tile_kernel<%s>", dedup ? "true" : "false");
    return FR_OK;
}
