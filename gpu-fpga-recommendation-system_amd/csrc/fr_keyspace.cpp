// Keyed lookups, host side (include/fleetrec_serving.h): key spaces, the list-form changes of a map (put, erase, admit) in their worker and context
// forms, the life cycle of a map (stats, export, rebuild), row pools and the resolves.  fr_worker_submit_keyed stays in fr_api.cpp, beside the submit
// paths it calls; what the two files call of each other is declared in fr_internal.h.
// The kernels are the third companion code object's (fr_keys.hip -> libfleetrec_keys.so, linked with an $ORIGIN rpath); slot layout, mix64 and the probe
// rule are fr_keys.h's; key spaces, tables, order and the host form are here, the CPU twins in fr_cpu.cpp.
#include <cstdio>
#include <cstring>

#include "fr_internal.h"

static uint32_t key_col_range(const fr_ctx *c, int col) {   // R_c: the row count the one-hot gather checks for index column col (build_words)
    const fr_model_desc &m = c->model;
    if (m.index_mode == FR_INDEX_PER_TABLE) return (uint32_t)c->tables[(size_t)col].rows;
    if (m.index_mode == FR_INDEX_PER_BANK) return (uint32_t)c->bank_rows[(size_t)col];
    int64_t r = c->tables[0].rows;
    for (const fr_table_desc &t : c->tables) r = t.rows < r ? t.rows : r;
    return (uint32_t)r;
}

static int key_col_check(const fr_ctx *c, int col, const char *who) {
    if (col < 0 || col >= (int)idx_cols(c)) FR_FAIL(FR_ERR_INVALID, "%s: column %d, the context has %zu index columns", who, col, idx_cols(c));
    return FR_OK;
}

static int key_col_mapped(const fr_ctx *c, int col, const char *who) {
    if (c->key_spaces.empty() || c->key_spaces[(size_t)col].mode != FR_KEYS_MAPPED)
        FR_FAIL(FR_ERR_STATE, "%s: column %d has no map: call fr_ctx_set_key_space(ctx, %d, FR_KEYS_MAPPED, ...) first", who, col, col);
    return FR_OK;
}

int fr_key_unsharded(const fr_ctx *c, const char *who) {
    if (c->n_shards > 1) FR_FAIL(FR_ERR_STATE, "%s: keyed lookups are not available on a sharded context (%d shards)", who, c->n_shards);
    return FR_OK;
}

static int key_max_keys_check(int64_t max_keys, const char *who) {
    if (max_keys < 1 || max_keys > (1ll << 30)) FR_FAIL(FR_ERR_INVALID, "%s: max_keys %lld outside [1, 2^30]", who, (long long)max_keys);
    return FR_OK;
}

static int key_grid_cap(const fr_ctx *c, int per_cu) { return per_cu * (c->n_cu > 0 ? c->n_cu : 256); }   // the most blocks of a grid-stride launch

// the records of every column as a resolve reads them, from key_spaces: on the device (synchronous copy) or, on the CPU back-end, in place
static int key_cols_upload(fr_ctx *c) {
    const size_t C = idx_cols(c);
    c->h_key_cols.resize(C);
    for (size_t i = 0; i < C; i++) {
        const fr_ctx::KeySpace &k = c->key_spaces[i];
        FrKeyCol &r = c->h_key_cols[i];
        r.seed = k.seed, r.slots = k.slots.p, r.mask = k.slots.p ? (uint32_t)(k.slots.count() - 1) : 0u;
        r.range = key_col_range(c, (int)i), r.miss_row = k.miss_row, r.mode = k.mode;
    }
    if (c->cpu) return FR_OK;
    FR_TRY(c->d_key_cols.grow(FrMem::DEVICE, C, "key-space records"));
    FR_HIP(hipMemcpy(c->d_key_cols, c->h_key_cols.data(), C * sizeof(FrKeyCol), hipMemcpyHostToDevice));
    return FR_OK;
}

// key spaces exist from the first call on: every column FR_KEYS_ROWS, the counts zero
static int key_spaces_init(fr_ctx *c) {
    if (!c->key_spaces.empty()) return FR_OK;
    const size_t C = idx_cols(c);
    FrBuf<uint32_t> counts;
    FR_TRY(counts.alloc(fr_mem_kind(c, FrMem::DEVICE), C, "key counts"));
    if (c->cpu) memset(counts.p, 0, C * sizeof(uint32_t));
    else FR_HIP(hipMemset(counts.p, 0, C * sizeof(uint32_t)));
    if (!c->cpu) FR_TRY(c->d_key_walk.alloc(FrMem::DEVICE, 3, "key-map walk counters"));
    c->d_key_counts.swap(counts);
    c->key_spaces.resize(C);
    return key_cols_upload(c);
}

// A new map for max_keys keys into `next`, every slot empty with miss_row: allocated, its fill enqueued on the set-up stream (the CPU back-end: done).
// Whatever the caller enqueues on that stream next follows the fill; a caller with nothing more to enqueue synchronises.
static int key_map_new(fr_ctx *c, fr_ctx::KeySpace &next, int64_t max_keys, int32_t miss_row) {
    next.max_keys = max_keys, next.miss_row = miss_row;
    const uint64_t slots = fr_key_slots((uint64_t)max_keys);
    FR_TRY(next.slots.alloc(fr_mem_kind(c, FrMem::DEVICE), (size_t)slots, "key map"));
    const FrKeyFillArgs f{next.slots.p, slots, miss_row};
    if (c->cpu) {
        frc_fill_keys(f);
        return FR_OK;
    }
    const int e = fr_key_fill_launch(&f, (void *)c->setup_stream);
    if (e) {
        (void)hipStreamSynchronize(c->setup_stream);
        FR_FAIL(FR_ERR_HIP, "the key map's fill launch failed: %s", hipGetErrorString((hipError_t)e));
    }
    return FR_OK;
}

static int key_count_set(fr_ctx *c, int col, uint32_t n) {   // n_keys of column col (no launch that counts is in flight)
    if (c->cpu) c->d_key_counts[col] = n;
    else FR_HIP(hipMemcpy(c->d_key_counts + col, &n, sizeof(n), hipMemcpyHostToDevice));
    return FR_OK;
}

// one 32-bit counter that launches of any worker may be changing: read behind everything in flight on the device
static int key_read_word(fr_ctx *c, const void *p, void *out) {
    if (c->cpu) {
        *(uint32_t *)out = __atomic_load_n((const uint32_t *)p, __ATOMIC_ACQUIRE);
        return FR_OK;
    }
    FR_SET_DEVICE(c);
    FR_HIP(hipDeviceSynchronize());
    FR_HIP(hipMemcpy(out, p, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return FR_OK;
}

extern "C" int fr_ctx_set_key_space(fr_ctx *ctx, int col, int mode, uint64_t seed, int64_t max_keys, int32_t miss_row) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    FR_TRY(key_col_check(ctx, col, "fr_ctx_set_key_space"));
    if (mode < FR_KEYS_ROWS || mode > FR_KEYS_MAPPED) FR_FAIL(FR_ERR_INVALID, "fr_ctx_set_key_space: mode %d is none of FR_KEYS_ROWS, FR_KEYS_HASHED, FR_KEYS_MAPPED", mode);
    const uint32_t range = key_col_range(ctx, col);
    if (mode == FR_KEYS_MAPPED) {
        FR_TRY(key_max_keys_check(max_keys, "fr_ctx_set_key_space"));
        if (miss_row != -1 && miss_row != FR_KEY_NO_ROW && !(miss_row >= 0 && (uint32_t)miss_row < range))
            FR_FAIL(FR_ERR_INVALID, "fr_ctx_set_key_space: miss_row %d is neither a row of column %d (%u rows), nor -1, nor FR_KEY_NO_ROW", miss_row, col, range);
    }
    FR_TRY(fr_key_unsharded(ctx, "fr_ctx_set_key_space"));
    FR_TRY(fr_pooling_busy(ctx, "fr_ctx_set_key_space"));
    if (!ctx->cpu) FR_SET_DEVICE(ctx);
    std::lock_guard<std::mutex> lk(ctx->key_mutex);   // (a first resolve on another thread makes the key spaces under the same lock)
    FR_TRY(key_spaces_init(ctx));
    fr_ctx::KeySpace next;
    next.mode = mode, next.seed = mode == FR_KEYS_ROWS ? 0 : seed;
    if (mode == FR_KEYS_MAPPED) {
        FR_TRY(key_map_new(ctx, next, max_keys, miss_row));
        if (!ctx->cpu) FR_HIP(hipStreamSynchronize(ctx->setup_stream));
    }
    FR_TRY(key_count_set(ctx, col, 0));
    std::swap(ctx->key_spaces[(size_t)col], next);   // (no worker has work in flight: whatever map the column had is released with `next`)
    if (mode != FR_KEYS_ROWS) ctx->keyed = true;
    return key_cols_upload(ctx);
}

extern "C" int fr_ctx_key_space(fr_ctx *ctx, int col, int *mode, uint64_t *seed, int64_t *max_keys, int64_t *n_keys, int32_t *miss_row) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    FR_TRY(key_col_check(ctx, col, "fr_ctx_key_space"));
    const fr_ctx::KeySpace none{};
    const fr_ctx::KeySpace &k = ctx->key_spaces.empty() ? none : ctx->key_spaces[(size_t)col];
    uint32_t n = 0;
    if (k.mode == FR_KEYS_MAPPED) FR_TRY(key_read_word(ctx, ctx->d_key_counts + col, &n));
    if (mode) *mode = k.mode;
    if (seed) *seed = k.seed;
    if (max_keys) *max_keys = k.max_keys;
    if (n_keys) *n_keys = (int64_t)n;
    if (miss_row) *miss_row = k.miss_row;
    return FR_OK;
}

static FrKeyPutArgs key_put_args(fr_ctx *c, int col, int n, const int64_t *keys, const int32_t *rows, int *err) {
    FrKeyPutArgs a{};
    a.col = c->h_key_cols[(size_t)col], a.n_keys = c->d_key_counts + col, a.max_keys = (uint32_t)c->key_spaces[(size_t)col].max_keys;
    a.n = n, a.keys = keys, a.rows = rows, a.err_flag = err;
    return a;
}

// what fr_worker_sync (or fr_ctx_put_keys itself) says about the bits of a status word; bit 0 is the lookups'
int fr_index_range_fail(int bits) {
    const char *lookup = (bits & 1) ? "a lookup index was outside its table (row 0 was read instead)" : "";
    if (bits & FR_KEYS_ERR_ADMIT) {   // an admit marks its bits; whatever else the word holds is named by the rest of the word, without the admit's
        char rest[640] = "";
        const int other = bits & ~(FR_KEYS_ERR_ADMIT | FR_KEYS_ERR_NO_FREE_ROW | FR_KEYS_ERR_EMPTY_KEY | FR_KEYS_ERR_FULL);
        if (other) {
            (void)fr_index_range_fail(other);
            snprintf(rest, sizeof rest, " %s", fr_last_error());
        }
        FR_FAIL(FR_ERR_INDEX_RANGE, "a key admit was not applied (every other key was):%s%s%s%s", (bits & FR_KEYS_ERR_EMPTY_KEY) ? " a key of -1 (FR_KEY_EMPTY);" : "",
                (bits & FR_KEYS_ERR_NO_FREE_ROW) ? " no free row: the column's row pool is exhausted (FR_KEYS_ERR_NO_FREE_ROW);" : "",
                (bits & FR_KEYS_ERR_FULL) ? " a new key for a map that holds max_keys keys (the row went back to the pool);" : "", rest);
    }
    const int put = bits & (FR_KEYS_ERR_EMPTY_KEY | FR_KEYS_ERR_ROW | FR_KEYS_ERR_FULL);
    const char *erase = (bits & FR_KEYS_ERR_ERASE_EMPTY) ? "a key erase was not applied (every other key was): a key of -1 (FR_KEY_EMPTY);" : "";
    if (!put) FR_FAIL(FR_ERR_INDEX_RANGE, "%s%s%s", lookup, (bits & 1) && *erase ? "; " : "", erase);
    FR_FAIL(FR_ERR_INDEX_RANGE, "%s%sa key put was not applied (every other pair was):%s%s%s%s%s", lookup, (bits & 1) ? "; " : "", (bits & FR_KEYS_ERR_EMPTY_KEY) ? " a key of -1 (FR_KEY_EMPTY);" : "",
            (bits & FR_KEYS_ERR_ROW) ? " a row that is neither one of the column's rows nor its miss_row;" : "", (bits & FR_KEYS_ERR_FULL) ? " a new key for a map that holds max_keys keys;" : "",
            *erase ? " " : "", erase);
}

// ---- the life cycle of a key map: erase, stats, export, rebuild (fleetrec_serving.h) --------------------------------------------------------------
// The kernels are the fifth companion code object's (fr_keymaint.hip -> libfleetrec_keymaint.so); the CPU twins are frc_erase_keys / frc_walk_keys.
// the pool of column col as the kernels and the twins take it (n_rows == 0: the column has none)
static FrKeyPool key_pool_of(const fr_ctx *c, int col) {
    const fr_ctx::KeySpace &k = c->key_spaces[(size_t)col];
    return FrKeyPool{k.pool_bits.p, k.pool_free.p, k.pool_first, k.pool_rows};
}

// An erase on a column with a pool gives the rows back (keyadmit_release_kernel of libfleetrec_admit.so; frc_release_keys); without one it is
// keymap_erase_kernel (frc_erase_keys), as ever.  -> the twin's bits on the CPU back-end, the launch's hipError_t value on the device.
static int key_erase_run(fr_ctx *c, int col, int n, const int64_t *keys, int *err, hipStream_t s) {
    const FrKeyPool pool = key_pool_of(c, col);
    if (pool.n_rows > 0) {
        const FrKeyReleaseArgs r{c->h_key_cols[(size_t)col], pool, n, keys, err};
        return c->cpu ? frc_release_keys(r) : fr_keyadmit_release_launch(&r, (void *)s);
    }
    FrKeyEraseArgs a{};
    a.col = c->h_key_cols[(size_t)col], a.n = n, a.keys = keys, a.err_flag = err;
    return c->cpu ? frc_erase_keys(a) : fr_keymap_erase_launch(&a, (void *)s);
}

// One walk of column col's map (under key_mutex) on the set-up stream, waited for: counts[3] are zeroed first and read back.  The CPU back-end: the twin.
static int key_walk(fr_ctx *c, FrKeyWalkArgs a, unsigned long long counts[3]) {
    counts[0] = counts[1] = counts[2] = 0;
    if (c->cpu) {
        a.counts = counts;
        frc_walk_keys(a);
        return FR_OK;
    }
    unsigned long long *d = c->d_key_walk.p;   // (made with the key spaces: no call of the life cycle changes what the context holds besides its maps)
    FR_HIP(hipMemsetAsync(d, 0, 3 * sizeof(unsigned long long), c->setup_stream));
    a.counts = d, a.max_blocks = key_grid_cap(c, 4);
    const int e = fr_keymap_walk_launch(&a, (void *)c->setup_stream);
    if (e) {
        (void)hipStreamSynchronize(c->setup_stream);
        FR_FAIL(FR_ERR_HIP, "the key-map walk launch failed: %s", hipGetErrorString((hipError_t)e));
    }
    FR_HIP(hipMemcpyAsync(counts, d, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->setup_stream));
    FR_HIP(hipStreamSynchronize(c->setup_stream));
    return FR_OK;
}

// what the three read-side calls share: the column is MAPPED, the device is idle
static int key_map_ready(fr_ctx *c, int col, const char *who) {
    FR_TRY(key_col_check(c, col, who));
    FR_TRY(key_col_mapped(c, col, who));
    if (!c->cpu) {
        FR_SET_DEVICE(c);
        FR_HIP(hipDeviceSynchronize());
    }
    return FR_OK;
}

extern "C" int fr_ctx_key_space_stats(fr_ctx *ctx, int col, int64_t *slots, int64_t *occupied, int64_t *live, int64_t *probe_sum) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    std::lock_guard<std::mutex> lk(ctx->key_mutex);
    FR_TRY(key_map_ready(ctx, col, "fr_ctx_key_space_stats"));
    FrKeyWalkArgs a{};
    a.col = ctx->h_key_cols[(size_t)col], a.sink = FR_KEYWALK_COUNT;
    unsigned long long n[3];
    FR_TRY(key_walk(ctx, a, n));
    if (slots) *slots = (int64_t)a.col.mask + 1;
    if (occupied) *occupied = (int64_t)n[0];
    if (live) *live = (int64_t)n[1];
    if (probe_sum) *probe_sum = (int64_t)n[2];
    return FR_OK;
}

extern "C" int fr_ctx_export_keys(fr_ctx *ctx, int col, int64_t cap, int64_t *h_keys, int32_t *h_rows, int64_t *n_out) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    if (n_out) *n_out = 0;
    if (cap < 0) FR_FAIL(FR_ERR_INVALID, "fr_ctx_export_keys: cap = %lld", (long long)cap);
    if (cap > 0 && (!h_keys || !h_rows)) FR_FAIL(FR_ERR_INVALID, "fr_ctx_export_keys: h_keys / h_rows is NULL with cap = %lld", (long long)cap);
    std::lock_guard<std::mutex> lk(ctx->key_mutex);
    FR_TRY(key_map_ready(ctx, col, "fr_ctx_export_keys"));
    FrKeyWalkArgs a{};
    a.col = ctx->h_key_cols[(size_t)col];
    unsigned long long n[3];
    a.sink = FR_KEYWALK_COUNT;   // the size first: nothing is written unless everything fits
    FR_TRY(key_walk(ctx, a, n));
    const uint64_t live = n[1];
    if (n_out) *n_out = (int64_t)live;
    if ((uint64_t)cap < live) FR_FAIL(FR_ERR_INVALID, "fr_ctx_export_keys: the map of column %d holds %llu live pairs, cap is %lld (nothing was written)", col, (unsigned long long)live, (long long)cap);
    if (live == 0) return FR_OK;
    a.sink = FR_KEYWALK_EXPORT, a.cap = live;   // (no put is in flight: the device was synchronised and the caller holds the map still)
    if (ctx->cpu) {
        a.out_keys = h_keys, a.out_rows = h_rows;
        return key_walk(ctx, a, n);
    }
    FrBuf<int64_t> d_keys;
    FrBuf<int32_t> d_rows;
    FR_TRY(d_keys.alloc(FrMem::DEVICE, (size_t)live, "key export keys"));
    FR_TRY(d_rows.alloc(FrMem::DEVICE, (size_t)live, "key export rows"));
    a.out_keys = d_keys.p, a.out_rows = d_rows.p;
    FR_TRY(key_walk(ctx, a, n));
    if (n[0] != live) FR_FAIL(FR_ERR_STATE, "fr_ctx_export_keys: the map of column %d changed during the call (%llu live pairs, then %llu): a put or erase is in flight", col, (unsigned long long)live, n[0]);
    FR_HIP(hipMemcpy(h_keys, d_keys.p, (size_t)live * sizeof(int64_t), hipMemcpyDeviceToHost));
    FR_HIP(hipMemcpy(h_rows, d_rows.p, (size_t)live * sizeof(int32_t), hipMemcpyDeviceToHost));
    return FR_OK;
}

extern "C" int fr_ctx_rebuild_key_space(fr_ctx *ctx, int col, uint64_t seed, int64_t max_keys) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    FR_TRY(key_col_check(ctx, col, "fr_ctx_rebuild_key_space"));
    FR_TRY(key_max_keys_check(max_keys, "fr_ctx_rebuild_key_space"));
    FR_TRY(fr_key_unsharded(ctx, "fr_ctx_rebuild_key_space"));
    FR_TRY(fr_pooling_busy(ctx, "fr_ctx_rebuild_key_space"));
    std::lock_guard<std::mutex> lk(ctx->key_mutex);
    FR_TRY(key_map_ready(ctx, col, "fr_ctx_rebuild_key_space"));
    fr_ctx::KeySpace &old = ctx->key_spaces[(size_t)col];
    FrKeyWalkArgs a{};
    a.col = ctx->h_key_cols[(size_t)col], a.sink = FR_KEYWALK_COUNT;
    unsigned long long n[3];
    FR_TRY(key_walk(ctx, a, n));
    const uint64_t live = n[1];
    if ((uint64_t)max_keys < live) FR_FAIL(FR_ERR_INVALID, "fr_ctx_rebuild_key_space: max_keys %lld is below the %llu live keys of column %d", (long long)max_keys, (unsigned long long)live, col);
    fr_ctx::KeySpace next;   // (whatever fails from here on: `next` releases the new map, the old one stays as it was)
    next.mode = FR_KEYS_MAPPED, next.seed = seed;
    FR_TRY(key_map_new(ctx, next, max_keys, old.miss_row));   // (the walk below follows the fill on the same stream)
    a.sink = FR_KEYWALK_REHASH, a.dst = a.col;
    a.dst.seed = seed, a.dst.slots = next.slots.p, a.dst.mask = (uint32_t)(next.slots.count() - 1);
    FR_TRY(key_walk(ctx, a, n));
    if (n[0] != live) FR_FAIL(FR_ERR_HIP, "fr_ctx_rebuild_key_space: %llu of the %llu live pairs of column %d reached the new map (the old map stays)", n[0], (unsigned long long)live, col);
    FR_TRY(key_count_set(ctx, col, (uint32_t)live));
    next.pool_first = old.pool_first, next.pool_rows = old.pool_rows;   // the row pool goes with the live keys: they keep their rows
    next.pool_bits.swap(old.pool_bits), next.pool_free.swap(old.pool_free);
    std::swap(old, next);   // (no worker has work in flight: the old map is released with `next`)
    return key_cols_upload(ctx);
}

// ---- row pools: admitting ids (fleetrec_serving.h) --------------------------------------------------------------------------------------------------
// The kernels are the sixth companion code object's (fr_keyadmit.hip -> libfleetrec_admit.so); the CPU twins are frc_admit_keys / frc_release_keys /
// frc_mark_pool.  The pool's bitmap and counter belong to the column's KeySpace: a rebuild hands them on, fr_ctx_set_key_space drops them.
extern "C" int fr_ctx_set_row_pool(fr_ctx *ctx, int col, int32_t first_row, int32_t n_rows) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    FR_TRY(key_col_check(ctx, col, "fr_ctx_set_row_pool"));
    if (n_rows < 0) FR_FAIL(FR_ERR_INVALID, "fr_ctx_set_row_pool: n_rows = %d", n_rows);
    const uint32_t range = key_col_range(ctx, col);
    if (n_rows > 0 && (first_row < 0 || (int64_t)first_row + n_rows > (int64_t)range))
        FR_FAIL(FR_ERR_INVALID, "fr_ctx_set_row_pool: rows [%d, %lld) are not inside the %u rows of column %d", first_row, (long long)first_row + n_rows, range, col);
    FR_TRY(fr_key_unsharded(ctx, "fr_ctx_set_row_pool"));
    FR_TRY(fr_pooling_busy(ctx, "fr_ctx_set_row_pool"));
    std::lock_guard<std::mutex> lk(ctx->key_mutex);
    FR_TRY(key_map_ready(ctx, col, "fr_ctx_set_row_pool"));
    fr_ctx::KeySpace &k = ctx->key_spaces[(size_t)col];
    if (n_rows == 0) {   // drop the pool
        k.pool_first = k.pool_rows = 0;
        k.pool_bits.reset(), k.pool_free.reset();
        return FR_OK;
    }
    if (k.miss_row >= first_row && k.miss_row - first_row < n_rows)
        FR_FAIL(FR_ERR_INVALID, "fr_ctx_set_row_pool: rows [%d, %d) contain the column's miss_row %d", first_row, first_row + n_rows, k.miss_row);
    // the free set is derived from the map as it stands: whatever fails from here on, the column keeps the pool it had
    FrBuf<uint32_t> bits;
    FrBuf<int32_t> free_rows;
    const uint32_t words = fr_key_pool_words(n_rows), pad = fr_key_pool_pad(n_rows);
    FR_TRY(bits.alloc(fr_mem_kind(ctx, FrMem::DEVICE), words, "row-pool bitmap"));
    FR_TRY(free_rows.alloc(fr_mem_kind(ctx, FrMem::DEVICE), 1, "row-pool counter"));
    FrKeyMarkArgs m{ctx->h_key_cols[(size_t)col], FrKeyPool{bits.p, free_rows.p, first_row, n_rows}, 0};
    if (ctx->cpu) {
        memset(bits.p, 0, words * sizeof(uint32_t));
        bits[words - 1] = pad, *free_rows = n_rows;
        frc_mark_pool(m);
    } else {
        hipStream_t s = ctx->setup_stream;
        hipError_t he = hipMemsetAsync(bits.p, 0, words * sizeof(uint32_t), s);
        if (he == hipSuccess && pad) he = hipMemcpyAsync(bits.p + words - 1, &pad, sizeof(pad), hipMemcpyHostToDevice, s);
        if (he == hipSuccess) he = hipMemcpyAsync(free_rows.p, &n_rows, sizeof(n_rows), hipMemcpyHostToDevice, s);
        m.max_blocks = key_grid_cap(ctx, 4);
        const int e = he == hipSuccess ? fr_keyadmit_mark_launch(&m, (void *)s) : (int)he;
        const hipError_t se = hipStreamSynchronize(s);   // (before `bits`, `pad` and `n_rows` leave)
        if (e) FR_FAIL(FR_ERR_HIP, "the row pool's mark launch failed: %s", hipGetErrorString((hipError_t)e));
        FR_HIP(se);
    }
    k.pool_first = first_row, k.pool_rows = n_rows;
    k.pool_bits.swap(bits), k.pool_free.swap(free_rows);   // (no worker has work in flight: the old bitmap is released with `bits`)
    return FR_OK;
}

extern "C" int fr_ctx_row_pool(fr_ctx *ctx, int col, int32_t *first_row, int32_t *n_rows, int64_t *free_rows) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    FR_TRY(key_col_check(ctx, col, "fr_ctx_row_pool"));
    const fr_ctx::KeySpace none{};
    const fr_ctx::KeySpace &k = ctx->key_spaces.empty() ? none : ctx->key_spaces[(size_t)col];
    int32_t n = 0;
    if (k.pool_rows > 0) FR_TRY(key_read_word(ctx, k.pool_free.p, &n));
    if (first_row) *first_row = k.pool_first;
    if (n_rows) *n_rows = k.pool_rows;
    if (free_rows) *free_rows = (int64_t)n;
    return FR_OK;
}

static FrKeyAdmitArgs key_admit_args(fr_ctx *c, int col, int n, const int64_t *keys, int32_t *rows, int *err) {
    FrKeyAdmitArgs a{};
    a.col = c->h_key_cols[(size_t)col], a.pool = key_pool_of(c, col), a.n_keys = c->d_key_counts + col, a.max_keys = (uint32_t)c->key_spaces[(size_t)col].max_keys;
    a.n = n, a.keys = keys, a.rows_out = rows, a.err_flag = err;
    return a;
}

// The launches of one admit on stream s: per piece of at most 2^20 keys the piece's own table is filled (key_fill_kernel), keyadmit_admit_kernel elects
// one occurrence of every key and admits it, keyadmit_settle_kernel hands its row to the others.  A key listed in two pieces is live by the second.
static int key_admit_enqueue(fr_ctx *c, int col, int n, const int64_t *keys, int32_t *rows, int *err, FrBuf<FrKeySlot> &tab, hipStream_t s) {
    constexpr int PIECE = 1 << 20;
    FR_TRY(tab.grow(FrMem::DEVICE, (size_t)fr_key_slots((uint64_t)(n < PIECE ? n : PIECE)), "key-admit table"));
    for (int at = 0; at < n; at += PIECE) {
        const int m = n - at < PIECE ? n - at : PIECE;
        const uint64_t slots = fr_key_slots((uint64_t)m);
        const FrKeyFillArgs f{tab.p, slots, FR_KEYS_NO_ROW};
        int e = fr_key_fill_launch(&f, (void *)s);
        FrKeyAdmitArgs a = key_admit_args(c, col, m, keys + at, rows + at, err);
        a.tab = tab.p, a.tab_mask = (uint32_t)(slots - 1);
        if (!e) e = fr_keyadmit_admit_launch(&a, (void *)s);
        if (!e) e = fr_keyadmit_settle_launch(&a, (void *)s);
        if (e) FR_FAIL(FR_ERR_HIP, "the key admit launch failed: %s", hipGetErrorString((hipError_t)e));
    }
    return FR_OK;
}

// One list-form change of a MAPPED column's map -- put, erase, admit -- as its worker form and its context form share it
struct KeyOp {
    enum Kind { PUT, ERASE, ADMIT } kind;
    const char *verb;          // "put" / "erase" / "admit", as the texts name it
    int col, n;
    const int64_t *keys;
    const int32_t *rows;       // PUT: the rows, read
    int32_t *rows_out;         // ADMIT: the rows, written
};

// side: 'd' (a worker's device lists) or 'h' (a context's host lists); n == 0 passes whatever the pointers are
static int key_op_check(fr_ctx *c, const KeyOp &o, char side, const char *who) {
    const void *rows = o.kind == KeyOp::PUT ? (const void *)o.rows : (const void *)o.rows_out;
    const char *rows_name = o.kind == KeyOp::PUT ? "rows" : "rows_out";
    const bool listed = o.kind != KeyOp::ERASE;   // the call takes a rows list
    FR_TRY(key_col_check(c, o.col, who));
    if (o.n < 0) FR_FAIL(FR_ERR_INVALID, "%s: n = %d %s", who, o.n, listed ? "pairs" : "keys");
    if (o.n > 0 && (!o.keys || (listed && !rows))) FR_FAIL(FR_ERR_INVALID, listed ? "%s: keys / rows is NULL" : "%s: keys is NULL", who);
    FR_TRY(key_col_mapped(c, o.col, who));
    if (o.kind == KeyOp::ADMIT && c->key_spaces[(size_t)o.col].pool_rows <= 0)
        FR_FAIL(FR_ERR_STATE, "%s: column %d has no row pool: call fr_ctx_set_row_pool(ctx, %d, first_row, n_rows) first", who, o.col, o.col);
    if (o.n == 0) return FR_OK;
    if (!listed && (uintptr_t)o.keys % 8) FR_FAIL(FR_ERR_INVALID, "%s: %c_keys must be 8-byte aligned", who, side);
    if (listed && ((uintptr_t)o.keys % 8 || (uintptr_t)rows % 4)) FR_FAIL(FR_ERR_INVALID, "%s: %c_keys must be 8-byte aligned, %c_%s 4-byte aligned", who, side, side, rows_name);
    return FR_OK;
}

// -> the twin's FR_KEYS_ERR_* bits (the CPU back-end; the callers hold lp_mutex)
static int key_op_cpu(fr_ctx *c, const KeyOp &o) {
    if (o.kind == KeyOp::PUT) return frc_put_keys(key_put_args(c, o.col, o.n, o.keys, o.rows, nullptr));
    if (o.kind == KeyOp::ERASE) return key_erase_run(c, o.col, o.n, o.keys, nullptr, nullptr);
    return frc_admit_keys(key_admit_args(c, o.col, o.n, o.keys, o.rows_out, nullptr));
}

// the launches of o (device lists) on stream s; what cannot be applied is marked in *err
static int key_op_enqueue(fr_ctx *c, const KeyOp &o, int *err, FrBuf<FrKeySlot> &tab, hipStream_t s) {
    if (o.kind == KeyOp::ADMIT) return key_admit_enqueue(c, o.col, o.n, o.keys, o.rows_out, err, tab, s);
    int e;
    if (o.kind == KeyOp::PUT) {
        const FrKeyPutArgs a = key_put_args(c, o.col, o.n, o.keys, o.rows, err);
        e = fr_key_put_launch(&a, (void *)s);
    } else {
        e = key_erase_run(c, o.col, o.n, o.keys, err, s);
    }
    if (e) FR_FAIL(FR_ERR_HIP, "the key %s launch failed: %s", o.verb, hipGetErrorString((hipError_t)e));
    return FR_OK;
}

// asynchronous on the worker's stream, ordered against its batches; what was not applied waits for fr_worker_sync
static int worker_key_op(fr_worker *w, const KeyOp &o, const char *who) {
    if (!w) FR_FAIL(FR_ERR_INVALID, "worker is NULL");
    fr_ctx *c = w->ctx;
    FR_TRY(key_op_check(c, o, 'd', who));
    if (o.n == 0) return FR_OK;
    FR_TRY(fr_host_fed_queued(w, o.verb));
    if (c->cpu) {   // computed before the call returns, one writer at a time; what was not applied waits in c_err for fr_worker_sync
        std::lock_guard<std::mutex> lk(c->lp_mutex);
        const int bad = key_op_cpu(c, o);
        if (bad) __atomic_fetch_or(&w->c_err, bad, __ATOMIC_ACQ_REL);
        return FR_OK;
    }
    FR_SET_DEVICE(c);
    FR_TRY(fr_fused_flush(w));   // batches queued for a fused launch were pushed BEFORE the change: whatever they read was resolved against the old map
    FR_TRY(key_op_enqueue(c, o, w->d_err, w->d_admit_tab, w->stream));
    w->in_flight = true;
    return FR_OK;
}

// synchronous on the set-up stream, legal beside workers in flight; what was not applied is this call's FR_ERR_INDEX_RANGE
static int ctx_key_op(fr_ctx *ctx, KeyOp o, const char *who) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    FR_TRY(key_op_check(ctx, o, 'h', who));
    if (o.n == 0) return FR_OK;
    std::lock_guard<std::mutex> lk(ctx->lp_mutex);   // one writer at a time; the set-up stream, the staging and the status word are fr_ctx_update_rows's too
    if (ctx->cpu) {
        const int bad = key_op_cpu(ctx, o);
        return bad ? fr_index_range_fail(bad) : FR_OK;
    }
    FR_SET_DEVICE(ctx);
    FR_TRY(fr_up_err_ensure(ctx));
    const size_t n = (size_t)o.n;
    FR_TRY(ctx->d_kp_keys.grow(FrMem::DEVICE, n, "key-put keys"));
    if (o.kind != KeyOp::ERASE) FR_TRY(ctx->d_kp_rows.grow(FrMem::DEVICE, n, "key-put rows"));
    FR_HIP(hipMemcpyAsync(ctx->d_kp_keys, o.keys, n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->setup_stream));
    if (o.kind == KeyOp::PUT) FR_HIP(hipMemcpyAsync(ctx->d_kp_rows, o.rows, n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->setup_stream));
    int32_t *const h_rows_out = o.rows_out;
    o.keys = ctx->d_kp_keys, o.rows = o.rows_out = ctx->d_kp_rows;
    const int rc = key_op_enqueue(ctx, o, ctx->d_up_err, ctx->d_ka_tab, ctx->setup_stream);
    FR_HIP(hipStreamSynchronize(ctx->setup_stream));
    if (rc) return rc;
    if (o.kind == KeyOp::ADMIT) FR_HIP(hipMemcpy(h_rows_out, ctx->d_kp_rows, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    const int bad = fr_up_err_take(ctx);
    return bad ? fr_index_range_fail(bad) : FR_OK;
}

extern "C" int fr_worker_put_keys(fr_worker *w, int col, int n, const int64_t *d_keys, const int32_t *d_rows) {
    return worker_key_op(w, KeyOp{KeyOp::PUT, "put", col, n, d_keys, d_rows, nullptr}, "fr_worker_put_keys");
}
extern "C" int fr_ctx_put_keys(fr_ctx *ctx, int col, int n, const int64_t *h_keys, const int32_t *h_rows) {
    return ctx_key_op(ctx, KeyOp{KeyOp::PUT, "put", col, n, h_keys, h_rows, nullptr}, "fr_ctx_put_keys");
}
extern "C" int fr_worker_erase_keys(fr_worker *w, int col, int n, const int64_t *d_keys) {
    return worker_key_op(w, KeyOp{KeyOp::ERASE, "erase", col, n, d_keys, nullptr, nullptr}, "fr_worker_erase_keys");
}
extern "C" int fr_ctx_erase_keys(fr_ctx *ctx, int col, int n, const int64_t *h_keys) {
    return ctx_key_op(ctx, KeyOp{KeyOp::ERASE, "erase", col, n, h_keys, nullptr, nullptr}, "fr_ctx_erase_keys");
}
extern "C" int fr_worker_admit_keys(fr_worker *w, int col, int n, const int64_t *d_keys, int32_t *d_rows_out) {
    return worker_key_op(w, KeyOp{KeyOp::ADMIT, "admit", col, n, d_keys, nullptr, d_rows_out}, "fr_worker_admit_keys");
}
extern "C" int fr_ctx_admit_keys(fr_ctx *ctx, int col, int n, const int64_t *h_keys, int32_t *h_rows_out) {
    return ctx_key_op(ctx, KeyOp{KeyOp::ADMIT, "admit", col, n, h_keys, nullptr, h_rows_out}, "fr_ctx_admit_keys");
}

// The word -> column tables of the six forms ([rows_kind][pooled]) for the pooling and the split as they stand, made again when either has changed
// since they were made (both change only while no worker has work in flight, so no launch reads the tables being replaced).  Under key_mutex.
static int key_tables_ensure(fr_ctx *c) {
    if (c->key_tab_made && c->key_tab_hots == c->pool_hots && c->key_tab_shared == c->req_shared) return FR_OK;
    const size_t C = idx_cols(c);
    const bool pool = c->pool_cols > 0, split = !c->req_shared.empty();
    std::vector<uint16_t> all;
    fr_ctx::KeyTable tab[3][2];
    for (int kind = FR_KEY_ROWS_FULL; kind <= FR_KEY_ROWS_CANDIDATE; kind++)
        for (int pooled = 0; pooled < 2; pooled++) {
            if ((pooled && !pool) || (kind != FR_KEY_ROWS_FULL && !split)) continue;
            tab[kind][pooled].first = all.size();
            for (size_t col = 0; col < C; col++) {
                if (kind != FR_KEY_ROWS_FULL && (c->req_shared[col] != 0) != (kind == FR_KEY_ROWS_REQUEST)) continue;
                all.insert(all.end(), pooled ? (size_t)c->pool_hots[col] : 1, (uint16_t)col);
            }
            tab[kind][pooled].words = (int)(all.size() - tab[kind][pooled].first);
        }
    FrBuf<uint16_t> d;
    FR_TRY(d.alloc(fr_mem_kind(c, FrMem::DEVICE), all.size() ? all.size() : 1, "key word tables"));
    if (c->cpu) memcpy(d.p, all.data(), all.size() * sizeof(uint16_t));
    else if (!all.empty()) FR_HIP(hipMemcpy(d.p, all.data(), all.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    c->d_key_wcol.swap(d);
    memcpy(c->key_tab, tab, sizeof(tab));
    c->key_tab_hots = c->pool_hots, c->key_tab_shared = c->req_shared, c->key_tab_made = true;
    return FR_OK;
}

// the one launch (the CPU back-end: the twin, computed here)
int fr_key_resolve_enqueue(fr_worker *w, int n_rows, int rows_kind, int pooled, const int64_t *keys, int32_t *out, const char *who) {
    fr_ctx *c = w->ctx;
    FR_TRY(fr_key_unsharded(c, who));
    if (rows_kind != FR_KEY_ROWS_FULL && c->req_shared.empty()) FR_FAIL(FR_ERR_STATE, "%s: request and candidate rows need a split: call fr_ctx_set_request_columns first", who);
    if (pooled && c->pool_cols <= 0) FR_FAIL(FR_ERR_STATE, "%s: the pooled forms need pooling: call fr_ctx_set_pooling first", who);
    if (!c->cpu) FR_SET_DEVICE(c);
    FrKeyResolveArgs a{};
    {
        std::lock_guard<std::mutex> lk(c->key_mutex);
        FR_TRY(key_spaces_init(c));
        FR_TRY(key_tables_ensure(c));
        const fr_ctx::KeyTable &t = c->key_tab[rows_kind][pooled];
        a.W = t.words, a.wcol = c->d_key_wcol + t.first;
    }
    if (a.W <= 0) FR_FAIL(FR_ERR_STATE, "%s: the split leaves no word to this side of the form", who);
    const uint64_t bound = (uint64_t)4000 << 20;
    a.total = (uint64_t)n_rows * (uint64_t)a.W;
    if (a.total * sizeof(int64_t) >= bound) FR_FAIL(FR_ERR_INVALID, "%s: %d rows of %d keys reach 4000 MiB", who, n_rows, a.W);
    if (!w->d_key_miss) {   // the worker's first resolve
        FR_TRY(w->d_key_miss.alloc(fr_mem_kind(c, FrMem::DEVICE), 1, "worker key misses"));
        if (c->cpu) *w->d_key_miss = 0;
        else FR_HIP(hipMemsetAsync(w->d_key_miss, 0, sizeof(unsigned long long), w->stream));   // in front of the launch, in stream order
    }
    a.keys = keys, a.out = out, a.misses = w->d_key_miss, a.n_cols = (int)idx_cols(c);
    if (c->cpu) {
        a.cols = c->h_key_cols.data();
        frc_resolve_keys(a);
        return FR_OK;
    }
    a.cols = c->d_key_cols, a.max_blocks = key_grid_cap(c, 8);
    const int e = fr_key_resolve_launch(&a, (void *)w->stream);
    if (e) FR_FAIL(FR_ERR_HIP, "the key resolve launch failed: %s", hipGetErrorString((hipError_t)e));
    w->in_flight = true;
    return FR_OK;
}

extern "C" int fr_worker_resolve_keys_device(fr_worker *w, int n_rows, int rows_kind, int pooled, const int64_t *d_keys, int32_t *d_idx_out) {
    if (!w) FR_FAIL(FR_ERR_INVALID, "worker is NULL");
    if (rows_kind < FR_KEY_ROWS_FULL || rows_kind > FR_KEY_ROWS_CANDIDATE) FR_FAIL(FR_ERR_INVALID, "rows_kind %d is none of FR_KEY_ROWS_FULL, _REQUEST, _CANDIDATE", rows_kind);
    if (pooled != 0 && pooled != 1) FR_FAIL(FR_ERR_INVALID, "pooled = %d is neither 0 nor 1", pooled);
    const int most = rows_kind == FR_KEY_ROWS_REQUEST ? (1 << 24) : w->max_batch;
    if (n_rows < 1 || n_rows > most) FR_FAIL(FR_ERR_INVALID, "n_rows = %d outside [1, %d]", n_rows, most);
    if (!d_keys || !d_idx_out) FR_FAIL(FR_ERR_INVALID, "d_keys / d_idx_out is NULL");
    if ((uintptr_t)d_keys % 8 || (uintptr_t)d_idx_out % 4) FR_FAIL(FR_ERR_INVALID, "d_keys must be 8-byte aligned, d_idx_out 4-byte aligned");
    return fr_key_resolve_enqueue(w, n_rows, rows_kind, pooled, d_keys, d_idx_out, "fr_worker_resolve_keys_device");
}

extern "C" int64_t *fr_worker_key_ptr(fr_worker *w) { return w ? w->h_keys.p : nullptr; }

extern "C" int fr_worker_key_misses(fr_worker *w, uint64_t *misses, int reset) {
    if (!w || !misses) FR_FAIL(FR_ERR_INVALID, "NULL argument");
    *misses = 0;
    if (!w->d_key_miss) return FR_OK;   // the worker has resolved nothing yet
    if (w->ctx->cpu) {
        *misses = reset ? __atomic_exchange_n(w->d_key_miss.p, 0ull, __ATOMIC_ACQ_REL) : __atomic_load_n(w->d_key_miss.p, __ATOMIC_ACQUIRE);
        return FR_OK;
    }
    FR_SET_DEVICE(w->ctx);
    FR_HIP(hipStreamSynchronize(w->stream));
    unsigned long long v = 0;
    FR_HIP(hipMemcpy(&v, w->d_key_miss, sizeof(v), hipMemcpyDeviceToHost));
    if (reset) {
        FR_HIP(hipMemsetAsync(w->d_key_miss, 0, sizeof(v), w->stream));
        FR_HIP(hipStreamSynchronize(w->stream));
    }
    *misses = (uint64_t)v;
    return FR_OK;
}
