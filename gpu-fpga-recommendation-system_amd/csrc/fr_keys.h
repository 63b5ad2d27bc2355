// Keyed lookups (fleetrec_serving.h, "Keyed lookups"): ONE definition of the slot layout, of mix64 and of the probe rule, included by the kernels
// (fr_keys.hip -> libfleetrec_keys.so, the third companion code object; fr_keymaint.hip -> libfleetrec_keymaint.so, the fifth; fr_keyadmit.hip ->
// libfleetrec_admit.so, the sixth), by the CPU back-end (fr_cpu.cpp) and, through fr_internal.h, by the host
// side.  Everything here is plain data or an inline function; nothing is a symbol of any library.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define FR_KEYS_HD static inline __host__ __device__
#else
#define FR_KEYS_HD static inline
#endif

constexpr int64_t FR_KEYS_EMPTY_KEY = -1;           // FR_KEY_EMPTY: the empty slot of a bag, and the key of an empty map slot; never a map key
constexpr int32_t FR_KEYS_NO_ROW = 0x7fffffff;      // FR_KEY_NO_ROW: out of range for every gather
constexpr int FR_KEYS_MODE_ROWS = 0, FR_KEYS_MODE_HASHED = 1, FR_KEYS_MODE_MAPPED = 2;   // FR_KEYS_ROWS / _HASHED / _MAPPED
constexpr int FR_KEYS_LDS_WORDS = 2048;             // words of the word -> column table a workgroup stages in LDS (4 KiB); a longer row: read in place
constexpr int FR_KEYS_LDS_COLS = 384;               // column records a workgroup of key_resolve_kernel stages in LDS (12 KiB); more: read in place
// what a put raises in the status word it is given (bit 0 stays the lookups' own "index outside its table")
constexpr int FR_KEYS_ERR_EMPTY_KEY = 2, FR_KEYS_ERR_ROW = 4, FR_KEYS_ERR_FULL = 8;
constexpr int FR_KEYS_ERR_ERASE_EMPTY = 16;         // what an erase raises there: a key of -1 in its list
// what an admit raises there: its own case (the pool has no free row), and, beside that bit or FR_KEYS_ERR_EMPTY_KEY / _FULL, the mark that the
// call was an admit and not a put (fr_worker_sync words its message by it)
constexpr int FR_KEYS_ERR_NO_FREE_ROW = 32, FR_KEYS_ERR_ADMIT = 64;

struct FrKeySlot {   // 16 bytes, 16-byte aligned: one probe is one load
    int64_t key;     // FR_KEYS_EMPTY_KEY: nobody has claimed the slot
    int32_t row;     // an empty slot holds the column's miss_row, so a reader that sees a key claimed and its row not yet stored reads "unknown"
    int32_t pad;
};

struct FrKeyCol {    // 32 bytes: what a resolve needs of one index column
    uint64_t seed;
    FrKeySlot *slots;    // MAPPED: the map (device memory; host memory on the CPU back-end); NULL otherwise
    uint32_t mask;       // slots - 1, slots a power of two <= 2^31
    uint32_t range;      // R_c: the row count the one-hot gather checks for the column
    int32_t miss_row;
    int32_t mode;
};

// the splitmix64 finaliser: mix64(5) = 13168350753275463132, mix64(4) = 13232826040865663252
FR_KEYS_HD uint64_t fr_mix64(uint64_t z) {
    z ^= z >> 30;
    z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 27;
    z *= 0x94d049bb133111ebull;
    z ^= z >> 31;
    return z;
}

// the smallest power of two >= 2 * max_keys (max_keys in 1 .. 2^30): the load of a map never exceeds 0.5, so a probe chain always ends
FR_KEYS_HD uint64_t fr_key_slots(uint64_t max_keys) {
    uint64_t s = 2;
    while (s < 2 * max_keys) s <<= 1;
    return s;
}

FR_KEYS_HD uint64_t fr_key_home(const FrKeyCol &c, int64_t k) { return fr_mix64((uint64_t)k ^ c.seed) & (uint64_t)c.mask; }

// The modes without a table, and the empty key of every mode.  -> true: *row is the answer; false: the key has to be looked up in the column's map.
FR_KEYS_HD bool fr_key_direct(const FrKeyCol &c, int64_t k, int32_t *row) {
    if (k == FR_KEYS_EMPTY_KEY) {
        *row = -1;
        return true;
    }
    if (c.mode == FR_KEYS_MODE_MAPPED) return false;
    if (c.mode == FR_KEYS_MODE_HASHED) *row = (int32_t)(uint32_t)(((fr_mix64((uint64_t)k ^ c.seed) >> 32) * (uint64_t)c.range) >> 32);   // < range <= 2^31 - 1
    else *row = (uint64_t)k < 0x7fffffffull ? (int32_t)k : FR_KEYS_NO_ROW;
    return true;
}

// One probe: the slot as ONE 16-byte load on the device (a reader sees a claimed key with either its old or its new row, never half a slot); the
// CPU back-end reads the key, then the row.
FR_KEYS_HD FrKeySlot fr_key_load_slot(const FrKeySlot *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int4 v = *reinterpret_cast<const int4 *>(p);
    FrKeySlot s;
    s.key = (int64_t)(((uint64_t)(uint32_t)v.y << 32) | (uint64_t)(uint32_t)v.x), s.row = v.z, s.pad = 0;
    return s;
#else
    FrKeySlot s;
    s.key = __atomic_load_n(&p->key, __ATOMIC_ACQUIRE), s.row = __atomic_load_n(&p->row, __ATOMIC_RELAXED), s.pad = 0;
    return s;
#endif
}

// The probe rule: from the home slot h (whose content `s` the caller has loaded already) linearly, wrapping, until the key or an empty slot is
// found.  At most `slots` probes WHATEVER the memory holds: a corrupt map may give a wrong row, it cannot spin.  *miss: no slot holds the key.
FR_KEYS_HD int32_t fr_key_probe(const FrKeyCol &c, int64_t k, uint64_t h, FrKeySlot s, bool *miss) {
    *miss = false;
    for (uint64_t left = (uint64_t)c.mask;; left--) {   // the slot in hand + mask more = slots probes
        if (s.key == k) return s.row;
        if (s.key == FR_KEYS_EMPTY_KEY || left == 0) break;
        h = (h + 1) & (uint64_t)c.mask;
        s = fr_key_load_slot(c.slots + h);
    }
    *miss = true;
    return c.miss_row;
}

// a whole lookup (the CPU back-end; the kernel issues its first probes early and finishes with fr_key_probe)
FR_KEYS_HD int32_t fr_key_resolve(const FrKeyCol &c, int64_t k, bool *miss) {
    int32_t row;
    *miss = false;
    if (fr_key_direct(c, k, &row)) return row;
    const uint64_t h = fr_key_home(c, k);
    return fr_key_probe(c, k, h, fr_key_load_slot(c.slots + h), miss);
}

// a row a put may store: one of the column's rows, or the column's own miss_row (which "forgets" the key)
FR_KEYS_HD bool fr_key_row_legal(uint32_t range, int32_t miss_row, int32_t row) { return row == miss_row || (row >= 0 && (uint32_t)row < range); }

// ---- the life cycle of a map (fr_*_erase_keys, fr_ctx_key_space_stats, fr_ctx_export_keys, fr_ctx_rebuild_key_space; fr_keymaint.hip and the CPU twins) ----
// A slot is OCCUPIED when it holds a key, DEAD when it is occupied and its row is the column's miss_row (an erased or "forgotten" key -- or a key put
// on purpose with a row equal to a miss_row that is a real row), LIVE when it is occupied and not dead.
FR_KEYS_HD bool fr_key_slot_occupied(const FrKeySlot &s) { return s.key != FR_KEYS_EMPTY_KEY; }
FR_KEYS_HD bool fr_key_slot_dead(const FrKeySlot &s, int32_t miss_row) { return s.key != FR_KEYS_EMPTY_KEY && s.row == miss_row; }
FR_KEYS_HD bool fr_key_slot_live(const FrKeySlot &s, int32_t miss_row) { return s.key != FR_KEYS_EMPTY_KEY && s.row != miss_row; }

// how far from its home slot the key of slot `at` sits (wrapping): 1 + the sum over the occupied slots / their number = the mean probes of a present key
FR_KEYS_HD uint64_t fr_key_displacement(const FrKeyCol &c, int64_t k, uint64_t at) { return (at - fr_key_home(c, k)) & (uint64_t)c.mask; }

// fr_key_probe's walk, returning WHERE the key sits: -> the slot index, or -1 when no slot holds the key.  At most `slots` probes whatever the memory holds.
FR_KEYS_HD int64_t fr_key_find(const FrKeyCol &c, int64_t k) {
    uint64_t h = fr_key_home(c, k);
    for (uint64_t left = (uint64_t)c.mask;; left--) {   // the home slot + mask more = slots probes
        const FrKeySlot s = fr_key_load_slot(c.slots + h);
        if (s.key == k) return (int64_t)h;
        if (s.key == FR_KEYS_EMPTY_KEY || left == 0) break;
        h = (h + 1) & (uint64_t)c.mask;
    }
    return -1;
}

// ---- row pools (fr_ctx_set_row_pool / fr_*_admit_keys; fr_keyadmit.hip and the CPU twins) ----
// The pool of a MAPPED column: the rows [first_row, first_row + n_rows), one bit per row (set = taken) in 32-bit words, and ONE counter of free rows.
// The pad bits past n_rows in the last word are set for good, so no scan hands them out.  The counter is signed: a taker subtracts first and gives
// back what went below zero.
struct FrKeyPool {
    uint32_t *bits;        // [fr_key_pool_words(n_rows)]
    int32_t *free_rows;    // = the clear bits, whenever no admit or erase is in flight
    int32_t first_row;
    int32_t n_rows;        // 0: the column has no pool
};

FR_KEYS_HD uint32_t fr_key_pool_words(int32_t n_rows) { return ((uint32_t)n_rows + 31u) >> 5; }
FR_KEYS_HD bool fr_key_pool_holds(const FrKeyPool &p, int32_t row) { return row >= p.first_row && row - p.first_row < p.n_rows; }   // (first_row + n_rows <= 2^31 - 1)
// the pad bits of the last word (0 when n_rows is a multiple of 32)
FR_KEYS_HD uint32_t fr_key_pool_pad(int32_t n_rows) { return ((uint32_t)n_rows & 31u) ? ~0u << ((uint32_t)n_rows & 31u) : 0u; }
