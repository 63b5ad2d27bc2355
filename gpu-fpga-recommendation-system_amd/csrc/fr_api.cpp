// Host side of the C-ABI (include/fleetrec.h): context = device + model + tables + weights,
// worker = stream + staging buffers, submit/sync = the hot-loop body of the reference's
// thread_consume() (GPU/final_network_cublasLt_1_node_no_FIFO_scatter/cuda_server.c:101-503) with
// the FPGA embedding stage (FPGA/kernel/user_krnl/embedding_*_krnl) pulled in front of the FC chain.
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "fr_internal.h"

// ---- errors -------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

void fr_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

#ifdef FR_EXPERIMENTS
int fr_knob_env(const char *name, int dflt) {  // experiments build only: the product library reads no environment variable
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}
#endif

static thread_local char g_kernel[96] = "";
void fr_note_kernel(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_kernel, sizeof(g_kernel), fmt, ap);
    va_end(ap);
}
const char *fr_noted_kernel() { return g_kernel; }
static void keep_kernel(fr_worker *w) { snprintf(w->last_kernel, sizeof(w->last_kernel), "%s", g_kernel); }
extern "C" const char *fr_worker_last_kernel(const fr_worker *w) { return w ? w->last_kernel : ""; }

extern "C" const char *fr_last_error(void) { return g_err; }
extern "C" int fr_abi_version(void) { return FR_ABI_VERSION; }

extern "C" int fr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

extern "C" int fr_cpu_set_threads(int n) {
    if (n < 0) FR_FAIL(FR_ERR_INVALID, "fr_cpu_set_threads(%d): n >= 1, or 0 for every usable core", n);
    return frc_set_threads(n);
}

static int select_device(int device) {
    int n = fr_device_count();
    if (n <= 0) FR_FAIL(FR_ERR_NO_DEVICE, "no HIP device visible (device >= 0 never falls back to the CPU; device = -1 asks for the CPU back-end)");
    if (device < 0 || device >= n) FR_FAIL(FR_ERR_NO_DEVICE, "device %d not available (%d visible)", device, n);
    hipDeviceProp_t prop;
    FR_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        FR_FAIL(FR_ERR_NO_DEVICE, "device %d is %s; this library carries gfx950 (MI355X) code objects only", device, prop.gcnArchName);
    FR_HIP(hipSetDevice(device));
    return FR_OK;
}

static unsigned long long *g_stamp_buffer = nullptr;  // diagnostics (tools/experiments): see fr_debug_set_stamp_buffer
extern "C" __attribute__((visibility("default"))) void fr_debug_set_stamp_buffer(void *dptr) { g_stamp_buffer = (unsigned long long *)dptr; }

static int fused_group_initial();
static bool fused_eligible(const fr_ctx *c);
static bool lp_image_applies_hs(const fr_ctx *c);
static int lp_ensure_image(fr_ctx *c, int prec);
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline int round_up(int v, int a) { return (v + a - 1) / a * a; }

// ---- memory (fr_mem.h): the one place that allocates and releases, and the tally of what is live -------------------------------------------
static std::atomic<uint64_t> g_live_bytes[2];   // [0] device, [1] host
static inline std::atomic<uint64_t> &live_of(FrMem kind) { return g_live_bytes[kind == FrMem::DEVICE ? 0 : 1]; }
void fr_mem_live_bytes(uint64_t out[2]) {
    for (int i = 0; i < 2; i++) out[i] = g_live_bytes[i].load(std::memory_order_relaxed);
}
#ifdef FR_EXPERIMENTS
extern "C" __attribute__((visibility("default"))) void fr_exp_live_bytes(uint64_t out[2]) { fr_mem_live_bytes(out); }   // experiments build only (no header)
#endif

int fr_mem_alloc(FrMem kind, size_t bytes, const char *what, void **out) {
    *out = nullptr;
    if (kind == FrMem::ARENA) {
        if (!(*out = frc_arena_alloc(bytes))) return FR_ERR_OOM;   // (it has said why)
    } else if (kind == FrMem::HOST) {
        if (!(*out = aligned_alloc(64, align_up(bytes ? bytes : 64, 64)))) FR_FAIL(FR_ERR_OOM, "out of host memory (%s, %zu bytes)", what, bytes);
    } else {
        const hipError_t e = kind == FrMem::DEVICE ? hipMalloc(out, bytes) : hipHostMalloc(out, bytes, kind == FrMem::PINNED_MAPPED ? hipHostMallocMapped : hipHostMallocDefault);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            *out = nullptr;
            FR_FAIL(e == hipErrorOutOfMemory ? FR_ERR_OOM : FR_ERR_HIP, "%s(%s, %zu bytes) failed: %s", kind == FrMem::DEVICE ? "hipMalloc" : "hipHostMalloc", what, bytes, hipGetErrorString(e));
        }
    }
    if (*out) live_of(kind).fetch_add(bytes, std::memory_order_relaxed);
    return FR_OK;
}

void fr_mem_release(FrMem kind, void *p, size_t bytes) {
    if (!p) return;
    if (kind == FrMem::ARENA) frc_arena_free(p, bytes);
    else if (kind == FrMem::HOST) free(p);
    else if (kind == FrMem::DEVICE) (void)hipFree(p);
    else (void)hipHostFree(p);
    live_of(kind).fetch_sub(bytes, std::memory_order_relaxed);
}

// ---- context --------------------------------------------------------------------------------------
static void ctx_free(fr_ctx *c) {   // every buffer is released by its holder (fr_mem.h)
    if (!c) return;
    if (!c->cpu && c->device >= 0) (void)hipSetDevice(c->device);
    if (c->setup_stream) (void)hipStreamDestroy(c->setup_stream);
    delete c;
}

// Contiguous, float-balanced split of the record's segments over n_shards (SURVEY section 8(e):
// "partition tables by table-ID ... balancing floats-per-item ... slices are whole segments").
void fr_shard_bounds(const fr_model_desc &m, int n_shards, std::vector<int> &seg_begin) {
    seg_begin.assign(n_shards + 1, m.n_segments);
    seg_begin[0] = 0;
    int s = 0;
    for (int g = 1; g < n_shards; g++) {
        const double target = (double)m.record_len * g / n_shards;
        // advance while the end of segment s is closer to (or before) the target than its start
        while (s < m.n_segments && m.segments[s].rec_offset + m.segments[s].len / 2.0 <= target) s++;
        // a COPY segment must stay with the table segment it duplicates only for locality, not correctness
        // at least one segment per shard: past the previous shard's first segment (two targets may fall inside one wide segment), and
        // leaving one for every shard still to come
        if (s <= seg_begin[g - 1]) s = seg_begin[g - 1] + 1;
        if (s > m.n_segments - (n_shards - g)) s = m.n_segments - (n_shards - g);
        seg_begin[g] = s;
    }
}

// XCD partition of the record words for gather_pack_xcd_kernel (FrGatherGroups): 8 contiguous runs of words cut on SOURCE-ROW
// boundaries, balanced by a cost per word run.  An "atom" is a maximal run of consecutive record words that one item reads from ONE
// source row -- a table row, a whole bank row in a bank-interleaved context (one contiguous 112-256-byte fetch), 128 bytes of the
// dense block.  Cutting inside an atom makes two XCDs fetch the same 128-byte line through two L2s: with Model-C's 992 words dealt
// 124 per group, 6 of the 7 cuts split a bank row -- 6 extra lines on 142 per item.  Cost of an atom = the bytes it writes + the
// 128-byte lines it fetches, weighted by where its table lives (FR_GATHER_COST = "write,l2,cache,hbm" weights; tables up to 2 MiB
// per XCD group are taken as L2-resident, up to 64 MiB as Infinity-Cache-resident); a linear-partition DP minimises the costliest
// group, then the sum of squares.  Groups wider than 256 words (the kernel's block) leave max_words = 0: the launcher then deals
// n_words / 8 words per group as before.
static void plan_gather_groups(fr_ctx *c) {
    FrGatherGroups &gg = c->gather_groups;
    gg = FrGatherGroups{};
    const int n = c->n_words;
    if (n < 64) return;
    double wt[4] = {1.0, 0.0, 0.0, 0.0};  // write, fetch from L2-class, cache-class, HBM-class tables
#ifdef FR_EXPERIMENTS
    if (const char *e = getenv("FR_GATHER_COST")) sscanf(e, "%lf,%lf,%lf,%lf", &wt[0], &wt[1], &wt[2], &wt[3]);
#endif
    struct Atom { int w0, nw; double cost; };
    std::vector<Atom> atoms;
    auto close_atom = [&](int w0, int w1) {
        const FrWordDesc &d = c->h_words[w0];
        const size_t bytes = (size_t)(w1 - w0) * 16;
        double fetch = 0.0;
        if (!(d.idx_col & FR_DESC_DENSE)) {
            size_t acc = 0;  // expected 128-byte lines per fetched row, over one period of the stride
            for (size_t r = 0; r < 128; r++) acc += ((d.src + r * d.stride) % 128 + bytes + 127) / 128;
            const double lines = (double)acc / 128.0;
            const double footprint = (double)d.rows * d.stride;
            fetch = lines * 128.0 * (footprint <= 2.0 * 1048576 ? wt[1] : footprint <= 64.0 * 1048576 ? wt[2] : wt[3]);
        }
        atoms.push_back(Atom{w0, w1 - w0, wt[0] * (double)bytes + fetch});
    };
    int a0 = 0;
    for (int w = 1; w <= n; w++) {
        bool same = false;
        if (w < n) {
            const FrWordDesc &p = c->h_words[w - 1], &q = c->h_words[w];
            const bool pd = (p.idx_col & FR_DESC_DENSE) != 0, qd = (q.idx_col & FR_DESC_DENSE) != 0;
            if (pd && qd) same = q.src == p.src + 16 && (w - a0) % 8 != 0;
            else if (!pd && !qd) same = p.idx_col == q.idx_col && p.stride == q.stride && (q.src > p.src ? q.src - p.src : p.src - q.src) < p.stride;
        }
        if (!same) {
            close_atom(a0, w);
            a0 = w;
        }
    }
    const int na = (int)atoms.size();
    if (na < 8) return;
    std::vector<double> pc(na + 1, 0.0);
    std::vector<int> pw(na + 1, 0);
    for (int i = 0; i < na; i++) {
        pc[i + 1] = pc[i] + atoms[i].cost;
        pw[i + 1] = pw[i] + atoms[i].nw;
    }
    const double INF = 1e300;
    struct Cell { double mx, sq; int from; };
    std::vector<std::vector<Cell>> dp(9, std::vector<Cell>(na + 1, Cell{INF, INF, -1}));
    dp[0][0] = Cell{0.0, 0.0, -1};
    for (int g = 1; g <= 8; g++)
        for (int i = g; i <= na - (8 - g); i++)
            for (int j = g - 1; j < i; j++) {
                if (dp[g - 1][j].mx >= INF || pw[i] - pw[j] > 256) continue;
                const double cst = pc[i] - pc[j];
                const double mx = dp[g - 1][j].mx > cst ? dp[g - 1][j].mx : cst, sq = dp[g - 1][j].sq + cst * cst;
                Cell &t = dp[g][i];
                if (mx < t.mx * (1.0 - 1e-12) || (mx <= t.mx * (1.0 + 1e-12) && sq < t.sq)) t = Cell{mx, sq, j};
            }
    if (dp[8][na].mx >= INF) return;
    int i = na;
    gg.start[8] = n;
    for (int g = 8; g >= 1; g--) {
        const int j = dp[g][i].from;
        gg.start[g - 1] = atoms[j].w0;
        const int width = gg.start[g] - gg.start[g - 1];
        if (width > gg.max_words) gg.max_words = width;
        i = j;
    }
}

static int build_words(fr_ctx *c) {
    const fr_model_desc &m = c->model;
    std::vector<int> seg_begin;
    int s0 = 0, s1 = m.n_segments;
    if (c->n_shards > 1) {
        fr_shard_bounds(m, c->n_shards, seg_begin);
        s0 = seg_begin[c->shard_rank];
        s1 = seg_begin[c->shard_rank + 1];
        int maxlen = 0;
        c->shard_offset.assign(c->n_shards, 0);
        c->shard_len.assign(c->n_shards, 0);
        for (int g = 0; g < c->n_shards; g++) {
            int b = seg_begin[g], e = seg_begin[g + 1];
            int len = (e > b) ? (m.segments[e - 1].rec_offset + m.segments[e - 1].len - m.segments[b].rec_offset) : 0;
            c->shard_offset[g] = (e > b) ? m.segments[b].rec_offset : 0;
            c->shard_len[g] = len;
            if (len > maxlen) maxlen = len;
        }
        c->slice_offset = m.segments[s0].rec_offset;
        c->slice_len = m.segments[s1 - 1].rec_offset + m.segments[s1 - 1].len - c->slice_offset;
        c->slice_padded = maxlen;
    } else {
        c->slice_offset = 0;
        c->slice_len = m.record_len;
        c->slice_padded = m.record_len;
        c->shard_offset.assign(1, 0);
        c->shard_len.assign(1, m.record_len);
    }
    // which tables are resident on this shard: those referenced by its segments
    for (auto &tm : c->table_mem) tm.resident = false;
    for (int s = s0; s < s1; s++)
        if (m.segments[s].kind != FR_SEG_DENSE) c->table_mem[m.segments[s].src].resident = true;
    // a shard of DENSE segments only holds no table: there is nothing to fill or upload, so it counts as loaded from the start
    bool any_resident = false;
    for (const auto &tm : c->table_mem) any_resident = any_resident || tm.resident;
    if (!any_resident) c->tables_filled = true;
    // arena layout
    c->n_banks = fr_bank_map(m, c->bank_of_table, c->bank_rows);
    size_t off = 0;
    std::vector<char> placed(m.n_tables, 0);
    if (m.index_mode == FR_INDEX_PER_BANK) {
        // Bank-interleaved regions: the resident tables of one bank share "bank rows" -- row r of every table side by side -- for the
        // rows every one of them has (r < min rows = the valid range of the bank's index); one bank costs one contiguous fetch per
        // item.  The bank-row stride is padded when that lowers the expected number of 128-byte lines a row touches (112 -> 128,
        // 224 -> 256 bytes: a fetch beyond L2 costs whole lines, profiles/archive/r01_experiments.md).
        for (int b = 0; b < c->n_banks; b++) {
            std::vector<int> members;
            size_t payload = 0;
            for (int t = 0; t < m.n_tables; t++)
                if (c->bank_of_table[t] == b && c->table_mem[t].resident) {
                    members.push_back(t);
                    payload += (size_t)m.tables[t].dim * 4;
                }
            if (members.size() < 2) continue;  // a lone table is its own bank row already
            auto lines_x128 = [](size_t stride, size_t bytes) {  // expected 128-byte lines per row, x128 (exact over one period)
                size_t acc = 0;
                for (size_t r = 0; r < 128; r++) acc += ((r * stride) % 128 + bytes + 127) / 128;
                return acc;
            };
            size_t best = payload;
            for (size_t cand : {align_up(payload, 32), align_up(payload, 64), align_up(payload, 128)})
                if (lines_x128(cand, payload) < lines_x128(best, payload)) best = cand;
            const uint64_t il_rows = (uint64_t)c->bank_rows[b];
            off = align_up(off, 256);
            size_t col = 0;
            for (int t : members) {
                FrTableMem &tm = c->table_mem[t];
                tm.byte_offset = off + col;
                tm.row_stride = best;
                tm.il_rows = il_rows;
                col += (size_t)m.tables[t].dim * 4;
                placed[t] = 1;
            }
            off = align_up(off + (size_t)il_rows * best, 256);
            for (int t : members) {  // rows beyond the bank's common range: contiguous, reachable only by upload / download / fill
                FrTableMem &tm = c->table_mem[t];
                tm.tail_offset = off;
                off = align_up(off + ((size_t)m.tables[t].rows - (size_t)il_rows) * m.tables[t].dim * 4, 256);
            }
        }
    }
    for (int t = 0; t < m.n_tables; t++) {
        if (!c->table_mem[t].resident || placed[t]) continue;
        c->table_mem[t].byte_offset = off;
        c->table_mem[t].row_stride = (uint64_t)m.tables[t].dim * 4;
        c->table_mem[t].il_rows = 0;
        off = align_up(off + (size_t)m.tables[t].rows * m.tables[t].dim * 4, 256);
    }
    c->table_arena_bytes = off;
    if (off) {
        const int rc = c->table_arena.alloc(c->cpu ? FrMem::ARENA : FrMem::DEVICE, off, "table arena");
        if (rc) return rc;
    }

    // source runs (for the BLOCKED layout)
    int src_start[3] = {0, 0, 0}, src_len[3] = {0, 0, 0};
    for (int s = 0; s < m.n_segments; s++) {
        const fr_segment &g = m.segments[s];
        if (src_len[g.source] == 0) src_start[g.source] = g.rec_offset;
        src_len[g.source] += g.len;
    }
    c->h_words.clear();
    c->h_word_table.clear();
    c->h_word_col.clear();
    for (int s = s0; s < s1; s++) {
        const fr_segment &g = m.segments[s];
        for (int j = 0; j < g.len / 4; j++) {
            FrWordDesc w{};
            c->h_word_table.push_back(g.kind == FR_SEG_DENSE ? -1 : g.src);
            c->h_word_col.push_back(g.src_col + 4 * j);
            if (g.kind == FR_SEG_DENSE) {
                w.src = (uint64_t)(g.src_col + 4 * j) * 4;
                w.stride = (uint32_t)m.dense_len * 4;
                w.idx_col = FR_DESC_DENSE;
                w.rows = 0xFFFFFFFFu;
            } else {
                const fr_table_desc &t = m.tables[g.src];
                w.src = (uint64_t)(uintptr_t)(c->table_arena + c->table_mem[g.src].byte_offset) + (uint64_t)(g.src_col + 4 * j) * 4;
                w.stride = (uint32_t)c->table_mem[g.src].row_stride;
                w.idx_col = m.index_mode == FR_INDEX_PER_TABLE ? (uint32_t)g.src : (m.index_mode == FR_INDEX_PER_BANK ? (uint32_t)c->bank_of_table[g.src] : 0u);
                // PER_BANK: the bank's index addresses every table of the bank, so it must stay below the smallest of them
                w.rows = m.index_mode == FR_INDEX_PER_BANK ? (uint32_t)c->bank_rows[c->bank_of_table[g.src]] : (uint32_t)t.rows;
            }
            const int rec_pos = g.rec_offset + 4 * j;
            if (c->n_shards > 1) {
                w.dst_off = (uint32_t)(rec_pos - c->slice_offset) / 4;
                w.dst_stride = (uint32_t)c->slice_padded / 4;
                w.dst_blk = 0;
            } else if (m.layout == FR_LAYOUT_BLOCKED) {
                w.dst_off = (uint32_t)(rec_pos - src_start[g.source]) / 4;
                w.dst_stride = (uint32_t)src_len[g.source] / 4;
                w.dst_blk = (uint32_t)src_start[g.source] / 4;
            } else {
                w.dst_off = (uint32_t)rec_pos / 4;
                w.dst_stride = (uint32_t)m.record_len / 4;
                w.dst_blk = 0;
            }
            c->h_words.push_back(w);
        }
    }
    c->n_words = (int)c->h_words.size();
    if (c->cpu) return FR_OK;   // the CPU back-end walks h_words
    plan_gather_groups(c);
    FR_TRY(c->d_words.alloc(FrMem::DEVICE, (size_t)c->n_words, "word descriptors"));
    FR_HIP(hipMemcpy(c->d_words, c->h_words.data(), sizeof(FrWordDesc) * c->n_words, hipMemcpyHostToDevice));
    // Item-tile gather plan (gather_tile_kernel): every record segment is cut in power-of-two pieces of <= 16 words, a piece of w words
    // becomes w passes (64 / w items each), consecutive pieces are grouped in chunks of <= FR_TILE_WORDS words.  The destination must
    // be item-major with one stride (SEMANTIC layout or a shard's slice).
    c->n_chunks = 0;
    if (m.layout == FR_LAYOUT_SEMANTIC || c->n_shards > 1) {
        std::vector<FrPassDesc> passes;
        std::vector<FrChunkDesc> chunks;
        FrChunkDesc cur{0, 0, 0, 0};
        int w = 0;  // index into h_words: words are listed segment by segment, in destination order
        for (int sg = s0; sg < s1; sg++) {
            int left = m.segments[sg].len / 4;
            while (left > 0) {
                int pw = 16;
                while (pw > left) pw >>= 1;
                if (cur.n_words + pw > FR_TILE_WORDS) {
                    chunks.push_back(cur);
                    cur = FrChunkDesc{(int)passes.size(), (int)passes.size(), 0, 0};
                }
                const FrWordDesc &wd = c->h_words[w];
                if (cur.n_words == 0) cur.word0 = (int)wd.dst_off;
                int lg = 0;
                while ((1 << lg) < pw) lg++;
                for (int k = 0; k < pw; k++) {
                    FrPassDesc pd{};
                    pd.src = wd.src;
                    pd.stride = wd.stride;
                    pd.idx_col = wd.idx_col;
                    pd.rows = wd.rows;
                    pd.tile_word = (uint16_t)((int)wd.dst_off - cur.word0);
                    pd.log2_words = (uint8_t)lg;
                    pd.item0 = (uint8_t)(k * (FR_TILE_ITEMS / pw));
                    passes.push_back(pd);
                }
                cur.n_words += pw;
                cur.pass_end = (int)passes.size();
                w += pw;
                left -= pw;
            }
        }
        if (cur.n_words) chunks.push_back(cur);
        c->n_chunks = (int)chunks.size();
        if (c->n_chunks) {
            FR_TRY(c->d_passes.alloc(FrMem::DEVICE, passes.size(), "gather passes"));
            FR_HIP(hipMemcpy(c->d_passes, passes.data(), sizeof(FrPassDesc) * passes.size(), hipMemcpyHostToDevice));
            FR_TRY(c->d_chunks.alloc(FrMem::DEVICE, chunks.size(), "gather chunks"));
            FR_HIP(hipMemcpy(c->d_chunks, chunks.data(), sizeof(FrChunkDesc) * chunks.size(), hipMemcpyHostToDevice));
            FR_TRY(c->d_merged.alloc(FrMem::DEVICE, 1, "dedup counter"));
            FR_HIP(hipMemset(c->d_merged, 0, sizeof(unsigned long long)));
        }
    }
    return FR_OK;
}

extern "C" int fr_ctx_create_sharded(const fr_model_desc *m, int device, int shard_rank, int n_shards, fr_ctx **out) {
    if (!out) FR_FAIL(FR_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int rc = fr_model_validate(m);
    if (rc) return rc;
    if (n_shards < 1 || shard_rank < 0 || shard_rank >= n_shards) FR_FAIL(FR_ERR_INVALID, "bad shard %d of %d", shard_rank, n_shards);
    if (n_shards > m->n_segments) FR_FAIL(FR_ERR_INVALID, "more shards (%d) than record segments (%d)", n_shards, m->n_segments);
    if (n_shards > 1 && m->layout != FR_LAYOUT_SEMANTIC) FR_FAIL(FR_ERR_INVALID, "table sharding requires the SEMANTIC layout");
    const bool cpu = device == -1;   // the CPU back-end (fr_cpu.cpp): no device is selected, no HIP call is made
    if (!cpu) {
        rc = select_device(device);
        if (rc) return rc;
    }
    fr_ctx *c = new (std::nothrow) fr_ctx();
    if (!c) FR_FAIL(FR_ERR_OOM, "out of host memory");
    c->device = device;
    c->cpu = cpu;
    c->tables.assign(m->tables, m->tables + m->n_tables);
    c->segments.assign(m->segments, m->segments + m->n_segments);
    c->model = *m;
    c->model.tables = c->tables.data();
    c->model.segments = c->segments.data();
    c->table_mem.assign(m->n_tables, FrTableMem{});
    c->shard_rank = shard_rank;
    c->n_shards = n_shards;
    c->stream_group.store(fused_group_initial(), std::memory_order_relaxed);
    hipError_t e = cpu ? hipSuccess : hipStreamCreateWithFlags(&c->setup_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        fr_set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
        ctx_free(c);
        return FR_ERR_HIP;
    }
    rc = build_words(c);
    if (rc) {
        ctx_free(c);
        return rc;
    }
    if (!cpu) {   // immutable after creation (read by every driver thread in fr_fused_flush without synchronisation): the device's compute units and
        // whether the persistent K-outer fused kernel applies to this context's descriptors and FC shape
        int n_cu = 0;
        if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) n_cu = 0;
        c->n_cu = n_cu > 0 ? n_cu : 256;
        c->hk_ok = frk_fused_hk_ok(m->fc[0], m->fc[1], m->fc[2], m->fc[3], c->h_words.data(), c->n_words) ? 1 : 0;
    }
    // fp32 master weights in the reference's column-major H x K layout (all the CPU chain reads), and on a device their q4 re-pack
    for (int l = 0; l < 4 && !rc; l++) {
        const size_t n = (size_t)m->fc[l] * m->fc[l + 1];
        rc = c->d_w[l].alloc(fr_mem_kind(c, FrMem::DEVICE), n, "weights");
        if (!rc && !cpu && l < 3) rc = c->d_wq[l].alloc(FrMem::DEVICE, n, "re-packed weights");
    }
    if (rc) {
        ctx_free(c);
        return rc;
    }
    *out = c;
    return FR_OK;
}

// Pure host query: the shard plan fr_ctx_create_sharded would use (no device needed).
extern "C" int fr_model_shard_plan(const fr_model_desc *m, int n_shards, int *slice_offset, int *slice_len, int *slice_padded_len) {
    int rc = fr_model_validate(m);
    if (rc) return rc;
    if (n_shards < 1 || n_shards > m->n_segments) FR_FAIL(FR_ERR_INVALID, "n_shards %d outside [1, %d segments]", n_shards, m->n_segments);
    std::vector<int> sb;
    if (n_shards > 1) fr_shard_bounds(*m, n_shards, sb);
    else sb = {0, m->n_segments};
    int maxlen = 0;
    for (int g = 0; g < n_shards; g++) {
        const int b = sb[g], e = sb[g + 1];
        const int off = m->segments[b].rec_offset;
        const int len = m->segments[e - 1].rec_offset + m->segments[e - 1].len - off;
        if (slice_offset) slice_offset[g] = off;
        if (slice_len) slice_len[g] = len;
        if (len > maxlen) maxlen = len;
    }
    if (slice_padded_len) *slice_padded_len = maxlen;
    return FR_OK;
}

extern "C" int fr_ctx_create(const fr_model_desc *m, int device, fr_ctx **out) { return fr_ctx_create_sharded(m, device, 0, 1, out); }
void fr_ctx_ref(fr_ctx *c) {
    if (c) c->life.fetch_add(1, std::memory_order_relaxed);
}
void fr_ctx_unref(fr_ctx *c) {
    if (c && c->life.fetch_sub(1, std::memory_order_acq_rel) == 1) ctx_free(c);
}
// Workers and communicators that are still alive keep the context (its tables, weights, descriptors) until the last of them is destroyed.
extern "C" void fr_ctx_destroy(fr_ctx *ctx) { fr_ctx_unref(ctx); }
extern "C" const fr_model_desc *fr_ctx_model(const fr_ctx *ctx) { return ctx ? &ctx->model : nullptr; }

extern "C" int fr_ctx_shard_info(const fr_ctx *ctx, int *shard_rank, int *n_shards, int *slice_offset, int *slice_len,
                                 int *slice_padded_len) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    if (shard_rank) *shard_rank = ctx->shard_rank;
    if (n_shards) *n_shards = ctx->n_shards;
    if (slice_offset) *slice_offset = ctx->slice_offset;
    if (slice_len) *slice_len = ctx->slice_len;
    if (slice_padded_len) *slice_padded_len = ctx->slice_padded;
    return FR_OK;
}

extern "C" int fr_ctx_fill_tables(fr_ctx *ctx, int mode, uint32_t seed) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    if (mode < FR_FILL_EVEN_ODD || mode > FR_FILL_TAGGED) FR_FAIL(FR_ERR_INVALID, "bad fill mode %d", mode);
    if (!ctx->cpu) FR_SET_DEVICE(ctx);
    for (int t = 0; t < ctx->model.n_tables; t++) {
        if (!ctx->table_mem[t].resident) continue;
        const fr_table_desc &d = ctx->tables[t];
        const FrTableMem &tm = ctx->table_mem[t];
        const int64_t head = tm.il_rows ? (int64_t)tm.il_rows : d.rows;  // rows at byte_offset (all of them unless interleaved)
        if (ctx->cpu) {
            frc_fill_table((float *)(ctx->table_arena + tm.byte_offset), 0, head, d.dim, (int64_t)tm.row_stride, mode, seed, fr_table_uid(d));
            if (head < d.rows) frc_fill_table((float *)(ctx->table_arena + tm.tail_offset), head, d.rows - head, d.dim, (int64_t)d.dim * 4, mode, seed, fr_table_uid(d));
            continue;
        }
        int rc = frk_fill_table((float *)(ctx->table_arena + tm.byte_offset), 0, head, d.dim, (int64_t)tm.row_stride, mode, seed, fr_table_uid(d), ctx->setup_stream);
        if (rc) return rc;
        if (head < d.rows) {
            rc = frk_fill_table((float *)(ctx->table_arena + tm.tail_offset), head, d.rows - head, d.dim, (int64_t)d.dim * 4, mode, seed, fr_table_uid(d), ctx->setup_stream);
            if (rc) return rc;
        }
    }
    if (!ctx->cpu) FR_HIP(hipStreamSynchronize(ctx->setup_stream));
    ctx->tables_filled = true;
    ctx->tables_gen++;   // an operand-type bank image made from older contents is stale (lp_ensure_image)
    return FR_OK;
}

// Copies rows [row0, row0 + nrows) of a table between host (dense rows of dim floats) and the arena, whatever the table's layout:
// a plain table is one contiguous span; a bank-interleaved one is a strided 2-D copy for its rows < il_rows plus a contiguous tail.
static int table_copy(fr_ctx *ctx, int table, int64_t row0, int64_t nrows, float *host_rows, bool to_device) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    if (table < 0 || table >= ctx->model.n_tables) FR_FAIL(FR_ERR_INVALID, "table %d out of range", table);
    if (!ctx->table_mem[table].resident) FR_FAIL(FR_ERR_STATE, "table %d is not resident on shard %d", table, ctx->shard_rank);
    const fr_table_desc &d = ctx->tables[table];
    if (row0 < 0 || nrows < 0 || row0 + nrows > d.rows) FR_FAIL(FR_ERR_INVALID, "rows [%lld,+%lld) outside table %d", (long long)row0, (long long)nrows, table);
    if (!host_rows && nrows) FR_FAIL(FR_ERR_INVALID, "host_rows is NULL");
    if (!ctx->cpu) FR_SET_DEVICE(ctx);
    const FrTableMem &tm = ctx->table_mem[table];
    const size_t row_bytes = (size_t)d.dim * 4;
    const int64_t head_rows = tm.il_rows ? (int64_t)tm.il_rows : d.rows;
    const int64_t n_head = row0 < head_rows ? (row0 + nrows < head_rows ? nrows : head_rows - row0) : 0;  // rows of the request below head_rows
    if (ctx->cpu) {   // host arena: plain copies, row by row where the table is one column block of a bank row
        for (int64_t r = 0; r < nrows; r++) {
            char *a = r < n_head ? ctx->table_arena + tm.byte_offset + (size_t)(row0 + r) * tm.row_stride
                                 : ctx->table_arena + tm.tail_offset + (size_t)(row0 + r - head_rows) * row_bytes;
            float *h = host_rows + (size_t)r * d.dim;
            if (to_device) memcpy(a, h, row_bytes);
            else memcpy(h, a, row_bytes);
        }
        return FR_OK;
    }
    if (n_head > 0) {
        char *dev = ctx->table_arena + tm.byte_offset + (size_t)row0 * tm.row_stride;
        if (tm.row_stride == row_bytes) {
            if (to_device) FR_HIP(hipMemcpy(dev, host_rows, (size_t)n_head * row_bytes, hipMemcpyHostToDevice));
            else FR_HIP(hipMemcpy(host_rows, dev, (size_t)n_head * row_bytes, hipMemcpyDeviceToHost));
        } else if (to_device) {
            FR_HIP(hipMemcpy2D(dev, tm.row_stride, host_rows, row_bytes, row_bytes, (size_t)n_head, hipMemcpyHostToDevice));
        } else {
            FR_HIP(hipMemcpy2D(host_rows, row_bytes, dev, tm.row_stride, row_bytes, (size_t)n_head, hipMemcpyDeviceToHost));
        }
    }
    if (nrows > n_head) {
        const int64_t t0 = row0 + n_head - head_rows;  // first tail row of the request
        char *dev = ctx->table_arena + tm.tail_offset + (size_t)t0 * row_bytes;
        float *host = host_rows + (size_t)n_head * d.dim;
        if (to_device) FR_HIP(hipMemcpy(dev, host, (size_t)(nrows - n_head) * row_bytes, hipMemcpyHostToDevice));
        else FR_HIP(hipMemcpy(host, dev, (size_t)(nrows - n_head) * row_bytes, hipMemcpyDeviceToHost));
    }
    return FR_OK;
}

extern "C" int fr_ctx_upload_table(fr_ctx *ctx, int table, int64_t row0, int64_t nrows, const float *host_rows) {
    int rc = table_copy(ctx, table, row0, nrows, const_cast<float *>(host_rows), true);
    if (rc) return rc;
    ctx->tables_filled = true;
    ctx->tables_gen++;   // an operand-type bank image made from older contents is stale (lp_ensure_image)
    return FR_OK;
}

extern "C" int fr_ctx_download_table(fr_ctx *ctx, int table, int64_t row0, int64_t nrows, float *host_rows) {
    return table_copy(ctx, table, row0, nrows, host_rows, false);
}

// ---- weights ----------------------------------------------------------------------------------------
static int floor_log2f(float v) {  // floor(log2(v)) for v > 0
    int e;
    (void)std::frexp(v, &e);  // v = m * 2^e, m in [0.5, 1)
    return e - 1;
}

// fp8 activation exponents from an rms estimate (until a calibration batch replaces them): inputs are taken as U(-1,1)
// (rms 0.58, the FR_FILL_HASH tables), each layer multiplies the rms by ||W||_F / sqrt(N), and 8 rms must still fit 448.
static void f8_estimate_act_exponents(fr_ctx *ctx) {
    if (ctx->f8_calibrated) return;
    float rms = 0.58f;
    for (int l = 0; l < 4; l++) {
        const float absmax_est = 8.0f * (rms > 0.0f ? rms : 1.0f);
        ctx->f8_e_act[l] = floor_log2f(448.0f / absmax_est);
        if (l < 3) rms *= ctx->f8_w_rms_gain[l];
    }
}

static int refresh_fp8(fr_ctx *ctx, int layer) {
    if (layer >= 3) return FR_OK;  // the output layer stays in fp32
    const int K = ctx->model.fc[layer], H = ctx->model.fc[layer + 1];
    const int KP = (K + 63) / 64 * 64;
    int rc = ctx->d_w_fp8[layer].grow(FrMem::DEVICE, (size_t)KP * H, "fp8 weights");
    if (!rc) rc = ctx->d_stats.grow(FrMem::DEVICE, 16, "reduction scratch");
    if (rc) return rc;
    rc = frk_stats(ctx->d_w[layer], (size_t)K * H, ctx->d_stats, ctx->setup_stream);
    if (rc) return rc;
    uint32_t st[2];
    FR_HIP(hipMemcpyAsync(st, ctx->d_stats, 8, hipMemcpyDeviceToHost, ctx->setup_stream));
    FR_HIP(hipStreamSynchronize(ctx->setup_stream));
    float absmax, sumsq;
    memcpy(&absmax, &st[0], 4);
    memcpy(&sumsq, &st[1], 4);
    ctx->f8_e_w[layer] = absmax > 0.0f ? floor_log2f(448.0f / absmax) : 0;  // max |W| * 2^e_w lands in (224, 448]
    ctx->f8_w_rms_gain[layer] = std::sqrt(sumsq / (float)H);
    f8_estimate_act_exponents(ctx);
    rc = frk_pack_weights_q16_fp8(ctx->d_w[layer], ctx->d_w_fp8[layer], K, H, ctx->f8_e_w[layer], ctx->setup_stream);
    if (rc) return rc;
#ifdef FR_EXPERIMENTS
    if (frk_fused_f8_ok(ctx->model.fc[0], ctx->model.fc[1], ctx->model.fc[2], ctx->model.fc[3])) {  // the persistent kernel's fp8 form (experiments build only)
        const int KP32 = (K + 31) / 32 * 32;
        rc = ctx->d_w_fp8h[layer].grow(FrMem::DEVICE, (size_t)KP32 * H, "fp8 weights (q16h)");
        if (!rc) rc = frk_pack_weights_q16h_fp8(ctx->d_w[layer], ctx->d_w_fp8h[layer], K, H, ctx->f8_e_w[layer], ctx->setup_stream);
    }
#endif
    return rc;
}

// derived copies of one layer's weights: the q4 re-pack for the fp32 chain, the bf16 / fp8 casts for the low-precision chains
static int refresh_bf16(fr_ctx *ctx, int layer) {
    if (layer < 3) {
        int rc = frk_pack_weights_q4(ctx->d_w[layer], ctx->d_wq[layer], ctx->model.fc[layer], ctx->model.fc[layer + 1], ctx->setup_stream);
        if (rc) return rc;
    }
    if (ctx->fc_precision == FR_FC_FP8) return refresh_fp8(ctx, layer);
    if (ctx->fc_precision != FR_FC_BF16) return FR_OK;
    size_t n = (size_t)ctx->model.fc[layer] * ctx->model.fc[layer + 1];
    FR_TRY(ctx->d_w_bf16[layer].grow(FrMem::DEVICE, n, "bf16 weights"));
    // Wh[k/8][h][k%8]; for the output layer (H == 1) this is simply the bf16 vector w[k]
    return frk_pack_weights_q8_bf16(ctx->d_w[layer], ctx->d_w_bf16[layer], ctx->model.fc[layer], ctx->model.fc[layer + 1], ctx->setup_stream);
}

extern "C" int fr_ctx_set_weights(fr_ctx *ctx, int layer, const float *w, size_t count) {
    if (!ctx || !w) FR_FAIL(FR_ERR_INVALID, "NULL argument");
    if (layer < 0 || layer > 3) FR_FAIL(FR_ERR_INVALID, "layer %d out of range", layer);
    size_t n = (size_t)ctx->model.fc[layer] * ctx->model.fc[layer + 1];
    if (count != n) FR_FAIL(FR_ERR_INVALID, "layer %d expects %zu weights (H=%d x K=%d), got %zu", layer, n, ctx->model.fc[layer + 1], ctx->model.fc[layer], count);
    if (ctx->cpu) {
        memcpy(ctx->d_w[layer], w, n * sizeof(float));
        ctx->weights_set = true;
        return FR_OK;
    }
    FR_SET_DEVICE(ctx);
    FR_HIP(hipMemcpy(ctx->d_w[layer], w, n * sizeof(float), hipMemcpyHostToDevice));
    int rc = refresh_bf16(ctx, layer);
    if (rc) return rc;
    FR_HIP(hipStreamSynchronize(ctx->setup_stream));
    ctx->weights_set = true;
    return FR_OK;
}

// ---- per-layer epilogue (fleetrec_serving.h) ------------------------------------------------------------------------------------------
// The bias stays fp32 in every chain (never rounded to bf16 / e4m3) and is read by the kernels that finish the layer; nothing derived is kept, so the
// fp8 exponents, the weight images, the chain width and the stream group are as they were.  Same rules as fr_ctx_set_weights: no launch in flight.
extern "C" int fr_ctx_set_epilogue(fr_ctx *ctx, int layer, const float *bias, size_t count, int act) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    if (layer < 0 || layer > 3) FR_FAIL(FR_ERR_INVALID, "layer %d out of range", layer);
    if (act != FR_ACT_NONE && act != FR_ACT_RELU) FR_FAIL(FR_ERR_INVALID, "unknown activation %d (FR_ACT_NONE, FR_ACT_RELU)", act);
    if (layer == 3 && act != FR_ACT_NONE) FR_FAIL(FR_ERR_INVALID, "the output layer takes FR_ACT_NONE only (a monotone transform does not change a ranking)");
    const size_t n = (size_t)ctx->model.fc[layer + 1];
    if (bias ? count != n : count != 0) FR_FAIL(FR_ERR_INVALID, "layer %d expects %zu bias values (or NULL and 0), got %zu", layer, n, count);
    if (!ctx->cpu && !ctx->d_negzero) {
        FR_SET_DEVICE(ctx);
        size_t widest = 4;
        for (int l = 1; l <= 4; l++) widest = std::max(widest, (size_t)ctx->model.fc[l]);
        const std::vector<float> nz(widest, -0.0f);
        FrBuf<float> fresh;   // taken by the context only once it is filled: a failed copy leaves no buffer of undefined contents behind
        FR_TRY(fresh.alloc(FrMem::DEVICE, widest, "epilogue zeros"));
        FR_HIP(hipMemcpy(fresh, nz.data(), widest * sizeof(float), hipMemcpyHostToDevice));
        ctx->d_negzero = std::move(fresh);
    }
    if (bias) {
        FR_TRY(ctx->d_bias[layer].grow(fr_mem_kind(ctx, FrMem::DEVICE), n, "layer bias"));
        if (ctx->cpu) {
            memcpy(ctx->d_bias[layer], bias, n * sizeof(float));
        } else {
            FR_SET_DEVICE(ctx);
            FR_HIP(hipMemcpy(ctx->d_bias[layer], bias, n * sizeof(float), hipMemcpyHostToDevice));
        }
    }
    ctx->has_bias[layer] = bias != nullptr;
    ctx->act[layer] = act;
    return FR_OK;
}

extern "C" int fr_ctx_epilogue(fr_ctx *ctx, int layer, float *bias_out, size_t count, int *has_bias, int *act) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    if (layer < 0 || layer > 3) FR_FAIL(FR_ERR_INVALID, "layer %d out of range", layer);
    const size_t n = (size_t)ctx->model.fc[layer + 1];
    if (bias_out && count != n) FR_FAIL(FR_ERR_INVALID, "layer %d holds %zu bias values, got %zu", layer, n, count);
    if (has_bias) *has_bias = ctx->has_bias[layer] ? 1 : 0;
    if (act) *act = ctx->act[layer];
    if (bias_out && ctx->has_bias[layer]) {
        if (ctx->cpu) {
            memcpy(bias_out, ctx->d_bias[layer], n * sizeof(float));
        } else {
            FR_SET_DEVICE(ctx);
            FR_HIP(hipMemcpy(bias_out, ctx->d_bias[layer], n * sizeof(float), hipMemcpyDeviceToHost));
        }
    }
    return FR_OK;
}

extern "C" int fr_ctx_fill_weights(fr_ctx *ctx, int mode, uint32_t seed) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    if (mode != FR_WEIGHTS_ONES && mode != FR_WEIGHTS_UNIFORM) FR_FAIL(FR_ERR_INVALID, "bad weight mode %d", mode);
    if (ctx->cpu) {
        for (int l = 0; l < 4; l++)
            frc_fill_weights(ctx->d_w[l], (size_t)ctx->model.fc[l] * ctx->model.fc[l + 1], mode, seed, (uint32_t)l, 1.0f / std::sqrt((float)ctx->model.fc[l]));
        ctx->weights_set = true;
        return FR_OK;
    }
    FR_SET_DEVICE(ctx);
    for (int l = 0; l < 4; l++) {
        size_t n = (size_t)ctx->model.fc[l] * ctx->model.fc[l + 1];
        float scale = 1.0f / std::sqrt((float)ctx->model.fc[l]);
        int rc = frk_fill_weights(ctx->d_w[l], n, mode, seed, (uint32_t)l, scale, ctx->setup_stream);
        if (rc) return rc;
        rc = refresh_bf16(ctx, l);
        if (rc) return rc;
    }
    FR_HIP(hipStreamSynchronize(ctx->setup_stream));
    ctx->weights_set = true;
    return FR_OK;
}

extern "C" int fr_ctx_get_weights(fr_ctx *ctx, int layer, float *w, size_t count) {
    if (!ctx || !w) FR_FAIL(FR_ERR_INVALID, "NULL argument");
    if (layer < 0 || layer > 3) FR_FAIL(FR_ERR_INVALID, "layer %d out of range", layer);
    size_t n = (size_t)ctx->model.fc[layer] * ctx->model.fc[layer + 1];
    if (count != n) FR_FAIL(FR_ERR_INVALID, "layer %d holds %zu weights, got %zu", layer, n, count);
    if (ctx->cpu) {
        memcpy(w, ctx->d_w[layer], n * sizeof(float));
        return FR_OK;
    }
    FR_SET_DEVICE(ctx);
    FR_HIP(hipMemcpy(w, ctx->d_w[layer], n * sizeof(float), hipMemcpyDeviceToHost));
    return FR_OK;
}

extern "C" int fr_ctx_set_fc_precision(fr_ctx *ctx, int precision) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    if (precision != FR_FC_FP32 && precision != FR_FC_BF16 && precision != FR_FC_FP8) FR_FAIL(FR_ERR_INVALID, "bad precision %d", precision);
    if (ctx->cpu) {
        if (precision != FR_FC_FP32) FR_FAIL(FR_ERR_INVALID, "the CPU back-end computes the FC chain in fp32 only (the reference's own precision, cuda_server.c:211)");
        return FR_OK;
    }
    FR_SET_DEVICE(ctx);
    if (precision == FR_FC_BF16) {
        for (int l = 0; l < 4; l++)
            if (ctx->model.fc[l] % 16) FR_FAIL(FR_ERR_INVALID, "bf16 chain needs fc[%d]=%d to be a multiple of 16", l, ctx->model.fc[l]);
    }
    if (precision == FR_FC_FP8) {  // the record is zero-padded to 64 k inside the q16 image; hidden widths are not
        for (int l = 1; l < 4; l++)
            if (ctx->model.fc[l] % 64) FR_FAIL(FR_ERR_INVALID, "fp8 chain needs fc[%d]=%d to be a multiple of 64", l, ctx->model.fc[l]);
    }
    ctx->fc_precision = precision;
    if (precision != FR_FC_FP32 && ctx->weights_set) {
        for (int l = 0; l < 4; l++) {
            int rc = refresh_bf16(ctx, l);
            if (rc) return rc;
        }
        FR_HIP(hipStreamSynchronize(ctx->setup_stream));
    }
    // fp8 on a model that streams through the fused item-tile kernels (Models A / B) is accepted and CORRECT, but it is not
    // where the e4m3 peak is: the chunked fr_fused_tile_f8_kernel gathers with the matrix pipes idle and then streams weights at the rate
    // the bf16 kernel does -- 0.19 of the fp8 peak, 14-19 % above the bf16 chain.  The caller is told instead of finding out from a profile:
    // the call succeeds and fr_last_error() carries the note (fleetrec.h, fr_fc_precision).
    if (precision == FR_FC_FP8 && fused_eligible(ctx))
        fr_set_error("note: FR_FC_FP8 on a fused-kernel model (record of %d floats) runs fr_fused_tile_f8_kernel at ~0.19 of the fp8 MFMA peak, 14-19 %% above FR_FC_BF16 "
                     "(the 64-item tile is bound by its gather phase and its weight stream, not by the matrix pipes); the scaled-MFMA chain that reaches 0.55 of the fp8 peak "
                     "is the GEMM path of chain models (Model-C shapes at batch >= 1024)", ctx->model.fc[0]);
    return FR_OK;
}

// ---- worker -----------------------------------------------------------------------------------------
// the context's list of live workers (fr_ctx_set_pooling asks each whether it has work in flight)
static void ctx_enlist(fr_ctx *c, fr_worker *w) {
    std::lock_guard<std::mutex> g(c->workers_mutex);
    c->workers.push_back(w);
}
static void ctx_delist(fr_ctx *c, fr_worker *w) {
    std::lock_guard<std::mutex> g(c->workers_mutex);
    for (size_t i = 0; i < c->workers.size(); i++)
        if (c->workers[i] == w) {
            c->workers.erase(c->workers.begin() + (long)i);
            break;
        }
}

extern "C" void fr_worker_destroy(fr_worker *w) {
    if (!w) return;
    if (w->ctx && w->counted) ctx_delist(w->ctx, w);
    if (w->ctx && !w->ctx->cpu) (void)hipSetDevice(w->ctx->device);
    // a sharded step still on the worker's host stream (a CPU worker's step; a GPU worker's staged exchange) is waited for (bounded), its communicator let go
    fr_comm_worker_release(w);
    const hipStream_t streams[] = {w->stream, w->hr.copy};
    for (hipStream_t s : streams)
        if (s) (void)hipStreamSynchronize(s);
    if (w->counted) w->ctx->n_workers.fetch_sub(1, std::memory_order_relaxed);
    fr_ctx *held = w->counted ? w->ctx : nullptr;
    delete w;   // every buffer and event is released by its holder (fr_mem.h), behind both streams
    for (hipStream_t s : streams)
        if (s) (void)hipStreamDestroy(s);
    fr_ctx_unref(held);   // (the last worker of a context that was already destroyed releases it)
}

size_t idx_cols(const fr_ctx *c) {
    const int mode = c->model.index_mode;
    return mode == FR_INDEX_PER_TABLE ? (size_t)c->model.n_tables : (mode == FR_INDEX_PER_BANK ? (size_t)c->n_banks : 1);
}

// request words per request the worker's pinned request buffers hold: max(Rs, Rs') ints (at least one), Rs' floats -- as the split and the pooling stand now
static void request_caps(const fr_ctx *c, fr_worker *w) {
    const int rs = c->req_form[FR_REQ_ONE_HOT].req_words, rp = c->req_form[FR_REQ_POOLED].desc.empty() ? 0 : c->req_form[FR_REQ_POOLED].req_words;
    w->req_idx_cap = rs > rp ? rs : rp;
    if (w->req_idx_cap < 1) w->req_idx_cap = 1;
    w->req_w_cap = w->pool_w_cap ? (rp > 0 ? rp : 1) : 0;
}

// the stream, buffers and events of a new worker, one sequence for both back-ends; a failure leaves what was made to fr_worker_destroy
static int worker_build(fr_worker *w) {
    fr_ctx *ctx = w->ctx;
    const int max_batch = w->max_batch;
    const fr_model_desc &m = ctx->model;
    const size_t B = (size_t)max_batch;
    // the index buffers hold one-hot rows and, when pooling is set already, pooled rows (fr_worker_submit_pooled)
    w->idx_cap = (int)idx_cols(ctx) > ctx->pool_cols ? (int)idx_cols(ctx) : ctx->pool_cols;
    w->pool_w_cap = ctx->pool_cols;   // per-sample weights of the host form (fr_worker_submit_pooled_weighted): only when pooling is set already
    if (!ctx->cpu) {
        // A model that runs the stage pipeline (several launches per step: Model-C, sharded contexts) gives its workers hardware queues of
        // their own: the HIP runtime keeps one pool of hardware queues per stream priority, four equal-priority streams share two queues
        // (profiles/archive/r04_C4096_chain_trace_bf16.txt), and there a small launch of one worker waits behind the other's FC1.  The workers
        // alternate between the HIGHEST and the LOWEST priority, never the default one: those two pools are this library's alone, so the
        // first four workers get four consecutively created queues = one per compute pipe of the command processor (queue id mod 4;
        // two workers whose queues share a pipe run 10 % behind the others: profiles/archive/r04_stream_queues_after_other_contexts.txt -- with
        // the default priority in the rotation, a context served earlier in the process had that effect).  Model-C 4096, four workers:
        // bf16 41.9 -> 43.1 M inf/s, fp8 65.5 -> 68.9 M = what GPU_MAX_HW_QUEUES=8 buys (profiles/archive/r04_stream_priorities_ab.txt).
        // Fused-kernel models (one launch per group) gain nothing from it and keep the default streams.
        // (a model no fused kernel of any precision serves -- the decision must not depend on the precision the context happens to have now)
        const bool any_fused = frk_fused_ok(m.fc[0], m.fc[1], m.fc[2], m.fc[3]) || frk_fused_h_ok(m.fc[0], m.fc[1], m.fc[2], m.fc[3]) ||
                               frk_fused_f8_ok(m.fc[0], m.fc[1], m.fc[2], m.fc[3]) || ctx->hk_ok == 1;
        const bool chain = !(ctx->n_shards == 1 && m.layout == FR_LAYOUT_SEMANTIC && any_fused);
        const int spread = FR_KNOB_ONCE("STREAM_PRIO", -1);   // experiment knob: 0 = never, 1 = always, 2 = rotate over every level (default included)
        int lo = 0, hi = 0;   // numerically lower = higher priority
        if (spread < 0 ? chain : spread != 0) FR_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
        // k = how many workers the context has EVER created (one fetch_add: two threads creating workers at once cannot draw the same k, and a
        // destroy + create keeps alternating -- ADVICE r04: the live count did neither)
        const int k = ctx->worker_seq.fetch_add(1, std::memory_order_relaxed);
        // (Round 6 tried to CHECK and REPAIR the outcome, and kept none of it -- profiles/r06_experiments.md section 4: after some stream churn in the
        // process one pair of a context's four workers takes turns (four Model-C chains 48 -> 37-45 M inf/s).  Handshake kernels on the two streams
        // see each other resident; a BURST of part-chip spin launches on both does expose the pair (0.8-1.2 kernels resident of 2 against 1.95-2.0)
        // -- but a stream that probes clean at creation pairs up again when the next queue is created, a pool of streams pairs up all the same,
        // and replacing streams after all workers exist does not converge.  What the library controls is what it does here.)
        if (lo > hi) FR_HIP(hipStreamCreateWithPriority(&w->stream, hipStreamNonBlocking, spread == 2 ? hi + k % (lo - hi + 1) : (k % 2 ? lo : hi)));
        else FR_HIP(hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking));
    }
    // Sizes and existence are stated once for both back-ends; on the CPU back-end (fr_mem_kind) every buffer is plain host memory behind the same
    // accessors (fr_worker_idx_ptr / dense_ptr / score_ptr), and the device-side stand-ins d_idx / d_dense / d_pool_w exist only with a request split.
    const bool cpu = ctx->cpu, split = !ctx->req_shared.empty();
    const FrMem pinned = fr_mem_kind(ctx, FrMem::PINNED), device = fr_mem_kind(ctx, FrMem::DEVICE);
    const size_t n_idx = B * (size_t)w->idx_cap, n_dense = B * m.dense_len, n_pool_w = B * (size_t)w->pool_w_cap;
    FR_TRY(w->h_idx.alloc(pinned, n_idx, "worker index rows"));
    if (w->pool_w_cap) FR_TRY(w->h_pool_w.alloc(pinned, n_pool_w, "worker per-sample weights"));   // read in place by the gather, like h_idx
    if (w->pool_w_cap) FR_TRY(w->h_pool_off.alloc(pinned, B * idx_cols(ctx) + 1, "worker bag offsets"));   // bag offsets of the offsets-form host call
    if (m.dense_len) FR_TRY(w->h_dense.alloc(pinned, n_dense, "worker dense rows"));
    FR_TRY(w->h_score.alloc(pinned, B, "worker scores"));
    if (cpu) {
        w->h_err = w->d_err = &w->c_err;
    } else {
        // index-range flag: pinned, device-visible host word.  Kernels touch it only on the error path
        // (system-scope atomicOr), so fr_worker_sync() needs no D2H copy -- it just reads the word after the stream drained.
        FR_TRY(w->err_word.alloc(FrMem::PINNED_MAPPED, 1, "worker status word"));
        w->h_err = w->err_word;
        *w->h_err = 0;
        FR_HIP(hipHostGetDevicePointer((void **)&w->d_err, w->h_err, 0));
    }
    if (!cpu || split || ctx->keyed) {
        FR_TRY(w->d_idx.alloc(device, n_idx, "worker index rows (device)"));
        if (m.dense_len) FR_TRY(w->d_dense.alloc(device, n_dense, "worker dense rows (device)"));
    }
    FR_TRY(w->d_records.alloc(device, B * (size_t)ctx->slice_padded, "worker records"));
    if (!cpu && ctx->n_shards == 1 && ctx->slice_padded != m.record_len) FR_FAIL(FR_ERR_STATE, "internal: unsharded ctx with a partial slice");
    if (cpu) {   // a call computes before it returns: the chain's scratch, and the records of the sharded FC entry points
        FR_TRY(w->c_scratch.alloc(FrMem::HOST, B * ((size_t)m.fc[1] + m.fc[2] + m.fc[3]), "worker chain scratch"));
        if (ctx->n_shards > 1) FR_TRY(w->c_x.alloc(FrMem::HOST, B * (size_t)m.fc[0], "worker records (sharded)"));
    } else {
        w->ld_max = round_up(max_batch, 64);
        for (int p = 0; p < 2; p++)
            FR_TRY(w->d_act[p].alloc(FrMem::DEVICE, (size_t)w->ld_max * ((size_t)m.fc[0] + 2 * ((size_t)m.fc[1] + m.fc[2] + m.fc[3])), "worker activations"));
        FR_TRY(w->d_score.alloc(FrMem::DEVICE, B, "worker scores (device)"));
    }
    if (split) {   // request-form host call: the request side's buffers (pinned: read in place by the expansion) and the expanded weights
        request_caps(ctx, w);
        FR_TRY(w->h_req_idx.alloc(pinned, B * (size_t)w->req_idx_cap, "worker request rows"));
        if (w->req_w_cap) FR_TRY(w->h_req_w.alloc(pinned, B * (size_t)w->req_w_cap, "worker request weights"));
        if (ctx->req_dense_shared) FR_TRY(w->h_req_dense.alloc(pinned, n_dense, "worker request dense rows"));
        FR_TRY(w->h_req_off.alloc(pinned, B + 1, "worker request offsets"));
        if (w->pool_w_cap) FR_TRY(w->d_pool_w.alloc(device, n_pool_w, "worker expanded weights"));
    }
    if (ctx->keyed) FR_TRY(w->h_keys.alloc(pinned, n_idx, "worker key rows"));   // keyed host form: read in place by the resolve
    if (!cpu) {
        FR_HIP(w->ev_start.create(hipEventDefault));
        FR_HIP(w->ev_stop.create(hipEventDefault));
        FR_HIP(w->ev_update.create(hipEventDisableTiming));
    }
    return FR_OK;
}

extern "C" int fr_worker_create(fr_ctx *ctx, int max_batch, fr_worker **out) {
    if (!ctx || !out) FR_FAIL(FR_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (max_batch <= 0 || max_batch > (1 << 24)) FR_FAIL(FR_ERR_INVALID, "max_batch %d out of range", max_batch);
    {   // the FC kernels address every operand through a buffer resource: 32-bit byte offsets, so each tensor must stay below 4 GiB
        int widest = 0;
        for (int l = 0; l < 4; l++) widest = ctx->model.fc[l] > widest ? ctx->model.fc[l] : widest;
        if ((uint64_t)widest * (uint64_t)round_up(max_batch, 64) * 4ull >= (1ull << 32))
            FR_FAIL(FR_ERR_INVALID, "max_batch %d: an activation tensor of %d x batch floats would reach 4 GiB (32-bit buffer offsets)", max_batch, widest);
    }
    FR_SET_DEVICE(ctx);
    fr_worker *w = new (std::nothrow) fr_worker();
    if (!w) FR_FAIL(FR_ERR_OOM, "out of host memory");
    w->ctx = ctx;
    w->max_batch = max_batch;
    const int rc = worker_build(w);
    if (rc) {
        fr_worker_destroy(w);
        return rc;
    }
    w->counted = true;
    fr_ctx_ref(ctx);
    ctx_enlist(ctx, w);
    const int live = ctx->n_workers.fetch_add(1, std::memory_order_relaxed) + 1;
    // A width frozen by an early launch is kept (scores in flight must not change), but the caller is told once per worker that outnumbers
    // it: the call succeeds and fr_last_error() carries the note.
    const int cw = ctx->chain_width.load(std::memory_order_relaxed);
    if (cw && cw < 4 && live > cw && ctx->chain_width_auto.load(std::memory_order_relaxed))
        fr_set_error("note: the context's chain width was frozen at %d by a launch made while %d worker(s) existed; %d workers are live now and share tiles sized for %d "
                     "side-by-side chains -- call fr_ctx_set_chain_width(ctx, %d) before streaming if that is not intended", cw, cw, live, cw, live > 4 ? 4 : live);
    *out = w;
    return FR_OK;
}

extern "C" int32_t *fr_worker_idx_ptr(fr_worker *w) { return w ? w->h_idx.p : nullptr; }
extern "C" float *fr_worker_pool_weights_ptr(fr_worker *w) { return w ? w->h_pool_w.p : nullptr; }
extern "C" int32_t *fr_worker_request_idx_ptr(fr_worker *w) { return w ? w->h_req_idx.p : nullptr; }
extern "C" float *fr_worker_request_weights_ptr(fr_worker *w) { return w ? w->h_req_w.p : nullptr; }
extern "C" float *fr_worker_request_dense_ptr(fr_worker *w) { return w ? w->h_req_dense.p : nullptr; }
extern "C" int32_t *fr_worker_request_offsets_ptr(fr_worker *w) { return w ? w->h_req_off.p : nullptr; }
extern "C" int32_t *fr_worker_pool_offsets_ptr(fr_worker *w) { return w ? w->h_pool_off.p : nullptr; }
extern "C" float *fr_worker_dense_ptr(fr_worker *w) { return w ? w->h_dense.p : nullptr; }
extern "C" float *fr_worker_score_ptr(fr_worker *w) { return w ? w->h_score.p : nullptr; }
extern "C" void *fr_worker_stream(fr_worker *w) { return w ? (void *)w->stream : nullptr; }
extern "C" float *fr_worker_records_dptr(fr_worker *w) { return w ? w->d_records.p : nullptr; }
extern "C" float *fr_worker_features_dptr(fr_worker *w, int *ld_max) {
    if (!w) return nullptr;
    if (ld_max) *ld_max = w->ld_max;
    return w->d_act[w->last_x_parity];
}

static int check_ready(fr_worker *w, int batch, bool need_tables, bool need_weights) {
    if (!w) FR_FAIL(FR_ERR_INVALID, "worker is NULL");
    if (batch <= 0 || batch > w->max_batch) FR_FAIL(FR_ERR_INVALID, "batch %d outside (0, max_batch=%d]", batch, w->max_batch);
    if (need_tables && !w->ctx->tables_filled) FR_FAIL(FR_ERR_STATE, "tables have not been filled or uploaded");
    if (need_weights && !w->ctx->weights_set) FR_FAIL(FR_ERR_STATE, "FC weights have not been set");
    return FR_OK;
}

// what a record or slice gather (one-hot or pooled) checks before it launches anything, its transport and layout rule included; sets the device
static int gather_ready(fr_worker *w, int batch, const void *d_out, const char *out_name, int transport) {
    const int rc = check_ready(w, batch, true, false);
    if (rc) return rc;
    if (!d_out) FR_FAIL(FR_ERR_INVALID, "%s is NULL", out_name);
    if (transport != FR_FC_FP32 && transport != FR_FC_BF16 && transport != FR_FC_FP8) FR_FAIL(FR_ERR_INVALID, "bad transport %d", transport);
    if (transport != FR_FC_FP32 && w->ctx->model.layout != FR_LAYOUT_SEMANTIC) FR_FAIL(FR_ERR_STATE, "low-precision transport: SEMANTIC layout only");
    FR_SET_DEVICE(w->ctx);
    return FR_OK;
}

// a gather (one-hot or pooled) of a context whose words read the dense features needs them
static int dense_check(const fr_ctx *c, const float *d_dense) {
    if (c->model.dense_len && !d_dense)
        for (const FrWordDesc &wd : c->h_words)
            if (wd.idx_col & FR_DESC_DENSE) FR_FAIL(FR_ERR_INVALID, "model has dense features but d_dense is NULL");
    return FR_OK;
}

static int launch_gather(fr_worker *w, int batch, const int32_t *d_idx, const float *d_dense, void *d_records, int transport = FR_FC_FP32) {
    fr_ctx *c = w->ctx;
    if (!d_idx) FR_FAIL(FR_ERR_INVALID, "d_idx is NULL");
    const int drc = dense_check(c, d_dense);
    if (drc) return drc;
    if (c->cpu) {
        if (transport != FR_FC_FP32) FR_FAIL(FR_ERR_STATE, "the CPU back-end gathers fp32 records only");
        return frc_gather(c->h_words.data(), c->n_words, d_idx, (int)idx_cols(c), d_dense, reinterpret_cast<float *>(d_records), batch, &w->c_err);
    }
    const int variant = c->gather_variant.load(std::memory_order_relaxed);
    const bool one_chunk = variant == FR_GATHER_WORD_MAJOR_ONE_CHUNK;
    if (variant != FR_GATHER_WORD_MAJOR && !one_chunk && transport == FR_FC_FP32 && c->n_chunks > 0)
        return frk_gather_tile(c->d_passes, c->d_chunks, c->n_chunks, d_idx, (int)idx_cols(c), d_dense, d_records, c->slice_padded / 4, batch, w->d_err,
                               variant != FR_GATHER_ITEM_TILE, variant == FR_GATHER_ITEM_TILE_DEDUP_COUNT ? c->d_merged.p : nullptr, w->stream);
    return frk_gather(c->d_words, c->n_words, c->gather_groups, d_idx, (int)idx_cols(c), d_dense, d_records, batch, w->d_err, transport, c->f8_e_act[0], w->stream,
                      c->slice_padded / 4, one_chunk);  // words per item of the destination: the record (any layout) or the shard's padded slice
}

extern "C" int fr_ctx_set_gather_variant(fr_ctx *ctx, int variant) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    if (variant < FR_GATHER_WORD_MAJOR || variant > FR_GATHER_WORD_MAJOR_ONE_CHUNK) FR_FAIL(FR_ERR_INVALID, "bad gather variant %d", variant);
    if (variant != FR_GATHER_WORD_MAJOR && variant != FR_GATHER_WORD_MAJOR_ONE_CHUNK && ctx->n_chunks == 0) FR_FAIL(FR_ERR_STATE, "the item-tile gather needs the SEMANTIC layout (or a shard slice)");
    ctx->gather_variant.store(variant, std::memory_order_relaxed);
    return FR_OK;
}

extern "C" int fr_ctx_gather_variant(const fr_ctx *ctx) { return ctx ? ctx->gather_variant.load(std::memory_order_relaxed) : FR_ERR_INVALID; }

extern "C" int fr_ctx_gather_groups(const fr_ctx *ctx, int starts[9]) {
    if (!ctx || !starts) FR_FAIL(FR_ERR_INVALID, "ctx or starts is NULL");
    if (ctx->gather_groups.max_words <= 0) FR_FAIL(FR_ERR_STATE, "no XCD partition for this record (%d words)", ctx->n_words);
    for (int g = 0; g <= 8; g++) starts[g] = ctx->gather_groups.start[g];
    return FR_OK;
}

extern "C" int fr_ctx_gather_merged_lookups(fr_ctx *ctx, uint64_t *merged, int reset) {
    if (!ctx || !merged) FR_FAIL(FR_ERR_INVALID, "NULL argument");
    *merged = 0;
    if (!ctx->d_merged) return FR_OK;
    FR_SET_DEVICE(ctx);
    FR_HIP(hipDeviceSynchronize());
    unsigned long long v = 0;
    FR_HIP(hipMemcpy(&v, ctx->d_merged, sizeof(v), hipMemcpyDeviceToHost));
    if (reset) FR_HIP(hipMemset(ctx->d_merged, 0, sizeof(v)));
    *merged = (uint64_t)v;
    return FR_OK;
}

// ---- the stage pipeline ------------------------------------------------------------------------------

// K-split of one FC layer into 2 workgroups per output tile (partials summed by the next stage's loads):
// only when the layer has fewer tiles than CUs and each wave still gets >= 16 k-pairs.
static int pick_nsplit(int K, int N, int ldm) {
    const long tiles = (long)(N / 32) * (ldm / 32);
    const int groups = K / 8;  // groups of 8 k = one 16-byte operand load per lane
    return (tiles < 256 && groups % 16 == 0 && groups / 16 >= 4) ? 2 : 1;
}

struct ActSet {
    float *x, *r1, *r2, *r3;
    size_t p1, p2, p3;  // partial strides
};
static ActSet act_set(const fr_worker *w, int parity) {
    const int32_t *fc = w->ctx->model.fc;
    const size_t ld = (size_t)w->ld_max;
    ActSet a;
    a.x = w->d_act[parity];
    a.r1 = a.x + (size_t)fc[0] * ld;
    a.p1 = (size_t)fc[1] * ld;
    a.r2 = a.r1 + 2 * a.p1;
    a.p2 = (size_t)fc[2] * ld;
    a.r3 = a.r2 + 2 * a.p2;
    a.p3 = (size_t)fc[3] * ld;
    return a;
}

// The context's chain width: frozen by the first low-precision GEMM-layer launch of a submit / push path at min(live workers, 4) unless
// fr_ctx_set_chain_width (or a driver) decided it before; from then on only that call changes it.  Diagnostic single-layer launches
// (freeze = false) and calibration batches (fp32 stages: they never get here) read the width they would run at and freeze nothing
// ("create one worker, calibrate or warm up, then create the other three" must not pin W = 1 by accident).
static int chain_width(fr_ctx *c, bool freeze = true) {
    int w = c->chain_width.load(std::memory_order_relaxed);
    if (w) return w;
    const int live = c->n_workers.load(std::memory_order_relaxed);
    const int want = live < 1 ? 1 : (live > 4 ? 4 : live);
    if (!freeze) return want;
    int expected = 0;
    if (!c->chain_width.compare_exchange_strong(expected, want, std::memory_order_relaxed)) return expected;
    c->chain_width_auto.store(true, std::memory_order_relaxed);
    return want;
}

extern "C" int fr_ctx_set_chain_width(fr_ctx *ctx, int width) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    if (width < 0 || width > 4) FR_FAIL(FR_ERR_INVALID, "chain width %d outside [0, 4] (0 = undecided again: the next low-precision GEMM-layer launch freezes it)", width);
    ctx->chain_width.store(width, std::memory_order_relaxed);
    ctx->chain_width_auto.store(false, std::memory_order_relaxed);
    return FR_OK;
}

#ifdef FR_EXPERIMENTS
int frk_spin_probe(hipStream_t s, int wgs, int lds_bytes, unsigned ticks);
// experiments build only (no header): n spin launches on wa's stream alone, then n on each of wa's and wb's streams interleaved -> microseconds per launch
extern "C" __attribute__((visibility("default"))) int fr_exp_burst_probe(fr_worker *wa, fr_worker *wb, int n, int wgs, int lds_bytes, int ticks, float *us_alone, float *us_pair) {
    if (!wa || !wb || !us_alone || !us_pair) FR_FAIL(FR_ERR_INVALID, "bad argument");
    FR_SET_DEVICE(wa->ctx);
    hipEvent_t e[4];
    for (auto &x : e) FR_HIP(hipEventCreate(&x));
    for (int i = 0; i < 3; i++) {   // warm both
        int rc = frk_spin_probe(wa->stream, wgs, lds_bytes, (unsigned)ticks);
        if (!rc) rc = frk_spin_probe(wb->stream, wgs, lds_bytes, (unsigned)ticks);
        if (rc) return rc;
    }
    FR_HIP(hipStreamSynchronize(wa->stream));
    FR_HIP(hipStreamSynchronize(wb->stream));
    FR_HIP(hipEventRecord(e[0], wa->stream));
    for (int i = 0; i < n; i++) {
        int rc = frk_spin_probe(wa->stream, wgs, lds_bytes, (unsigned)ticks);
        if (rc) return rc;
    }
    FR_HIP(hipEventRecord(e[1], wa->stream));
    FR_HIP(hipStreamSynchronize(wa->stream));
    float ms = 0;
    FR_HIP(hipEventElapsedTime(&ms, e[0], e[1]));
    *us_alone = 1e3f * ms / n;
    FR_HIP(hipEventRecord(e[0], wa->stream));
    FR_HIP(hipEventRecord(e[2], wb->stream));
    for (int i = 0; i < n; i++) {
        int rc = frk_spin_probe(wa->stream, wgs, lds_bytes, (unsigned)ticks);
        if (!rc) rc = frk_spin_probe(wb->stream, wgs, lds_bytes, (unsigned)ticks);
        if (rc) return rc;
    }
    FR_HIP(hipEventRecord(e[1], wa->stream));
    FR_HIP(hipEventRecord(e[3], wb->stream));
    FR_HIP(hipStreamSynchronize(wa->stream));
    FR_HIP(hipStreamSynchronize(wb->stream));
    float ma = 0, mb = 0;
    FR_HIP(hipEventElapsedTime(&ma, e[0], e[1]));
    FR_HIP(hipEventElapsedTime(&mb, e[2], e[3]));
    *us_pair = 1e3f * (ma > mb ? ma : mb) / n;
    for (auto &x : e) (void)hipEventDestroy(x);
    return FR_OK;
}
#endif

extern "C" int fr_ctx_chain_width(const fr_ctx *ctx) { return ctx ? ctx->chain_width.load(std::memory_order_relaxed) : FR_ERR_INVALID; }


// ---- operand-type bank image (fr_internal.h, fr_ctx::lp_arena) ------------------------------------------------------------------------
// Which launches read one.  (a) The large-batch gather of a chain model (Model-C) on a FR_INDEX_PER_BANK context, bf16 / fp8 chain: fewer lines
// per item.  (Per-table chain contexts gain nothing there: a row is one 128-byte line whatever its element type -- that gather is bound by
// the fabric's REQUEST rate)  (b) EXPERIMENTS build only (FR_FUSED_LP_ROWS=1): the persistent bf16 fused kernel
// (fr_fused_tile_hs_kernel, any index mode) -- 8-byte row words are twice the row sets in flight in its producers' registers; measured
// slower (profiles/r06_experiments.md section 3), so frk_fused_hk_takes_lp_rows() is false in the product.
static bool lp_image_applies_hs(const fr_ctx *c) {
    return !c->cpu && c->fc_precision == FR_FC_BF16 && c->n_words > 0 && c->lp_image_on.load(std::memory_order_relaxed) != 0;
}
static bool lp_image_applies(const fr_ctx *c, int prec) {
    return !c->cpu && c->model.index_mode == FR_INDEX_PER_BANK && (prec == FR_FC_BF16 || prec == FR_FC_FP8) && c->n_words > 0 &&
           c->lp_image_on.load(std::memory_order_relaxed) != 0;
}

extern "C" int fr_ctx_set_lp_bank_image(fr_ctx *ctx, int on) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    ctx->lp_image_on.store(on ? 1 : 0, std::memory_order_relaxed);
    return FR_OK;
}
extern "C" size_t fr_ctx_lp_bank_image_bytes(const fr_ctx *ctx) { return (ctx && ctx->lp_prec) ? ctx->lp_arena.count() : 0; }
extern "C" long long fr_ctx_lp_bank_image_builds(const fr_ctx *ctx) { return ctx ? ctx->lp_builds.load(std::memory_order_relaxed) : 0; }

// Make the image current for (prec, X exponent, table contents).  Called by the launch path right before a gather that reads it; the
// rebuild runs on the context's set-up stream and is waited for (tens of milliseconds for Model-C, once per change of precision /
// calibration / table contents -- set-up calls, which by contract do not run beside a stream in flight).  Row updates (fr_worker_update_rows)
// DO run beside streams in flight and never make the image stale; a rebuild that some other change asks for first makes the set-up stream
// wait for the last update of every live worker, so that it does not read the arena under a scatter still running on another stream.
static int lp_ensure_image(fr_ctx *c, int prec) {
    const int e_x = prec == FR_FC_FP8 ? c->f8_e_act[0] : 0;
    std::lock_guard<std::mutex> lk(c->lp_mutex);
    if (c->lp_prec == prec && c->lp_e_x == e_x && c->lp_tables_gen == c->tables_gen && c->d_words_lp) return FR_OK;
    const fr_model_desc &m = c->model;
    const size_t esz = prec == FR_FC_BF16 ? 2 : 1;
    // a "bank" of the image = the tables one index addresses: a memory bank of a FR_INDEX_PER_BANK context (rows: the bank's common range),
    // a single table otherwise (rows: its own)
    const bool per_bank = m.index_mode == FR_INDEX_PER_BANK;
    struct Bank { std::vector<int> members; size_t payload_floats = 0, lp_off = 0, lp_stride = 0; uint64_t rows = 0; };
    const int n_groups = per_bank ? c->n_banks : m.n_tables;
    std::vector<int> group_of(m.n_tables, 0);
    std::vector<Bank> banks(n_groups);
    for (int t = 0; t < m.n_tables; t++) {
        group_of[t] = per_bank ? c->bank_of_table[t] : t;
        if (c->table_mem[t].resident) {
            Bank &b = banks[group_of[t]];
            b.members.push_back(t);
            b.payload_floats += (size_t)m.tables[t].dim;
            b.rows = per_bank ? (uint64_t)c->bank_rows[group_of[t]] : (uint64_t)m.tables[t].rows;
        }
    }
    auto lines_x128 = [](size_t stride, size_t bytes) {  // expected 128-byte lines per row, x128 (exact over one period) -- as for the fp32 bank rows
        size_t acc = 0;
        for (size_t r = 0; r < 128; r++) acc += ((r * stride) % 128 + bytes + 127) / 128;
        return acc;
    };
    size_t off = 0;
    for (int bi = 0; bi < n_groups; bi++) {
        Bank &b = banks[bi];
        if (b.members.empty()) continue;
        const size_t payload = b.payload_floats * esz;
        size_t best = align_up(payload, 8);
        for (size_t cand : {align_up(payload, 16), align_up(payload, 32), align_up(payload, 64), align_up(payload, 128)})
            if (lines_x128(cand, payload) < lines_x128(best, payload)) best = cand;
        b.lp_stride = best;
        b.lp_off = align_up(off, 256);
        off = b.lp_off + (size_t)b.rows * best;
    }
    off = align_up(off, 256);
    FR_SET_DEVICE(c);
    {
        std::lock_guard<std::mutex> g(c->workers_mutex);
        for (fr_worker *w : c->workers)
            if (w->update_recorded) FR_HIP(hipStreamWaitEvent(c->setup_stream, w->ev_update, 0));
    }
    if (off != c->lp_arena.count()) {
        c->lp_prec = 0;
        FR_TRY(c->lp_arena.alloc(FrMem::DEVICE, off, "operand-type bank image"));
    }
    std::vector<size_t> lp_base(m.n_tables, 0);   // offset of (row 0, column 0) of every resident table inside lp_arena
    c->lp_tables.assign(m.n_tables, fr_ctx::LpTable{});
    for (Bank &b : banks) {
        size_t col = 0;
        for (int t : b.members) {
            const FrTableMem &tm = c->table_mem[t];
            lp_base[t] = b.lp_off + col * esz;
            // a table's reachable rows: the bank-interleaved region (il_rows = the bank's rows), or a lone table's own rows
            int rc = frk_convert_rows_lp(prec, c->table_arena + tm.byte_offset, (size_t)tm.row_stride, c->lp_arena + lp_base[t], b.lp_stride, (int64_t)b.rows, m.tables[t].dim, e_x,
                                         c->setup_stream);
            if (rc) return rc;
            c->lp_tables[t].base = lp_base[t];
            c->lp_tables[t].stride = b.lp_stride;
            c->lp_tables[t].rows = b.rows;
            col += (size_t)m.tables[t].dim;
        }
    }
    std::vector<FrWordDesc> lw(c->h_words);
    for (int i = 0; i < c->n_words; i++) {
        const int t = c->h_word_table[i];
        if (t < 0) continue;   // dense words come from the request, in fp32
        lw[i].src = (uint64_t)(uintptr_t)(c->lp_arena + lp_base[t]) + (uint64_t)c->h_word_col[i] * esz;
        lw[i].stride = (uint32_t)banks[group_of[t]].lp_stride;
    }
    FR_TRY(c->d_words_lp.grow(FrMem::DEVICE, (size_t)c->n_words, "word descriptors of the bank image"));
    FR_HIP(hipMemcpyAsync(c->d_words_lp, lw.data(), sizeof(FrWordDesc) * c->n_words, hipMemcpyHostToDevice, c->setup_stream));
    FR_HIP(hipStreamSynchronize(c->setup_stream));
    c->lp_prec = prec;
    c->lp_e_x = e_x;
    c->lp_tables_gen = c->tables_gen;
    c->lp_builds.fetch_add(1, std::memory_order_relaxed);
    return FR_OK;
}

// Issue ONE pipeline launch: every in-flight batch advances by one stage; `fresh` (may be NULL) enters at stage 0.
// only_stage >= 0: debugging/roofline -- run just that stage of the (single) in-flight batch as its own kernel.
static int pipeline_step(fr_worker *w) {
    fr_ctx *c = w->ctx;
    const int32_t *fc = c->model.fc;
    const uint64_t L = w->launch_no;
    const int par = (int)(L & 1);
    const ActSet wr = act_set(w, par), rd = act_set(w, par ^ 1);
    const int prec = w->calibrating ? (int)FR_FC_FP32 : c->fc_precision;  // a calibration batch runs the fp32 chain
    FrPipeArgs a{};
    a.words = c->d_words;
    a.n_words = c->n_words;
    a.idx_stride = (int)idx_cols(c);
    a.err_flag = w->d_err;
    a.stamps = g_stamp_buffer;
    int blocks = 0, n_stages = 0, only = -1;
    for (int s = 0; s < FR_N_STAGES; s++) {
        FrStageArgs &st = a.st[s];
        st.block_begin = blocks;
        if (L < (uint64_t)s) continue;
        fr_worker::Slot &sl = w->ring[(L - s) % 8];
        if (!sl.active || sl.launch0 != L - s || s < sl.first_stage) continue;
        st.batch = sl.batch;
        st.ldm = sl.ldm;
        const int ldm = sl.ldm;
        // K-split plan of the three FC layers of this batch
        const bool bf16 = prec == FR_FC_BF16, fp8 = prec == FR_FC_FP8;  // no K-split partials in the low-precision chains
        const bool one = bf16 || fp8 || w->calibrating;                // (nor while calibrating: whole activations are measured)
        const int ns1 = one ? 1 : pick_nsplit(fc[0], fc[1], ldm), ns2 = one ? 1 : pick_nsplit(fc[1], fc[2], ldm),
                  ns3 = one ? 1 : pick_nsplit(fc[2], fc[3], ldm);
        const float *wl[4];
        for (int l = 0; l < 4; l++) {
            if (bf16) wl[l] = reinterpret_cast<const float *>(c->d_w_bf16[l].p);
            else if (fp8 && l < 3) wl[l] = reinterpret_cast<const float *>(c->d_w_fp8[l].p);
            else wl[l] = (l < 3 && !fp8) ? c->d_wq[l] : c->d_w[3];
        }
        if (fp8) {  // power-of-two quantisation exponents of this stage's operands / result
            st.e_w = (s >= 1 && s <= 3) ? c->f8_e_w[s - 1] : 0;
            st.e_in = s >= 1 ? c->f8_e_act[s - 1] : 0;
            st.e_out = s <= 3 ? c->f8_e_act[s] : 0;
        }
        switch (s) {
            case 0: {
                a.idx = sl.d_idx;
                a.dense = sl.d_dense;
                st.out = wr.x;
                st.K = fc[0];
                w->last_x_parity = par;
                const int trv = frk_gather_tr_variant(sl.batch, a.idx_stride);
                const int trb = frk_gather_tr_blocks(c->n_words, ldm, trv);
                if (trb > 0) {  // large batch: LDS-transposing gather
                    st.variant = trv;
                    if (trv == 2 && lp_image_applies(c, prec)) {   // ... of bank rows that are already in the chain's operand type
                        const int irc = lp_ensure_image(c, prec);
                        if (irc == FR_ERR_OOM) {
                            // no HBM left for the image: the gather reads the fp32 rows and converts them itself -- the same scores, bit for bit
                            c->lp_image_on.store(0, std::memory_order_relaxed);
                        } else if (irc) {
                            return irc;
                        } else {
                            a.words = c->d_words_lp;
                            a.src_lp = 1;
                        }
                    }
                    blocks += (trb + 7) / 8 * 8;
                    n_stages++;
                    only = s;
                    continue;
                }
                if (fp8) {  // the q16 gather has its own grid shape
                    blocks += frk_stage_blocks_f8_gather(fc[0], ldm);
                    n_stages++;
                    only = s;
                    continue;
                }
                break;
            }
            case 1:
                st.K = fc[0]; st.N = fc[1]; st.nsplit = ns1; st.nparts_in = 1;
                st.in = rd.x; st.in_part_stride = 0; st.out = wr.r1; st.part_stride = (int)wr.p1; st.w = wl[0];
                break;
            case 2:
                st.K = fc[1]; st.N = fc[2]; st.nsplit = ns2; st.nparts_in = ns1;
                st.in = rd.r1; st.in_part_stride = (int)rd.p1; st.out = wr.r2; st.part_stride = (int)wr.p2; st.w = wl[1];
                break;
            case 3:
                st.K = fc[2]; st.N = fc[3]; st.nsplit = ns3; st.nparts_in = ns2;
                st.in = rd.r2; st.in_part_stride = (int)rd.p2; st.out = wr.r3; st.part_stride = (int)wr.p3; st.w = wl[2];
                break;
            case 4:
                st.K = fc[3]; st.N = 1; st.nsplit = 1; st.nparts_in = ns3;
                st.in = rd.r3; st.in_part_stride = (int)rd.p3; st.out = sl.d_scores; st.w = wl[3];
                break;
        }
        // the context's epilogues (fr_ctx_set_epilogue): a stage that stores whole sums applies its own layer's; a split stage stores raw partials and
        // the stage that combines them (nparts_in == 2) applies the producing layer's to their sum -- one fp32 add after the WHOLE K sum either way
        if (s >= 1) {
            if (st.nsplit == 1) a.epi[s] = c->epi(s - 1);
            if (s >= 2 && st.nparts_in == 2) a.epi_in[s] = c->epi(s - 2);
            a.has_epi = c->any_epi() ? 1 : 0;
        }
        if (s == 3 && st.nparts_in == 1 && st.nsplit == 1 && !w->calibrating && frk_fc_lp_gemm_ok(prec, st.K, st.N, ldm) && frk_fc_tail_ok(prec, st.K, st.N, ldm)) {
            // large batch, bf16 / fp8: FC3 and the output layer of this batch in ONE launch (fc_tail_kernel); the batch leaves the pipeline here
            int rc = frk_fc_tail(prec, st.w, st.in, wl[3], sl.d_scores, st.K, st.N, ldm, sl.batch, st.e_w, st.e_in, st.e_out, a.epi[s], c->epi(3), w->stream);
            if (rc) return rc;
            st.batch = 0;
            sl.active = false;
            w->n_active--;
            continue;
        }
        if (s >= 1 && s <= 3 && st.nparts_in == 1 && st.nsplit == 1 && frk_fc_lp_gemm_ok(prec, st.K, st.N, ldm)) {
            // a layer big enough to fill the chip alone runs as its own LDS-tiled GEMM launch (same stream, same step)
            // a MINOR layer (at most half the work of the chain's heaviest) may sit on fewer CUs than its share: see lp_gemm_mu
            long heaviest = 0;
            for (int l = 0; l < 3; l++) heaviest = std::max(heaviest, (long)fc[l] * fc[l + 1]);
            const bool minor = 2 * (long)st.K * st.N <= heaviest;
            int rc = frk_fc_lp_gemm(prec, st.w, st.in, st.out, st.K, st.N, ldm, st.e_w, st.e_in, st.e_out, prec == FR_FC_FP32 ? 1 : chain_width(c, !w->diag_launch), minor, a.epi[s], w->stream);
            if (rc) return rc;
            st.batch = 0;  // inactive in the combined launch
            continue;
        }
        blocks += frk_stage_blocks(s, c->n_words, st.K, st.N, ldm, st.nsplit);
        n_stages++;
        only = s;
        if (s == FR_N_STAGES - 1) {  // the batch leaves the pipeline with this launch
            sl.active = false;
            w->n_active--;
        }
    }
    a.n_blocks = blocks;
    w->launch_no = L + 1;
    if (n_stages == 0) return FR_OK;
    if (n_stages == 1) {  // a lone stage runs as its own, separately named kernel (rocprof attribution)
        const int begin = a.st[only].block_begin;
        for (int s = 0; s < FR_N_STAGES; s++) a.st[s].block_begin -= (s >= only) ? begin : 0;
        a.st[only].block_begin = 0;
        return frk_pipeline_launch(a, only, prec, w->stream);
    }
    return frk_pipeline_launch(a, -1, prec, w->stream);
}

static int pipeline_push(fr_worker *w, int batch, int first_stage, const int32_t *d_idx, const float *d_dense, float *d_scores) {
    const uint64_t L0 = w->launch_no - (uint64_t)first_stage;  // launch number its (virtual) stage 0 had
    fr_worker::Slot &sl = w->ring[L0 % 8];
    if (sl.active) FR_FAIL(FR_ERR_STATE, "internal: pipeline ring slot still busy");
    sl.active = true;
    sl.launch0 = L0;
    sl.first_stage = first_stage;
    sl.batch = batch;
    sl.ldm = round_up(batch, 32);
    sl.d_idx = d_idx;
    sl.d_dense = d_dense;
    sl.d_scores = d_scores;
    w->n_active++;
    return pipeline_step(w);
}

static int pipeline_flush(fr_worker *w) {
    while (w->n_active > 0) {
        int rc = pipeline_step(w);
        if (rc) return rc;
    }
    return FR_OK;
}

// ---- fused item-tile path (fr_fused_tile_kernel): used by the streaming push for models whose activations fit in LDS --
// Batches per fused launch: a per-CONTEXT knob (fr_ctx_set_stream_group; env FR_FUSED_GROUP sets the initial value of every new
// context).  64 batches of 256 = one 64-item workgroup per CU, so ONE stream's launch fills the chip; lower it to trade throughput
// for latency.  Atomic: driver threads read it while a control thread may change it.
static int fused_group_initial() {
    const int g = FR_KNOB_ONCE("FUSED_GROUP", FR_FUSED_DEFAULT_BATCHES);
    return g < 1 ? 1 : (g > FR_FUSED_MAX_QUEUE ? FR_FUSED_MAX_QUEUE : g);
}
static int fused_group(const fr_ctx *c) { return c->stream_group.load(std::memory_order_relaxed); }

static bool fused_eligible(const fr_ctx *c) {
    const int enabled = FR_KNOB_ONCE("FUSED", 1);  // experiment knob
    const int32_t *fc = c->model.fc;
    if (!enabled || c->n_shards != 1 || c->model.layout != FR_LAYOUT_SEMANTIC) return false;
    if (c->fc_precision == FR_FC_FP8) return frk_fused_f8_ok(fc[0], fc[1], fc[2], fc[3]);
    // bf16: the chunked kernel exists for the two reference records (352 / 880 floats); any other record the K-outer persistent kernel
    // accepts (64 .. 880 floats in whole k-groups, frk_fused_hk_ok) streams through that kernel at every launch size
    // (... unless the context has an epilogue, which that kernel does not carry: see fr_fused_flush)
    if (c->fc_precision == FR_FC_BF16) return frk_fused_h_ok(fc[0], fc[1], fc[2], fc[3]) || (c->hk_ok == 1 && !c->any_epi());
    return frk_fused_ok(fc[0], fc[1], fc[2], fc[3]);
}

// Batches one streaming launch carries on this context: 1 for the stage pipeline, the fused kernel's group otherwise.
extern "C" int fr_ctx_set_stream_group(fr_ctx *ctx, int batches_per_launch) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    if (batches_per_launch < 1 || batches_per_launch > FR_FUSED_MAX_QUEUE)
        FR_FAIL(FR_ERR_INVALID, "batches_per_launch %d outside [1, %d]", batches_per_launch, FR_FUSED_MAX_QUEUE);
    ctx->stream_group.store(batches_per_launch, std::memory_order_relaxed);  // queues already holding more are launched by their next push / sync
    return FR_OK;
}

extern "C" int fr_ctx_set_small_block(fr_ctx *ctx, int max_batches) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    if (max_batches < 0 || max_batches > 8) FR_FAIL(FR_ERR_INVALID, "max_batches %d outside [0, 8]", max_batches);
    ctx->small_block.store(max_batches, std::memory_order_relaxed);
    return FR_OK;
}

extern "C" int fr_ctx_stream_group(const fr_ctx *ctx) { return (ctx && !ctx->cpu && fused_eligible(ctx)) ? fused_group(ctx) : 1; }   // (a CPU context computes every push at once)

// One launch of the kernarg-fed fused kernels: batches [first, first + n) of the worker's queue (n <= FR_FUSED_MAX_BATCHES).
static int fused_launch_slice(fr_worker *w, FrFusedArgs &a, int first, int n) {
    fr_ctx *c = w->ctx;
    const bool bf16 = c->fc_precision == FR_FC_BF16, fp8 = c->fc_precision == FR_FC_FP8;
    // fp32: the 64-item kernel needs 64 queued batches to cover the chip; smaller groups keep the 32-item kernel (experiments: FR_FUSED_M2=0/1 forces)
    const int m2_forced = FR_KNOB_ONCE("FUSED_M2", -1);
    // ... and a PARTIAL launch (fr_worker_sync with a few batches queued) that would put 64-item workgroups on at most half of the CUs
    // takes the 32-item kernel as well: twice the workgroups, 133 instead of 236 us each, bit-identical scores
    int tiles64 = 0;
    for (int i = 0; i < n; i++) tiles64 += (w->pending[first + i].batch + 63) / 64;
    const bool m2 = !bf16 && c->fc_precision == FR_FC_FP32 && frk_fused_m2_ok(c->model.fc[0], c->model.fc[1], c->model.fc[2], c->model.fc[3]) &&
                    (m2_forced == 1 || (m2_forced != 0 && fused_group(c) >= 64 && tiles64 > 128));
    const int per_wg = (bf16 || fp8) ? frk_fused_h_items_per_wg() : (m2 ? 64 : 32);  // items per workgroup
    int max_tiles = 0;
    for (int i = 0; i < n; i++) {
        a.b[i] = w->pending[first + i];
        const int tiles = (a.b[i].batch + per_wg - 1) / per_wg;
        if (tiles > max_tiles) max_tiles = tiles;
    }
    a.n_batches = n;
    a.tiles_per_batch = max_tiles;
    a.blist = nullptr;
    if (fp8) return frk_fused_f8_launch(a, w->stream);
    if (m2) return frk_fused_m2_launch(a, w->stream);
    if (bf16) return frk_fused_h_launch(a, w->stream);
    return frk_fused_launch(a, w->stream);
}

int fr_fused_flush(fr_worker *w) {
    if (w->n_pending == 0) return FR_OK;
    fr_ctx *c = w->ctx;
    FrFusedArgs a{};
    const bool bf16 = c->fc_precision == FR_FC_BF16, fp8 = c->fc_precision == FR_FC_FP8;
    a.words = c->d_words;
    a.n_words = c->n_words;
    a.idx_stride = (int)idx_cols(c);
    a.err_flag = w->d_err;
    if (fp8) {  // e4m3 q16 copies of FC1..FC3, fp32 output weights, the quantisation exponents
        a.w1q = reinterpret_cast<const float4 *>(c->d_w_fp8[0].p);
        a.w2q = reinterpret_cast<const float4 *>(c->d_w_fp8[1].p);
        a.w3q = reinterpret_cast<const float4 *>(c->d_w_fp8[2].p);
        a.wout = c->d_w[3];
        for (int l = 0; l < 3; l++) a.e_w[l] = c->f8_e_w[l];
        for (int l = 0; l < 4; l++) a.e_act[l] = c->f8_e_act[l];
    } else if (bf16) {  // the bf16 kernels read the q8-packed bf16 copies through the same argument slots
        a.w1q = reinterpret_cast<const float4 *>(c->d_w_bf16[0].p);
        a.w2q = reinterpret_cast<const float4 *>(c->d_w_bf16[1].p);
        a.w3q = reinterpret_cast<const float4 *>(c->d_w_bf16[2].p);
        a.wout = reinterpret_cast<const float *>(c->d_w_bf16[3].p);
    } else {
        a.w1q = reinterpret_cast<const float4 *>(c->d_wq[0].p);
        a.w2q = reinterpret_cast<const float4 *>(c->d_wq[1].p);
        a.w3q = reinterpret_cast<const float4 *>(c->d_wq[2].p);
        a.wout = c->d_w[3];
    }
    if (c->any_epi())   // the epilogue forms of the fused kernels are branch-free: a layer without a bias adds -0.0f
        for (int l = 0; l < 4; l++) a.epi[l] = FrEpi{c->has_bias[l] ? c->d_bias[l].p : c->d_negzero.p, c->act[l] == FR_ACT_RELU ? 1 : 0, 0};
    a.K = c->model.fc[0];
    a.H1 = c->model.fc[1];
    a.H2 = c->model.fc[2];
    a.H3 = c->model.fc[3];
    a.stamps = g_stamp_buffer;
    const int n_all = w->n_pending;
    w->n_pending = 0;
    w->pending_items = 0;
    struct Keep {  // whichever launcher returns below, the worker remembers the kernel it enqueued
        fr_worker *w;
        ~Keep() { keep_kernel(w); }
    } keep{w};
    // (fp8: the persistent kernel's fp8 form exists in the experiments build only and is opt-in there, FR_FUSED_HK=1 -- it is slower than the chunked fp8 kernel)
    if (bf16 || (fp8 && FR_KNOB_ONCE("FUSED_HK", -1) == 1 && c->d_w_fp8h[0] && c->d_w_fp8h[1] && c->d_w_fp8h[2])) {
        // The K-outer, persistent, wave-specialised kernel (fr_fused_ko.hip; bf16 and fp8 forms) whenever the context's descriptors fit its packed form AND the
        // launch gives every workgroup at least two tiles: the first tile of a workgroup pays the whole dependent chain index -> row -> LDS
        // (13-14 us, all workgroups at once), which only a second tile amortises.  Smaller launches (64 batches of 256 items = one tile per
        // compute unit, partial groups at fr_worker_sync) keep the chunked kernel.  Its batch list travels through device memory, so one
        // launch carries up to FR_FUSED_MAX_QUEUE batches (fr_ctx_set_stream_group above 64).
        int tiles = 0, max_tiles = 0;
        for (int i = 0; i < n_all; i++) {
            const int t_ = (w->pending[i].batch + 63) / 64;
            tiles += t_;
            if (t_ > max_tiles) max_tiles = t_;
        }
        const int hk = FR_KNOB_ONCE("FUSED_HK", -1);  // experiments build: 0 = never, 1 = whenever it applies
        // Where the persistent kernel starts to pay (re-measured in round 4, after its scratch was removed: profiles/archive/r04_fused_hs_threshold.txt):
        // K <= 352 (Model-A) level with the chunked kernel at ONE tile per compute unit (451 vs 452 M inf/s, the kernel alone 46.4 vs 49.0 us)
        // and 10-30 % ahead from 1.25 on; K = 880 (Model-B) 5 % behind at one tile (305 vs 320 M), 5 % ahead at 1.25, level at 1.5, 6 % ahead at 2.
        const int hs_from = a.K <= 352 ? c->n_cu : c->n_cu + c->n_cu / 4;
        const bool only_hs = bf16 && !frk_fused_h_ok(a.K, a.H1, a.H2, a.H3);   // a record the chunked kernel has no instantiation for
        // A context WITH an epilogue never takes the persistent kernel: its consumers hold 128 accumulators in a budget of 168 registers and FC1's tile
        // stores run beside the first half of FC2's weight ring -- nothing is left for the bias fragments without scratch.  Its launches stay on the
        // chunked fr_fused_tile_h_kernel (fused_eligible() has already sent a record that kernel has no instantiation for to the stage pipeline).
        if (c->hk_ok == 1 && !c->any_epi() && (only_hs || (hk != 0 && (hk == 1 || tiles >= hs_from)))) {
            if (!w->ev_blist[FR_BLIST_RING - 1]) {   // first use (a partial failure is made up for: grow and create keep what is there)
                FR_TRY(w->h_blist.grow(FrMem::PINNED, (size_t)FR_FUSED_MAX_QUEUE * FR_BLIST_RING, "batch lists"));
                FR_TRY(w->d_blist.grow(FrMem::DEVICE, (size_t)FR_FUSED_MAX_QUEUE * FR_BLIST_RING, "batch lists (device)"));
                for (FrEvent &e : w->ev_blist) FR_HIP(e.create(hipEventDisableTiming));
            }
            const int k = w->blist_cur;
            w->blist_cur = (k + 1) % FR_BLIST_RING;
            if (w->blist_busy[k]) FR_HIP(hipEventSynchronize(w->ev_blist[k]));  // the copy that read this host block four launches ago has executed
            FrFusedBatch *hb = w->h_blist + (size_t)k * FR_FUSED_MAX_QUEUE, *db = w->d_blist + (size_t)k * FR_FUSED_MAX_QUEUE;
            memcpy(hb, w->pending, sizeof(FrFusedBatch) * n_all);
            FR_HIP(hipMemcpyAsync(db, hb, sizeof(FrFusedBatch) * n_all, hipMemcpyHostToDevice, w->stream));
            FR_HIP(hipEventRecord(w->ev_blist[k], w->stream));
            w->blist_busy[k] = true;
            a.blist = db;
            a.n_batches = n_all;
            a.tiles_per_batch = max_tiles;
            if (bf16 && frk_fused_hk_takes_lp_rows(a.K) && lp_image_applies_hs(c)) {   // rows already bf16: twice the row sets in flight in the producers' registers
                const int irc = lp_ensure_image(c, FR_FC_BF16);
                if (irc) return irc;
                a.words = c->d_words_lp;
                a.src_lp = 1;
            }
            if (bf16 && FR_KNOB_ONCE("FUSED_HS_ABLATE", 0)) a.e_act[3] = -776 - FR_KNOB_ONCE("FUSED_HS_ABLATE", 0);   // experiments build: the kernel's timing ablations (1: no row loads, 2: every row load reads row 0)
            if (fp8) {  // the "q16h" copies of the weights (the non-scaled fp8 MFMA's operand layout)
                a.w1q = reinterpret_cast<const float4 *>(c->d_w_fp8h[0].p);
                a.w2q = reinterpret_cast<const float4 *>(c->d_w_fp8h[1].p);
                a.w3q = reinterpret_cast<const float4 *>(c->d_w_fp8h[2].p);
            }
            return frk_fused_hk_launch(a, c->n_cu, c->fc_precision, w->stream);
        }
    }
    for (int first = 0; first < n_all; first += FR_FUSED_MAX_BATCHES) {  // the kernarg-fed kernels: slices of at most 64 batches
        const int n = n_all - first < FR_FUSED_MAX_BATCHES ? n_all - first : FR_FUSED_MAX_BATCHES;
        int rc = fused_launch_slice(w, a, first, n);
        if (rc) return rc;
    }
    return FR_OK;
}

static int check_gather_args(fr_worker *w, const int32_t *d_idx, const float *d_dense) {
    fr_ctx *c = w->ctx;
    if (!d_idx) FR_FAIL(FR_ERR_INVALID, "d_idx is NULL");
    if (c->model.dense_len && !d_dense) FR_FAIL(FR_ERR_INVALID, "model has dense features but d_dense is NULL");
    return FR_OK;
}

// fc_only diagnostic: item-major records in the model's layout -> scores (pipeline must be idle)
static int launch_fc(fr_worker *w, int batch, const float *d_records, float *d_scores) {
    fr_ctx *c = w->ctx;
    if (c->n_shards > 1) FR_FAIL(FR_ERR_STATE, "fc on a sharded ctx needs the all-gathered records (use the sharded driver: fr_worker_submit_sharded, fr_worker_submit_sharded_pooled)");
    if (c->cpu) {
        const float *const wl[4] = {c->d_w[0], c->d_w[1], c->d_w[2], c->d_w[3]};
        const FrEpi ep[4] = {c->epi(0), c->epi(1), c->epi(2), c->epi(3)};
        frc_fc_chain(c->model.fc, wl, ep, d_records, batch, w->c_scratch, d_scores);
        return FR_OK;
    }
    if (w->n_active) FR_FAIL(FR_ERR_STATE, "pipeline busy: call fr_worker_sync first");
    if (w->launch_no == 0) w->launch_no = 1;  // stage 1 of the next launch reads the set the (virtual) previous launch wrote
    const int ldm = round_up(batch, 32);
    const int par_prev = (int)((w->launch_no - 1) & 1);
    int rc;
    if (c->fc_precision == FR_FC_FP8) rc = frk_records_to_q16_fp8(d_records, act_set(w, par_prev).x, batch, c->model.fc[0], ldm, c->f8_e_act[0], w->stream);
    else if (c->fc_precision == FR_FC_BF16) rc = frk_records_to_q8_bf16(d_records, act_set(w, par_prev).x, batch, c->model.fc[0], ldm, w->stream);
    else rc = frk_transpose_records(d_records, act_set(w, par_prev).x, batch, c->model.fc[0], ldm, w->stream);
    if (rc) return rc;
    rc = pipeline_push(w, batch, 1, nullptr, nullptr, d_scores);
    if (rc) return rc;
    return pipeline_flush(w);
}

// Sharded mode, after the all-gather: d_gathered = [n_shards][batch_total][slice_padded] floats (every shard's padded slice,
// item-major).  Runs the FC chain for items [item0, item0 + n_items) of the batch; d_scores receives n_items floats.
// Shared body of fr_worker_fc_from_slices / fr_worker_calibrate_fp8_slices.  Returns the launch number the batch's stage 1 ran in.
static int fc_from_slices_impl(fr_worker *w, int batch_total, int item0, int n_items, const float *d_gathered, float *d_scores, uint64_t *stage1_launch) {
    int rc = check_ready(w, n_items, false, true);
    if (rc) return rc;
    fr_ctx *c = w->ctx;
    if (!d_gathered || !d_scores) FR_FAIL(FR_ERR_INVALID, "NULL device pointer");
    if (batch_total < 1 || item0 < 0 || item0 + n_items > batch_total) FR_FAIL(FR_ERR_INVALID, "items [%d,+%d) outside batch %d", item0, n_items, batch_total);
    if (w->n_active || w->n_pending) FR_FAIL(FR_ERR_STATE, "pipeline busy: call fr_worker_sync first");
    if (c->cpu) {
        if (c->n_shards < 2) FR_FAIL(FR_ERR_STATE, "fc_from_slices needs a sharded context");
        frc_slices_to_records(d_gathered, c->n_shards, batch_total, c->slice_padded, c->shard_offset.data(), c->shard_len.data(), item0, n_items, w->c_x, c->model.fc[0]);
        const float *const wl[4] = {c->d_w[0], c->d_w[1], c->d_w[2], c->d_w[3]};
        const FrEpi ep[4] = {c->epi(0), c->epi(1), c->epi(2), c->epi(3)};
        frc_fc_chain(c->model.fc, wl, ep, w->c_x, n_items, w->c_scratch, d_scores);
        return FR_OK;
    }
    FR_SET_DEVICE(c);
    if (w->launch_no == 0) w->launch_no = 1;
    const int ldm = round_up(n_items, 32);
    const int par_prev = (int)((w->launch_no - 1) & 1);
    const int prec = w->calibrating ? (int)FR_FC_FP32 : c->fc_precision;
    // the slices arrive as fp32: transpose them into q4 elements, then (low-precision chains) re-pack that image; the other
    // activation set's X region is free scratch while the pipeline is idle
    float *xq = prec == FR_FC_FP32 ? act_set(w, par_prev).x : act_set(w, par_prev ^ 1).x;
    rc = frk_transpose_slices(d_gathered, c->n_shards, batch_total, c->slice_padded, c->shard_offset.data(), c->shard_len.data(), item0, n_items, xq, ldm,
                              w->stream);
    if (rc) return rc;
    if (prec != FR_FC_FP32) {
        rc = frk_q4_to_lp(prec, xq, act_set(w, par_prev).x, c->model.fc[0], ldm, c->f8_e_act[0], w->stream);
        if (rc) return rc;
    }
    if (stage1_launch) *stage1_launch = w->launch_no;
    rc = pipeline_push(w, n_items, 1, nullptr, nullptr, d_scores);
    if (rc) return rc;
    return pipeline_flush(w);
}

// Sharded mode, after the all-gather: d_gathered = [n_shards][batch_total][slice_padded] floats (every shard's padded slice,
// item-major).  Runs the FC chain (in the context's precision) for items [item0, item0 + n_items) of the batch; d_scores
// receives n_items floats.
extern "C" int fr_worker_fc_from_slices(fr_worker *w, int batch_total, int item0, int n_items, const float *d_gathered, float *d_scores) {
    if (!w) FR_FAIL(FR_ERR_INVALID, "worker is NULL");
    int rc = fc_from_slices_impl(w, batch_total, item0, n_items, d_gathered, d_scores, nullptr);
    if (rc) return rc;
    w->in_flight = true;
    return FR_OK;
}

// whole hot path for ONE batch, unpipelined: index rows -> scores (five dependent launches)
static int launch_pipeline(fr_worker *w, int batch, const int32_t *d_idx, const float *d_dense, float *d_scores) {
    fr_ctx *c = w->ctx;
    if (c->n_shards > 1) FR_FAIL(FR_ERR_STATE, "submit on a sharded ctx: use the sharded driver (gather_only + all-gather + fc_only)");
    if (c->cpu) {   // the record in the model's layout (SEMANTIC, or the 3-node buffer read as B x K item-major), then the chain
        int rc = launch_gather(w, batch, d_idx, d_dense, w->d_records);
        if (rc) return rc;
        return launch_fc(w, batch, w->d_records, d_scores);
    }
    if (c->model.layout != FR_LAYOUT_SEMANTIC) {
        // literal 3-node buffer arithmetic (F8): materialise the blocked records, then read them as B x K item-major
        int rc = launch_gather(w, batch, d_idx, d_dense, w->d_records);
        if (rc) return rc;
        return launch_fc(w, batch, w->d_records, d_scores);
    }
    int rc = check_gather_args(w, d_idx, d_dense);
    if (rc) return rc;
    rc = pipeline_push(w, batch, 0, d_idx, d_dense, d_scores);
    if (rc) return rc;
    return pipeline_flush(w);
}

extern "C" int fr_worker_gather_only(fr_worker *w, int batch, const int32_t *d_idx, const float *d_dense, float *d_records) {
    int rc = gather_ready(w, batch, d_records, "d_records", FR_FC_FP32);
    if (rc) return rc;
    rc = launch_gather(w, batch, d_idx, d_dense, d_records);
    keep_kernel(w);
    if (rc) return rc;
    w->in_flight = true;
    return FR_OK;
}

// ---- multi-hot pooled lookups (fleetrec_serving.h) -------------------------------------------------------
// Pooling is stated per index column; the pooled descriptors (one FrPoolDesc per FrWordDesc) follow from h_words: a TABLE / COPY word's bag
// is its index column's, a DENSE word is a bag of one.  The column's mode (fr_ctx_set_pooling_modes) rides in the descriptor's hots word.
// what every stream-ordered worker call but a host-fed push itself says while host-fed batches wait in a block that has not been launched
int fr_host_fed_queued(fr_worker *w, const char *verb) {
    int queued = 0;
    (void)fr_worker_host_pending(w, &queued, nullptr, nullptr);
    if (queued > 0 || w->hr.staged)
        FR_FAIL(FR_ERR_STATE, "host-fed batches are queued on this worker (fr_worker_push_host / push_staged): flush first (fr_worker_flush), then %s", verb);
    return FR_OK;
}

int fr_pooling_busy(fr_ctx *ctx, const char *who) {
    std::lock_guard<std::mutex> g(ctx->workers_mutex);
    for (const fr_worker *w : ctx->workers)
        if (w->in_flight || w->n_active || w->n_pending || w->sh_comm)
            FR_FAIL(FR_ERR_STATE, "%s: a worker of the context has work in flight: call fr_worker_sync first", who);
    return FR_OK;
}

// The request-form descriptor tables (further below) follow the pooling: they are PREPARED for the hots about to be installed -- built and
// uploaded beside the ones in use -- before any pooling state changes, and committed together with it (a commit cannot fail).
struct RequestTables {
    fr_ctx::ReqForm f[3];
    FrBuf<int32_t> d;       // the new device allocation (GPU contexts with a split): the context's own once committed, released with this otherwise
    bool made = false;      // false: the context has no split, nothing to commit
};
static int request_prepare(fr_ctx *ctx, const std::vector<int32_t> &shared, bool dense_shared, const int32_t *hots, RequestTables &t);   // hots NULL: no pooling
static void request_commit(fr_ctx *ctx, RequestTables &t);

// the descriptors of hots[] x modes[] (modes == NULL: every column SUM), uploaded; the context's copies are replaced only when all of it worked
static int pooling_install(fr_ctx *ctx, const int32_t *hots, const int32_t *modes) {
    const int cols = (int)idx_cols(ctx);
    RequestTables rt;   // a request split survives: its pooled widths follow the new hots
    const int rrc = request_prepare(ctx, ctx->req_shared, ctx->req_dense_shared, hots, rt);
    if (rrc) return rrc;
    std::vector<uint32_t> prefix(cols + 1, 0);
    int max_hots = 1;
    bool wide = true, any_mean = false;
    for (int c = 0; c < cols; c++) {
        prefix[c + 1] = prefix[c] + (uint32_t)hots[c];
        max_hots = hots[c] > max_hots ? hots[c] : max_hots;
        wide = wide && hots[c] % 4 == 0;   // then every bag starts on a multiple of 4 slots too, and so does every item's row
        any_mean = any_mean || (modes && modes[c] == FR_POOL_MEAN);
    }
    // a second array for the offsets (CSR) form: the word needs its COLUMN there (its bag is found through offsets[b * cols + col]), hots is the cap
    std::vector<FrPoolDesc> pool(ctx->h_words.size()), csr(ctx->h_words.size());
    for (size_t i = 0; i < pool.size(); i++) {
        const uint32_t col = ctx->h_words[i].idx_col;
        pool[i] = (col & FR_DESC_DENSE) ? FrPoolDesc{0u, 1u}
                                        : FrPoolDesc{prefix[col], (uint32_t)hots[col] | (modes && modes[col] == FR_POOL_MEAN ? FR_POOL_DESC_MEAN : 0u)};
        csr[i] = (col & FR_DESC_DENSE) ? FrPoolDesc{0u, 1u} : FrPoolDesc{col, pool[i].hots};
    }
    if (!ctx->cpu) {
        FrBuf<FrPoolDesc> d;   // (released on every way out; the context's own after the swap)
        const size_t n = pool.size();
        FR_TRY(d.alloc(FrMem::DEVICE, n ? 2 * n : 1, "pooled descriptors"));
        hipError_t e = hipMemcpy(d, pool.data(), sizeof(FrPoolDesc) * n, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d + n, csr.data(), sizeof(FrPoolDesc) * n, hipMemcpyHostToDevice);
        if (e != hipSuccess) FR_FAIL(FR_ERR_HIP, "hipMemcpy(pooled descriptors) failed: %s", hipGetErrorString(e));
        ctx->d_pool.swap(d);
        ctx->d_pool_csr = ctx->d_pool + n;
    }
    std::vector<int32_t> h(hots, hots + cols), md(cols, FR_POOL_SUM);   // (hots may be ctx->pool_hots itself: copied before it is replaced)
    if (modes) md.assign(modes, modes + cols);
    ctx->h_pool.swap(pool);
    ctx->h_pool_csr.swap(csr);
    ctx->pool_hots.swap(h);
    ctx->pool_modes.swap(md);
    ctx->pool_any_mean = any_mean;
    ctx->pool_cols = (int)prefix[cols];
    ctx->pool_max_hots = max_hots;
    ctx->pool_wide = wide;
    request_commit(ctx, rt);
    return FR_OK;
}

// A sharded context's pooling is stated when the context is created and never changes: every rank of a job must agree on the pooled row layout, and
// exchange and worker buffers are sized once.  fr_ctx_create_sharded followed by pooling_install -- the descriptors follow the shard's own h_words.
extern "C" int fr_ctx_create_sharded_pooled(const fr_model_desc *m, int device, int shard_rank, int n_shards, const int32_t *hots, const int32_t *modes, int n_cols, fr_ctx **out) {
    if (!out) FR_FAIL(FR_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!hots) FR_FAIL(FR_ERR_INVALID, "fr_ctx_create_sharded_pooled: hots is NULL");
    int rc = fr_model_validate(m);
    if (rc) return rc;
    const int cols = fr_model_index_cols(m);
    if (n_cols != cols) FR_FAIL(FR_ERR_INVALID, "fr_ctx_create_sharded_pooled: n_cols %d, the model has %d index columns", n_cols, cols);
    for (int c = 0; c < cols; c++) {
        if (hots[c] < 1 || hots[c] > FR_POOL_MAX_HOTS) FR_FAIL(FR_ERR_INVALID, "fr_ctx_create_sharded_pooled: hots[%d] = %d outside [1, %d]", c, hots[c], FR_POOL_MAX_HOTS);
        if (modes && modes[c] != FR_POOL_SUM && modes[c] != FR_POOL_MEAN) FR_FAIL(FR_ERR_INVALID, "fr_ctx_create_sharded_pooled: modes[%d] = %d is no pooling mode", c, modes[c]);
    }
    fr_ctx *c = nullptr;
    rc = fr_ctx_create_sharded(m, device, shard_rank, n_shards, &c);
    if (rc) return rc;
    const int ctx_cols = (int)idx_cols(c);
    if (ctx_cols != cols) {
        fr_ctx_destroy(c);
        FR_FAIL(FR_ERR_STATE, "internal: the context has %d index columns, the model %d", ctx_cols, cols);
    }
    rc = pooling_install(c, hots, modes);
    if (rc) {
        char text[400];
        snprintf(text, sizeof(text), "%s", fr_last_error());
        fr_ctx_destroy(c);
        fr_set_error("%s", text);
        return rc;
    }
    *out = c;
    return FR_OK;
}

extern "C" int fr_ctx_set_pooling(fr_ctx *ctx, const int32_t *hots, int n_cols) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    if (ctx->n_shards > 1) FR_FAIL(FR_ERR_STATE, "the pooling of a sharded context (%d shards) is fixed when it is created: fr_ctx_create_sharded_pooled", ctx->n_shards);
    const int cols = (int)idx_cols(ctx);
    if (hots) {
        if (n_cols != cols) FR_FAIL(FR_ERR_INVALID, "fr_ctx_set_pooling: n_cols %d, the context has %d index columns", n_cols, cols);
        for (int c = 0; c < cols; c++)
            if (hots[c] < 1 || hots[c] > FR_POOL_MAX_HOTS) FR_FAIL(FR_ERR_INVALID, "fr_ctx_set_pooling: hots[%d] = %d outside [1, %d]", c, hots[c], FR_POOL_MAX_HOTS);
    }
    const int rc = fr_pooling_busy(ctx, "fr_ctx_set_pooling");
    if (rc) return rc;
    if (!ctx->cpu) FR_SET_DEVICE(ctx);
    if (!hots) {
        RequestTables rt;   // (a request split keeps its one-hot and dense forms)
        const int rrc = request_prepare(ctx, ctx->req_shared, ctx->req_dense_shared, nullptr, rt);
        if (rrc) return rrc;
        ctx->d_pool.reset();
        ctx->d_pool_csr = nullptr;
        ctx->h_pool.clear();
        ctx->h_pool_csr.clear();
        ctx->pool_hots.clear();
        ctx->pool_modes.clear();
        ctx->pool_any_mean = false;
        ctx->pool_cols = ctx->pool_max_hots = 0;
        ctx->pool_wide = false;
        request_commit(ctx, rt);
        return FR_OK;
    }
    return pooling_install(ctx, hots, nullptr);   // every mode is SUM again
}

extern "C" int fr_ctx_set_pooling_modes(fr_ctx *ctx, const int32_t *modes, int n_cols) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    if (ctx->n_shards > 1) FR_FAIL(FR_ERR_STATE, "the pooling of a sharded context (%d shards) is fixed when it is created: fr_ctx_create_sharded_pooled", ctx->n_shards);
    if (ctx->pool_cols <= 0) return fr_pooling_unset(FR_NO_POOLING_PLAIN);
    const int cols = (int)idx_cols(ctx);
    if (modes) {
        if (n_cols != cols) FR_FAIL(FR_ERR_INVALID, "fr_ctx_set_pooling_modes: n_cols %d, the context has %d index columns", n_cols, cols);
        for (int c = 0; c < cols; c++)
            if (modes[c] != FR_POOL_SUM && modes[c] != FR_POOL_MEAN) FR_FAIL(FR_ERR_INVALID, "fr_ctx_set_pooling_modes: modes[%d] = %d is no pooling mode", c, modes[c]);
    }
    const int rc = fr_pooling_busy(ctx, "fr_ctx_set_pooling_modes");
    if (rc) return rc;
    if (!ctx->cpu) FR_SET_DEVICE(ctx);
    return pooling_install(ctx, ctx->pool_hots.data(), modes);   // the descriptors are rebuilt and uploaded again
}

extern "C" int fr_ctx_pooling_mode(const fr_ctx *ctx, int col) {
    if (!ctx || col < 0 || (size_t)col >= ctx->pool_modes.size()) return FR_POOL_SUM;
    return ctx->pool_modes[(size_t)col];
}

extern "C" int fr_ctx_pooled_index_cols(const fr_ctx *ctx) { return ctx ? ctx->pool_cols : 0; }

// ---- a pooled batch on its way to the gather (FrPooledBatch, FrPooledOut: fr_internal.h).  First the refusals its entry points share, fr_comm.cpp's too ----
int fr_pooling_unset(FrNoPooling who) {
    const char *advice = who == FR_NO_POOLING_PLAIN ? "call fr_ctx_set_pooling first" : "create it with fr_ctx_create_sharded_pooled";
    FR_FAIL(FR_ERR_STATE, "no pooling is set on the %scontext: %s", who == FR_NO_POOLING_SHARD ? "sharded " : "", advice);
}
int fr_pooled_weights_need_sum(const fr_ctx *c) {
    if (c->pool_any_mean) FR_FAIL(FR_ERR_STATE, "per-sample weights need every column's pooling mode to be FR_POOL_SUM: the context has a FR_POOL_MEAN column");
    return FR_OK;
}
// the host knows the offsets of its offsets-form batch: the first and the last are checked before anything is enqueued (the per-bag checks are the gather's)
int fr_pooled_host_offsets(const fr_worker *w, int batch, const char *who, int64_t *nnz) {
    const fr_ctx *c = w->ctx;
    *nnz = w->h_pool_off[(size_t)batch * idx_cols(c)];
    if (w->h_pool_off[0] != 0) FR_FAIL(FR_ERR_INVALID, "%s: offsets[0] is %d, not 0", who, w->h_pool_off[0]);
    if (*nnz < 0 || *nnz > (int64_t)batch * c->pool_cols)
        FR_FAIL(FR_ERR_INVALID, "%s: offsets[batch * cols] = %lld entries, outside [0, batch %d x %d pooled columns]", who, (long long)*nnz, batch, c->pool_cols);
    return FR_OK;
}
// Everything a pooled gather refuses, for both back-ends and every destination.  A batch with weights takes the weighted fold, which needs every column's
// mode SUM; the offsets form's three 4000 MiB bounds are checked here, once (its entry points refuse a NULL d_offsets themselves).
static int pooled_check(const fr_worker *w, const FrPooledBatch &b, const FrPooledOut &o) {
    const fr_ctx *c = w->ctx;
    if (c->pool_cols <= 0) return fr_pooling_unset(c->n_shards > 1 ? FR_NO_POOLING_SHARD : FR_NO_POOLING_PLAIN);
    if (o.kind == FrPooledOut::LP_SLICE && c->cpu) FR_FAIL(FR_ERR_STATE, "the CPU back-end gathers fp32 records only");
    if (b.offsets) {
        if (b.nnz < 0) FR_FAIL(FR_ERR_INVALID, "nnz %lld is negative", (long long)b.nnz);
        if (b.nnz > 0 && !b.idx) FR_FAIL(FR_ERR_INVALID, "d_indices is NULL with nnz %lld", (long long)b.nnz);
        const size_t off_bytes = ((size_t)b.batch * idx_cols(c) + 1) * 4, rec_bytes = (size_t)b.batch * (size_t)c->slice_padded * 4;
        if (off_bytes >= ((size_t)4000 << 20) || (uint64_t)b.nnz * 4 >= ((uint64_t)4000 << 20) || rec_bytes >= ((size_t)4000 << 20))
            FR_FAIL(FR_ERR_INVALID, "pooled gather: the batch's offsets (%zu bytes), entries%s (%llu bytes) or records (%zu bytes) reach 4000 MiB", off_bytes, b.weights ? " / weights" : "",
                    (unsigned long long)b.nnz * 4, rec_bytes);
    } else if (!b.idx) {
        FR_FAIL(FR_ERR_INVALID, "d_idx is NULL");
    }
    if (b.need_weights && !b.weights) FR_FAIL(FR_ERR_INVALID, "d_weights is NULL");
    if (b.weights) {
        const int rc = fr_pooled_weights_need_sum(c);
        if (rc) return rc;
    }
    return dense_check(c, b.dense);
}

// The context's and the worker's part of a pooled launch, for both back-ends: the one place that picks the padded or the offsets form's descriptors
static FrPooledPlan pooled_plan(fr_worker *w, const FrPooledBatch &b, const FrPooledOut &o) {
    const fr_ctx *c = w->ctx;
    const bool csr = b.offsets != nullptr;
    FrPooledPlan p;
    p.words = c->cpu ? c->h_words.data() : c->d_words;
    p.pool = c->cpu ? (csr ? c->h_pool_csr : c->h_pool).data() : (csr ? c->d_pool_csr : c->d_pool);
    p.groups = &c->gather_groups;
    p.n_words = c->n_words;
    p.out_words = (o.kind == FrPooledOut::OPERAND ? c->model.fc[0] : c->slice_padded) / 4;
    p.pool_cols = c->pool_cols, p.max_hots = c->pool_max_hots;
    p.n_icols = csr ? (int)idx_cols(c) : 0;
    p.wide = c->pool_wide && !csr;   // the offsets form gives 4-byte alignment only
    p.any_mean = c->pool_any_mean, p.e_x = c->f8_e_act[0];
    p.err_flag = c->cpu ? &w->c_err : w->d_err;
    return p;
}

// check, then the one launch (-> FR_POOL_NO_OPERAND_ARM: frk_gather_pooled).  On a sharded context the words are the shard's own: its slice is written.
static int gather_pooled(fr_worker *w, FrPooledBatch b, const FrPooledOut &o) {
    const int rc = pooled_check(w, b, o);
    if (rc) return rc;
    if (b.offsets && b.nnz == 0) b.idx = nullptr;   // (no entry is ever read: the resource is empty)
    const FrPooledPlan p = pooled_plan(w, b, o);
    return w->ctx->cpu ? frc_gather_pooled(p, b, o) : frk_gather_pooled(p, b, o, w->stream);
}

// fp32 records, or a shard's slice in the transport type: fp32 is the record arm of gather_pooled_kernel (a shard's words place themselves in its slice);
// bf16 / e4m3 are the item-major form of its operand-store arms, rounded as store_word rounds
static int gather_pooled_impl(fr_worker *w, const FrPooledBatch &b, void *d_out, const char *out_name, int transport) {
    int rc = gather_ready(w, b.batch, d_out, out_name, transport);
    if (rc) return rc;
    FrPooledOut o{d_out};
    if (transport != FR_FC_FP32) o.kind = FrPooledOut::LP_SLICE, o.precision = transport;
    rc = gather_pooled(w, b, o);
    if (rc) return rc;
    keep_kernel(w);
    w->in_flight = true;
    return FR_OK;
}

static FrPooledBatch pooled_batch_weighted(int batch, const int32_t *idx, const float *weights, const float *dense) {
    FrPooledBatch b{batch, idx, weights, dense};
    b.need_weights = true;
    return b;
}

// the offsets form's entry points refuse a NULL d_offsets before anything else
static int pooled_batch_csr(FrPooledBatch *b, int batch, const int32_t *offsets, const int32_t *idx, int64_t nnz, const float *weights, const float *dense) {
    if (!offsets) FR_FAIL(FR_ERR_INVALID, "d_offsets is NULL");
    *b = FrPooledBatch{batch, idx, weights, dense, offsets, nnz};
    return FR_OK;
}

extern "C" int fr_worker_gather_pooled(fr_worker *w, int batch, const int32_t *d_idx, const float *d_dense, float *d_records) {
    return gather_pooled_impl(w, FrPooledBatch{batch, d_idx, nullptr, d_dense}, d_records, "d_records", FR_FC_FP32);
}

extern "C" int fr_worker_gather_pooled_weighted(fr_worker *w, int batch, const int32_t *d_idx, const float *d_weights, const float *d_dense, float *d_records) {
    return gather_pooled_impl(w, pooled_batch_weighted(batch, d_idx, d_weights, d_dense), d_records, "d_records", FR_FC_FP32);
}

// pooled records into the worker's record buffer, then the chain fr_worker_fc_only runs from records (launch_fc), on the same stream
static int submit_pooled_impl(fr_worker *w, const FrPooledBatch &b, float *d_scores) {
    if (w->n_active || w->n_pending) FR_FAIL(FR_ERR_STATE, "pipeline busy (push_device in flight): call fr_worker_sync first");
    if (w->ctx->n_shards > 1)   // (before the gather is enqueued: launch_fc would refuse the shard behind it)
        FR_FAIL(FR_ERR_STATE, "a pooled submit on a sharded ctx: the chain needs the all-gathered slices (fr_worker_submit_sharded_pooled on a context created by fr_ctx_create_sharded_pooled)");
    int rc = gather_pooled(w, b, FrPooledOut{w->d_records});
    if (rc) return rc;
    w->in_flight = true;   // the gather is enqueued whatever the chain's launch says
    return launch_fc(w, b.batch, w->d_records, d_scores);
}

static int submit_pooled_device_impl(fr_worker *w, const FrPooledBatch &b, float *d_scores) {
    int rc = check_ready(w, b.batch, true, true);
    if (rc) return rc;
    if (!d_scores) FR_FAIL(FR_ERR_INVALID, "d_scores is NULL");
    FR_SET_DEVICE(w->ctx);
    return submit_pooled_impl(w, b, d_scores);
}

extern "C" int fr_worker_submit_pooled_device(fr_worker *w, int batch, const int32_t *d_idx, const float *d_dense, float *d_scores) {
    return submit_pooled_device_impl(w, FrPooledBatch{batch, d_idx, nullptr, d_dense}, d_scores);
}

extern "C" int fr_worker_submit_pooled_weighted_device(fr_worker *w, int batch, const int32_t *d_idx, const float *d_weights, const float *d_dense, float *d_scores) {
    return submit_pooled_device_impl(w, pooled_batch_weighted(batch, d_idx, d_weights, d_dense), d_scores);
}

// what both host forms (padded and offsets) ask of the worker before they read its pinned buffers (a shard is refused further down, by submit_pooled_impl)
static int pooled_host_ready(fr_worker *w, int batch, bool weighted) {
    int rc = check_ready(w, batch, true, true);
    if (rc) return rc;
    if (w->in_flight) FR_FAIL(FR_ERR_STATE, "a batch is already in flight on this worker: call fr_worker_sync first");
    fr_ctx *c = w->ctx;
    if (c->pool_cols <= 0) return fr_pooling_unset(FR_NO_POOLING_PLAIN);
    if (w->idx_cap < c->pool_cols)
        FR_FAIL(FR_ERR_STATE, "the worker's index buffers hold %d columns per item, pooled rows have %d: create the worker after fr_ctx_set_pooling", w->idx_cap, c->pool_cols);
    if (weighted && (!w->h_pool_w || w->pool_w_cap < c->pool_cols))
        FR_FAIL(FR_ERR_STATE, "the worker's weight buffer holds %d columns per item, pooled rows have %d: create the worker after fr_ctx_set_pooling", w->pool_w_cap, c->pool_cols);
    return FR_OK;
}

// the host forms: as fr_worker_submit, the gather reads the pinned index rows (weights, offsets, dense features) in place, the output layer writes the pinned scores
static int submit_pooled_host_impl(fr_worker *w, int batch, bool weighted, const char *csr_who) {
    int rc = pooled_host_ready(w, batch, weighted);
    if (rc) return rc;
    fr_ctx *c = w->ctx;
    FrPooledBatch b{batch, w->h_idx, weighted ? w->h_pool_w.p : nullptr, c->model.dense_len ? w->h_dense.p : nullptr};
    b.need_weights = weighted;
    if (csr_who) {
        if (!w->h_pool_off) FR_FAIL(FR_ERR_STATE, "the worker has no offsets buffer: create the worker after fr_ctx_set_pooling");
        b.offsets = w->h_pool_off;
        rc = fr_pooled_host_offsets(w, batch, csr_who, &b.nnz);
        if (rc) return rc;
    }
    FR_SET_DEVICE(c);
    rc = submit_pooled_impl(w, b, w->h_score);
    if (!rc) w->host_batch = batch;   // (fr_worker_topk ranks it)
    return rc;
}

extern "C" int fr_worker_submit_pooled(fr_worker *w, int batch) { return submit_pooled_host_impl(w, batch, false, nullptr); }
extern "C" int fr_worker_submit_pooled_weighted(fr_worker *w, int batch) { return submit_pooled_host_impl(w, batch, true, nullptr); }
extern "C" int fr_worker_submit_pooled_csr(fr_worker *w, int batch, int weighted) { return submit_pooled_host_impl(w, batch, weighted != 0, "fr_worker_submit_pooled_csr"); }

// ---- the offsets (CSR) form of the pooled lookups: the same gather, fold and chain; only the way a bag is found differs ----
extern "C" int fr_worker_gather_pooled_csr(fr_worker *w, int batch, const int32_t *d_offsets, const int32_t *d_indices, int64_t nnz, const float *d_weights, const float *d_dense,
                                           float *d_records) {
    FrPooledBatch b;
    const int rc = pooled_batch_csr(&b, batch, d_offsets, d_indices, nnz, d_weights, d_dense);
    return rc ? rc : gather_pooled_impl(w, b, d_records, "d_records", FR_FC_FP32);
}

extern "C" int fr_worker_submit_pooled_csr_device(fr_worker *w, int batch, const int32_t *d_offsets, const int32_t *d_indices, int64_t nnz, const float *d_weights, const float *d_dense,
                                                  float *d_scores) {
    FrPooledBatch b;
    const int rc = pooled_batch_csr(&b, batch, d_offsets, d_indices, nnz, d_weights, d_dense);
    return rc ? rc : submit_pooled_device_impl(w, b, d_scores);
}

// Sharded mode, low-precision transport: the shard's slice [batch][slice_padded] as bf16 or e4m3 (x 2^e of the context's X exponent)
// instead of fp32 -- what travels through the all-gather.  transport = FR_FC_FP32 is fr_worker_gather_only.
extern "C" int fr_worker_gather_slices(fr_worker *w, int batch, const int32_t *d_idx, const float *d_dense, void *d_slice, int transport) {
    int rc = gather_ready(w, batch, d_slice, "d_slice", transport);
    if (rc) return rc;
    rc = launch_gather(w, batch, d_idx, d_dense, d_slice, transport);
    keep_kernel(w);
    if (rc) return rc;
    w->in_flight = true;
    return FR_OK;
}

// The pooled siblings: the slice of a pooled batch (padded or offsets form) in the transport type (gather_pooled_impl)
extern "C" int fr_worker_gather_slices_pooled(fr_worker *w, int batch, const int32_t *d_idx, const float *d_weights, const float *d_dense, void *d_slice, int transport) {
    return gather_pooled_impl(w, FrPooledBatch{batch, d_idx, d_weights, d_dense}, d_slice, "d_slice", transport);
}

extern "C" int fr_worker_gather_slices_pooled_csr(fr_worker *w, int batch, const int32_t *d_offsets, const int32_t *d_indices, int64_t nnz, const float *d_weights, const float *d_dense,
                                                  void *d_slice, int transport) {
    FrPooledBatch b;
    const int rc = pooled_batch_csr(&b, batch, d_offsets, d_indices, nnz, d_weights, d_dense);
    return rc ? rc : gather_pooled_impl(w, b, d_slice, "d_slice", transport);
}

// ... and the receiving side: d_gathered = [n_shards][batch_total][slice_padded] elements of the transport type.  The transport must
// be the context's FC precision (the slices become the chain's operand image without another rounding).
extern "C" int fr_worker_fc_from_slices_lp(fr_worker *w, int batch_total, int item0, int n_items, const void *d_gathered, int transport, float *d_scores) {
    if (!w) FR_FAIL(FR_ERR_INVALID, "worker is NULL");
    if (transport == FR_FC_FP32) return fr_worker_fc_from_slices(w, batch_total, item0, n_items, reinterpret_cast<const float *>(d_gathered), d_scores);
    int rc = check_ready(w, n_items, false, true);
    if (rc) return rc;
    fr_ctx *c = w->ctx;
    if (transport != c->fc_precision) FR_FAIL(FR_ERR_STATE, "slice transport %d does not match the context's FC precision %d", transport, c->fc_precision);
    if (!d_gathered || !d_scores) FR_FAIL(FR_ERR_INVALID, "NULL device pointer");
    if (batch_total < 1 || item0 < 0 || item0 + n_items > batch_total) FR_FAIL(FR_ERR_INVALID, "items [%d,+%d) outside batch %d", item0, n_items, batch_total);
    if (w->n_active || w->n_pending) FR_FAIL(FR_ERR_STATE, "pipeline busy: call fr_worker_sync first");
    FR_SET_DEVICE(c);
    if (w->launch_no == 0) w->launch_no = 1;
    const int ldm = round_up(n_items, 32);
    const int par_prev = (int)((w->launch_no - 1) & 1);
    rc = frk_transpose_slices_lp(transport, d_gathered, c->n_shards, batch_total, c->slice_padded, c->shard_offset.data(), c->shard_len.data(), item0, n_items,
                                 act_set(w, par_prev).x, c->model.fc[0], ldm, w->stream);
    if (rc) return rc;
    rc = pipeline_push(w, n_items, 1, nullptr, nullptr, d_scores);
    if (rc) return rc;
    rc = pipeline_flush(w);
    if (rc) return rc;
    w->in_flight = true;
    return FR_OK;
}

extern "C" int fr_worker_fc_only(fr_worker *w, int batch, const float *d_records, float *d_scores) {
    int rc = check_ready(w, batch, false, true);
    if (rc) return rc;
    if (!d_records || !d_scores) FR_FAIL(FR_ERR_INVALID, "NULL device pointer");
    FR_SET_DEVICE(w->ctx);
    rc = launch_fc(w, batch, d_records, d_scores);
    if (rc) return rc;
    w->in_flight = true;
    return FR_OK;
}

// Roofline hook: launch ONE stage of the chain (1..3 = FC1..FC3, 4 = output layer; 0 is not available here) on the
// worker's resident activations, exactly as an unpipelined submit launches it.  API layer index = stage - 1.
extern "C" int fr_worker_fc_layer_only(fr_worker *w, int batch, int layer) {
    int rc = check_ready(w, batch, false, true);
    if (rc) return rc;
    if (layer < 0 || layer > 3) FR_FAIL(FR_ERR_INVALID, "layer %d out of range", layer);
    FR_NOT_ON_CPU(w->ctx, "fr_worker_fc_layer_only");
    if (w->n_active) FR_FAIL(FR_ERR_STATE, "pipeline busy: call fr_worker_sync first");
    fr_ctx *c = w->ctx;
    FR_SET_DEVICE(c);
    // place a virtual batch so that the next launch runs exactly stage layer+1 of it, then drop it again
    const int stage = layer + 1;
    if (w->launch_no < (uint64_t)stage) w->launch_no = stage;
    const uint64_t L0 = w->launch_no - (uint64_t)stage;
    fr_worker::Slot &sl = w->ring[L0 % 8];
    sl.active = true;
    sl.launch0 = L0;
    sl.first_stage = stage;
    sl.batch = batch;
    sl.ldm = round_up(batch, 32);
    sl.d_idx = nullptr;
    sl.d_dense = nullptr;
    sl.d_scores = w->d_score;
    w->n_active++;
    w->diag_launch = true;   // a diagnostic launch never freezes the context's chain width
    rc = pipeline_step(w);
    w->diag_launch = false;
    keep_kernel(w);  // the layer's kernel, as launched (fr_worker_last_kernel)
    if (sl.active) {  // stages 1..3 leave the batch in flight: retire it by hand
        sl.active = false;
        w->n_active--;
    }
    if (rc) return rc;
    w->in_flight = true;
    return FR_OK;
}

extern "C" int fr_worker_fc_layer_repeat(fr_worker *w, int batch, int layer, int n) {
    if (n < 0) FR_FAIL(FR_ERR_INVALID, "n = %d", n);
    for (int i = 0; i < n; i++) {
        const int rc = fr_worker_fc_layer_only(w, batch, layer);
        if (rc) return rc;
    }
    return FR_OK;
}

// Streaming form of the hot loop body: enqueue batch after batch without synchronising (cuda_server.c:406-497 does
// exactly that).  Each call issues ONE launch in which this batch is gathered while the previous four batches of
// this worker advance through FC1, FC2, FC3 and the output layer.  d_scores of a pushed batch are complete after
// four more pushes have executed, or after fr_worker_sync() (which drains the pipeline).  The caller keeps
// d_idx / d_dense / d_scores valid and distinct for every batch still in the pipeline (up to 5).
extern "C" int fr_worker_push_device(fr_worker *w, int batch, const int32_t *d_idx, const float *d_dense, float *d_scores) {
    int rc = check_ready(w, batch, true, true);
    if (rc) return rc;
    if (!d_scores) FR_FAIL(FR_ERR_INVALID, "d_scores is NULL");
    fr_ctx *c = w->ctx;
    if (c->n_shards > 1 || c->model.layout != FR_LAYOUT_SEMANTIC)
        FR_FAIL(FR_ERR_STATE, "push_device needs an unsharded SEMANTIC-layout context");
    rc = check_gather_args(w, d_idx, d_dense);
    if (rc) return rc;
    if (c->cpu) {   // the CPU back-end has nothing to queue behind: the batch is computed before the call returns
        rc = launch_pipeline(w, batch, d_idx, d_dense, d_scores);
        if (rc) return rc;
        w->in_flight = true;
        return FR_OK;
    }
    FR_SET_DEVICE(c);
    // Launch groups below FR_FUSED_MIN_GROUP ride the stage pipeline even on a fused-eligible context: a fused launch of g batches takes
    // one item tile's time (~130 us for Model-A) whatever g is, so small groups give 7 M (g = 1) .. 35 M inferences/s (g = 8) at 145 us,
    // where the pipelined stage launches give 43 M at 36 us (profiles/archive/r02_launch_group_paths.txt).
    // the fused kernels read the index rows through a buffer resource with 32-bit offsets (out-of-range items come back as 0 without a
    // branch): an index buffer of 4000 MiB or more rides the stage pipeline, whose gather stage has a 64-bit fallback
    const bool idx_fits = (size_t)batch * idx_cols(c) * sizeof(int32_t) < ((size_t)4000 << 20);
    const bool fused = fused_eligible(c) && fused_group(c) >= FR_FUSED_MIN_GROUP && idx_fits;
    if (fused && w->n_active > 0) {          // the group was raised while batches were riding the stage pipeline: drain them first
        rc = pipeline_flush(w);
        if (rc) return rc;
    }
    if (!fused && w->n_pending > 0) {        // ... or lowered with batches queued for a fused launch
        rc = fr_fused_flush(w);
        if (rc) return rc;
    }
    if (fused) {
        // whole-path-per-item-tile kernel: queue the batch, launch when a group is full (fr_worker_sync launches the rest)
        FrFusedBatch &fb = w->pending[w->n_pending++];
        fb.idx = d_idx;
        fb.dense = d_dense;
        fb.scores = d_scores;
        fb.batch = batch;
        w->pending_items += batch;
        w->in_flight = true;
        // a launch is due when the group is full or when the queue already covers the chip (256 CUs x 64 items): large batches
        // need fewer of them per launch
        // a launch carries at most 16384 items (one 64-item tile per compute unit) -- in the bf16 chain, whose persistent kernel's workgroups
        // overlap the gather of their next tile with the FC phases of the current one, as many as the launch group allows (up to 256 batches
        // of 1024 items): every launch exposes its first tile's gather once (13-14 us), so more tiles per workgroup amortise it -- Model-B
        // 1024: 330 M inf/s at 4 tiles per workgroup (group 64), 340 M at 8 (group 128), 342 M at 16 (profiles/archive/r03_fused_hs_items_ab.txt)
        const bool big = c->fc_precision == FR_FC_BF16 || (c->fc_precision == FR_FC_FP8 && FR_KNOB_ONCE("FUSED_HK", -1) == 1);
        const int64_t max_items = FR_KNOB_ONCE("FUSED_ITEMS", 0) ? FR_KNOB_ONCE("FUSED_ITEMS", 0) : (big ? 4096 * 64 : 256 * 64);
        return (w->n_pending >= fused_group(c) || w->pending_items >= max_items || w->n_pending >= FR_FUSED_MAX_QUEUE) ? fr_fused_flush(w) : FR_OK;
    }
    rc = pipeline_push(w, batch, 0, d_idx, d_dense, d_scores);
    if (rc) return rc;
    w->in_flight = true;
    return FR_OK;
}

extern "C" int fr_worker_push_device_list(fr_worker *w, int n, const int *batch, const int32_t *const *d_idx, const float *const *d_dense,
                                          float *const *d_scores) {
    if (!w) FR_FAIL(FR_ERR_INVALID, "worker is NULL");
    if (n < 0 || (n > 0 && (!batch || !d_idx || !d_scores))) FR_FAIL(FR_ERR_INVALID, "push_device_list: n = %d needs batch, d_idx and d_scores arrays", n);
    for (int i = 0; i < n; i++) {
        const int rc = fr_worker_push_device(w, batch[i], d_idx[i], d_dense ? d_dense[i] : nullptr, d_scores[i]);
        if (rc) return rc;
    }
    return FR_OK;
}

// ---- streaming pushes of pooled lookups: the pooled gather writes the chain's stage-1 operand itself and the batch enters the stage pipeline at
// stage 1 of the next launch, un-flushed -- its FC1 shares that launch with FC2 / FC3 / the output layer of the pushes before it ----
static int push_pooled_impl(fr_worker *w, const FrPooledBatch &b, float *d_scores) {
    const int batch = b.batch;
    int rc = check_ready(w, batch, true, true);
    if (rc) return rc;
    if (!d_scores) FR_FAIL(FR_ERR_INVALID, "d_scores is NULL");
    fr_ctx *c = w->ctx;
    if (c->pool_cols <= 0) return fr_pooling_unset(c->n_shards > 1 ? FR_NO_POOLING_SHARD : FR_NO_POOLING_PLAIN);
    if (c->n_shards > 1) FR_FAIL(FR_ERR_STATE, "a pooled push on a sharded ctx: the chain needs the all-gathered slices (fr_worker_submit_sharded_pooled)");
    if (c->model.layout != FR_LAYOUT_SEMANTIC) FR_FAIL(FR_ERR_STATE, "a pooled push needs a SEMANTIC-layout context");
    if (c->cpu) {   // the CPU back-end has nothing to queue behind: the batch is computed before the call returns
        rc = submit_pooled_impl(w, b, d_scores);
        if (rc) return rc;
        w->in_flight = true;
        return FR_OK;
    }
    FR_TRY(fr_host_fed_queued(w, "push"));
    if (c->slice_padded != c->model.fc[0]) FR_FAIL(FR_ERR_STATE, "internal: a record of %d floats on a chain of K = %d", c->slice_padded, c->model.fc[0]);
    FR_SET_DEVICE(c);
    rc = fr_fused_flush(w);   // batches fr_worker_push_device queued for a fused launch were pushed before this one: launched first, not waited for
    if (rc) return rc;
    if (w->launch_no == 0) w->launch_no = 1;   // stage 1 of the next launch reads the set the (virtual) previous launch wrote
    // a one-hot batch gathered by the previous launch holds the slot (and the X operand) this batch would take: one launch without a new batch
    // moves it on -- at most once, nothing entered the launch that this makes the previous one
    while (w->ring[(w->launch_no - 1) % 8].active) {
        rc = pipeline_step(w);
        if (rc) return rc;
    }
    const int ldm = round_up(batch, 32);
    const int par_prev = (int)((w->launch_no - 1) & 1);
    float *x = act_set(w, par_prev).x;
    // experiments build only: FR_POOL_PUSH_TWO_LAUNCH = 1 takes the two-launch form for every shape (tools/pooled_stream_bench.py, form (c))
    FrPooledOut operand{x};
    operand.kind = FrPooledOut::OPERAND, operand.precision = c->fc_precision, operand.ldm = ldm;
    rc = FR_KNOB("POOL_PUSH_TWO_LAUNCH", 0) ? FR_POOL_NO_OPERAND_ARM : gather_pooled(w, b, operand);
    if (rc == FR_POOL_NO_OPERAND_ARM) {
        // the two-launch form: fp32 records into the worker's record buffer, then the conversion launch of fr_worker_fc_only -- for the (shape,
        // operand type) pairs of gather_pooled_kernel that carry no operand-store arm (fr_gather.hip, pooled_operand_forms: <4, 2, false> and
        // <2, 4, false> on a bf16 / fp8 chain); stream order keeps the buffer safe
        rc = gather_pooled(w, b, FrPooledOut{w->d_records});
        if (rc) return rc;
        keep_kernel(w);
        w->in_flight = true;
        if (c->fc_precision == FR_FC_FP8) rc = frk_records_to_q16_fp8(w->d_records, x, batch, c->model.fc[0], ldm, c->f8_e_act[0], w->stream);
        else if (c->fc_precision == FR_FC_BF16) rc = frk_records_to_q8_bf16(w->d_records, x, batch, c->model.fc[0], ldm, w->stream);
        else rc = frk_transpose_records(w->d_records, x, batch, c->model.fc[0], ldm, w->stream);
    } else if (rc == FR_OK) {
        keep_kernel(w);   // the gather, as launched (fr_worker_last_kernel)
        w->in_flight = true;
    }
    if (rc) return rc;
    rc = pipeline_push(w, batch, 1, nullptr, nullptr, d_scores);   // no flush: fr_worker_sync drains
    if (rc) return rc;
    w->last_x_parity = par_prev;   // fr_worker_features_dptr names this operand
    return FR_OK;
}

extern "C" int fr_worker_push_pooled_device(fr_worker *w, int batch, const int32_t *d_idx, const float *d_weights, const float *d_dense, float *d_scores) {
    return push_pooled_impl(w, FrPooledBatch{batch, d_idx, d_weights, d_dense}, d_scores);
}

extern "C" int fr_worker_push_pooled_csr_device(fr_worker *w, int batch, const int32_t *d_offsets, const int32_t *d_indices, int64_t nnz, const float *d_weights, const float *d_dense,
                                                float *d_scores) {
    FrPooledBatch b;
    const int rc = pooled_batch_csr(&b, batch, d_offsets, d_indices, nnz, d_weights, d_dense);
    return rc ? rc : push_pooled_impl(w, b, d_scores);
}

extern "C" int fr_worker_push_pooled_device_list(fr_worker *w, int n, const int *batch, const int32_t *const *d_idx, const float *const *d_weights, const float *const *d_dense,
                                                 float *const *d_scores) {
    if (!w) FR_FAIL(FR_ERR_INVALID, "worker is NULL");
    if (n < 0 || (n > 0 && (!batch || !d_idx || !d_scores))) FR_FAIL(FR_ERR_INVALID, "push_pooled_device_list: n = %d needs batch, d_idx and d_scores arrays", n);
    for (int i = 0; i < n; i++) {
        const int rc = push_pooled_impl(w, FrPooledBatch{batch[i], d_idx[i], d_weights ? d_weights[i] : nullptr, d_dense ? d_dense[i] : nullptr}, d_scores[i]);
        if (rc) return rc;
    }
    return FR_OK;
}

extern "C" int fr_worker_submit_device(fr_worker *w, int batch, const int32_t *d_idx, const float *d_dense, float *d_scores) {
    int rc = check_ready(w, batch, true, true);
    if (rc) return rc;
    if (!d_scores) FR_FAIL(FR_ERR_INVALID, "d_scores is NULL");
    FR_SET_DEVICE(w->ctx);
    if (w->n_active || w->n_pending) FR_FAIL(FR_ERR_STATE, "pipeline busy (push_device in flight): call fr_worker_sync first");
    rc = launch_pipeline(w, batch, d_idx, d_dense, d_scores);
    if (rc) return rc;
    w->in_flight = true;
    return FR_OK;
}

extern "C" int fr_worker_submit(fr_worker *w, int batch) {
    int rc = check_ready(w, batch, true, true);
    if (rc) return rc;
    if (w->in_flight) FR_FAIL(FR_ERR_STATE, "a batch is already in flight on this worker: call fr_worker_sync first");
    fr_ctx *c = w->ctx;
    if (c->cpu) {
        rc = launch_pipeline(w, batch, w->h_idx, c->model.dense_len ? w->h_dense.p : nullptr, w->h_score);
        if (rc) return rc;
        w->in_flight = true, w->host_batch = batch;
        return FR_OK;
    }
    FR_SET_DEVICE(c);
    // Default: no copy commands on the stream -- the gather stage reads the index rows (and dense features) straight from the worker's
    // pinned host buffers over PCIe and the output layer writes the scores straight into the pinned score buffer.  Against the
    // reference's H2D / D2H commands (cuda_server.c:460-461,494-495; FR_SUBMIT_ZEROCOPY=0 keeps them) that takes 4-8 us off a submit +
    // sync at every batch size (batch 256: 46.1 -> 38.4 us p50) and costs 5 % of the rate of 16 workers submitting at once
    // (profiles/archive/r02_submit_latency.txt): this entry point is the latency path, the streaming entry points are the throughput path.
    const int zero_copy = FR_KNOB_ONCE("SUBMIT_ZEROCOPY", 1);
    if (zero_copy) {
        rc = launch_pipeline(w, batch, w->h_idx, c->model.dense_len ? w->h_dense.p : nullptr, w->h_score);
        if (rc) return rc;
        w->in_flight = true, w->host_batch = batch;
        return FR_OK;
    }
    // input H2D (cuda_server.c:460-461) -- indices instead of the already-gathered features
    FR_HIP(hipMemcpyAsync(w->d_idx, w->h_idx, (size_t)batch * idx_cols(c) * sizeof(int32_t), hipMemcpyHostToDevice, w->stream));
    if (c->model.dense_len)
        FR_HIP(hipMemcpyAsync(w->d_dense, w->h_dense, (size_t)batch * c->model.dense_len * sizeof(float), hipMemcpyHostToDevice, w->stream));
    rc = launch_pipeline(w, batch, w->d_idx, w->d_dense, w->d_score);
    if (rc) return rc;
    // output D2H (cuda_server.c:494-495)
    FR_HIP(hipMemcpyAsync(w->h_score, w->d_score, (size_t)batch * sizeof(float), hipMemcpyDeviceToHost, w->stream));
    w->in_flight = true, w->host_batch = batch;
    return FR_OK;
}

// ---- host-fed streaming ------------------------------------------------------------------------------
// The reference's loop reads a batch from the socket into pinned memory and enqueues H2D + GEMMs + D2H for it
// (cuda_server.c:425-495).  Here batches that arrive in host memory are staged in pinned blocks of `g` batches; a full block
// travels as one H2D copy, one fused launch and one D2H copy, and FR_HOST_BLOCKS blocks rotate so that copies, kernels and the
// host's staging of the next block overlap.
static int host_ring_init(fr_worker *w) {
    fr_worker::HostRing &r = w->hr;
    if (r.g) return FR_OK;
    fr_ctx *c = w->ctx;
    int g = 16384 / (w->max_batch > 0 ? w->max_batch : 1);  // the queue launches once it holds 256 x 64 items
    if (g < 1) g = 1;
    if (g > fused_group(c)) g = fused_group(c);
    if (g > FR_FUSED_MAX_BATCHES) g = FR_FUSED_MAX_BATCHES;   // the host-fed blocks stay within one kernarg-fed launch
    r.idx_slot = (size_t)w->max_batch * idx_cols(c);
    r.dense_slot = (size_t)w->max_batch * c->model.dense_len;
    r.score_slot = (size_t)w->max_batch;
    const size_t slots = (size_t)g * FR_HOST_BLOCKS;
    // (r.g is set last: a call that failed half-way is run again, and keeps what the first one made -- alloc releases, create and the stream skip)
    FR_TRY(r.h_idx.alloc(FrMem::PINNED, slots * r.idx_slot, "host ring index rows"));
    FR_TRY(r.d_idx.alloc(FrMem::DEVICE, slots * r.idx_slot, "host ring index rows (device)"));
    if (r.dense_slot) {
        FR_TRY(r.h_dense.alloc(FrMem::PINNED, slots * r.dense_slot, "host ring dense rows"));
        FR_TRY(r.d_dense.alloc(FrMem::DEVICE, slots * r.dense_slot, "host ring dense rows (device)"));
    }
    FR_TRY(r.h_sc.alloc(FrMem::PINNED, slots * r.score_slot, "host ring scores"));
    FR_TRY(r.d_sc.alloc(FrMem::DEVICE, slots * r.score_slot, "host ring scores (device)"));
    for (FrEvent &e : r.ev) FR_HIP(e.create(hipEventDisableTiming));
    if (!r.copy) {   // The copy stream lives in the LOWEST stream priority's pool of hardware queues: the HIP runtime pools queues per priority, and in the
        // default pool the marker packet behind a block's copy (its event) would sit in a hardware queue that some worker's launches share --
        // that worker's next launch then waits out another worker's 65 us copy (seen as a bimodal 97 % / 99 % of the HBM-resident rate,
        // by which queue the runtime happened to hand out: profiles/r05_experiments.md section 1).  Fused-kernel models keep their worker
        // streams on the default priority, so the low pool is the copy streams' alone.
        int lo = 0, hi = 0;
        FR_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
        if (lo > hi) FR_HIP(hipStreamCreateWithPriority(&r.copy, hipStreamNonBlocking, lo));
        else FR_HIP(hipStreamCreateWithFlags(&r.copy, hipStreamNonBlocking));
    }
    for (FrEvent &e : r.ev_in) FR_HIP(e.create(hipEventDisableTiming));
    r.g = g;
    return FR_OK;
}

// scores of a finished block -> the callers' buffers
static int host_block_deliver(fr_worker *w, int b) {
    fr_worker::HostRing &r = w->hr;
    if (!r.inflight[b]) return FR_OK;
    FR_HIP(hipEventSynchronize(r.ev[b]));
    for (int i = 0; i < r.count[b]; i++)
        memcpy(r.dst[b][i], r.h_sc + ((size_t)b * r.g + i) * r.score_slot, (size_t)r.bsz[b][i] * sizeof(float));
    r.delivered += r.count[b];
    r.inflight[b] = false;
    r.count[b] = 0;
    return FR_OK;
}

// the block being filled leaves: H2D, fused launch, D2H, event
static int host_block_launch(fr_worker *w) {
    fr_worker::HostRing &r = w->hr;
    const int b = r.cur, n = r.count[b];
    if (n == 0) return FR_OK;
    int rc = fr_fused_flush(w);  // batches queued by fr_worker_push_device go first
    if (rc) return rc;
    const size_t s0 = (size_t)b * r.g;
    if (n <= w->ctx->small_block.load(std::memory_order_relaxed) && w->n_active == 0) {
        // A block of very few batches (fr_worker_flush on a nearly idle server): one batch through the fused kernel is 8 workgroups working
        // through the whole chain for 133 us; the stage launches of fr_worker_submit spread the same batch over the chip in ~25 us.  The
        // kernels read the staged rows and write the scores in the pinned staging itself (no copy commands), exactly as fr_worker_submit
        // does; the scores are fr_worker_submit's, bit for bit (not the fused kernel's: another fp32 summation order, equal to ~1e-6).
        // The block's batches follow each other through the stage pipeline (launch L = gather of batch L | FC1 of L-1 | ... | out of L-4) and
        // four more launches drain it: n + 4 launches for the block, not 5 n.
        const int serial = FR_KNOB_ONCE("SMALL_BLOCK_SERIAL", 0);  // experiment knob: 1 = five launches per batch
        for (int i = 0; i < n; i++) {
            rc = pipeline_push(w, r.bsz[b][i], 0, r.h_idx + (s0 + i) * r.idx_slot, r.dense_slot ? r.h_dense + (s0 + i) * r.dense_slot : nullptr,
                               r.h_sc + (s0 + i) * r.score_slot);
            if (rc == FR_OK && serial) rc = pipeline_flush(w);
            if (rc) return rc;
        }
        rc = pipeline_flush(w);
        if (rc) return rc;
        FR_HIP(hipEventRecord(r.ev[b], w->stream));
        r.inflight[b] = true;
        r.cur = (b + 1) % FR_HOST_BLOCKS;
        return FR_OK;
    }
    // The two PCIe hops of the reference's loop (cuda_server.c:460-461,494-495), arranged so that the worker's stream carries NOTHING but its
    // kernels: the block's index rows travel as one H2D copy on the worker's COPY stream -- issued now, while the previous block's kernel
    // still runs, and joined by an event the launch waits for (long satisfied when the launch reaches the head of its hardware queue) --
    // and the output layer writes the scores straight into the pinned staging (no D2H command).  With both copies as commands of the one
    // stream (round 4) a block's H2D could not start before the previous block's D2H, its 130 us sat between two launches of the stream,
    // and the barrier packet in front of the launch held back every other stream that shares the hardware queue: 95-96 % of the
    // HBM-resident rate with 8 streams on 4 queues; this form: 98-99 % (profiles/r05_host_fed_timeline.txt).
    // Experiments build: FR_HOST_ZEROCOPY 0 = round 4's commands, 1 = no H2D either (the kernel reads the rows over PCIe: slower), 2 = H2D on the worker's stream.
    const int zc = FR_KNOB_ONCE("HOST_ZEROCOPY", 3);
    hipStream_t cs = zc == 3 ? r.copy : w->stream;
    const int pending0 = w->n_pending;
    auto issue = [&]() -> int {
        if (zc != 1) {
            FR_HIP(hipMemcpyAsync(r.d_idx + s0 * r.idx_slot, r.h_idx + s0 * r.idx_slot, (size_t)n * r.idx_slot * sizeof(int32_t), hipMemcpyHostToDevice, cs));
            if (r.dense_slot)
                FR_HIP(hipMemcpyAsync(r.d_dense + s0 * r.dense_slot, r.h_dense + s0 * r.dense_slot, (size_t)n * r.dense_slot * sizeof(float), hipMemcpyHostToDevice, cs));
            if (zc == 3) {   // (the device block is free: host_slot_prepare delivered its previous use -- its kernel has finished -- before refilling the staging)
                FR_HIP(hipEventRecord(r.ev_in[b], r.copy));
                FR_HIP(hipStreamWaitEvent(w->stream, r.ev_in[b], 0));
            }
        }
        for (int i = 0; i < n; i++) {
            FrFusedBatch &fb = w->pending[w->n_pending++];
            fb.idx = (zc == 1 ? r.h_idx : r.d_idx) + (s0 + i) * r.idx_slot;
            fb.dense = r.dense_slot ? (zc == 1 ? r.h_dense : r.d_dense) + (s0 + i) * r.dense_slot : nullptr;
            fb.scores = (zc ? r.h_sc : r.d_sc) + (s0 + i) * r.score_slot;
            fb.batch = r.bsz[b][i];
        }
        int rc2 = fr_fused_flush(w);
        if (rc2) return rc2;
        if (!zc) FR_HIP(hipMemcpyAsync(r.h_sc + s0 * r.score_slot, r.d_sc + s0 * r.score_slot, (size_t)n * r.score_slot * sizeof(float), hipMemcpyDeviceToHost, w->stream));
        FR_HIP(hipEventRecord(r.ev[b], w->stream));
        return FR_OK;
    };
    rc = issue();
    if (rc) {
        // the block's H2D copy may already be queued while the block is NOT marked in flight -- the caller could refill the
        // pinned staging of block b under the pending copy.  Drain both streams before handing the error back (the message of the failing
        // call stays in fr_last_error), and forget the batches that were queued for the launch that did not happen.
        (void)hipStreamSynchronize(cs);
        (void)hipStreamSynchronize(w->stream);
        if (w->n_pending > pending0) w->n_pending = pending0;
        return rc;
    }
    r.inflight[b] = true;
    r.cur = (b + 1) % FR_HOST_BLOCKS;
    return FR_OK;
}

// The staging slot of the next pushed batch: the oldest block is delivered first if its staging memory is about to be reused.
static int host_slot_prepare(fr_worker *w, int batch, int32_t **idx_slot, float **dense_slot) {
    int rc = check_ready(w, batch, true, true);
    if (rc) return rc;
    fr_ctx *c = w->ctx;
    FR_NOT_ON_CPU(c, "host-fed streaming (fr_worker_push_host / fr_worker_stage_acquire)");
    if (!fused_eligible(c)) FR_FAIL(FR_ERR_STATE, "host-fed streaming needs a model that streams through the fused item-tile kernel (use fr_worker_submit)");
    FR_SET_DEVICE(c);
    rc = host_ring_init(w);
    if (rc) return rc;
    fr_worker::HostRing &r = w->hr;
    const int b = r.cur;
    if (r.inflight[b]) {  // the oldest block: wait for its scores and hand them out before its staging memory is reused
        rc = host_block_deliver(w, b);
        if (rc) return rc;
    }
    const int i = r.count[b];
    *idx_slot = r.h_idx + ((size_t)b * r.g + i) * r.idx_slot;
    *dense_slot = r.dense_slot ? r.h_dense + ((size_t)b * r.g + i) * r.dense_slot : nullptr;
    return FR_OK;
}

// The batch written into the current slot joins its block; a full block leaves (H2D, fused launch, D2H).
static int host_slot_commit(fr_worker *w, int batch, float *h_scores) {
    fr_worker::HostRing &r = w->hr;
    const int b = r.cur, i = r.count[b];
    r.dst[b][i] = h_scores;
    r.bsz[b][i] = batch;
    r.count[b] = i + 1;
    w->in_flight = true;
    return (r.count[b] >= r.g) ? host_block_launch(w) : FR_OK;
}

extern "C" int fr_worker_push_host(fr_worker *w, int batch, const int32_t *h_idx, const float *h_dense, float *h_scores) {
    if (!w) FR_FAIL(FR_ERR_INVALID, "worker is NULL");
    if (!h_idx || !h_scores) FR_FAIL(FR_ERR_INVALID, "NULL host pointer");
    if (w->ctx->model.dense_len && !h_dense) FR_FAIL(FR_ERR_INVALID, "model has dense features but h_dense is NULL");
    if (w->hr.staged) FR_FAIL(FR_ERR_STATE, "a staging slot is acquired: push it with fr_worker_push_staged first");
    int32_t *si = nullptr;
    float *sd = nullptr;
    int rc = host_slot_prepare(w, batch, &si, &sd);
    if (rc) return rc;
    memcpy(si, h_idx, (size_t)batch * idx_cols(w->ctx) * sizeof(int32_t));
    if (sd) memcpy(sd, h_dense, (size_t)batch * w->ctx->model.dense_len * sizeof(float));
    return host_slot_commit(w, batch, h_scores);
}

extern "C" int fr_worker_stage_acquire(fr_worker *w, int batch, int32_t **h_idx, float **h_dense) {
    if (!w) FR_FAIL(FR_ERR_INVALID, "worker is NULL");
    if (!h_idx) FR_FAIL(FR_ERR_INVALID, "h_idx is NULL");
    if (w->ctx->model.dense_len && !h_dense) FR_FAIL(FR_ERR_INVALID, "model has dense features but h_dense is NULL");
    if (w->hr.staged) FR_FAIL(FR_ERR_STATE, "a staging slot is already acquired");
    int32_t *si = nullptr;
    float *sd = nullptr;
    int rc = host_slot_prepare(w, batch, &si, &sd);
    if (rc) return rc;
    *h_idx = si;
    if (h_dense) *h_dense = sd;
    w->hr.staged = batch;
    return FR_OK;
}

extern "C" int fr_worker_push_staged(fr_worker *w, int batch, float *h_scores) {
    if (!w) FR_FAIL(FR_ERR_INVALID, "worker is NULL");
    if (!h_scores) FR_FAIL(FR_ERR_INVALID, "h_scores is NULL");
    if (!w->hr.staged) FR_FAIL(FR_ERR_STATE, "no staging slot acquired (fr_worker_stage_acquire)");
    if (batch < 1 || batch > w->hr.staged) FR_FAIL(FR_ERR_INVALID, "batch %d outside (0, %d] acquired", batch, w->hr.staged);
    w->hr.staged = 0;
    return host_slot_commit(w, batch, h_scores);
}

static int host_ring_drain(fr_worker *w) {
    fr_worker::HostRing &r = w->hr;
    if (!r.g) return FR_OK;
    r.staged = 0;                   // an acquired slot that was never pushed is dropped
    int rc = host_block_launch(w);  // partial block
    if (rc) return rc;
    for (int k = 0; k < FR_HOST_BLOCKS; k++) {
        rc = host_block_deliver(w, (r.cur + k) % FR_HOST_BLOCKS);  // oldest first
        if (rc) return rc;
    }
    return FR_OK;
}

extern "C" int fr_ctx_get_fp8_exponents(const fr_ctx *ctx, int act_exp[4], int w_exp[3]) {
    if (!ctx || !act_exp || !w_exp) FR_FAIL(FR_ERR_INVALID, "NULL argument");
    for (int l = 0; l < 4; l++) act_exp[l] = ctx->f8_e_act[l];
    for (int l = 0; l < 3; l++) w_exp[l] = ctx->f8_e_w[l];
    return FR_OK;
}

extern "C" int fr_ctx_set_fp8_act_exponents(fr_ctx *ctx, const int act_exp[4]) {
    if (!ctx || !act_exp) FR_FAIL(FR_ERR_INVALID, "NULL argument");
    for (int l = 0; l < 4; l++)
        if (act_exp[l] < -100 || act_exp[l] > 100) FR_FAIL(FR_ERR_INVALID, "act_exp[%d]=%d outside [-100, 100]", l, act_exp[l]);
    for (int l = 0; l < 4; l++) ctx->f8_e_act[l] = act_exp[l];
    ctx->f8_calibrated = true;
    return FR_OK;
}

// max |.| of X, R1, R2, R3 of the batch whose (virtual) stage 0 ran in launch L0 -> the context's activation exponents
static int f8_calibrate_finish(fr_worker *w, uint64_t L0, int batch) {
    fr_ctx *c = w->ctx;
    const int32_t *fc = c->model.fc;
    const size_t ldm = (size_t)round_up(batch, 32);
    const float *reg[4] = {act_set(w, (int)(L0 & 1)).x, act_set(w, (int)((L0 + 1) & 1)).r1, act_set(w, (int)((L0 + 2) & 1)).r2,
                           act_set(w, (int)((L0 + 3) & 1)).r3};
    for (int l = 0; l < 4; l++) {
        // with an epilogue the buffers hold the POST-activation R1..R3 (the calibration batch runs unsplit: every stage applies its own layer's), and the
        // pad items hold relu(b) instead of zeros: they are left out
        int rc = frk_stats(reg[l], (size_t)fc[l] * ldm, c->d_stats + 2 * l, w->stream, c->any_epi() ? (int)ldm : 0, batch);
        if (rc) return rc;
    }
    uint32_t st[8];
    FR_HIP(hipMemcpyAsync(st, c->d_stats, sizeof(st), hipMemcpyDeviceToHost, w->stream));
    FR_HIP(hipStreamSynchronize(w->stream));
    if (__atomic_load_n(w->h_err, __ATOMIC_ACQUIRE)) {
        __atomic_store_n(w->h_err, 0, __ATOMIC_RELEASE);
        FR_FAIL(FR_ERR_INDEX_RANGE, "a lookup index of the calibration batch was outside its table");
    }
    for (int l = 0; l < 4; l++) {
        float absmax;
        memcpy(&absmax, &st[2 * l], 4);
        if (absmax > 0.0f && std::isfinite(absmax)) c->f8_e_act[l] = floor_log2f(448.0f / (2.0f * absmax));  // one binade of headroom
    }
    c->f8_calibrated = true;
    return FR_OK;
}

extern "C" int fr_worker_calibrate_fp8(fr_worker *w, int batch) {
    int rc = check_ready(w, batch, true, true);
    if (rc) return rc;
    fr_ctx *c = w->ctx;
    FR_NOT_ON_CPU(c, "fr_worker_calibrate_fp8");
    if (c->n_shards > 1 || c->model.layout != FR_LAYOUT_SEMANTIC) FR_FAIL(FR_ERR_STATE, "fp8 calibration from index rows: unsharded SEMANTIC contexts only (sharded: fr_worker_calibrate_fp8_slices)");
    if (w->in_flight || w->n_active || w->n_pending) FR_FAIL(FR_ERR_STATE, "worker busy: call fr_worker_sync first");
    FR_SET_DEVICE(c);
    FR_TRY(c->d_stats.grow(FrMem::DEVICE, 16, "reduction scratch"));
    FR_HIP(hipMemcpyAsync(w->d_idx, w->h_idx, (size_t)batch * idx_cols(c) * sizeof(int32_t), hipMemcpyHostToDevice, w->stream));
    if (c->model.dense_len)
        FR_HIP(hipMemcpyAsync(w->d_dense, w->h_dense, (size_t)batch * c->model.dense_len * sizeof(float), hipMemcpyHostToDevice, w->stream));
    rc = check_gather_args(w, w->d_idx, w->d_dense);
    if (rc) return rc;
    const uint64_t L0 = w->launch_no;
    w->calibrating = true;  // fp32 stages, no K-split partials: every activation buffer holds whole sums
    rc = pipeline_push(w, batch, 0, w->d_idx, w->d_dense, w->d_score);
    if (!rc) rc = pipeline_flush(w);
    w->calibrating = false;
    if (rc) return rc;
    return f8_calibrate_finish(w, L0, batch);
}

// The sharded form: calibrate on all-gathered slices (same arguments as fr_worker_fc_from_slices, no scores returned).
extern "C" int fr_worker_calibrate_fp8_slices(fr_worker *w, int batch_total, int item0, int n_items, const float *d_gathered) {
    if (!w) FR_FAIL(FR_ERR_INVALID, "worker is NULL");
    fr_ctx *c = w->ctx;
    FR_NOT_ON_CPU(c, "fr_worker_calibrate_fp8_slices");
    if (w->in_flight) FR_FAIL(FR_ERR_STATE, "worker busy: call fr_worker_sync first");
    FR_SET_DEVICE(c);
    FR_TRY(c->d_stats.grow(FrMem::DEVICE, 16, "reduction scratch"));
    uint64_t L1 = 0;
    w->calibrating = true;
    int rc = fc_from_slices_impl(w, batch_total, item0, n_items, d_gathered, w->d_score, &L1);
    w->calibrating = false;
    if (rc) return rc;
    return f8_calibrate_finish(w, L1 - 1, n_items);
}

// ---- sparse row updates (fleetrec_serving.h) ---------------------------------------------------------------------------------------
// The status word of the set-up stream's list-form calls (fr_ctx_update_rows, fr_ctx_put_keys / _erase_keys / _admit_keys), under lp_mutex: made by
// the first of them, taken -- read and cleared -- by each behind its own launches.
int fr_up_err_ensure(fr_ctx *ctx) {
    if (ctx->h_up_err) return FR_OK;
    FR_TRY(ctx->h_up_err.alloc(FrMem::PINNED_MAPPED, 1, "row-update status word"));
    *ctx->h_up_err = 0;
    FR_HIP(hipHostGetDevicePointer((void **)&ctx->d_up_err, ctx->h_up_err, 0));
    return FR_OK;
}
int fr_up_err_take(fr_ctx *ctx) { return __atomic_exchange_n(ctx->h_up_err.p, 0, __ATOMIC_ACQ_REL); }

static int update_check(fr_ctx *ctx, int table, int n, const void *ids, const void *rows) {
    if (table < 0 || table >= ctx->model.n_tables) FR_FAIL(FR_ERR_INVALID, "table %d out of range", table);
    if (n < 0) FR_FAIL(FR_ERR_INVALID, "n = %d rows", n);
    if (n > 0 && (!ids || !rows)) FR_FAIL(FR_ERR_INVALID, "row_ids / rows is NULL");
    if ((int64_t)n * ctx->tables[table].dim / 4 >= (1ll << 31)) FR_FAIL(FR_ERR_INVALID, "%d rows of %d floats exceed one update (2^31 16-byte words)", n, ctx->tables[table].dim);
    if (!ctx->table_mem[table].resident) FR_FAIL(FR_ERR_STATE, "table %d is not resident on shard %d", table, ctx->shard_rank);
    return FR_OK;
}

// The two launches of an update on stream s, under lp_mutex: the scatter into the fp32 arena, then -- when an operand-type bank image exists and is
// current for the table contents -- the conversion of the same listed rows, read back from the arena, at the image's own X exponent.
static int update_enqueue(fr_ctx *c, int table, int n, const int32_t *d_ids, const float *d_rows, int *d_err, hipStream_t s) {
    const fr_table_desc &d = c->tables[table];
    const FrTableMem &tm = c->table_mem[table];
    const int64_t head_rows = tm.il_rows ? (int64_t)tm.il_rows : d.rows;
    int rc = frk_scatter_rows((float *)(c->table_arena + tm.byte_offset), (int64_t)tm.row_stride, (float *)(c->table_arena + tm.tail_offset), head_rows, d.rows, d.dim, n, d_ids, d_rows,
                              d_err, s);
    if (rc) return rc;
    if (c->lp_prec != 0 && c->lp_tables_gen == c->tables_gen && c->d_words_lp && (size_t)table < c->lp_tables.size() && c->lp_tables[table].rows) {
        const fr_ctx::LpTable &lt = c->lp_tables[table];
        const int64_t image_rows = (int64_t)lt.rows < head_rows ? (int64_t)lt.rows : head_rows;   // (always lt.rows: the image holds rows of the head region only)
        rc = frk_convert_rows_lp(c->lp_prec, c->table_arena + tm.byte_offset, (size_t)tm.row_stride, c->lp_arena + lt.base, lt.stride, n, d.dim, c->lp_e_x, s, d_ids, image_rows);
    }
    return rc;
}

extern "C" int fr_worker_update_rows(fr_worker *w, int table, int n, const int32_t *d_row_ids, const float *d_rows) {
    if (!w) FR_FAIL(FR_ERR_INVALID, "worker is NULL");
    fr_ctx *c = w->ctx;
    int rc = update_check(c, table, n, d_row_ids, d_rows);
    if (rc) return rc;
    if (n == 0) return FR_OK;
    if (c->cpu) {   // computed before the call returns; a range error waits in c_err for fr_worker_sync, like the gathers'
        if (frc_update_rows(c->table_arena, c->table_mem[table], c->tables[table].dim, c->tables[table].rows, n, d_row_ids, d_rows)) __atomic_store_n(&w->c_err, 1, __ATOMIC_RELEASE);
        return FR_OK;
    }
    if ((uintptr_t)d_rows % 16) FR_FAIL(FR_ERR_INVALID, "d_rows must be 16-byte aligned");
    FR_TRY(fr_host_fed_queued(w, "update"));
    FR_SET_DEVICE(c);
    rc = fr_fused_flush(w);   // batches fr_worker_push_device queued for a fused launch were pushed BEFORE the update: they gather the old rows
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->lp_mutex);
    rc = update_enqueue(c, table, n, d_row_ids, d_rows, w->d_err, w->stream);
    // (recorded even when the second launch failed: the first may be running)
    if (hipEventRecord(w->ev_update, w->stream) == hipSuccess) w->update_recorded = true;
    return rc;
}

extern "C" int fr_ctx_update_rows(fr_ctx *ctx, int table, int n, const int32_t *h_row_ids, const float *h_rows) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    int rc = update_check(ctx, table, n, h_row_ids, h_rows);
    if (rc) return rc;
    if (n == 0) return FR_OK;
    const int dim = ctx->tables[table].dim;
    if (ctx->cpu) {
        if (frc_update_rows(ctx->table_arena, ctx->table_mem[table], dim, ctx->tables[table].rows, n, h_row_ids, h_rows))
            FR_FAIL(FR_ERR_INDEX_RANGE, "a listed row id was outside table %d (that row was not written, the others were)", table);
        return FR_OK;
    }
    FR_SET_DEVICE(ctx);
    std::lock_guard<std::mutex> lk(ctx->lp_mutex);   // also serialises the set-up stream and the staging buffers against other updates and an image build
    FR_TRY(fr_up_err_ensure(ctx));
    const size_t n_floats = (size_t)n * (size_t)dim;
    FR_TRY(ctx->d_up_ids.grow(FrMem::DEVICE, (size_t)n, "row-update ids"));
    FR_TRY(ctx->d_up_rows.grow(FrMem::DEVICE, n_floats, "row-update rows"));
    FR_HIP(hipMemcpyAsync(ctx->d_up_ids, h_row_ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->setup_stream));
    FR_HIP(hipMemcpyAsync(ctx->d_up_rows, h_rows, n_floats * sizeof(float), hipMemcpyHostToDevice, ctx->setup_stream));
    rc = update_enqueue(ctx, table, n, ctx->d_up_ids, ctx->d_up_rows, ctx->d_up_err, ctx->setup_stream);
    FR_HIP(hipStreamSynchronize(ctx->setup_stream));
    if (rc) return rc;
    if (fr_up_err_take(ctx)) FR_FAIL(FR_ERR_INDEX_RANGE, "a listed row id was outside table %d (that row was not written, the others were)", table);
    return FR_OK;
}

// ---- segmented top-K ranking (fleetrec_serving.h) -----------------------------------------------------------------------------------------
// The kernels are the companion code object's (fr_rank.hip -> libfleetrec_rank.so, linked with an $ORIGIN rpath); state, order and the CPU twin are here.
static int topk_check(fr_worker *w, int n, const void *scores, int n_seg, int k, const void *top_idx) {
    if (!w) FR_FAIL(FR_ERR_INVALID, "worker is NULL");
    if (k < 1 || k > FR_TOPK_MAX_K) FR_FAIL(FR_ERR_INVALID, "k = %d outside [1, %d]", k, FR_TOPK_MAX_K);
    if (n < 1 || n > (1 << 24)) FR_FAIL(FR_ERR_INVALID, "n = %d scores outside [1, 2^24]", n);
    if (n_seg < 1 || n_seg > n + 1) FR_FAIL(FR_ERR_INVALID, "n_seg = %d outside [1, n + 1 = %d]", n_seg, n + 1);
    if (!scores || !top_idx) FR_FAIL(FR_ERR_INVALID, "d_scores / d_top_idx is NULL");
    return FR_OK;
}

// behind everything submitted or pushed on w: queued fused batches are launched, the stage pipeline is drained by launches; nothing is waited for
static int topk_enqueue(fr_worker *w, int n, const float *d_scores, int n_seg, const int32_t *d_off, int k, int32_t *d_top_idx, float *d_top_scores) {
    fr_ctx *c = w->ctx;
    FR_TRY(fr_host_fed_queued(w, "rank"));
    if (w->sh_comm) FR_FAIL(FR_ERR_STATE, "a table-sharded step is in flight on this worker: call fr_worker_sync first, then rank");
    FR_SET_DEVICE(c);
    FrRankArgs a{};
    a.scores = d_scores, a.off = d_off, a.n = n, a.n_seg = n_seg, a.k = k;
    a.top_idx = d_top_idx, a.top_scores = d_top_scores, a.err_flag = w->d_err;
    a.u_cap = fr_rank_units(n);
    if (a.u_cap) {   // a segment may be longer than one workgroup streams: unit records and candidate lists in the worker's scratch
        const size_t map_bytes = align_up((size_t)a.u_cap * sizeof(int4), 256);
        const size_t need = 256 + map_bytes + (size_t)a.u_cap * FR_TOPK_MAX_K * sizeof(unsigned long long);
        if (need > w->d_rank.count()) {
            if (w->d_rank) FR_HIP(hipStreamSynchronize(w->stream));   // an earlier ranking may still read it
            FR_TRY(w->d_rank.grow(FrMem::DEVICE, need, "ranking scratch"));
        }
        a.hdr = reinterpret_cast<int *>(w->d_rank.p);
        a.unitmap = reinterpret_cast<int4 *>(w->d_rank + 256);
        a.cand = reinterpret_cast<unsigned long long *>(w->d_rank + 256 + map_bytes);
    }
    int rc = fr_fused_flush(w);
    if (!rc) rc = pipeline_flush(w);
    if (rc) return rc;
    // a wave per segment when the segments are short on average (the host does not know the offsets: any length is ranked correctly by either form)
    const int wave_form = n / n_seg <= 512;
    const int e = fr_rank_launch(&a, wave_form, (void *)w->stream);
    if (e) FR_FAIL(FR_ERR_HIP, "the ranking launch failed: %s", hipGetErrorString((hipError_t)e));
    w->in_flight = true;
    return FR_OK;
}

extern "C" int fr_worker_topk_device(fr_worker *w, int n, const float *d_scores, int n_seg, const int32_t *d_seg_offsets, int k, int32_t *d_top_idx, float *d_top_scores) {
    int rc = topk_check(w, n, d_scores, n_seg, k, d_top_idx);
    if (rc) return rc;
    if (w->ctx->cpu) {   // computed before the call returns; a malformed segment waits in c_err for fr_worker_sync
        if (frc_rank_topk(d_scores, n, n_seg, d_seg_offsets, k, d_top_idx, d_top_scores)) __atomic_store_n(&w->c_err, 1, __ATOMIC_RELEASE);
        return FR_OK;
    }
    return topk_enqueue(w, n, d_scores, n_seg, d_seg_offsets, k, d_top_idx, d_top_scores);
}

extern "C" int fr_worker_topk(fr_worker *w, int batch, int n_seg, const int32_t *h_seg_offsets, int k, int32_t *h_top_idx, float *h_top_scores) {
    int rc = topk_check(w, batch, w ? w->h_score.p : nullptr, n_seg, k, h_top_idx);
    if (rc) return rc;
    if (w->sh_comm || w->ctx->n_shards > 1) FR_FAIL(FR_ERR_STATE, "fr_worker_topk ranks a host-form batch; a table-sharded step is not one");
    if (!w->host_batch)
        FR_FAIL(FR_ERR_STATE, "no host-form batch is in flight on this worker (fr_worker_submit, fr_worker_submit_pooled, _pooled_weighted, _pooled_csr): submit first, rank, then sync");
    if (batch != w->host_batch) FR_FAIL(FR_ERR_INVALID, "batch %d, but the host-form batch in flight has %d items", batch, w->host_batch);
    if (w->ctx->cpu) {
        if (frc_rank_topk(w->h_score, batch, n_seg, h_seg_offsets, k, h_top_idx, h_top_scores)) __atomic_store_n(&w->c_err, 1, __ATOMIC_RELEASE);
        return FR_OK;
    }
    if (w->tk_count) FR_FAIL(FR_ERR_STATE, "a host-form ranking is already in flight on this worker: call fr_worker_sync first");
    FR_SET_DEVICE(w->ctx);
    const size_t n_off = h_seg_offsets ? (size_t)n_seg + 1 : 0, n_out = (size_t)n_seg * (size_t)k;
    if (n_off > w->h_tk_off.count() || n_out > w->h_tk_idx.count() || n_out > w->h_tk_sc.count()) {   // a grow waits for the stream before pinned memory is released (the header says so)
        FR_HIP(hipStreamSynchronize(w->stream));
        if (n_off) FR_TRY(w->h_tk_off.grow(FrMem::PINNED, n_off, "ranking offsets"));
        FR_TRY(w->h_tk_idx.grow(FrMem::PINNED, n_out, "ranking results"));
        FR_TRY(w->h_tk_sc.grow(FrMem::PINNED, n_out, "ranking result scores"));
    }
    if (n_off) memcpy(w->h_tk_off, h_seg_offsets, n_off * sizeof(int32_t));
    // as fr_worker_submit's scores: the kernels read the pinned scores and offsets in place and write the pinned results
    rc = topk_enqueue(w, batch, w->h_score, n_seg, n_off ? w->h_tk_off.p : nullptr, k, w->h_tk_idx, h_top_scores ? w->h_tk_sc.p : nullptr);
    if (rc) return rc;
    w->tk_dst_idx = h_top_idx, w->tk_dst_sc = h_top_scores, w->tk_count = n_out;
    return FR_OK;
}

// ---- request-form batches (fleetrec_serving.h) -------------------------------------------------------------------------------------------------
// The kernel is the second companion code object's (fr_request.hip -> libfleetrec_request.so, linked with an $ORIGIN rpath); the descriptor tables,
// state and the host form are here, the CPU twin in fr_cpu.cpp.
// The tables of the three forms from a mask, dense_shared and the hots (NULL: no pooling) they are to serve: word w of a full row is word desc[w] of the candidate row
// (desc[w] >= 0) or word ~desc[w] of the request row (desc[w] < 0); both sides keep their columns in ascending order, a pooled column its slots.
static int request_prepare(fr_ctx *ctx, const std::vector<int32_t> &shared, bool dense_shared, const int32_t *hots, RequestTables &t) {
    if (shared.empty()) return FR_OK;
    const int cols = (int)idx_cols(ctx);
    for (int form = FR_REQ_ONE_HOT; form <= FR_REQ_POOLED; form++) {
        if (form == FR_REQ_POOLED && !hots) continue;
        for (int c = 0; c < cols; c++)
            for (int h = 0, n = form == FR_REQ_POOLED ? hots[c] : 1; h < n; h++)
                t.f[form].desc.push_back(shared[(size_t)c] ? ~(t.f[form].req_words++) : t.f[form].cand_words++);
    }
    if (dense_shared) {
        for (int k = 0; k < ctx->model.dense_len; k++) t.f[FR_REQ_DENSE].desc.push_back(~k);
        t.f[FR_REQ_DENSE].req_words = ctx->model.dense_len;
    }
    size_t total = 0;
    for (int form = 0; form < 3; form++) t.f[form].d_first = total, total += t.f[form].desc.size();
    if (!ctx->cpu) {
        FR_TRY(t.d.alloc(FrMem::DEVICE, total ? total : 1, "request-form descriptors"));
        for (int form = 0; form < 3; form++) {
            if (t.f[form].desc.empty()) continue;
            const hipError_t e = hipMemcpy(t.d + t.f[form].d_first, t.f[form].desc.data(), sizeof(int32_t) * t.f[form].desc.size(), hipMemcpyHostToDevice);
            if (e != hipSuccess) FR_FAIL(FR_ERR_HIP, "hipMemcpy(request-form descriptors) failed: %s", hipGetErrorString(e));
        }
    }
    t.made = true;
    return FR_OK;
}

static void request_commit(fr_ctx *ctx, RequestTables &t) {
    if (!t.made) return;
    ctx->d_req_desc.swap(t.d);
    for (int form = 0; form < 3; form++) std::swap(ctx->req_form[form], t.f[form]);
}

extern "C" int fr_ctx_set_request_columns(fr_ctx *ctx, const int32_t *shared, int n_cols, int dense_shared) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    if (ctx->n_shards > 1) FR_FAIL(FR_ERR_STATE, "fr_ctx_set_request_columns: request-form batches are not available on a sharded context (%d shards)", ctx->n_shards);
    const int cols = (int)idx_cols(ctx);
    if (shared) {
        if (n_cols != cols) FR_FAIL(FR_ERR_INVALID, "fr_ctx_set_request_columns: n_cols %d, the context has %d index columns", n_cols, cols);
        if (dense_shared != 0 && dense_shared != 1) FR_FAIL(FR_ERR_INVALID, "fr_ctx_set_request_columns: dense_shared = %d is neither 0 nor 1", dense_shared);
        if (dense_shared && !ctx->model.dense_len) FR_FAIL(FR_ERR_INVALID, "fr_ctx_set_request_columns: dense_shared on a model without dense features");
        int n_shared = 0;
        for (int c = 0; c < cols; c++) {
            if (shared[c] != 0 && shared[c] != 1) FR_FAIL(FR_ERR_INVALID, "fr_ctx_set_request_columns: shared[%d] = %d is neither 0 nor 1", c, shared[c]);
            n_shared += shared[c];
        }
        if (!n_shared && !dense_shared) FR_FAIL(FR_ERR_INVALID, "fr_ctx_set_request_columns: nothing is shared (no shared column, no shared dense features)");
        if (n_shared == cols && (!ctx->model.dense_len || dense_shared))
            FR_FAIL(FR_ERR_INVALID, "fr_ctx_set_request_columns: nothing is left per item (every column is shared and there are no per-item dense features)");
    }
    const int rc = fr_pooling_busy(ctx, "fr_ctx_set_request_columns");
    if (rc) return rc;
    if (!ctx->cpu) FR_SET_DEVICE(ctx);
    if (!shared) {
        ctx->d_req_desc.reset();
        ctx->req_shared.clear();
        ctx->req_dense_shared = false;
        for (fr_ctx::ReqForm &f : ctx->req_form) f = fr_ctx::ReqForm{};
        return FR_OK;
    }
    std::vector<int32_t> mask(shared, shared + cols);
    RequestTables rt;
    const int irc = request_prepare(ctx, mask, dense_shared != 0, ctx->pool_cols > 0 ? ctx->pool_hots.data() : nullptr, rt);
    if (irc) return irc;   // the split that was set stays
    ctx->req_shared.swap(mask);
    ctx->req_dense_shared = dense_shared != 0;
    request_commit(ctx, rt);
    return FR_OK;
}

// the form's table, or the reason there is none (FR_ERR_STATE)
static int request_form(const fr_ctx *c, int form, const fr_ctx::ReqForm **out) {
    if (c->req_shared.empty()) FR_FAIL(FR_ERR_STATE, "no request split is set on the context: call fr_ctx_set_request_columns first");
    if (form == FR_REQ_POOLED && c->pool_cols <= 0) FR_FAIL(FR_ERR_STATE, "the pooled request form needs pooling: call fr_ctx_set_pooling first");
    if (form == FR_REQ_DENSE && !c->req_dense_shared) FR_FAIL(FR_ERR_STATE, "the dense request form needs dense_shared (fr_ctx_set_request_columns)");
    *out = &c->req_form[form];
    return FR_OK;
}

extern "C" int fr_ctx_request_words(const fr_ctx *ctx, int form, int *req_words, int *cand_words, int *row_words) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    if (form < FR_REQ_ONE_HOT || form > FR_REQ_DENSE) FR_FAIL(FR_ERR_INVALID, "form %d is no request form", form);
    const fr_ctx::ReqForm *f = nullptr;
    const int rc = request_form(ctx, form, &f);
    if (rc) return rc;
    if (req_words) *req_words = f->req_words;
    if (cand_words) *cand_words = f->cand_words;
    if (row_words) *row_words = (int)f->desc.size();
    return FR_OK;
}

// the one launch (the CPU back-end: the twin, computed here; malformed offsets wait in the sticky word)
static int request_enqueue(fr_worker *w, const fr_ctx::ReqForm &f, int batch, int n_req, const int32_t *off, const void *req, const void *cand, void *out) {
    fr_ctx *c = w->ctx;
    FrRequestArgs a{};
    a.off = off, a.req = static_cast<const uint32_t *>(req), a.cand = static_cast<const uint32_t *>(cand), a.out = static_cast<uint32_t *>(out);
    a.batch = batch, a.n_req = n_req, a.W = (int)f.desc.size(), a.Rs = f.req_words, a.Rc = f.cand_words;
    a.tile = fr_request_tile(a.W);
    if (c->cpu) {
        a.desc = f.desc.data(), a.err_flag = &w->c_err;
        if (frc_expand_requests(a)) __atomic_store_n(&w->c_err, 1, __ATOMIC_RELEASE);
        return FR_OK;
    }
    a.desc = c->d_req_desc + f.d_first, a.err_flag = w->d_err;
    const int e = fr_request_launch(&a, (void *)w->stream);
    if (e) FR_FAIL(FR_ERR_HIP, "the request expansion launch failed: %s", hipGetErrorString((hipError_t)e));
    w->in_flight = true;
    return FR_OK;
}

extern "C" int fr_worker_expand_requests_device(fr_worker *w, int batch, int n_req, const int32_t *d_seg_offsets, const void *d_req_rows, const void *d_cand_rows, int form,
                                                void *d_rows_out) {
    if (!w) FR_FAIL(FR_ERR_INVALID, "worker is NULL");
    if (batch <= 0 || batch > w->max_batch) FR_FAIL(FR_ERR_INVALID, "batch %d outside (0, max_batch=%d]", batch, w->max_batch);
    if (n_req < 1 || n_req > (1 << 24)) FR_FAIL(FR_ERR_INVALID, "n_req = %d outside [1, 2^24]", n_req);
    if (form < FR_REQ_ONE_HOT || form > FR_REQ_DENSE) FR_FAIL(FR_ERR_INVALID, "form %d is no request form", form);
    if (!d_req_rows || !d_rows_out) FR_FAIL(FR_ERR_INVALID, "d_req_rows / d_rows_out is NULL");
    const fr_ctx::ReqForm *f = nullptr;
    const int rc = request_form(w->ctx, form, &f);
    if (rc) return rc;
    if (f->cand_words && !d_cand_rows) FR_FAIL(FR_ERR_INVALID, "d_cand_rows is NULL, the form has %d candidate words per item", f->cand_words);
    if (!d_seg_offsets && batch % n_req) FR_FAIL(FR_ERR_INVALID, "NULL offsets ask for %d equal requests, batch %d is no multiple", n_req, batch);
    const uint64_t bound = (uint64_t)4000 << 20;
    if ((uint64_t)batch * f->desc.size() * 4 >= bound || (uint64_t)batch * (uint64_t)f->cand_words * 4 >= bound || (uint64_t)n_req * (uint64_t)f->req_words * 4 >= bound ||
        ((uint64_t)n_req + 1) * 4 >= bound)
        FR_FAIL(FR_ERR_INVALID, "request expansion: the expanded rows (%d x %zu words), the candidate rows, the request rows (%d x %d words) or the offsets reach 4000 MiB", batch,
                f->desc.size(), n_req, f->req_words);
    if (!w->ctx->cpu) FR_SET_DEVICE(w->ctx);
    return request_enqueue(w, *f, batch, n_req, d_seg_offsets, d_req_rows, d_cand_rows, d_rows_out);
}

extern "C" int fr_worker_submit_requests(fr_worker *w, int batch, int n_req, int pooled) {
    int rc = check_ready(w, batch, true, true);
    if (rc) return rc;
    if (pooled < 0 || pooled > 2) FR_FAIL(FR_ERR_INVALID, "pooled = %d: 0 one-hot, 1 pooled, 2 pooled weighted", pooled);
    if (n_req < 1 || n_req > w->max_batch) FR_FAIL(FR_ERR_INVALID, "n_req = %d outside [1, max_batch=%d]", n_req, w->max_batch);
    fr_ctx *c = w->ctx;
    const bool weighted = pooled == 2;
    const fr_ctx::ReqForm *f = nullptr, *fd = nullptr;
    rc = request_form(c, pooled ? FR_REQ_POOLED : FR_REQ_ONE_HOT, &f);
    if (rc) return rc;
    if (!w->h_req_idx || !w->h_req_off || (c->req_dense_shared && !w->h_req_dense) || !w->d_idx)
        FR_FAIL(FR_ERR_STATE, "the worker has no request buffers: create the worker after fr_ctx_set_request_columns");
    if (pooled) {
        rc = pooled_host_ready(w, batch, weighted);
        if (rc) return rc;
        if (weighted) rc = fr_pooled_weights_need_sum(c);
        if (rc) return rc;
        if (weighted && (!w->h_req_w || !w->d_pool_w || w->req_w_cap < f->req_words))
            FR_FAIL(FR_ERR_STATE, "the worker's request weight buffer holds %d words per request, the split needs %d: create the worker after fr_ctx_set_pooling and fr_ctx_set_request_columns",
                    w->req_w_cap, f->req_words);
    } else if (w->in_flight) {
        FR_FAIL(FR_ERR_STATE, "a batch is already in flight on this worker: call fr_worker_sync first");
    }
    if (w->req_idx_cap < f->req_words)
        FR_FAIL(FR_ERR_STATE, "the worker's request index buffer holds %d words per request, the split needs %d: create the worker after the split and the pooling are set", w->req_idx_cap,
                f->req_words);
    if (w->n_active || w->n_pending) FR_FAIL(FR_ERR_STATE, "pipeline busy (push_device in flight): call fr_worker_sync first");
    if (c->req_dense_shared) {
        rc = request_form(c, FR_REQ_DENSE, &fd);
        if (rc) return rc;
    }
    // the host knows the offsets: the two ends are checked here, before anything is enqueued (the pair checks are the expansion's)
    if (w->h_req_off[0] != 0) FR_FAIL(FR_ERR_INVALID, "fr_worker_submit_requests: offsets[0] is %d, not 0", w->h_req_off[0]);
    if (w->h_req_off[n_req] != batch) FR_FAIL(FR_ERR_INVALID, "fr_worker_submit_requests: offsets[n_req] is %d, the batch has %d items", w->h_req_off[n_req], batch);
    if (!c->cpu) FR_SET_DEVICE(c);
    // up to three expansions read the pinned arrays in place and write the worker's device buffers; the unchanged submit runs behind them
    rc = request_enqueue(w, *f, batch, n_req, w->h_req_off, w->h_req_idx, w->h_idx, w->d_idx);
    if (!rc && weighted) rc = request_enqueue(w, *f, batch, n_req, w->h_req_off, w->h_req_w, w->h_pool_w, w->d_pool_w);
    if (!rc && fd) rc = request_enqueue(w, *fd, batch, n_req, w->h_req_off, w->h_req_dense, nullptr, w->d_dense);
    if (rc) return rc;
    const float *dense = fd ? w->d_dense.p : (c->model.dense_len ? w->h_dense.p : nullptr);
    if (pooled) rc = submit_pooled_impl(w, weighted ? pooled_batch_weighted(batch, w->d_idx, w->d_pool_w, dense) : FrPooledBatch{batch, w->d_idx, nullptr, dense}, w->h_score);
    else rc = launch_pipeline(w, batch, w->d_idx, dense, w->h_score);
    if (rc) return rc;
    w->in_flight = true, w->host_batch = batch;   // (fr_worker_topk ranks it)
    return FR_OK;
}

// ---- keyed lookups (fleetrec_serving.h): fr_keyspace.cpp; the host form's submit is here, beside the submit paths it calls ---------------------------
extern "C" int fr_worker_submit_keyed(fr_worker *w, int batch, int pooled) {
    int rc = check_ready(w, batch, true, true);
    if (rc) return rc;
    if (pooled < 0 || pooled > 2) FR_FAIL(FR_ERR_INVALID, "pooled = %d: 0 one-hot, 1 pooled, 2 pooled weighted", pooled);
    fr_ctx *c = w->ctx;
    const bool weighted = pooled == 2;
    if (!w->h_keys || !w->d_idx) FR_FAIL(FR_ERR_STATE, "the worker has no key buffer: create the worker after the context's first fr_ctx_set_key_space");
    if (pooled) {
        rc = pooled_host_ready(w, batch, weighted);
        if (!rc && weighted) rc = fr_pooled_weights_need_sum(c);
        if (rc) return rc;
    } else if (w->in_flight) {
        FR_FAIL(FR_ERR_STATE, "a batch is already in flight on this worker: call fr_worker_sync first");
    }
    if (w->n_active || w->n_pending) FR_FAIL(FR_ERR_STATE, "pipeline busy (push_device in flight): call fr_worker_sync first");
    FR_TRY(fr_key_unsharded(c, "fr_worker_submit_keyed"));
    if (!c->cpu) FR_SET_DEVICE(c);
    // the resolve reads the pinned keys in place and writes the worker's device index buffer; the unchanged submit runs behind it
    rc = fr_key_resolve_enqueue(w, batch, FR_KEY_ROWS_FULL, pooled ? 1 : 0, w->h_keys, w->d_idx, "fr_worker_submit_keyed");
    if (rc) return rc;
    const float *dense = c->model.dense_len ? w->h_dense.p : nullptr;
    if (pooled) rc = submit_pooled_impl(w, weighted ? pooled_batch_weighted(batch, w->d_idx, w->h_pool_w, dense) : FrPooledBatch{batch, w->d_idx, nullptr, dense}, w->h_score);
    else rc = launch_pipeline(w, batch, w->d_idx, dense, w->h_score);
    if (rc) return rc;
    w->in_flight = true, w->host_batch = batch;   // (fr_worker_topk ranks it)
    return FR_OK;
}

// Launch what is queued -- the partially filled host block, the batches queued by fr_worker_push_device -- without waiting for it.
extern "C" int fr_worker_flush(fr_worker *w) {
    if (!w) FR_FAIL(FR_ERR_INVALID, "worker is NULL");
    if (w->hr.staged) FR_FAIL(FR_ERR_STATE, "a staging slot is acquired: push it with fr_worker_push_staged first");
    FR_SET_DEVICE(w->ctx);
    if (w->hr.g) {
        int rc = host_block_launch(w);
        if (rc) return rc;
    }
    return fr_fused_flush(w);
}

// Hand out the scores of the host-fed blocks that have finished, oldest first, WITHOUT waiting for the others; *delivered = host-fed
// batches delivered since the worker was created (they are delivered in push order).
extern "C" int fr_worker_host_poll(fr_worker *w, long long *delivered) {
    if (!w) FR_FAIL(FR_ERR_INVALID, "worker is NULL");
    fr_worker::HostRing &r = w->hr;
    if (r.g) {
        FR_SET_DEVICE(w->ctx);
        for (int k = 0; k < FR_HOST_BLOCKS; k++) {
            const int b = (r.cur + k) % FR_HOST_BLOCKS;  // oldest first
            if (!r.inflight[b]) continue;
            const hipError_t q = hipEventQuery(r.ev[b]);
            if (q == hipErrorNotReady) break;
            if (q != hipSuccess) FR_FAIL(FR_ERR_HIP, "hipEventQuery: %s", hipGetErrorString(q));
            int rc = host_block_deliver(w, b);
            if (rc) return rc;
        }
    }
    if (delivered) *delivered = r.delivered;
    return FR_OK;
}

// Host-fed batches that are queued in the block being filled (not launched yet) and that are launched but not delivered yet.
extern "C" int fr_worker_host_pending(const fr_worker *w, int *queued, int *in_flight, int *blocks_in_flight) {
    if (!w) FR_FAIL(FR_ERR_INVALID, "worker is NULL");
    const fr_worker::HostRing &r = w->hr;
    int q = 0, f = 0, nb = 0;
    if (r.g)
        for (int b = 0; b < FR_HOST_BLOCKS; b++) {
            (r.inflight[b] ? f : q) += r.count[b];
            nb += r.inflight[b] ? 1 : 0;
        }
    if (queued) *queued = q;
    if (in_flight) *in_flight = f;
    if (blocks_in_flight) *blocks_in_flight = nb;
    return FR_OK;
}

extern "C" int fr_worker_sync(fr_worker *w) {
    if (!w) FR_FAIL(FR_ERR_INVALID, "worker is NULL");
    // whatever this sync returns, the host-form batch is no longer in flight and an undelivered host-form ranking is dropped
    struct TopkDone {
        fr_worker *w;
        ~TopkDone() { w->host_batch = 0, w->tk_count = 0; }
    } topk_done{w};
    if (w->ctx->cpu) {   // everything was computed inside the calls -- but for a table-sharded step, which runs on the worker's host stream
        const int crc = fr_comm_wait(w);   // (bounded wait + the ranks' status words, fr_comm.cpp; FR_OK at once when no such step is in flight)
        w->in_flight = false;
        if (crc) return crc;
        const int bits = __atomic_exchange_n(&w->c_err, 0, __ATOMIC_ACQ_REL);
        return bits ? fr_index_range_fail(bits) : FR_OK;
    }
    FR_SET_DEVICE(w->ctx);
    if (w->sh_comm && w->sh_host_stream) {
        // a sharded step of a STAGED exchange is issued by the worker's host stream (it blocks in rendezvous): nothing below may touch the worker's
        // pipeline state while that thread still runs the FC chain's launches -- the bounded wait comes first
        const int crc0 = fr_comm_wait(w);
        if (crc0) {
            w->in_flight = false;
            return crc0;
        }
    }
    int frc = host_ring_drain(w);  // host-fed blocks: launch the partial one, deliver every block's scores
    if (!frc) frc = fr_fused_flush(w);  // launch batches still queued by fr_worker_push_device
    if (!frc) frc = pipeline_flush(w);  // drain the stage pipeline
    if (frc) {
        fr_comm_forget(w);   // a sharded step in flight keeps no hold on its communicator past a failed sync
        return frc;
    }
    const int crc = fr_comm_wait(w);  // a table-sharded step in flight: bounded wait + the ranks' status words (fr_comm.cpp)
    if (crc) {
        w->in_flight = false;
        return crc;
    }
    FR_HIP(hipStreamSynchronize(w->stream));
    w->in_flight = false;
    if (w->tk_count) {   // the host-form ranking: out of the pinned staging, as a host-fed block's scores are delivered
        memcpy(w->tk_dst_idx, w->h_tk_idx, w->tk_count * sizeof(int32_t));
        if (w->tk_dst_sc) memcpy(w->tk_dst_sc, w->h_tk_sc, w->tk_count * sizeof(float));
    }
    const int bits = __atomic_exchange_n(w->h_err, 0, __ATOMIC_ACQ_REL);   // (bit 0: the lookups'; the others: a key put's, FR_KEYS_ERR_*)
    return bits ? fr_index_range_fail(bits) : FR_OK;
}

extern "C" int fr_worker_timer_start(fr_worker *w) {
    if (!w) FR_FAIL(FR_ERR_INVALID, "worker is NULL");
    if (w->ctx->cpu) {
        w->c_t0 = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
        return FR_OK;
    }
    FR_SET_DEVICE(w->ctx);
    FR_HIP(hipEventRecord(w->ev_start, w->stream));
    return FR_OK;
}

extern "C" int fr_worker_timer_stop_ms(fr_worker *w, float *ms) {
    if (!w || !ms) FR_FAIL(FR_ERR_INVALID, "NULL argument");
    if (w->ctx->cpu) {
        *ms = (float)(1e3 * (std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() - w->c_t0));
        return FR_OK;
    }
    FR_SET_DEVICE(w->ctx);
    FR_HIP(hipEventRecord(w->ev_stop, w->stream));
    FR_HIP(hipEventSynchronize(w->ev_stop));
    FR_HIP(hipEventElapsedTime(ms, w->ev_start, w->ev_stop));
    return FR_OK;
}

// ---- device memory helpers ------------------------------------------------------------------------------
// fr_device_malloc hands the allocation to the caller; its size is kept for the tally until fr_device_free brings it back
struct Handed {
    void *p;
    size_t bytes;
};
static std::mutex g_handed_mutex;
static std::vector<Handed> g_handed;
extern "C" int fr_device_malloc(fr_ctx *ctx, size_t bytes, void **dptr) {
    if (!ctx || !dptr) FR_FAIL(FR_ERR_INVALID, "NULL argument");
    FR_SET_DEVICE(ctx);   // ("device memory" of the CPU back-end is host memory: the same calling code runs against either)
    FR_TRY(fr_mem_alloc(fr_mem_kind(ctx, FrMem::DEVICE), bytes ? bytes : 1, "fr_device_malloc", dptr));
    std::lock_guard<std::mutex> g(g_handed_mutex);
    g_handed.push_back(Handed{*dptr, bytes ? bytes : 1});
    return FR_OK;
}
extern "C" int fr_device_free(fr_ctx *ctx, void *dptr) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    FR_SET_DEVICE(ctx);
    size_t bytes = 0;
    {
        std::lock_guard<std::mutex> g(g_handed_mutex);
        if (!dptr) return FR_OK;
        size_t i = 0;
        while (i < g_handed.size() && g_handed[i].p != dptr) i++;
        if (i == g_handed.size()) FR_FAIL(FR_ERR_INVALID, "fr_device_free: %p was not handed out by fr_device_malloc (or was freed already)", dptr);
        bytes = g_handed[i].bytes;
        g_handed[i] = g_handed.back();
        g_handed.pop_back();
    }
    fr_mem_release(fr_mem_kind(ctx, FrMem::DEVICE), dptr, bytes);
    return FR_OK;
}
extern "C" int fr_memcpy_h2d(fr_ctx *ctx, void *dptr, const void *host, size_t bytes) {
    if (!ctx || (bytes && (!dptr || !host))) FR_FAIL(FR_ERR_INVALID, "NULL argument");
    if (ctx->cpu) {
        if (bytes) memcpy(dptr, host, bytes);
        return FR_OK;
    }
    FR_SET_DEVICE(ctx);
    if (bytes) FR_HIP(hipMemcpy(dptr, host, bytes, hipMemcpyHostToDevice));
    return FR_OK;
}
extern "C" int fr_memcpy_d2h(fr_ctx *ctx, void *host, const void *dptr, size_t bytes) {
    if (!ctx || (bytes && (!dptr || !host))) FR_FAIL(FR_ERR_INVALID, "NULL argument");
    if (ctx->cpu) {
        if (bytes) memcpy(host, dptr, bytes);
        return FR_OK;
    }
    FR_SET_DEVICE(ctx);
    if (bytes) FR_HIP(hipMemcpy(host, dptr, bytes, hipMemcpyDeviceToHost));
    return FR_OK;
}
extern "C" int fr_device_synchronize(fr_ctx *ctx) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    if (ctx->cpu) return FR_OK;
    FR_SET_DEVICE(ctx);
    FR_HIP(hipDeviceSynchronize());
    return FR_OK;
}
