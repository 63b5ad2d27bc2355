// pooled_csr_san -- the offsets (CSR) form of the pooled lookups (fr_worker_gather_pooled_csr, fr_worker_submit_pooled_csr) on the CPU back-end
// under AddressSanitizer + UBSan, as a program of its own (`make -C gpu-fpga-recommendation-system_amd/csrc san-pooled-csr` links it with the
// library's host sources built under -fsanitize=address,undefined and runs it).  The model is the one of tools/update_rows_san.cpp (one bank
// of three tables and a lone table, a COPY pad), per-bank and per-table, caps 1 .. 9.  Well-formed bags (empty ones, full ones, -1 entries
// inside) run through the offsets form and through the padded form on the same context: the records must be equal byte for byte, for SUM,
// MEAN and weighted.  Then one case of every malformed class (longer than the cap, end > nnz, decreasing offsets, a negative start, an entry
// equal to the row count, an entry of -2): FR_ERR_INDEX_RANGE at sync, and a clean batch right after gives the clean records again.
// offsets, indices, weights and records are heap blocks of exactly the size the call may touch, so a read or write one element past either
// end is a report.  Exit status 0 and "pooled_csr_san: ok" = clean.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "fleetrec.h"
#include "fleetrec_serving.h"

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, fr_last_error()); \
            exit(1);                                                                     \
        }                                                                                \
    } while (0)

static std::mt19937 rng(6400);

template <typename T>
static T *exact(const std::vector<T> &v) {   // a heap block of exactly v's bytes (never NULL: one byte for an empty vector)
    T *p = (T *)malloc(v.empty() ? 1 : v.size() * sizeof(T));
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

struct Bags {
    std::vector<int32_t> off, ind;
    std::vector<float> wt;
};

// -> status of the sync; records into `out` (exact size)
static int run_csr(fr_worker *wk, int B, const Bags &g, int64_t nnz, bool weighted, std::vector<uint32_t> &out) {
    int32_t *off = exact(g.off), *ind = exact(g.ind);
    float *wt = exact(g.wt);
    uint32_t *rec = (uint32_t *)malloc(out.size() * 4);
    CHECK(fr_worker_gather_pooled_csr(wk, B, off, nnz ? ind : nullptr, nnz, weighted ? wt : nullptr, nullptr, reinterpret_cast<float *>(rec)) == FR_OK);
    const int rc = fr_worker_sync(wk);
    memcpy(out.data(), rec, out.size() * 4);
    free(off), free(ind), free(wt), free(rec);
    return rc;
}

static void run(int index_mode) {
    const int dims[4] = {4, 16, 32, 8}, banks[4] = {0, 0, 0, 1};
    const int64_t rows[4] = {300, 333, 420, 515};
    fr_table_desc tabs[4];
    fr_segment segs[5];
    int pos = 0;
    for (int t = 0; t < 4; t++) {
        tabs[t] = fr_table_desc{};
        tabs[t].table_id = t, tabs[t].dim = dims[t], tabs[t].rows = rows[t], tabs[t].bank = banks[t];
        segs[t] = fr_segment{};
        segs[t].kind = FR_SEG_TABLE, segs[t].src = t, segs[t].rec_offset = pos, segs[t].len = dims[t];
        pos += dims[t];
    }
    segs[4] = fr_segment{};
    segs[4].kind = FR_SEG_COPY, segs[4].src = 0, segs[4].rec_offset = pos, segs[4].len = 4;
    pos += 4;
    fr_model_desc d{};
    snprintf(d.name, sizeof(d.name), "csr_san");
    d.n_tables = 4, d.n_segments = 5, d.tables = tabs, d.segments = segs, d.record_len = pos, d.dense_len = 0;
    d.fc[0] = pos, d.fc[1] = 64, d.fc[2] = 32, d.fc[3] = 32, d.fc[4] = 1;
    fr_model_desc *m = nullptr;
    CHECK(fr_model_clone_scaled(&d, 1.0, 1, 0, &m) == FR_OK);
    m->index_mode = index_mode;
    fr_ctx *ctx = nullptr;
    CHECK(fr_ctx_create(m, -1, &ctx) == FR_OK);
    for (int t = 0; t < 4; t++) {
        std::vector<float> tab((size_t)rows[t] * dims[t]);
        for (auto &v : tab) v = (float)((int)(rng() % 2001) - 1000) / 64.0f;
        CHECK(fr_ctx_upload_table(ctx, t, 0, rows[t], tab.data()) == FR_OK);
    }
    CHECK(fr_ctx_fill_weights(ctx, FR_WEIGHTS_UNIFORM, 5) == FR_OK);
    const int C = fr_model_index_cols(m);
    const int64_t range = index_mode == FR_INDEX_PER_BANK ? 300 : 0;   // a bank's rows: its shortest table's; per table: the table's own
    const int32_t caps_of[4] = {9, 1, 4, 5};
    std::vector<int32_t> caps(caps_of, caps_of + C), modes((size_t)C);
    int P = 0;
    for (int c = 0; c < C; c++) P += caps[c], modes[c] = c % 2 ? FR_POOL_MEAN : FR_POOL_SUM;
    CHECK(fr_ctx_set_pooling(ctx, caps.data(), C) == FR_OK);
    const int B = 13;
    fr_worker *wk = nullptr;
    CHECK(fr_worker_create(ctx, B, &wk) == FR_OK);
    auto rows_of = [&](int c) { return (uint32_t)(range ? (c == 0 ? range : rows[3]) : rows[c]); };

    // well-formed bags: lengths 0 .. cap (item 3: every bag empty, item 4: every bag full), a sixth of the entries -1
    std::vector<int32_t> rect((size_t)B * P, -1);
    std::vector<float> wrect((size_t)B * P, 0.0f);
    Bags good;
    good.off.push_back(0);
    for (int b = 0; b < B; b++) {
        int p0 = 0;
        for (int c = 0; c < C; p0 += caps[c], c++) {
            const int len = b == 3 ? 0 : b == 4 ? caps[c] : (int)(rng() % (uint32_t)(caps[c] + 1));
            for (int j = 0; j < len; j++) {
                const int32_t r = rng() % 6 == 0 ? -1 : (int32_t)(rng() % rows_of(c));
                const float w = 0.5f + (float)(rng() % 1024) / 1024.0f;
                good.ind.push_back(r), good.wt.push_back(w);
                rect[(size_t)b * P + p0 + j] = r, wrect[(size_t)b * P + p0 + j] = w;
            }
            good.off.push_back((int32_t)good.ind.size());
        }
    }
    const int64_t nnz = (int64_t)good.ind.size();
    const size_t n_rec = (size_t)B * pos;
    std::vector<uint32_t> want[3], got(n_rec);
    int32_t *p_rect = exact(rect);
    float *p_w = exact(wrect);
    for (int kind = 0; kind < 3; kind++) {   // 0 SUM, 1 MEAN (alternating columns), 2 weighted
        CHECK(fr_ctx_set_pooling_modes(ctx, kind == 1 ? modes.data() : nullptr, kind == 1 ? C : 0) == FR_OK);
        want[kind].resize(n_rec);
        uint32_t *rec = (uint32_t *)malloc(n_rec * 4);
        if (kind == 2) CHECK(fr_worker_gather_pooled_weighted(wk, B, p_rect, p_w, nullptr, reinterpret_cast<float *>(rec)) == FR_OK);
        else CHECK(fr_worker_gather_pooled(wk, B, p_rect, nullptr, reinterpret_cast<float *>(rec)) == FR_OK);
        CHECK(fr_worker_sync(wk) == FR_OK);
        memcpy(want[kind].data(), rec, n_rec * 4);
        free(rec);
        CHECK(run_csr(wk, B, good, nnz, kind == 2, got) == FR_OK);
        CHECK(got == want[kind]);
        // the host form: offsets, flat entries and flat weights in the worker's own buffers; scores against the padded host form
        std::vector<float> sc_padded((size_t)B), sc_csr((size_t)B);
        memcpy(fr_worker_idx_ptr(wk), rect.data(), rect.size() * 4);
        memcpy(fr_worker_pool_weights_ptr(wk), wrect.data(), wrect.size() * 4);
        CHECK((kind == 2 ? fr_worker_submit_pooled_weighted(wk, B) : fr_worker_submit_pooled(wk, B)) == FR_OK);
        CHECK(fr_worker_sync(wk) == FR_OK);
        memcpy(sc_padded.data(), fr_worker_score_ptr(wk), (size_t)B * 4);
        CHECK(fr_worker_pool_offsets_ptr(wk) != nullptr);
        memcpy(fr_worker_pool_offsets_ptr(wk), good.off.data(), good.off.size() * 4);
        memcpy(fr_worker_idx_ptr(wk), good.ind.data(), good.ind.size() * 4);
        memcpy(fr_worker_pool_weights_ptr(wk), good.wt.data(), good.wt.size() * 4);
        CHECK(fr_worker_submit_pooled_csr(wk, B, kind == 2) == FR_OK);
        CHECK(fr_worker_sync(wk) == FR_OK);
        memcpy(sc_csr.data(), fr_worker_score_ptr(wk), (size_t)B * 4);
        CHECK(memcmp(sc_padded.data(), sc_csr.data(), (size_t)B * 4) == 0);
        fr_worker_pool_offsets_ptr(wk)[0] = 1;
        CHECK(fr_worker_submit_pooled_csr(wk, B, 0) == FR_ERR_INVALID);
        fr_worker_pool_offsets_ptr(wk)[0] = 0;
        fr_worker_pool_offsets_ptr(wk)[(size_t)B * C] = B * P + 1;
        CHECK(fr_worker_submit_pooled_csr(wk, B, 0) == FR_ERR_INVALID);

        // malformed bags, one class at a time, in the first and in the last item
        for (int place = 0; place < 2; place++) {
            const int item = place ? B - 1 : 0;
            for (int what = 0; what < 6; what++) {
                Bags g = good;
                int64_t n = nnz;
                const int k = item * C + (place ? C - 1 : 0), c = k % C;
                switch (what) {
                    case 0: {   // longer than the cap
                        const int fill = caps[c] + 1 - (g.off[k + 1] - g.off[k]);
                        g.ind.insert(g.ind.begin() + g.off[k + 1], (size_t)fill, 0);
                        g.wt.insert(g.wt.begin() + g.off[k + 1], (size_t)fill, 1.0f);
                        for (size_t i = (size_t)k + 1; i < g.off.size(); i++) g.off[i] += fill;
                        n += fill;
                        break;
                    }
                    case 1: g.off[place ? (size_t)B * C : 1] = (int32_t)nnz + 3; break;    // end > nnz
                    case 2: g.off[k + (place ? 0 : 1)] = g.off[k + (place ? 1 : 2)] + 2; break;   // decreasing: an offset above the next one
                    case 3: g.off[place ? k : 0] = -1; break;                            // a negative start
                    default: {  // an entry equal to the row count / an entry of -2, in a bag that has an entry (bag (4, c) is full)
                        const int kk = 4 * C + c;
                        g.ind[(size_t)g.off[kk]] = what == 4 ? (int32_t)rows_of(c) : -2;
                        break;
                    }
                }
                CHECK(run_csr(wk, B, g, n, kind == 2, got) == FR_ERR_INDEX_RANGE);
                CHECK(run_csr(wk, B, good, nnz, kind == 2, got) == FR_OK);   // the flag does not stick
                CHECK(got == want[kind]);
            }
        }
    }
    // nnz == 0: NULL indices and weights, every bag empty
    CHECK(fr_ctx_set_pooling_modes(ctx, nullptr, 0) == FR_OK);
    Bags none;
    none.off.assign((size_t)B * C + 1, 0);
    CHECK(run_csr(wk, B, none, 0, false, got) == FR_OK);
    for (uint32_t v : got) CHECK(v == 0u);
    CHECK(run_csr(wk, B, none, 0, true, got) == FR_OK);
    // argument errors touch nothing
    CHECK(fr_worker_gather_pooled_csr(wk, B, nullptr, nullptr, 0, nullptr, nullptr, reinterpret_cast<float *>(got.data())) == FR_ERR_INVALID);
    CHECK(fr_worker_gather_pooled_csr(wk, B, none.off.data(), nullptr, 4, nullptr, nullptr, reinterpret_cast<float *>(got.data())) == FR_ERR_INVALID);
    CHECK(fr_worker_gather_pooled_csr(wk, B, none.off.data(), nullptr, -1, nullptr, nullptr, reinterpret_cast<float *>(got.data())) == FR_ERR_INVALID);
    free(p_rect), free(p_w);
    fr_worker_destroy(wk);
    fr_ctx_destroy(ctx);
    fr_model_free(m);
}

int main() {
    fr_cpu_set_threads(4);
    run(FR_INDEX_PER_BANK);
    run(FR_INDEX_PER_TABLE);
    printf("pooled_csr_san: ok\n");
    return 0;
}
