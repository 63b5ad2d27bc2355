// update_rows_san -- fr_ctx_update_rows / fr_worker_update_rows on the CPU back-end under AddressSanitizer + UBSan, as a program of its own
// (`make -C gpu-fpga-recommendation-system_amd/csrc san-update-rows` links it with the library's host sources built under
// -fsanitize=address,undefined and runs it).  The model is the one of tests/update_rows.py: one bank of three tables (dims 4 / 16 / 32, rows
// 300 / 333 / 420: bank rows + two tails) and a lone table of dim 8, per-bank and per-table.  Every table takes: one row, 257 rows, the edges
// of head and tail, a permutation of all rows, a list with -1 / rows / 2^31 - 1 among valid ids, a list that names a row twice -- through the
// host form and the worker form, each checked against a plain model of the table kept here.  The buffers are heap blocks of exactly the
// size the call may touch, so a read or write one element past either end is a report.  Exit status 0 and "update_rows_san: ok" = clean.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
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

static std::mt19937 rng(4800);

struct Case {
    std::vector<int32_t> ids;
    bool bad = false;
};

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
    segs[4] = fr_segment{};   // a 4-float COPY pad: records are whole groups of 8 floats
    segs[4].kind = FR_SEG_COPY, segs[4].src = 0, segs[4].rec_offset = pos, segs[4].len = 4;
    pos += 4;
    fr_model_desc d{};
    snprintf(d.name, sizeof(d.name), "ur_san");
    d.n_tables = 4, d.n_segments = 5, d.tables = tabs, d.segments = segs, d.record_len = pos, d.dense_len = 0;
    d.fc[0] = pos, d.fc[1] = 64, d.fc[2] = 32, d.fc[3] = 32, d.fc[4] = 1;
    fr_model_desc *m = nullptr;
    CHECK(fr_model_clone_scaled(&d, 1.0, 1, 0, &m) == FR_OK);
    m->index_mode = index_mode;
    fr_ctx *ctx = nullptr;
    CHECK(fr_ctx_create(m, -1, &ctx) == FR_OK);
    fr_worker *wk = nullptr;
    CHECK(fr_worker_create(ctx, 16, &wk) == FR_OK);
    std::vector<std::vector<uint32_t>> model(4);
    for (int t = 0; t < 4; t++) {
        model[t].resize((size_t)rows[t] * dims[t]);
        for (auto &v : model[t]) v = rng();
        CHECK(fr_ctx_upload_table(ctx, t, 0, rows[t], reinterpret_cast<const float *>(model[t].data())) == FR_OK);
    }
    for (int form = 0; form < 2; form++)
        for (int t = 0; t < 4; t++) {
            const int32_t R = (int32_t)rows[t];
            std::vector<int32_t> perm((size_t)R);
            std::iota(perm.begin(), perm.end(), 0);
            std::shuffle(perm.begin(), perm.end(), rng);
            std::vector<Case> cases(6);
            cases[0].ids = {(int32_t)(rng() % (uint32_t)R)};
            cases[1].ids.assign(perm.begin(), perm.begin() + 257);
            cases[2].ids = {0, R - 1};
            if (R > 300) cases[2].ids.insert(cases[2].ids.end(), {299, 300});
            cases[3].ids = perm;
            cases[4].ids = {3, -1, R - 1, R, 7, INT32_MAX, 298, 0};
            cases[4].bad = true;
            cases[5].ids = {17, 5, R - 1, 17, 9, R - 1};   // the CPU back-end writes a row listed twice from its LAST listing
            for (const Case &c : cases) {
                const int n = (int)c.ids.size();
                // exact-size heap blocks: the sanitizer sees the first byte past either
                int32_t *ids = (int32_t *)malloc((size_t)n * sizeof(int32_t));
                uint32_t *src = (uint32_t *)malloc((size_t)n * dims[t] * sizeof(uint32_t));
                memcpy(ids, c.ids.data(), (size_t)n * sizeof(int32_t));
                for (size_t i = 0; i < (size_t)n * dims[t]; i++) src[i] = rng();
                int rc;
                if (form == 0) {
                    rc = fr_ctx_update_rows(ctx, t, n, ids, reinterpret_cast<const float *>(src));
                } else {
                    CHECK(fr_worker_update_rows(wk, t, n, ids, reinterpret_cast<const float *>(src)) == FR_OK);
                    rc = fr_worker_sync(wk);
                }
                CHECK(rc == (c.bad ? FR_ERR_INDEX_RANGE : FR_OK));
                for (int i = 0; i < n; i++)
                    if (ids[i] >= 0 && ids[i] < R) memcpy(&model[t][(size_t)ids[i] * dims[t]], src + (size_t)i * dims[t], (size_t)dims[t] * 4);
                free(ids);
                free(src);
                for (int u = 0; u < 4; u++) {   // every table, whole: the updated one and its neighbours in the bank row
                    std::vector<uint32_t> got((size_t)rows[u] * dims[u]);
                    CHECK(fr_ctx_download_table(ctx, u, 0, rows[u], reinterpret_cast<float *>(got.data())) == FR_OK);
                    CHECK(got == model[u]);
                }
            }
            CHECK(fr_ctx_update_rows(ctx, t, 0, nullptr, nullptr) == FR_OK);
            CHECK(fr_worker_update_rows(wk, t, -1, nullptr, nullptr) == FR_ERR_INVALID);
        }
    CHECK(fr_ctx_update_rows(ctx, 4, 1, nullptr, nullptr) == FR_ERR_INVALID);
    fr_worker_destroy(wk);
    fr_ctx_destroy(ctx);
    fr_model_free(m);
}

int main() {
    fr_cpu_set_threads(4);
    run(FR_INDEX_PER_BANK);
    run(FR_INDEX_PER_TABLE);
    printf("update_rows_san: ok\n");
    return 0;
}
