// rank_topk_san -- fr_worker_topk_device / fr_worker_topk on the CPU back-end under AddressSanitizer + UBSan, as a program of its own
// (`make -C gpu-fpga-recommendation-system_amd/csrc san-rank-topk` links it with the library's host sources built under
// -fsanitize=address,undefined and runs it).  The cases are the classes of tests/rank_topk.py: every value class (random bit patterns, all-equal,
// five values, +-0, +-inf and NaNs, denormals, ramps) x lengths around every tile size x the ks; segment lists with empty segments, offsets inside
// the array, 1000 short segments, the NULL-offsets form, indices only; one list of every malformed-offset class among clean segments; the host
// form behind a submit.  Every result is checked against a plain stable sort of the contract's keys kept here.  Scores, offsets and both
// outputs are heap blocks of exactly the size the call may touch, so a read or write one element past either end is a report.
// Exit status 0 and "rank_topk_san: ok" = clean.
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

static std::mt19937 rng(5000);

static uint32_t key_of(uint32_t u) { return (u & 0x7fffffffu) > 0x7f800000u ? 0u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u)); }

static std::vector<uint32_t> values(int cls, size_t n) {
    std::vector<uint32_t> v(n);
    const uint32_t five[5] = {0xc0200000u, 0u, 0x3f800000u, 0x3f800001u, 0x7f61b1e6u}, infs[5] = {0x7f800000u, 0xff800000u, 0x3f800000u, 0x7fc00000u, 0xffc00001u};
    for (size_t i = 0; i < n; i++) {
        float f;
        switch (cls) {
        case 0: v[i] = rng(); break;
        case 1: v[i] = 0x3f200000u; break;
        case 2: v[i] = five[rng() % 5]; break;
        case 3: v[i] = (rng() & 1) ? 0x80000000u : 0u; break;
        case 4: v[i] = infs[rng() % 5]; break;
        case 5: v[i] = (1u + rng() % 0x7fffffu) | ((rng() & 1) << 31); break;
        default:
            f = cls == 6 ? (float)i - (float)(n / 2) : (float)(n / 2) - (float)i;
            memcpy(&v[i], &f, 4);
        }
    }
    return v;
}

// One device-form call on exact-size heap blocks, checked against the stable sort; -> fr_worker_sync's status.
static int run(fr_worker *wk, const std::vector<uint32_t> &bits, const std::vector<int64_t> *off, int k, bool with_scores) {
    const int n = (int)bits.size(), n_seg = off ? (int)off->size() - 1 : 1;
    float *sc = (float *)malloc((size_t)n * 4);
    memcpy(sc, bits.data(), (size_t)n * 4);
    int32_t *o = off ? (int32_t *)malloc(off->size() * 4) : nullptr;
    for (size_t i = 0; off && i < off->size(); i++) o[i] = (int32_t)(*off)[i];
    int32_t *ti = (int32_t *)malloc((size_t)n_seg * k * 4);
    float *ts = with_scores ? (float *)malloc((size_t)n_seg * k * 4) : nullptr;
    CHECK(fr_worker_topk_device(wk, n, sc, n_seg, o, k, ti, ts) == FR_OK);
    const int rc = fr_worker_sync(wk);
    bool any_bad = false;
    for (int s = 0; s < n_seg; s++) {
        int64_t a = off ? (*off)[(size_t)s] : 0, b = off ? (*off)[(size_t)s + 1] : n;
        if (a < 0 || b < a || b > n) any_bad = true, a = b = 0;
        std::vector<int32_t> order((size_t)(b - a));
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return key_of(bits[(size_t)a + x]) > key_of(bits[(size_t)a + y]); });
        for (int j = 0; j < k; j++) {
            const bool real = (size_t)j < order.size();
            CHECK(ti[(size_t)s * k + j] == (real ? order[(size_t)j] : -1));
            if (ts) {
                uint32_t got;
                memcpy(&got, &ts[(size_t)s * k + j], 4);
                CHECK(got == (real ? bits[(size_t)a + order[(size_t)j]] : 0xff800000u));
            }
        }
    }
    CHECK(rc == (any_bad ? FR_ERR_INDEX_RANGE : FR_OK));
    free(sc), free(o), free(ti), free(ts);
    return rc;
}

int main() {
    fr_cpu_set_threads(4);
    fr_model_desc *m = nullptr;
    CHECK(fr_model_clone_scaled(fr_model_builtin(FR_MODEL_A), 1.0, 200, 200, &m) == FR_OK);
    fr_ctx *ctx = nullptr;
    CHECK(fr_ctx_create(m, -1, &ctx) == FR_OK);
    CHECK(fr_ctx_fill_tables(ctx, FR_FILL_HASH, 7) == FR_OK && fr_ctx_fill_weights(ctx, FR_WEIGHTS_UNIFORM, 11) == FR_OK);
    fr_worker *wk = nullptr;
    CHECK(fr_worker_create(ctx, 64, &wk) == FR_OK);
    // values x lengths x k, one segment in the NULL-offsets form
    const size_t lengths[] = {1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 16384, 16385, 70001};
    const int ks[] = {1, 2, 7, 64, 255, 256};
    for (int cls = 0; cls < 8; cls++)
        for (size_t n : lengths) {
            const std::vector<uint32_t> bits = values(cls, n);
            for (int k : ks)
                if (n < 5000 || k == 7 || k == 256) run(wk, bits, nullptr, k, true);
        }
    // segment lists
    {
        const std::vector<uint32_t> bits = values(0, 9000);
        std::vector<int64_t> empty_among = {0, 0, 4096, 4096, 4096, 4353, 9000, 9000}, inside = {37, 1000, 1000, 8001, 8990}, len0 = {5, 5};
        std::vector<int64_t> shorts(1001, 0);
        for (size_t s = 0; s < 1000; s++) shorts[s + 1] = shorts[s] + (int64_t)(s % 10);
        for (int k : {1, 7, 256}) {
            run(wk, bits, &empty_among, k, true);
            run(wk, bits, &inside, k, true);
            run(wk, bits, &shorts, k, true);
            run(wk, bits, &len0, k, true);
            run(wk, bits, &inside, k, false);   // indices only
        }
        std::vector<int64_t> most(8);   // n + 1 segments
        const std::vector<uint32_t> seven = values(2, 7);
        std::iota(most.begin() + 1, most.end(), 0);
        run(wk, seven, &most, 3, true);
    }
    // one list of every malformed class among clean segments; a clean call follows each
    {
        const std::vector<uint32_t> bits = values(0, 1000);
        const std::vector<std::vector<int64_t>> lists = {
            {0, 100, -5, 300, 700, 1000},                        // a start below 0 (and the end below the start before it)
            {0, 400, 200, 650, 1000},                            // an end below its start
            {0, 100, 1001, 1001, 600, 1000},                     // an end above n, a start above n
            {0, 500, INT32_MAX, INT32_MIN, 20, 1000},            // the int32 extremes
            {0, 100, -5, 200, 150, 400, 2000, 600, 1000}};       // every class
        std::vector<int64_t> clean = {0, 500, 1000};
        for (const auto &l : lists) {
            CHECK(run(wk, bits, &l, 9, true) == FR_ERR_INDEX_RANGE);
            CHECK(run(wk, bits, &clean, 9, true) == FR_OK);
        }
    }
    // the host form behind a submit: exact-size offsets and outputs
    {
        const int B = 64, K = 5;
        const int cols = fr_model_index_cols(m);
        int32_t *idx = fr_worker_idx_ptr(wk);
        for (int i = 0; i < B * cols; i++) idx[i] = (int32_t)(rng() % 200u);
        CHECK(fr_worker_submit(wk, B) == FR_OK && fr_worker_sync(wk) == FR_OK);
        std::vector<uint32_t> plain(B);
        memcpy(plain.data(), fr_worker_score_ptr(wk), (size_t)B * 4);
        int32_t *off = (int32_t *)malloc(4 * 4), *ti = (int32_t *)malloc(3 * K * 4);
        float *ts = (float *)malloc(3 * K * 4);
        off[0] = 0, off[1] = 20, off[2] = 20, off[3] = B;
        CHECK(fr_worker_topk(wk, B, 3, off, K, ti, ts) == FR_ERR_STATE);   // no batch in flight
        CHECK(fr_worker_submit(wk, B) == FR_OK);
        CHECK(fr_worker_topk(wk, B, 3, off, K, ti, ts) == FR_OK && fr_worker_sync(wk) == FR_OK);
        for (int s = 0; s < 3; s++) {
            std::vector<int32_t> order((size_t)(off[s + 1] - off[s]));
            std::iota(order.begin(), order.end(), 0);
            std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return key_of(plain[(size_t)off[s] + x]) > key_of(plain[(size_t)off[s] + y]); });
            for (int j = 0; j < K; j++) CHECK(ti[s * K + j] == ((size_t)j < order.size() ? order[(size_t)j] : -1));
        }
        free(off), free(ti), free(ts);
    }
    CHECK(fr_worker_topk_device(wk, 10, nullptr, 1, nullptr, 4, nullptr, nullptr) == FR_ERR_INVALID);
    fr_worker_destroy(wk);
    fr_ctx_destroy(ctx);
    fr_model_free(m);
    printf("rank_topk_san: ok\n");
    return 0;
}
