// The CPU back-end behind the same symbols: fr_ctx_create(model, device = -1, ...) ("device /* -1 = CPU backend */";
// BASELINE configs[0]: Model-A batch 1 on the host CPU, no accelerator -- the reference's `make check TARGET=sw_emu` plumbing run,
// FPGA/Makefile:154-158).  Plain C++17 and std::thread; no HIP call, no GPU needed.  It is the product's own code: it walks the SAME
// FrWordDesc list the gfx950 gather kernels walk (fr_api.cpp build_words) and runs the FC chain as a k-ordered fp32 multiply-add chain
// (CUBLAS_COMPUTE_32F, cuda_server.c:211) over the fp32 master weights in the reference's column-major H x K layout (cuda_server.c:215).
// Scope (fleetrec.h): context set-up, fr_worker_submit / submit_device / push_device / sync, gather_only, fc_only, the fp32 forms of the
// table-sharded entry points, the request-driver core.  fp32 only; everything else returns FR_ERR_STATE on a CPU context.
#include <pthread.h>
#include <sys/mman.h>
#include <sched.h>
#include <unistd.h>

#include <cstdio>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "fr_content.h"
#include "fr_internal.h"

// ---- a small persistent thread pool (one parallel region at a time; the caller takes part) -------------------------------------------
namespace {
class Pool {
  public:
    static Pool &get() {
        // Never destroyed: helper threads may outlive static destructors.  A fork()ed child (Python's multiprocessing) inherits the object but
        // none of its threads -- and possibly its mutexes in a locked state: the child's atfork handler drops the pointer, the child's first
        // call builds a pool of its own (the parent's object is leaked there).
        Pool *p = inst_.load(std::memory_order_acquire);
        if (p) return *p;
        Pool *n = new Pool(first_size_.load(std::memory_order_relaxed));
        if (inst_.compare_exchange_strong(p, n, std::memory_order_acq_rel)) return *n;
        n->stop_helpers();   // another thread was first
        delete n;
        return *p;
    }
    // fr_cpu_set_threads(n) BEFORE the first parallel region: the pool is built with n threads straight away (it used to
    // start one helper per usable core first and shrink afterwards)
    static bool exists() { return inst_.load(std::memory_order_acquire) != nullptr; }
    static void set_first_size(int n) { first_size_.store(n, std::memory_order_relaxed); }
    int size() {
        std::lock_guard<std::mutex> g(run_m_);
        return n_;
    }
    int resize(int n) {
        std::lock_guard<std::mutex> g(run_m_);
        if (n <= 0) n = usable_cpus();
        if (n > 1024) n = 1024;
        if (n == n_) return n_;
        stop_helpers();
        n_ = n;
        start_helpers();
        return n_;
    }
    // fn(u) for every u in [0, units); returns when all of them have run
    void run(int units, const std::function<void(int)> &fn) {
        if (units <= 0) return;
        std::lock_guard<std::mutex> region(run_m_);
        if (n_ <= 1 || units == 1) {
            for (int u = 0; u < units; u++) fn(u);
            return;
        }
        {
            std::lock_guard<std::mutex> lk(m_);
            job_ = &fn;
            units_ = units;
            next_.store(0, std::memory_order_relaxed);
            pending_.store((int)helpers_.size(), std::memory_order_relaxed);
            generation_.fetch_add(1, std::memory_order_release);
        }
        cv_work_.notify_all();
        work();
        for (int spin = 0; spin < kSpin && pending_.load(std::memory_order_acquire) != 0; spin++) cpu_relax();
        if (pending_.load(std::memory_order_acquire) != 0) {
            std::unique_lock<std::mutex> lk(m_);
            cv_done_.wait(lk, [&] { return pending_.load(std::memory_order_acquire) == 0; });
        }
        job_ = nullptr;
    }

  private:
    explicit Pool(int n) : n_(n > 0 ? (n > 1024 ? 1024 : n) : usable_cpus()) {
        static const int once = pthread_atfork(nullptr, nullptr, [] { inst_.store(nullptr, std::memory_order_release); });
        (void)once;
        start_helpers();
    }
    static std::atomic<Pool *> inst_;
    static std::atomic<int> first_size_;
    static int usable_cpus() {
        int n = (int)std::thread::hardware_concurrency();
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof(set), &set) == 0) {
            const int a = CPU_COUNT(&set);
            if (a > 0 && (n <= 0 || a < n)) n = a;
        }
        return n > 0 ? n : 1;
    }
    void work() {
        for (;;) {
            const int u = next_.fetch_add(1, std::memory_order_relaxed);
            if (u >= units_) return;
            (*job_)(u);
        }
    }
    void start_helpers() {
        stop_.store(false, std::memory_order_relaxed);
        for (int i = 1; i < n_; i++)
            helpers_.emplace_back([this] {
                uint64_t seen = 0;
                for (;;) {
                    // a request is several parallel regions a few hundred microseconds apart (gather, four layers): a helper that went to sleep
                    // between them costs a futex wake-up per region (measured here: 11 ms instead of 2.4 ms for a batch of 256) -- spin briefly first
                    for (int spin = 0; spin < kSpin && generation_.load(std::memory_order_acquire) == seen && !stop_.load(std::memory_order_relaxed); spin++) cpu_relax();
                    if (generation_.load(std::memory_order_acquire) == seen) {
                        std::unique_lock<std::mutex> lk(m_);
                        cv_work_.wait(lk, [&] { return stop_.load(std::memory_order_relaxed) || generation_.load(std::memory_order_acquire) != seen; });
                    }
                    if (stop_.load(std::memory_order_relaxed)) return;
                    seen = generation_.load(std::memory_order_acquire);
                    work();
                    if (pending_.fetch_sub(1, std::memory_order_acq_rel) == 1) {
                        std::lock_guard<std::mutex> lk(m_);
                        cv_done_.notify_one();
                    }
                }
            });
    }
    void stop_helpers() {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_.store(true, std::memory_order_relaxed);
        }
        cv_work_.notify_all();
        for (auto &t : helpers_) t.join();
        helpers_.clear();
    }
    std::mutex run_m_, m_;
    std::condition_variable cv_work_, cv_done_;
    std::vector<std::thread> helpers_;
    const std::function<void(int)> *job_ = nullptr;
    static constexpr int kSpin = 40000;   // ~100-200 us of pause instructions before a thread blocks
#if defined(__x86_64__)
    static void cpu_relax() { __builtin_ia32_pause(); }
#else
    static void cpu_relax() { std::atomic_signal_fence(std::memory_order_seq_cst); }   // portable: a compiler barrier, no pause hint
#endif
    std::atomic<int> next_{0}, pending_{0};
    int units_ = 0, n_ = 1;
    std::atomic<uint64_t> generation_{0};
    std::atomic<bool> stop_{false};
};
std::atomic<Pool *> Pool::inst_{nullptr};
std::atomic<int> Pool::first_size_{0};
}  // namespace

int frc_set_threads(int n) {
    if (!Pool::exists()) Pool::set_first_size(n);
    return Pool::get().resize(n);
}
int frc_threads() { return Pool::get().size(); }

// ---- memory ------------------------------------------------------------------------------------------------------------------------
// Table arena: anonymous zero pages, committed when first written (a table that is never filled costs nothing).  Refused up front when
// it could not fit the host's physical memory: the kernel would otherwise kill the process half-way through the fill.
void *frc_arena_alloc(size_t bytes) {
    if (bytes == 0) bytes = 4096;
    const long pages = sysconf(_SC_PHYS_PAGES), psz = sysconf(_SC_PAGESIZE);
    double limit = pages > 0 && psz > 0 ? (double)pages * (double)psz : 0.0;
    for (const char *path : {"/sys/fs/cgroup/memory.max", "/sys/fs/cgroup/memory/memory.limit_in_bytes"}) {   // a container's own limit, where one is set
        if (FILE *f = fopen(path, "r")) {
            double v = 0.0;
            if (fscanf(f, "%lf", &v) == 1 && v > 0.0 && (limit == 0.0 || v < limit)) limit = v;
            fclose(f);
        }
    }
    if (limit > 0.0 && (double)bytes > 0.85 * limit) {
        fr_set_error("CPU back-end: %.1f GB of tables do not fit this host's %.1f GB of memory", bytes / 1e9, limit / 1e9);
        return nullptr;
    }
    void *p = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (p == MAP_FAILED) {
        fr_set_error("CPU back-end: mmap of %zu bytes failed", bytes);
        return nullptr;
    }
    return p;
}
void frc_arena_free(void *p, size_t bytes) {
    if (p) munmap(p, bytes ? bytes : 4096);
}

// ---- procedural contents (fr_content.h: the same functions the gfx950 fill kernels run) -------------------------------------------------
int frc_fill_table(float *base, int64_t row0, int64_t rows, int dim, int64_t row_stride_bytes, int mode, uint32_t seed, uint32_t uid) {
    const uint32_t h0 = fr_table_hash_seed(seed, uid);
    const int64_t chunk = 4096;
    const int units = (int)((rows + chunk - 1) / chunk);
    char *b = reinterpret_cast<char *>(base);
    Pool::get().run(units, [&](int u) {
        const int64_t r0 = (int64_t)u * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
        for (int64_t lr = r0; lr < r1; lr++) {
            uint32_t *dst = reinterpret_cast<uint32_t *>(b + (size_t)lr * (size_t)row_stride_bytes);
            for (int c = 0; c < dim; c++) dst[c] = fr_content_bits(mode, h0, uid, (uint64_t)(row0 + lr), (uint32_t)c);
        }
    });
    return FR_OK;
}

// Row updates: the work is dealt by DESTINATION (blocks of 64 table rows, round-robin over the units), every unit walks the whole id list in
// order -- two listings of one row are then written by one thread, the later one last, and no two threads ever write the same bytes.
int frc_update_rows(char *arena, const FrTableMem &tm, int dim, int64_t rows, int n, const int32_t *ids, const float *src) {
    const size_t row_bytes = (size_t)dim * 4;
    const int64_t head_rows = tm.il_rows ? (int64_t)tm.il_rows : rows;
    const int units = n < 4096 ? 1 : Pool::get().size();
    std::atomic<int> bad{0};
    Pool::get().run(units, [&](int u) {
        int any_bad = 0;
        for (int i = 0; i < n; i++) {
            const int64_t r = ids[i];
            if (r < 0 || r >= rows) {
                any_bad = 1;
                continue;
            }
            if ((int)((r >> 6) % units) != u) continue;
            char *a = r < head_rows ? arena + tm.byte_offset + (size_t)r * tm.row_stride : arena + tm.tail_offset + (size_t)(r - head_rows) * row_bytes;
            memcpy(a, src + (size_t)i * dim, row_bytes);
        }
        if (any_bad) bad.store(1, std::memory_order_relaxed);
    });
    return bad.load(std::memory_order_relaxed);
}

// Segmented top-K ranking: the composites of fr_rank.hip -- (key << 32) | (0xffffffff - position), all distinct inside a segment -- and a partial
// sort of them per segment; contiguous runs of segments are dealt to the pool's threads.  The score is copied through the winning position (a NaN's
// payload is not in its key).
int frc_rank_topk(const float *scores, int n, int n_seg, const int32_t *off, int k, int32_t *top_idx, float *top_scores) {
    const int units = (n < 8192 || n_seg < 2) ? 1 : (Pool::get().size() < n_seg ? Pool::get().size() : n_seg);
    std::atomic<int> bad{0};
    Pool::get().run(units, [&](int u) {
        std::vector<uint64_t> comp;
        const int s0 = (int)((int64_t)n_seg * u / units), s1 = (int)((int64_t)n_seg * (u + 1) / units);
        for (int s = s0; s < s1; s++) {
            int64_t a = off ? off[s] : 0, b = off ? off[s + 1] : n;
            if (a < 0 || b < a || b > n) {
                bad.store(1, std::memory_order_relaxed);
                a = b = 0;
            }
            const size_t len = (size_t)(b - a), top = len < (size_t)k ? len : (size_t)k;
            comp.resize(len);
            for (size_t i = 0; i < len; i++) {
                uint32_t bits;
                memcpy(&bits, scores + a + i, 4);
                comp[i] = ((uint64_t)fr_rank_key(bits) << 32) | (uint64_t)(0xffffffffu - (uint32_t)i);
            }
            std::partial_sort(comp.begin(), comp.begin() + (ptrdiff_t)top, comp.end(), std::greater<uint64_t>());
            int32_t *oi = top_idx + (size_t)s * (size_t)k;
            float *os = top_scores ? top_scores + (size_t)s * (size_t)k : nullptr;
            const uint32_t ninf = 0xff800000u;
            for (size_t j = 0; j < (size_t)k; j++) {
                const uint32_t pos = j < top ? 0xffffffffu - (uint32_t)comp[j] : 0u;
                oi[j] = j < top ? (int32_t)pos : -1;
                if (os) memcpy(os + j, j < top ? (const void *)(scores + a + pos) : (const void *)&ninf, 4);
            }
        }
    });
    return bad.load(std::memory_order_relaxed);
}

int frc_fill_weights(float *w, size_t count, int mode, uint32_t seed, uint32_t layer, float scale) {
    const uint32_t h0 = fr_weight_hash_seed(seed, layer);
    const size_t chunk = 1 << 16;
    Pool::get().run((int)((count + chunk - 1) / chunk), [&](int u) {
        const size_t i0 = (size_t)u * chunk, i1 = i0 + chunk < count ? i0 + chunk : count;
        for (size_t i = i0; i < i1; i++) w[i] = fr_weight_value(mode, h0, (uint64_t)i, scale);
    });
    return FR_OK;
}

// ---- the gather: load_single_embedding_* + the packers (embedding_47_krnl.cpp:916-1217), as the word descriptors state them -------------
// Record word w of item b = the 16 bytes at words[w].src + idx[b][words[w].idx_col] * words[w].stride, stored at word
// dst_blk * batch + b * dst_stride + dst_off of `out` -- exactly what gather_pack_kernel (fr_gather.hip) does per thread.  An index
// outside its table reads row 0 and raises *err_flag (reference: silent out-of-bounds read, embedding_47_krnl.cpp:927-933).
int frc_gather(const FrWordDesc *words, int n_words, const int32_t *idx, int idx_stride, const float *dense, float *out, int batch, int *err_flag) {
    const int chunk = 32;
    std::atomic<int> bad{0};
    char *o = reinterpret_cast<char *>(out);
    Pool::get().run((batch + chunk - 1) / chunk, [&](int u) {
        const int b0 = u * chunk, b1 = b0 + chunk < batch ? b0 + chunk : batch;
        int local_bad = 0;
        for (int b = b0; b < b1; b++) {
            const int32_t *row = idx + (size_t)b * idx_stride;
            for (int w = 0; w < n_words; w++) {
                const FrWordDesc &d = words[w];
                const char *src;
                if (d.idx_col & FR_DESC_DENSE) {
                    src = reinterpret_cast<const char *>(dense) + d.src + (size_t)b * d.stride;
                } else {
                    uint32_t r = (uint32_t)row[d.idx_col];
                    if (r >= d.rows) {
                        local_bad = 1;
                        r = 0;
                    }
                    src = reinterpret_cast<const char *>(d.src) + (uint64_t)r * d.stride;
                }
                memcpy(o + ((size_t)d.dst_blk * (size_t)batch + (size_t)b * d.dst_stride + d.dst_off) * 16, src, 16);
            }
        }
        if (local_bad) bad.store(1, std::memory_order_relaxed);
    });
    if (bad.load() && err_flag) __atomic_store_n(err_flag, 1, __ATOMIC_RELEASE);
    return FR_OK;
}

// The pooled (multi-hot) gather, exactly as gather_pooled_kernel (fr_gather.hip) folds a bag: slot -1 is empty, the first non-empty slot's
// row word is taken as a bit copy, every further one is added to it in fp32, one add per lane, in ascending slot order; an all-empty
// bag gives +0.0f.  A MEAN word (FR_POOL_DESC_MEAN in its descriptor) is that fold divided once by the count of non-empty slots when the
// count is 2 or more.  With weights (float [batch][pool_cols], parallel to idx) every non-empty slot's word is first multiplied by the slot's
// weight -- a product rounded to fp32 on its own; the product build compiles this file for baseline x86-64, which has no FMA to contract into,
// and fp-contract=off below only keeps that true should the file ever be built with -mfma / -march -- and the first product starts the accumulator; an empty slot's weight is never read.  Plain IEEE operations on both sides (no
// fast-math in either build): the records are bit-identical to the GPU's (a NaN's payload excepted).
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
int frc_gather_pooled(const FrPooledPlan &p, const FrPooledBatch &pb, const FrPooledOut &po) {
    // pb.offsets != NULL: the offsets form -- bag (b, c) = idx[offsets[b * n_icols + c] .. offsets[b * n_icols + c + 1]), c = pool[w].first, cap = pool[w].hots;
    // a malformed bag (fleetrec_serving.h) raises the flag and is folded as an empty one: nothing outside the three arrays is read
    const int chunk = 32;
    std::atomic<int> bad{0};
    char *o = static_cast<char *>(po.ptr);
    Pool::get().run((pb.batch + chunk - 1) / chunk, [&](int u) {
        const int b0 = u * chunk, b1 = b0 + chunk < pb.batch ? b0 + chunk : pb.batch;
        int local_bad = 0;
        for (int b = b0; b < b1; b++) {
            const int32_t *row = pb.offsets ? nullptr : pb.idx + (size_t)b * p.pool_cols;
            const float *wrow = pb.weights && !pb.offsets ? pb.weights + (size_t)b * p.pool_cols : nullptr;
            for (int w = 0; w < p.n_words; w++) {
                const FrWordDesc &d = p.words[w];
                char *dst = o + ((size_t)d.dst_blk * (size_t)pb.batch + (size_t)b * d.dst_stride + d.dst_off) * 16;
                if (d.idx_col & FR_DESC_DENSE) {
                    memcpy(dst, reinterpret_cast<const char *>(pb.dense) + d.src + (size_t)b * d.stride, 16);
                    continue;
                }
                uint32_t hots = p.pool[w].hots & ~FR_POOL_DESC_MEAN;
                const int32_t *bag = row ? row + p.pool[w].first : nullptr;
                const float *wbag = wrow ? wrow + p.pool[w].first : nullptr;
                if (pb.offsets) {
                    const int64_t s0 = pb.offsets[(size_t)b * p.n_icols + p.pool[w].first], s1 = pb.offsets[(size_t)b * p.n_icols + p.pool[w].first + 1];
                    if (s0 < 0 || s1 < s0 || s1 > pb.nnz || s1 - s0 > (int64_t)hots) {
                        local_bad = 1;
                        hots = 0;
                    } else {
                        hots = (uint32_t)(s1 - s0);
                        bag = hots ? pb.idx + s0 : nullptr;
                        wbag = pb.weights && hots ? pb.weights + s0 : nullptr;
                    }
                }
                uint32_t acc[4] = {0u, 0u, 0u, 0u};
                uint32_t cnt = 0;
                for (uint32_t j = 0; j < hots; j++) {
                    uint32_t r = (uint32_t)bag[j];
                    if (r == 0xFFFFFFFFu) continue;   // an empty slot
                    if (r >= d.rows) {
                        local_bad = 1;
                        r = 0;
                    }
                    uint32_t x[4];
                    memcpy(x, reinterpret_cast<const char *>(d.src) + (uint64_t)r * d.stride, 16);
                    if (wbag) {
                        const float wj = wbag[j];
                        for (int k = 0; k < 4; k++) {
                            float v;
                            memcpy(&v, &x[k], 4);
                            v = wj * v;
                            memcpy(&x[k], &v, 4);
                        }
                    }
                    for (int k = 0; k < 4; k++) {
                        if (cnt) {
                            float a, v;
                            memcpy(&a, &acc[k], 4);
                            memcpy(&v, &x[k], 4);
                            a = a + v;
                            memcpy(&acc[k], &a, 4);
                        } else {
                            acc[k] = x[k];
                        }
                    }
                    cnt++;
                }
                if ((p.pool[w].hots & FR_POOL_DESC_MEAN) && cnt > 1) {
                    const float n = (float)cnt;
                    for (int k = 0; k < 4; k++) {
                        float a;
                        memcpy(&a, &acc[k], 4);
                        a = a / n;
                        memcpy(&acc[k], &a, 4);
                    }
                }
                memcpy(dst, acc, 16);
            }
        }
        if (local_bad) bad.store(1, std::memory_order_relaxed);
    });
    if (bad.load() && p.err_flag) __atomic_store_n(p.err_flag, 1, __ATOMIC_RELEASE);
    return FR_OK;
}
#pragma GCC pop_options

// ---- the FC chain: 4 x cublasLtMatmul, alpha = 1, beta = 0 (cuda_server.c:211-217,468-491); bias and activation only where fr_ctx_set_epilogue set them ----
// Y[b][h] = sum over k, IN k ORDER, of W[h + k * H] * X[b][k], each step one fused multiply-add in fp32.  A tile of MB items x HT outputs
// keeps its sums in registers while k runs; W is read in its own (column-major: h contiguous) order.
namespace {
template <int MB, int HT>
static inline __attribute__((always_inline)) void fc_tile(const float *W, int H, int K, const float *const x[MB], float *const y[MB], int h0) {
    float acc[MB][HT];
    for (int b = 0; b < MB; b++)
        for (int j = 0; j < HT; j++) acc[b][j] = 0.0f;
    for (int k = 0; k < K; k++) {
        const float *wr = W + (size_t)k * H + h0;
        for (int b = 0; b < MB; b++) {
            const float xv = x[b][k];
            for (int j = 0; j < HT; j++) acc[b][j] = __builtin_fmaf(wr[j], xv, acc[b][j]);
        }
    }
    for (int b = 0; b < MB; b++)
        if (y[b])
            for (int j = 0; j < HT; j++) y[b][h0 + j] = acc[b][j];
}

// The layer's epilogue (fr_ctx_set_epilogue) on finished sums, in place: v = sum + b[h] (one fp32 add), then ReLU -- v > 0 ? v : +0, a NaN stays a NaN
// (it fails the compare).  {NULL, 0}: nothing is touched.  A pass of its own behind the layer: the k-ordered chains above stay what they were.
void fc_epilogue(float *Y, int ldy, int H, int batch, const FrEpi &e) {
    if (!e.bias && !e.relu) return;
    Pool::get().run((batch + 63) / 64, [&](int u) {
        for (int b = u * 64; b < batch && b < (u + 1) * 64; b++) {
            float *y = Y + (size_t)b * ldy;
            if (e.bias)
                for (int h = 0; h < H; h++) y[h] = y[h] + e.bias[h];
            if (e.relu)
                for (int h = 0; h < H; h++) y[h] = y[h] <= 0.0f ? 0.0f : y[h];
        }
    });
}

// one unit of a layer: items [b0, b0 + MB) x outputs [h0, h0 + HT) (ragged item blocks compute item b0 again and do not store it)
template <int MB, int HT>
static inline __attribute__((always_inline)) void fc_unit(const float *W, int H, int K, const float *X, int ldx, float *Y, int ldy, int batch, int b0, int h0) {
    const float *x[MB];
    float *y[MB];
    for (int b = 0; b < MB; b++) {
        const bool in = b0 + b < batch;
        x[b] = X + (size_t)(in ? b0 + b : b0) * ldx;
        y[b] = in ? Y + (size_t)(b0 + b) * ldy : nullptr;
    }
    fc_tile<MB, HT>(W, H, K, x, y, h0);
}

constexpr int FC_MB = 4, FC_HT = 32;   // H is a multiple of 32 (fr_model_validate)
// a unit = FC_MB items x FC_HT outputs; the last, ragged item block of a batch runs item by item (a request of one item must not pay for four)
template <int MB>
static inline __attribute__((always_inline)) void fc_unit_any(const float *W, int H, int K, const float *X, int ldx, float *Y, int ldy, int batch, int b0, int h0) {
    if (b0 + MB <= batch) {
        fc_unit<MB, FC_HT>(W, H, K, X, ldx, Y, ldy, batch, b0, h0);
        return;
    }
    for (int b = b0; b < batch; b++) fc_unit<1, FC_HT>(W, H, K, X, ldx, Y, ldy, batch, b, h0);
}
#if defined(__x86_64__)
// Per-function ISA clones, each naming EXACTLY the features pick_fc_unit() checks (target("arch=x86-64-v3") also licenses
// BMI / LZCNT / MOVBE / F16C, which a VM may mask while it shows AVX2 + FMA).
__attribute__((target("avx512f,avx512vl,avx512bw,avx512dq,avx2,fma"))) void fc_unit_v4(const float *W, int H, int K, const float *X, int ldx, float *Y, int ldy, int batch, int b0, int h0) {
    fc_unit_any<FC_MB>(W, H, K, X, ldx, Y, ldy, batch, b0, h0);
}
__attribute__((target("avx2,fma"))) void fc_unit_v3(const float *W, int H, int K, const float *X, int ldx, float *Y, int ldy, int batch, int b0, int h0) {
    fc_unit_any<FC_MB>(W, H, K, X, ldx, Y, ldy, batch, b0, h0);
}
#endif
void fc_unit_base(const float *W, int H, int K, const float *X, int ldx, float *Y, int ldy, int batch, int b0, int h0) {   // no FMA unit: fmaf() in software, still one rounding per step
    fc_unit_any<FC_MB>(W, H, K, X, ldx, Y, ldy, batch, b0, h0);
}
using FcUnitFn = void (*)(const float *, int, int, const float *, int, float *, int, int, int, int);
FcUnitFn pick_fc_unit() {
#if defined(__x86_64__)
    __builtin_cpu_init();
    const bool v3 = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma");
    if (v3 && __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512vl") && __builtin_cpu_supports("avx512bw") && __builtin_cpu_supports("avx512dq")) return fc_unit_v4;
    if (v3) return fc_unit_v3;
#endif
    return fc_unit_base;   // any other host: the compiler's baseline (fmaf() keeps one rounding per step everywhere)
}

void fc_layer_sums(const float *W, int H, int K, const float *X, int ldx, float *Y, int ldy, int batch) {
    static const FcUnitFn unit = pick_fc_unit();
    if (H % FC_HT) {   // the output layer (H = 1) and any narrow layer: one k-ordered chain per (item, output)
        Pool::get().run(batch, [&](int b) {
            const float *x = X + (size_t)b * ldx;
            for (int h = 0; h < H; h++) {
                float acc = 0.0f;
                for (int k = 0; k < K; k++) acc = __builtin_fmaf(W[h + (size_t)k * H], x[k], acc);
                Y[(size_t)b * ldy + h] = acc;
            }
        });
        return;
    }
    const int nb = (batch + FC_MB - 1) / FC_MB, nh = H / FC_HT;
    if ((double)batch * H * K < 4e6) {   // a request of a few items: a parallel region's hand-over would cost more than the work
        for (int u = 0; u < nb * nh; u++) unit(W, H, K, X, ldx, Y, ldy, batch, (u / nh) * FC_MB, (u % nh) * FC_HT);
        return;
    }
    // a work unit = ONE 32-output slice of W (K x 128 bytes: it stays in the core's L1 / L2) against a run of FC_IB item blocks: the weights are
    // streamed once per run instead of once per item block (batch 16384, Model-A FC1: 0.7 GB of X re-reads instead of 5.9 GB of W re-reads)
    constexpr int FC_IB = 16;
    const int nr = (nb + FC_IB - 1) / FC_IB;
    Pool::get().run(nr * nh, [&](int u) {
        const int h0 = (u % nh) * FC_HT, ib0 = (u / nh) * FC_IB, ib1 = ib0 + FC_IB < nb ? ib0 + FC_IB : nb;
        for (int ib = ib0; ib < ib1; ib++) unit(W, H, K, X, ldx, Y, ldy, batch, ib * FC_MB, h0);
    });
}

void fc_layer(const float *W, int H, int K, const float *X, int ldx, float *Y, int ldy, int batch, const FrEpi &e) {
    fc_layer_sums(W, H, K, X, ldx, Y, ldy, batch);
    fc_epilogue(Y, ldy, H, batch, e);
}
}  // namespace

// X: item-major records [batch][K] (for the BLOCKED layout: the 3-node buffer read "as if it were B x K item-major", 3-node
// cuda_server.c:216-217).  scratch: batch * (H1 + H2 + H3) floats.  w[l]: column-major H x K (fr_ctx_set_weights).
void frc_fc_chain(const int32_t fc[5], const float *const w[4], const FrEpi epi[4], const float *X, int batch, float *scratch, float *scores) {
    float *r1 = scratch, *r2 = r1 + (size_t)batch * fc[1], *r3 = r2 + (size_t)batch * fc[2];
    fc_layer(w[0], fc[1], fc[0], X, fc[0], r1, fc[1], batch, epi[0]);   // R1 = W1 * X        cuda_server.c:468-472
    fc_layer(w[1], fc[2], fc[1], r1, fc[1], r2, fc[2], batch, epi[1]);  // R2 = W2 * R1       :474-478
    fc_layer(w[2], fc[3], fc[2], r2, fc[2], r3, fc[3], batch, epi[2]);  // R3 = W3 * R2       :480-484
    fc_layer(w[3], fc[4], fc[3], r3, fc[3], scores, fc[4], batch, epi[3]);  // out = Wout * R3 :486-491
}

// Table-sharded mode after the exchange: gathered = [n_shards][batch_total][slice_padded] floats -> item-major records [n_items][K] of
// items [item0, item0 + n_items) (the 3-node server's three-part receive buffer generalised to G parts, 3-node cuda_server.c:513-591).
void frc_slices_to_records(const float *gathered, int n_shards, int batch_total, int slice_padded, const int *offs, const int *lens, int item0, int n_items, float *X, int K) {
    Pool::get().run(n_items, [&](int i) {
        for (int g = 0; g < n_shards; g++)
            memcpy(X + (size_t)i * K + offs[g], gathered + ((size_t)g * batch_total + item0 + i) * slice_padded, (size_t)lens[g] * sizeof(float));
    });
}

// ---- request-form batches: the CPU twin of request_expand_kernel (fr_request.hip) ------------------------------------------------------------
// The same words for every input: the owner of item i is the same clamped binary search over off[0 .. n_req), so no byte outside off[0 .. n_req],
// req[0 .. n_req * Rs), cand[0 .. batch * Rc) is read and none outside out[0 .. batch * W) written, whatever off holds.  -> 1: off was malformed.
int frc_expand_requests(const FrRequestArgs &a) {
    int bad = 0;
    if (a.off) {
        bad = a.off[0] != 0 || a.off[a.n_req] != a.batch;
        for (int j = 0; j < a.n_req && !bad; j++) bad = a.off[j] > a.off[j + 1];
    }
    auto owner = [&](int i) {
        int r = a.off ? 0 : i / (a.batch / a.n_req);
        if (a.off) {
            int lo = 0, hi = a.n_req;
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if (a.off[mid] <= i) lo = mid + 1;
                else hi = mid;
            }
            r = lo - 1;
        }
        return r < 0 ? 0 : (r >= a.n_req ? a.n_req - 1 : r);
    };
    Pool::get().run((a.batch + 255) / 256, [&](int u) {   // a unit = 256 items
        for (int i = u * 256; i < a.batch && i < (u + 1) * 256; i++) {
            const uint32_t *rq = a.req + (size_t)owner(i) * (size_t)a.Rs, *cd = a.Rc ? a.cand + (size_t)i * (size_t)a.Rc : nullptr;
            uint32_t *o = a.out + (size_t)i * (size_t)a.W;
            for (int w = 0; w < a.W; w++) {
                const int d = a.desc[w];
                o[w] = d >= 0 ? cd[d] : rq[~d];
            }
        }
    });
    return bad;
}

// ---- keyed lookups: the CPU twins of key_resolve_kernel, key_put_kernel and key_fill_kernel (fr_keys.hip) ---------------------------------------
// The rows are fr_keys.h's own functions of the key, the column record and the map, so they are the device's bit for bit.
void frc_resolve_keys(const FrKeyResolveArgs &a) {
    const uint64_t unit = 4096;   // words per unit of work
    std::atomic<unsigned long long> misses{0};
    Pool::get().run((int)((a.total + unit - 1) / unit), [&](int u) {
        const uint64_t e0 = (uint64_t)u * unit, e1 = e0 + unit < a.total ? e0 + unit : a.total;
        unsigned long long mine = 0;
        unsigned word = (unsigned)(e0 % (uint64_t)a.W);
        for (uint64_t e = e0; e < e1; e++) {
            bool miss = false;
            a.out[e] = fr_key_resolve(a.cols[a.wcol[word]], a.keys[e], &miss);
            mine += miss;
            if (++word == (unsigned)a.W) word = 0;
        }
        if (mine) misses.fetch_add(mine, std::memory_order_relaxed);
    });
    if (a.misses) __atomic_fetch_add(a.misses, misses.load(), __ATOMIC_RELAXED);
}

int frc_put_keys(const FrKeyPutArgs &a) {
    int bad = 0;
    for (int i = 0; i < a.n; i++) {
        const int64_t k = a.keys[i];
        if (k == FR_KEYS_EMPTY_KEY) {
            bad |= FR_KEYS_ERR_EMPTY_KEY;
            continue;
        }
        if (!fr_key_row_legal(a.col.range, a.col.miss_row, a.rows[i])) {
            bad |= FR_KEYS_ERR_ROW;
            continue;
        }
        uint64_t h = fr_key_home(a.col, k);
        bool found = false;
        for (uint64_t left = (uint64_t)a.col.mask + 1; left && !found; left--) {
            FrKeySlot *s = a.col.slots + h;
            const int64_t cur = __atomic_load_n(&s->key, __ATOMIC_RELAXED);
            if (cur == FR_KEYS_EMPTY_KEY) {
                if (*a.n_keys >= a.max_keys) break;   // the map is full: nothing is claimed
                ++*a.n_keys;
                __atomic_store_n(&s->key, k, __ATOMIC_RELEASE);   // the key first (the slot still holds miss_row) ...
                found = true;
            } else if (cur == k) {
                found = true;
            } else {
                h = (h + 1) & (uint64_t)a.col.mask;
            }
        }
        if (found) __atomic_store_n(&a.col.slots[h].row, a.rows[i], __ATOMIC_RELEASE);   // ... the row second
        else bad |= FR_KEYS_ERR_FULL;
    }
    return bad;
}

void frc_fill_keys(const FrKeyFillArgs &a) {
    for (uint64_t i = 0; i < a.n; i++) a.slots[i] = FrKeySlot{FR_KEYS_EMPTY_KEY, a.miss_row, 0};
}

// ---- the life cycle of a key map: the CPU twins of keymap_erase_kernel and keymap_walk_kernel (fr_keymaint.hip), on the same fr_keys.h functions ----
int frc_erase_keys(const FrKeyEraseArgs &a) {
    int bad = 0;
    for (int i = 0; i < a.n; i++) {
        const int64_t k = a.keys[i];
        if (k == FR_KEYS_EMPTY_KEY) {
            bad |= FR_KEYS_ERR_ERASE_EMPTY;
            continue;
        }
        const int64_t at = fr_key_find(a.col, k);
        if (at >= 0) __atomic_store_n(&a.col.slots[at].row, a.col.miss_row, __ATOMIC_RELEASE);
    }
    return bad;
}

void frc_walk_keys(const FrKeyWalkArgs &a) {
    const uint64_t n = (uint64_t)a.col.mask + 1;
    unsigned long long occupied = 0, live = 0, psum = 0;
    for (uint64_t i = 0; i < n; i++) {
        const FrKeySlot s = fr_key_load_slot(a.col.slots + i);
        if (!fr_key_slot_occupied(s)) continue;
        const bool l = fr_key_slot_live(s, a.col.miss_row);
        if (a.sink == FR_KEYWALK_COUNT) {
            occupied++, live += l, psum += fr_key_displacement(a.col, s.key, i);
        } else if (a.sink == FR_KEYWALK_EXPORT) {
            if (l && live < a.cap) a.out_keys[live] = s.key, a.out_rows[live] = s.row;
            live += l;
        } else if (l) {
            uint64_t h = fr_key_home(a.dst, s.key);
            for (uint64_t left = (uint64_t)a.dst.mask + 1; left; left--) {   // at most the new map's slots
                FrKeySlot *d = a.dst.slots + h;
                if (d->key == FR_KEYS_EMPTY_KEY) {
                    d->key = s.key, d->row = s.row;
                    live++;
                    break;
                }
                h = (h + 1) & (uint64_t)a.dst.mask;
            }
        }
    }
    if (a.sink == FR_KEYWALK_COUNT) a.counts[0] += occupied, a.counts[1] += live, a.counts[2] += psum;
    else a.counts[0] += live;
}

// ---- row pools: the CPU twins of keyadmit_admit_kernel + keyadmit_settle_kernel, keyadmit_release_kernel and keyadmit_mark_kernel (fr_keyadmit.hip) ----
// Sequential, ONE writer at a time (the callers hold fr_ctx::lp_mutex): a key listed twice finds itself live the second time, so there is nothing to
// elect and nothing to give back but the row of a key the full map refused.  The LOWEST free row is taken first.
static int32_t frc_pool_take(const FrKeyPool &p) {
    if (*p.free_rows <= 0) return -1;
    const uint32_t words = fr_key_pool_words(p.n_rows);
    for (uint32_t w = 0; w < words; w++) {
        if (p.bits[w] == ~0u) continue;
        const uint32_t b = (uint32_t)__builtin_ctz(~p.bits[w]);
        p.bits[w] |= 1u << b;
        --*p.free_rows;
        return p.first_row + (int32_t)(w * 32u + b);
    }
    return -1;   // (a counter that disagrees with its bitmap)
}

static void frc_pool_give(const FrKeyPool &p, int32_t row) {
    const uint32_t o = (uint32_t)(row - p.first_row), bit = 1u << (o & 31u);
    if (p.bits[o >> 5] & bit) p.bits[o >> 5] &= ~bit, ++*p.free_rows;
}

int frc_admit_keys(const FrKeyAdmitArgs &a) {
    int bad = 0;
    for (int i = 0; i < a.n; i++) {
        const int64_t k = a.keys[i];
        if (k == FR_KEYS_EMPTY_KEY) {
            bad |= FR_KEYS_ERR_EMPTY_KEY | FR_KEYS_ERR_ADMIT;
            a.rows_out[i] = -1;
            continue;
        }
        uint64_t h = fr_key_home(a.col, k);
        bool found = false, empty = false;
        for (uint64_t left = (uint64_t)a.col.mask + 1; left; left--) {
            const int64_t cur = __atomic_load_n(&a.col.slots[h].key, __ATOMIC_RELAXED);
            found = cur == k, empty = cur == FR_KEYS_EMPTY_KEY;
            if (found || empty) break;
            h = (h + 1) & (uint64_t)a.col.mask;
        }
        FrKeySlot *s = a.col.slots + h;
        if (found && s->row != a.col.miss_row) {   // live: nothing is written
            a.rows_out[i] = s->row;
            continue;
        }
        a.rows_out[i] = FR_KEYS_NO_ROW;
        const int32_t r = frc_pool_take(a.pool);
        if (r < 0) {
            bad |= FR_KEYS_ERR_NO_FREE_ROW | FR_KEYS_ERR_ADMIT;
            continue;
        }
        if (!found) {
            if (!empty || *a.n_keys >= a.max_keys) {   // the map is full: nothing is claimed, the row goes back
                frc_pool_give(a.pool, r);
                bad |= FR_KEYS_ERR_FULL | FR_KEYS_ERR_ADMIT;
                continue;
            }
            ++*a.n_keys;
            __atomic_store_n(&s->key, k, __ATOMIC_RELEASE);   // the key first (the slot still holds miss_row) ...
        }
        __atomic_store_n(&s->row, r, __ATOMIC_RELEASE);       // ... the row second
        a.rows_out[i] = r;
    }
    return bad;
}

int frc_release_keys(const FrKeyReleaseArgs &a) {
    int bad = 0;
    for (int i = 0; i < a.n; i++) {
        const int64_t k = a.keys[i];
        if (k == FR_KEYS_EMPTY_KEY) {
            bad |= FR_KEYS_ERR_ERASE_EMPTY;
            continue;
        }
        const int64_t at = fr_key_find(a.col, k);
        if (at < 0) continue;
        const int32_t was = __atomic_exchange_n(&a.col.slots[at].row, a.col.miss_row, __ATOMIC_ACQ_REL);
        if (was != a.col.miss_row && fr_key_pool_holds(a.pool, was)) frc_pool_give(a.pool, was);
    }
    return bad;
}

void frc_mark_pool(const FrKeyMarkArgs &a) {
    const uint64_t n = (uint64_t)a.col.mask + 1;
    for (uint64_t i = 0; i < n; i++) {
        const FrKeySlot s = fr_key_load_slot(a.col.slots + i);
        if (!fr_key_slot_live(s, a.col.miss_row) || !fr_key_pool_holds(a.pool, s.row)) continue;
        const uint32_t o = (uint32_t)(s.row - a.pool.first_row), bit = 1u << (o & 31u);
        if (!(a.pool.bits[o >> 5] & bit)) a.pool.bits[o >> 5] |= bit, --*a.pool.free_rows;
    }
}
