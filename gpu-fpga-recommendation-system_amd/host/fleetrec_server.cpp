// fleetrec_server -- the reference GPU server's request/batch shell on top of libfleetrec.so.
//
// Counterpart of GPU/final_network_cublasLt_1_node_no_FIFO_scatter/cuda_server.c (and the 3-node variant):
//   main()            : device/model set-up once, THREAD_NUM threads, join, latency statistics   (cuda_server.c:505-595)
//   thread_consume()  : listen/accept on PORT+i (:359-399), then the hot loop (:406-497):
//                       { lock; id = global_batch_count++; unlock } -> blocking read() of ONE fixed-size block into
//                       the pinned request buffer -> enqueue -> ... ; first five outputs printed at the end (:499-502)
// What changed on the wire: the lookup moved behind the boundary, so a block is B x T int32 indices
// (+ B x 64 dense floats for Model-C) instead of B x K gathered floats; framing is the reference's
// (no header, fixed-size little-endian blocks, constant.h:37-38).  Optionally the B scores are written back
// (--reply), which the reference never did (its "Finish receiving." message is defined but never sent, :363).
//
// Usage: fleetrec_server --model A|B|C [--batch 256] [--threads 4] [--port 8080] [--total 1024] [--device 0]
//        [--stream [--reply [--flush-us 50] [--flush-min 32]]]: streaming with score replies and adaptive batching -- see thread_consume
//                        [--tables evenodd|hash] [--weights ones|uniform] [--per-item | --per-bank] [--reply] [--row-cap N]
//                        [--shards G [--one-device] [--precision f32|bf16|fp8] [--exchange allgather|alltoall]]
//        [--hots N]: multi-hot pooled lookups (fr_ctx_set_pooling): a bag of N slots on every index column, a block is B x (index columns x N)
//                        int32 (slot -1 = empty), every batch goes through fr_worker_submit_pooled + fr_worker_sync.  Not with --stream or --shards.
//        [--pool sum|mean|weighted] (with --hots N; sum is the default): mean = every column FR_POOL_MEAN (fr_ctx_set_pooling_modes); weighted = the
//                        block's index rows are followed by float32 [B][index columns x N] per-sample weights, read into fr_worker_pool_weights_ptr,
//                        and every batch goes through fr_worker_submit_pooled_weighted (fleetrec_sender --hots N --pool weighted).
//        [--csr] (with --hots N, any --pool): the blocks come in the offsets form -- int32 offsets[B x index columns + 1], then int32 indices[nnz]
//                        with nnz taken from the last offset, then float32 weights[nnz] with --pool weighted, then the dense rows -- and every batch goes
//                        through fr_worker_submit_pooled_csr; N is the cap of every column.  A block whose offsets[0] is not 0 or whose nnz is outside
//                        [0, B x columns x N] ends the connection with an error status before anything more is read (fleetrec_sender --hots N --csr).
//        [--update-port P]: sparse row updates of the tables while serving (fr_ctx_update_rows).  A second listening socket, served by one thread of its
//                        own beside the serving threads.  One message = int32 table, int32 n, int32 ids[n], float32 rows[n x dim of that table],
//                        little-endian: row i of `rows` becomes table row ids[i]; the answer is one int32 status (0, or the library's FR_ERR_* --
//                        FR_ERR_INDEX_RANGE for an id outside the table, whose other rows were still written).  Messages are taken until the peer
//                        closes, then the next connection is accepted; a malformed header (table out of range, n < 0 or beyond 2^24 rows) closes
//                        the connection.  Legal with every serving mode (submit-and-sync, --stream, --hots, --device -1); with --shards the message
//                        is applied on every shard context the table is resident on.  Requests in flight meanwhile see old or new 16-byte row
//                        words; every request received after the status came back sees the new rows.
//        [--topk K [--segments S]]: the block is ranked on the device (fr_worker_topk, behind the block's own submit, before its sync) as S requests of
//                        batch / S candidates each (batch % S == 0; S defaults to 1; K = 1 .. 256).  With --reply the block's answer is S x K little-endian
//                        (int32 position inside the request, float32 score) pairs instead of B floats; a request shorter than K is padded with (-1, -inf).
//                        Legal on the submit-and-sync path, with --hots in every --pool form and --csr, and with --device -1.  Not with --stream
//                        (its blocks are host-fed: no host-form batch is in flight to rank) and not with --shards (the scores of a sharded step are
//                        gathered over the communicator, outside the worker's stream order) (fleetrec_sender --topk K --segments S).
//        [--requests S --shared-cols N [--shared-dense]]: request-form blocks (fr_ctx_set_request_columns / fr_worker_submit_requests).  The first N index
//                        columns are the request's, with --shared-dense the dense features too; a block is S equal requests of batch / S candidates
//                        (batch % S == 0).  On the wire: int32 [S][Rs] request rows, then float32 [S][dense_len] with --shared-dense, then int32 [B][Rc]
//                        candidate rows, then the per-item dense rows where they are not shared (Rs = N, Rc = index columns - N; with --hots H both x H,
//                        and the call is fr_worker_submit_requests(..., pooled = 1) in the sum or mean fold).  The rows are expanded on the device; the
//                        scores, and with --topk K the S x K pairs of the reply (--segments, if given, must equal S; omitted it is S), are those of the
//                        expanded block.  Not with --stream, --shards, --csr or --pool weighted; N = 1 .. index columns - 1 unless --shared-dense
//                        (fleetrec_sender takes the same three options).
//        [--relu] [--bias-seed S]: the per-layer epilogue of the FC chain (fr_ctx_set_epilogue), a context setting: legal with every mode above, set on
//                        every shard context with --shards.  --relu puts FR_ACT_RELU on the three hidden layers.  --bias-seed S gives every layer l = 0..3
//                        a bias made here on the host, scaled like --weights uniform: with fmix32 the 32-bit murmur3 finaliser
//                        (h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16),
//                          g = fmix32(fmix32(S ^ ((l + 1) * 0x9E3779B1)) ^ h),   b_l[h] = ((float)(g >> 8) / 8388608 - 1) / sqrtf(fc[l])
//                        for h = 0 .. fc[l + 1] - 1, all in float32 (fc[l] = the layer's input width).  fleetrec_sender is unchanged.
// --shards G: BASELINE configs[3]/[4] -- the tables are sharded by table-ID over GPUs device .. device + G - 1 of this node, or with
// --device -1 over G CPU shard contexts of this process exchanging through the library's in-process host exchange (one
// context and one worker per shard, fr_comm_init_all); every batch goes through fr_worker_submit_sharded on all shards (slices
// all-gathered over RCCL, FC on batch / G items per GPU, scores all-gathered).  The counterpart of the 3-node server, whose batch
// arrives in three parts from three senders (3-node cuda_server.c:513-591).  --exchange alltoall: every shard receives only the rows of
// its own batch / G items from each shard (fr_comm_set_exchange; 1/G of the all-gather's bytes, the same scores).
#include <arpa/inet.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <poll.h>
#include <sys/socket.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "fleetrec.h"
#include "fleetrec_serving.h"

struct Options {
    int model = FR_MODEL_A, batch = 256, threads = 4, port = 8080, device = 0;
    long total = 1024;
    int tables = FR_FILL_EVEN_ODD, weights = FR_WEIGHTS_ONES;
    bool relu = false, bias_seed_given = false;   // the FC chain's per-layer epilogue (fr_ctx_set_epilogue)
    uint32_t bias_seed = 0;
    bool per_item = false, per_bank = false, reply = false;
    int shards = 0;            // > 0: table-sharded over `shards` GPUs
    bool one_device = false;   // --shards G --one-device: all G shard contexts on GPU `device` (the library's staged host exchange: a G-rank job rehearsed on one GPU)
    int precision = FR_FC_FP32;
    int exchange = FR_EXCHANGE_ALLGATHER;   // --shards: how the slices travel (fr_comm_set_exchange)
    bool exchange_given = false;
    bool stream = false;   // throughput mode: fr_worker_push_host (blocks of batches per launch) instead of submit + sync per batch
    long flush_us = 50;    // --stream --reply: how long the socket must stay dry before a partial block is launched
    int flush_min = 32;    // ... while earlier blocks are still in flight: only once this many requests are queued (with nothing in flight: any number)
    int small_block = 8;   // --stream --reply: blocks of at most this many batches ride the stage pipeline, n + 4 launches (fr_ctx_set_small_block)
    bool latency = false;  // latency-measurement mode: per-batch recv -> enqueued -> scores times (measure_network_cuda_cp_latency_*/cuda_server.c)
    long row_cap = 0;
    int hots = 0;          // --hots N: pooled lookups, N slots per index column (0: one-hot)
    int pool = -1;         // --pool: 0 sum, 1 mean, 2 weighted (-1: not given)
    bool csr = false;      // --csr: blocks in the offsets form (with --hots)
    int update_port = 0;   // --update-port P: the row-update socket (0: none)
    int topk = 0;          // --topk K: every block is ranked on the device, K per request (0: plain scores)
    bool topk_given = false;
    int segments = 1;      // --segments S: requests per block (with --topk)
    bool segments_given = false;
    int requests = 0;      // --requests S: request-form blocks of S equal requests (0: full rows)
    int shared_cols = 0;   // --shared-cols N: the first N index columns are the request's
    bool shared_cols_given = false, shared_dense = false;   // --shared-dense: the dense features are the request's too
};

static bool read_exact(int fd, void *buf, size_t n) {  // the recv loop of cuda_server.c:425-450
    char *p = (char *)buf;
    while (n) {
        ssize_t r = read(fd, p, n);
        if (r <= 0) return false;
        p += r;
        n -= (size_t)r;
    }
    return true;
}

static bool write_exact(int fd, const void *buf, size_t n) {
    const char *p = (const char *)buf;
    while (n) {
        ssize_t r = send(fd, p, n, MSG_NOSIGNAL);
        if (r <= 0) return false;
        p += r;
        n -= (size_t)r;
    }
    return true;
}

static std::mutex g_mtx;            // pthread_mutex_t mtx            (cuda_server.c:25)
static long g_global_batch_count = 0;  // int global_batch_count      (cuda_server.c:23)
static std::atomic<long long> g_first_connection_ns{0};  // steady-clock time of the first accepted connection (throughput without the wait for the sender)

// The sharded engine: G persistent threads, one per shard (RCCL's collectives of one communicator must come from one thread per
// rank).  A connection thread that holds a complete batch takes the engine, every shard thread copies the request into its worker's
// pinned buffers and runs fr_worker_submit_sharded + fr_worker_sync, shard 0's pinned score buffer then holds all scores.
struct ShardedEngine {
    int G = 0, batch = 0;
    std::vector<fr_ctx *> ctxs;
    std::vector<fr_comm *> comms;
    std::vector<fr_worker *> workers;
    std::vector<std::thread> threads;
    std::mutex mtx, user;  // mtx guards the hand-over state; user serialises the connection threads
    std::condition_variable cv;
    long generation = 0;
    int pending = 0;
    bool stop = false;
    const int32_t *req_idx = nullptr;
    const float *req_dense = nullptr;
    size_t idx_bytes = 0, dense_bytes = 0;
    int status = 0;
    std::string error;

    void shard_loop(int r) {
        long seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> lk(mtx);
            cv.wait(lk, [&] { return stop || generation != seen; });
            if (stop) return;
            seen = generation;
            lk.unlock();
            memcpy(fr_worker_idx_ptr(workers[r]), req_idx, idx_bytes);
            if (dense_bytes) memcpy(fr_worker_dense_ptr(workers[r]), req_dense, dense_bytes);
            int rc = fr_worker_submit_sharded(workers[r], comms[r], batch);
            if (rc == FR_OK) rc = fr_worker_sync(workers[r]);
            lk.lock();
            if (rc != FR_OK && status == 0) {
                status = rc;
                error = fr_last_error();
            }
            if (--pending == 0) cv.notify_all();
        }
    }
    // -> 0 and scores in fr_worker_score_ptr(workers[0]); called under `user`
    int run(const int32_t *idx, const float *dense) {
        std::unique_lock<std::mutex> lk(mtx);
        req_idx = idx;
        req_dense = dense;
        pending = G;
        generation++;
        cv.notify_all();
        cv.wait(lk, [&] { return pending == 0; });
        return status;
    }
    void shutdown() {
        {
            std::lock_guard<std::mutex> lk(mtx);
            stop = true;
        }
        cv.notify_all();
        for (auto &t : threads) t.join();
        for (auto *w : workers) fr_worker_destroy(w);
        for (auto *c : comms) fr_comm_destroy(c);
        for (auto *c : ctxs) fr_ctx_destroy(c);
    }
};
static ShardedEngine *g_engine = nullptr;

// --update-port: one thread, one connection at a time, one message at a time (see the usage comment).  `ctxs`: the context, or every shard context.
static std::atomic<bool> g_update_stop{false};
static bool read_exact_or_stop(int fd, void *buf, size_t n) {   // read_exact that gives up when the server is shutting down
    char *p = (char *)buf;
    while (n) {
        pollfd pfd{fd, POLLIN, 0};
        const int pr = poll(&pfd, 1, 100);
        if (g_update_stop.load()) return false;
        if (pr == 0 || (pr < 0 && errno == EINTR)) continue;
        if (pr < 0) return false;
        ssize_t r = read(fd, p, n);
        if (r <= 0) return false;
        p += r;
        n -= (size_t)r;
    }
    return true;
}
static void thread_update(int port, std::vector<fr_ctx *> ctxs) {
    const fr_model_desc *m = fr_ctx_model(ctxs[0]);
    int server_fd = socket(AF_INET, SOCK_STREAM, 0), opt = 1;
    setsockopt(server_fd, SOL_SOCKET, SO_REUSEADDR, &opt, sizeof(opt));
    sockaddr_in addr{};
    addr.sin_family = AF_INET;
    addr.sin_addr.s_addr = INADDR_ANY;
    addr.sin_port = htons((uint16_t)port);
    if (server_fd < 0 || bind(server_fd, (sockaddr *)&addr, sizeof(addr)) < 0 || listen(server_fd, 3) < 0) {
        fprintf(stderr, "update port %d: socket/bind/listen: %s\n", port, strerror(errno));
        if (server_fd >= 0) close(server_fd);
        return;
    }
    std::vector<int32_t> ids;
    std::vector<float> rows;
    while (!g_update_stop.load()) {
        pollfd pfd{server_fd, POLLIN, 0};
        if (poll(&pfd, 1, 100) <= 0) continue;
        const int sock = accept(server_fd, nullptr, nullptr);
        if (sock < 0) continue;
        setsockopt(sock, IPPROTO_TCP, TCP_NODELAY, &opt, sizeof(opt));
        for (;;) {
            int32_t head[2];
            if (!read_exact_or_stop(sock, head, sizeof(head))) break;   // the peer closed (or the server is done)
            const int32_t table = head[0], n = head[1];
            if (table < 0 || table >= m->n_tables || n < 0 || n > (1 << 24)) break;   // malformed: the stream cannot be followed any further
            ids.resize((size_t)n);
            rows.resize((size_t)n * (size_t)m->tables[table].dim);
            if (n && (!read_exact_or_stop(sock, ids.data(), ids.size() * sizeof(int32_t)) || !read_exact_or_stop(sock, rows.data(), rows.size() * sizeof(float)))) break;
            // a shard context the table is not resident on answers FR_ERR_STATE and changes nothing: the message goes to every context, the
            // status is that of the contexts that hold the table
            int32_t status = FR_ERR_STATE;
            for (fr_ctx *c : ctxs) {
                const int rc = fr_ctx_update_rows(c, table, n, ids.data(), rows.data());
                if (rc == FR_ERR_STATE && ctxs.size() > 1) continue;
                if (status == FR_ERR_STATE || status == FR_OK) status = rc;
            }
            if (!write_exact(sock, &status, sizeof(status))) break;
        }
        close(sock);
    }
    close(server_fd);
}

struct ThreadInfo {  // struct CUDA_thread_info (cuda_server.c:91-98)
    int port;
    fr_ctx *ctx;
    std::vector<double> recv_to_submit_us;
    std::vector<double> recv_to_scores_us;  // latency mode: batch fully received -> its scores are in host memory
    std::vector<float> first_scores;
    long batches = 0;
    int status = 0;
    std::string error;
};

static void thread_consume(ThreadInfo *t, const Options &o) {
    const fr_model_desc *m = fr_ctx_model(t->ctx);
    fr_worker *wk = nullptr;
    if (fr_worker_create(t->ctx, o.batch, &wk) != FR_OK) {
        t->status = -1;
        t->error = fr_last_error();
        return;
    }
    // --hots: the block carries the pooled index rows (the worker was created after fr_ctx_set_pooling: its pinned buffer holds them)
    const size_t idx_cols = o.hots > 0 ? (size_t)fr_ctx_pooled_index_cols(t->ctx) : (size_t)fr_model_index_cols(m);
    const size_t idx_bytes = (size_t)o.batch * idx_cols * sizeof(int32_t);
    const size_t dense_bytes = (size_t)o.batch * m->dense_len * sizeof(float);
    // --requests: what a block carries per request and per candidate, and the (equal) requests' offsets in the worker's pinned buffer
    int rq_words = 0, cand_words = 0;
    if (o.requests > 0) {
        int32_t *roff = fr_worker_request_offsets_ptr(wk);
        if (fr_ctx_request_words(t->ctx, o.hots > 0 ? FR_REQ_POOLED : FR_REQ_ONE_HOT, &rq_words, &cand_words, nullptr) != FR_OK || !roff) {
            t->status = -1;
            t->error = roff ? fr_last_error() : "the worker has no request buffers";
            fr_worker_destroy(wk);
            return;
        }
        for (int r = 0; r <= o.requests; r++) roff[r] = r * (o.batch / o.requests);
    }
    const size_t rq_bytes = (size_t)o.requests * (size_t)rq_words * sizeof(int32_t), rq_dense_bytes = o.shared_dense ? (size_t)o.requests * m->dense_len * sizeof(float) : 0;
    const size_t cand_bytes = (size_t)o.batch * (size_t)cand_words * sizeof(int32_t);
    const size_t weight_bytes = o.pool == 2 ? (size_t)o.batch * idx_cols * sizeof(float) : 0;   // --pool weighted: the weights follow the index rows
    // --topk K --segments S: the requests of a block, what fr_worker_sync delivers for them and the (position, score) pairs of the reply
    std::vector<int32_t> seg_off((size_t)o.segments + 1), top_idx(o.topk > 0 ? (size_t)o.segments * (size_t)o.topk : 0);
    std::vector<float> top_sc(top_idx.size());
    std::vector<uint32_t> top_pairs(2 * top_idx.size());
    for (int sg = 0; sg <= o.segments; sg++) seg_off[(size_t)sg] = sg * (o.batch / o.segments);
    int server_fd = socket(AF_INET, SOCK_STREAM, 0), opt = 1;
    setsockopt(server_fd, SOL_SOCKET, SO_REUSEADDR, &opt, sizeof(opt));
    sockaddr_in addr{};
    addr.sin_family = AF_INET;
    addr.sin_addr.s_addr = INADDR_ANY;
    addr.sin_port = htons((uint16_t)t->port);
    int sock = -1;
    if (server_fd < 0 || bind(server_fd, (sockaddr *)&addr, sizeof(addr)) < 0 || listen(server_fd, 3) < 0) {
        t->status = -2;
        t->error = std::string("socket/bind/listen on port ") + std::to_string(t->port) + ": " + strerror(errno);
    } else {
        socklen_t len = sizeof(addr);
        sock = accept(server_fd, (sockaddr *)&addr, &len);
        if (sock < 0) {
            t->status = -3;
            t->error = std::string("accept: ") + strerror(errno);
        }
    }
    if (t->status == 0) {
        setsockopt(sock, IPPROTO_TCP, TCP_NODELAY, &opt, sizeof(opt));
        printf("Successfully built connection on port %d.\n", t->port);
        {
            long long expect = 0;
            g_first_connection_ns.compare_exchange_strong(expect, std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count());
        }
        // --stream: every batch is read into the worker's staging (fr_worker_stage_acquire / fr_worker_push_staged); scores come back
        // in blocks, the last batch's are available after the final sync
        constexpr long long kStreamRing = 512;  // score slots per connection: at most 4 blocks x 64 batches are undelivered at any time
        std::vector<float> stream_scores(o.stream ? (size_t)kStreamRing * o.batch : 0);
        std::vector<int32_t> sh_idx(g_engine ? idx_bytes / sizeof(int32_t) : 0);
        std::vector<float> sh_dense(g_engine ? dense_bytes / sizeof(float) : 0), sh_scores(g_engine ? (size_t)o.batch : 0);
        while (g_engine) {   // table-sharded mode: the whole batch is received here, then every shard works on it
            {
                std::lock_guard<std::mutex> g(g_mtx);
                if (g_global_batch_count >= o.total) break;
                g_global_batch_count++;
            }
            if (!read_exact(sock, sh_idx.data(), idx_bytes) || (dense_bytes && !read_exact(sock, sh_dense.data(), dense_bytes))) {
                t->status = -4;
                t->error = "Receiving data UNSUCCESSFUL (peer closed before the batch was complete)";
                break;
            }
            const auto t_recv = std::chrono::steady_clock::now();
            {
                std::lock_guard<std::mutex> u(g_engine->user);
                if (g_engine->run(sh_idx.data(), dense_bytes ? sh_dense.data() : nullptr) != 0) {
                    t->status = -5;
                    t->error = g_engine->error;
                    break;
                }
                memcpy(sh_scores.data(), fr_worker_score_ptr(g_engine->workers[0]), (size_t)o.batch * sizeof(float));
            }
            t->recv_to_scores_us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_recv).count());
            if (o.reply && !write_exact(sock, sh_scores.data(), (size_t)o.batch * sizeof(float))) {
                t->status = -7;
                t->error = "sending scores failed";
                break;
            }
            t->batches++;
        }
        if (g_engine)
            for (int j = 0; j < 5 && j < o.batch && t->batches > 0; j++) t->first_scores.push_back(sh_scores[j]);
        // --stream --reply: scores go back over the socket, block by block, in request order.  fr_worker_host_poll says how many of the
        // pushed batches have their scores; when the socket has nothing to read and requests are still queued, fr_worker_flush launches the
        // partial block instead of waiting for it to fill (light load: latency of one launch; heavy load: full blocks).
        long long replied = 0;
        auto send_ready = [&]() -> bool {
            long long delivered = 0;
            if (fr_worker_host_poll(wk, &delivered) != FR_OK) {
                t->status = -5;
                t->error = fr_last_error();
                return false;
            }
            for (; replied < delivered; replied++)
                if (!write_exact(sock, stream_scores.data() + (size_t)(replied % kStreamRing) * o.batch, (size_t)o.batch * sizeof(float))) {
                    t->status = -7;
                    t->error = "sending scores failed";
                    return false;
                }
            return true;
        };
        while (o.stream && !g_engine) {
            {   // (a full counter ends the loop before anything is read; the slot itself is taken below, once a request is known to be coming)
                std::lock_guard<std::mutex> g(g_mtx);
                if (g_global_batch_count >= o.total) break;
            }
            if (o.reply) {  // wait for the next request without letting queued ones sit
                // Requests of a burst arrive microseconds apart: the socket must stay dry for --flush-us (default 50 us) before the partial
                // block is launched, or every request of the burst would become its own launch.
                bool flushed = false;
                const auto t_dry = std::chrono::steady_clock::now();
                for (;;) {
                    pollfd pfd{sock, POLLIN, 0};
                    const bool waiting = t->batches > replied;
                    const int pr = poll(&pfd, 1, waiting ? 0 : -1);
                    if (pr != 0) break;  // data, EOF or an error: the read below sorts it out
                    if (!flushed) {
                        int queued0 = 0, blocks0 = 0;
                        fr_worker_host_pending(wk, &queued0, nullptr, &blocks0);
                        // an idle worker with only a few requests queued waits a fifth of --flush-us (they take the stage launches, there is
                        // little to gain from collecting more); otherwise the socket must stay dry for --flush-us first
                        const bool few_and_idle = blocks0 == 0 && queued0 > 0 && queued0 <= o.small_block;
                        const double grace = few_and_idle ? (double)o.flush_us / 5.0 : (double)o.flush_us;  // 10 us is enough to see the rest of a burst coming
                        if (std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_dry).count() < grace) continue;  // spin
                        // adaptive batching: a launch costs the worker's stream >= 150 us whatever it carries.  With nothing in flight the
                        // queued requests leave at once (latency); with blocks in flight they leave once they are worth a launch of their own
                        // (--flush-min, default half a block) -- fewer would only queue behind the running ones, so they keep collecting
                        int queued = 0, blocks = 0;
                        fr_worker_host_pending(wk, &queued, nullptr, &blocks);
                        if (blocks == 0 || queued >= o.flush_min || queued == 0) {
                            if (fr_worker_flush(wk) != FR_OK) {
                                t->status = -5;
                                t->error = fr_last_error();
                                break;
                            }
                            flushed = true;
                        }
                    }
                    if (!send_ready()) break;
                    if (t->batches > replied) {  // scores still on their way and nothing to read: spin for the first 200 us (a small block is
                        pollfd p2{sock, POLLIN, 0};  // back in < 100 us and a sleep's granularity is ~60 us), then yield
                        if (poll(&p2, 1, 0) == 0 && std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_dry).count() > 200.0) usleep(20);
                    }
                }
                if (t->status) break;
            }
            // End of stream?  A sender that is done half-closes its side (fleetrec_sender --window W: shutdown(SHUT_WR)) and still expects
            // the replies of everything it sent.  EOF with ZERO bytes of the next request is therefore a clean end: no counter slot is
            // taken, no staging slot is acquired, the requests already accepted are synchronised and answered below, and the thread ends
            // with status 0.  (-4 stays for a request that is cut off part-way.)  ADVICE r02: the slot used to be taken before the read, so a
            // fast connection that hit EOF dropped up to W pending replies and left a slower connection one request short.
            {
                char probe;
                ssize_t pk;
                do pk = recv(sock, &probe, 1, MSG_PEEK); while (pk < 0 && errno == EINTR);
                if (pk == 0) break;   // orderly shutdown, nothing pending on the wire
                if (pk < 0) {
                    t->status = -4;
                    t->error = "Receiving data UNSUCCESSFUL (socket error)";
                    break;
                }
            }
            {
                std::lock_guard<std::mutex> g(g_mtx);
                if (g_global_batch_count >= o.total) break;   // another connection took the last slot meanwhile: its request stays unread
                g_global_batch_count++;
            }
            // the socket is read straight into the worker's pinned staging slot (the reference reads into its pinned input_feature,
            // cuda_server.c:437), then the slot is queued: no copy between the socket buffer and the H2D source
            int32_t *slot_idx = nullptr;
            float *slot_dense = nullptr;
            if (fr_worker_stage_acquire(wk, o.batch, &slot_idx, &slot_dense) != FR_OK) {
                t->status = -5;
                t->error = fr_last_error();
                break;
            }
            if (!read_exact(sock, slot_idx, idx_bytes) || (dense_bytes && !read_exact(sock, slot_dense, dense_bytes))) {
                t->status = -4;
                t->error = "Receiving data UNSUCCESSFUL (peer closed before the batch was complete)";
                break;
            }
            if (fr_worker_push_staged(wk, o.batch, stream_scores.data() + (size_t)(t->batches % kStreamRing) * o.batch) != FR_OK) {
                t->status = -5;
                t->error = fr_last_error();
                break;
            }
            t->batches++;
            if (o.reply && (t->batches & 15) == 0 && !send_ready()) break;  // (the dry-socket path above polls too: nothing waits on this one)
        }
        if (o.stream && !g_engine) {
            if (t->status == 0 && fr_worker_sync(wk) != FR_OK) {
                t->status = -6;
                t->error = fr_last_error();
            }
            if (t->status == 0 && o.reply) send_ready();  // everything is delivered after the sync: the rest of the replies
            if (t->batches > 0)
                for (int j = 0; j < 5 && j < o.batch; j++) t->first_scores.push_back(stream_scores[(size_t)((t->batches - 1) % kStreamRing) * o.batch + j]);
        }
        while (!o.stream && !g_engine) {
            {
                std::lock_guard<std::mutex> g(g_mtx);
                if (g_global_batch_count >= o.total) break;
                g_global_batch_count++;
            }
            if (o.csr) {   // offsets first: they say how many entries follow; a block that lies about them is refused before its entries are read
                const size_t n_off = (size_t)o.batch * (size_t)fr_model_index_cols(m) + 1;
                int32_t *off = fr_worker_pool_offsets_ptr(wk);
                if (!off || !read_exact(sock, off, n_off * sizeof(int32_t))) {
                    t->status = -4;
                    t->error = off ? "Receiving data UNSUCCESSFUL (peer closed before the batch was complete)" : "the worker has no offsets buffer";
                    break;
                }
                const int64_t nnz = off[n_off - 1];
                if (off[0] != 0 || nnz < 0 || nnz > (int64_t)o.batch * (int64_t)idx_cols) {
                    t->status = -8;
                    t->error = "malformed offsets-form block: offsets[0] = " + std::to_string(off[0]) + ", nnz = " + std::to_string(nnz) + " outside [0, " +
                               std::to_string((int64_t)o.batch * (int64_t)idx_cols) + "]";
                    break;
                }
                const size_t nz = (size_t)nnz * 4;
                if ((nz && !read_exact(sock, fr_worker_idx_ptr(wk), nz)) || (nz && o.pool == 2 && !read_exact(sock, fr_worker_pool_weights_ptr(wk), nz)) ||
                    (dense_bytes && !read_exact(sock, fr_worker_dense_ptr(wk), dense_bytes))) {
                    t->status = -4;
                    t->error = "Receiving data UNSUCCESSFUL (peer closed before the batch was complete)";
                    break;
                }
            } else if (o.requests > 0) {   // request rows (, their dense rows), candidate rows (, the per-item dense rows)
                if ((rq_bytes && !read_exact(sock, fr_worker_request_idx_ptr(wk), rq_bytes)) || (rq_dense_bytes && !read_exact(sock, fr_worker_request_dense_ptr(wk), rq_dense_bytes)) ||
                    (cand_bytes && !read_exact(sock, fr_worker_idx_ptr(wk), cand_bytes)) || (dense_bytes && !o.shared_dense && !read_exact(sock, fr_worker_dense_ptr(wk), dense_bytes))) {
                    t->status = -4;
                    t->error = "Receiving data UNSUCCESSFUL (peer closed before the batch was complete)";
                    break;
                }
            } else if (!read_exact(sock, fr_worker_idx_ptr(wk), idx_bytes) || (weight_bytes && !read_exact(sock, fr_worker_pool_weights_ptr(wk), weight_bytes)) ||
                       (dense_bytes && !read_exact(sock, fr_worker_dense_ptr(wk), dense_bytes))) {
                t->status = -4;
                t->error = "Receiving data UNSUCCESSFUL (peer closed before the batch was complete)";
                break;
            }
            const auto t_recv = std::chrono::steady_clock::now();  // network_time / cuda_time pair of cuda_server.c:429,462
            if ((o.requests > 0 ? fr_worker_submit_requests(wk, o.batch, o.requests, o.hots > 0 ? 1 : 0) : o.csr ? fr_worker_submit_pooled_csr(wk, o.batch, o.pool == 2) : weight_bytes ? fr_worker_submit_pooled_weighted(wk, o.batch) : o.hots > 0 ? fr_worker_submit_pooled(wk, o.batch) : fr_worker_submit(wk, o.batch)) != FR_OK) {
                t->status = -5;
                t->error = fr_last_error();
                break;
            }
            if (o.topk > 0 && fr_worker_topk(wk, o.batch, o.segments, o.segments > 1 ? seg_off.data() : nullptr, o.topk, top_idx.data(), top_sc.data()) != FR_OK) {
                t->status = -5;
                t->error = fr_last_error();
                break;
            }
            t->recv_to_submit_us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_recv).count());
            if (fr_worker_sync(wk) != FR_OK) {
                t->status = -6;
                t->error = fr_last_error();
                break;
            }
            if (o.latency) t->recv_to_scores_us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_recv).count());
            if (o.topk > 0) {   // S x K (position, score) pairs, the scores as bit copies
                for (size_t j = 0; j < top_idx.size(); j++) {
                    memcpy(&top_pairs[2 * j], &top_idx[j], 4);
                    memcpy(&top_pairs[2 * j + 1], &top_sc[j], 4);
                }
            }
            if (o.reply && !(o.topk > 0 ? write_exact(sock, top_pairs.data(), top_pairs.size() * 4) : write_exact(sock, fr_worker_score_ptr(wk), (size_t)o.batch * sizeof(float)))) {
                t->status = -7;
                t->error = "sending scores failed";
                break;
            }
            t->batches++;
        }
        if (!o.stream && !g_engine) {
            const float *sc = fr_worker_score_ptr(wk);
            for (int j = 0; j < 5 && j < o.batch; j++) t->first_scores.push_back(sc[j]);  // cuda_server.c:499-502
        }
    }
    if (sock >= 0) close(sock);
    if (server_fd >= 0) close(server_fd);
    fr_worker_destroy(wk);
}

// --relu / --bias-seed: the context's epilogues (the formula is in the usage comment)
static uint32_t fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
static bool set_epilogues(fr_ctx *ctx, const fr_model_desc *model, const Options &o) {
    if (!o.relu && !o.bias_seed_given) return true;
    for (int l = 0; l < 4; l++) {
        std::vector<float> b;
        if (o.bias_seed_given) {
            const uint32_t hl = fmix32(o.bias_seed ^ ((uint32_t)(l + 1) * 0x9E3779B1u));
            const float scale = 1.0f / sqrtf((float)model->fc[l]);
            for (int h = 0; h < model->fc[l + 1]; h++) b.push_back(((float)(fmix32(hl ^ (uint32_t)h) >> 8) * (1.0f / 8388608.0f) - 1.0f) * scale);
        }
        if (fr_ctx_set_epilogue(ctx, l, b.empty() ? nullptr : b.data(), b.size(), o.relu && l < 3 ? FR_ACT_RELU : FR_ACT_NONE) != FR_OK) return false;
    }
    return true;
}

int main(int argc, char **argv) {
    Options o;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto next = [&]() -> const char * { return (i + 1 < argc) ? argv[++i] : ""; };
        if (a == "--model") { std::string v = next(); o.model = v == "A" ? FR_MODEL_A : v == "B" ? FR_MODEL_B : FR_MODEL_C; }
        else if (a == "--batch") o.batch = atoi(next());
        else if (a == "--threads") o.threads = atoi(next());
        else if (a == "--port") o.port = atoi(next());
        else if (a == "--total") o.total = atol(next());
        else if (a == "--device") o.device = atoi(next());
        else if (a == "--tables") o.tables = std::string(next()) == "hash" ? FR_FILL_HASH : FR_FILL_EVEN_ODD;
        else if (a == "--weights") o.weights = std::string(next()) == "uniform" ? FR_WEIGHTS_UNIFORM : FR_WEIGHTS_ONES;
        else if (a == "--per-item") o.per_item = true;
        else if (a == "--per-bank") o.per_bank = true;
        else if (a == "--shards") o.shards = atoi(next());
        else if (a == "--one-device") o.one_device = true;
        else if (a == "--precision") { std::string v = next(); o.precision = v == "bf16" ? FR_FC_BF16 : v == "fp8" ? FR_FC_FP8 : FR_FC_FP32; }
        else if (a == "--reply") o.reply = true;
        else if (a == "--latency") o.latency = true;
        else if (a == "--stream") o.stream = true;
        else if (a == "--flush-us") o.flush_us = atol(next());
        else if (a == "--flush-min") o.flush_min = atoi(next());
        else if (a == "--small-block") o.small_block = atoi(next());
        else if (a == "--row-cap") o.row_cap = atol(next());
        else if (a == "--relu") o.relu = true;
        else if (a == "--bias-seed") { o.bias_seed = (uint32_t)strtoul(next(), nullptr, 0); o.bias_seed_given = true; }
        else if (a == "--hots") o.hots = atoi(next());
        else if (a == "--csr") o.csr = true;
        else if (a == "--update-port") o.update_port = atoi(next());
        else if (a == "--topk") { o.topk = atoi(next()); o.topk_given = true; }
        else if (a == "--segments") { o.segments = atoi(next()); o.segments_given = true; }
        else if (a == "--requests") o.requests = atoi(next());
        else if (a == "--shared-cols") { o.shared_cols = atoi(next()); o.shared_cols_given = true; }
        else if (a == "--shared-dense") o.shared_dense = true;
        else if (a == "--pool") {
            std::string v = next();
            if (v != "sum" && v != "mean" && v != "weighted") { fprintf(stderr, "--pool: sum, mean or weighted, not '%s'\n", v.c_str()); return 2; }
            o.pool = v == "sum" ? 0 : v == "mean" ? 1 : 2;
        }
        else if (a == "--exchange") {
            std::string v = next();
            if (v != "allgather" && v != "alltoall") { fprintf(stderr, "--exchange: allgather or alltoall, not '%s'\n", v.c_str()); return 2; }
            o.exchange = v == "alltoall" ? FR_EXCHANGE_ALLTOALL : FR_EXCHANGE_ALLGATHER;
            o.exchange_given = true;
        }
        else { fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
    }
    if (o.exchange_given && o.shards <= 0) { fprintf(stderr, "--exchange needs --shards G\n"); return 2; }
    if (o.hots < 0 || o.hots > FR_POOL_MAX_HOTS) { fprintf(stderr, "--hots: 1 .. %d slots per index column, not %d\n", FR_POOL_MAX_HOTS, o.hots); return 2; }
    if (o.hots > 0 && (o.stream || o.shards > 0)) {
        fprintf(stderr, "--hots (pooled lookups) serves the submit-and-sync path only: not with --stream or --shards (their producers are one-hot)\n");
        return 2;
    }
    if (o.requests == 0 && (o.shared_cols_given || o.shared_dense)) { fprintf(stderr, "--shared-cols / --shared-dense need --requests S\n"); return 2; }
    if (o.requests != 0) {   // request-form blocks: the submit-and-sync path, full or padded pooled rows, unweighted
        const char *with = o.stream ? "--stream (its blocks are host-fed full rows)" : o.shards > 0 ? "--shards (a sharded context takes no request split)" :
                           o.csr ? "--csr (the request form cuts padded rows)" : o.pool == 2 ? "--pool weighted" : nullptr;
        if (with) { fprintf(stderr, "--requests is not served with %s\n", with); return 2; }
        if (o.requests < 1 || o.batch % o.requests != 0) {
            fprintf(stderr, "--requests %d: a block of --batch %d candidates must divide into S >= 1 equal requests (batch %% S == 0)\n", o.requests, o.batch);
            return 2;
        }
        if (o.topk > 0 && o.segments_given && o.segments != o.requests) {
            fprintf(stderr, "--requests %d with --topk --segments %d: the segments of the ranking are the requests (omit --segments, or give S)\n", o.requests, o.segments);
            return 2;
        }
        if (o.topk > 0) o.segments = o.requests;
    }
    if (o.segments != 1 && o.topk <= 0) { fprintf(stderr, "--segments S needs --topk K\n"); return 2; }
    if (o.topk_given && (o.topk < 1 || o.topk > FR_TOPK_MAX_K)) { fprintf(stderr, "--topk: 1 .. %d ranked scores per request, not %d\n", FR_TOPK_MAX_K, o.topk); return 2; }
    if (o.topk > 0 && (o.segments < 1 || o.batch % o.segments != 0)) {
        fprintf(stderr, "--topk --segments %d: a block of --batch %d candidates must divide into S >= 1 equal requests (batch %% S == 0)\n", o.segments, o.batch);
        return 2;
    }
    if (o.topk > 0 && o.stream) {
        fprintf(stderr, "--topk ranks the host-form batch in flight (fr_worker_topk); not with --stream: its blocks are host-fed, no such batch is in flight to rank\n");
        return 2;
    }
    if (o.topk > 0 && o.shards > 0) {
        fprintf(stderr, "--topk is not served with --shards: a sharded step's scores are gathered over the communicator, outside the worker's stream order\n");
        return 2;
    }
    if (o.csr && o.hots <= 0) { fprintf(stderr, "--csr (offsets-form blocks) needs --hots N\n"); return 2; }
    if (o.pool >= 0 && o.hots <= 0) { fprintf(stderr, "--pool sum|mean|weighted needs --hots N\n"); return 2; }
    printf("HIP devices visible: %d\n", fr_device_count());  // device probe of cuda_server.c:508-522
    fr_model_desc *model = nullptr;
    if (fr_model_clone_scaled(fr_model_builtin(o.model), 1.0, 1, o.row_cap, &model) != FR_OK) { fprintf(stderr, "%s\n", fr_last_error()); return 1; }
    if (o.per_item) model->index_mode = FR_INDEX_PER_ITEM;
    if (o.per_bank) model->index_mode = FR_INDEX_PER_BANK;
    fr_ctx *ctx = nullptr;
    ShardedEngine engine;
    if (o.shards > 0) {  // one context + worker + communicator handle per shard, devices device .. device + G - 1
        engine.G = o.shards;
        engine.batch = o.batch;
        engine.ctxs.assign(o.shards, nullptr);
        engine.comms.assign(o.shards, nullptr);
        engine.workers.assign(o.shards, nullptr);
        for (int r = 0; r < o.shards; r++) {
            // GPUs device .. device + G - 1, or (--device -1) G CPU shard contexts exchanging in process (fr_comm_init_all picks the transport)
            if (fr_ctx_create_sharded(model, o.device < 0 ? -1 : (o.one_device ? o.device : o.device + r), r, o.shards, &engine.ctxs[r]) != FR_OK || fr_ctx_fill_tables(engine.ctxs[r], o.tables, 0xF1EE7) != FR_OK ||
                fr_ctx_fill_weights(engine.ctxs[r], o.weights, 99) != FR_OK || fr_ctx_set_fc_precision(engine.ctxs[r], o.precision) != FR_OK ||
                !set_epilogues(engine.ctxs[r], model, o) || fr_worker_create(engine.ctxs[r], o.batch, &engine.workers[r]) != FR_OK) {
                fprintf(stderr, "shard %d set-up failed: %s\n", r, fr_last_error());
                return 1;
            }
        }
        if (fr_comm_init_all(engine.ctxs.data(), o.shards, engine.comms.data()) != FR_OK) {
            fprintf(stderr, "exchange set-up failed: %s\n", fr_last_error());
            return 1;
        }
        for (int r = 0; r < o.shards; r++)
            if (fr_comm_set_exchange(engine.comms[r], o.exchange) != FR_OK) {
                fprintf(stderr, "exchange mode of shard %d: %s\n", r, fr_last_error());
                return 1;
            }
        engine.idx_bytes = (size_t)o.batch * (size_t)fr_model_index_cols(model) * sizeof(int32_t);
        engine.dense_bytes = (size_t)o.batch * model->dense_len * sizeof(float);
        for (int r = 0; r < o.shards; r++) engine.threads.emplace_back(&ShardedEngine::shard_loop, &engine, r);
        g_engine = &engine;
        ctx = engine.ctxs[0];
        const bool a2a = o.exchange == FR_EXCHANGE_ALLTOALL;
        if (o.device < 0) printf("table-sharded over %d CPU shard contexts (in-process host %s of the looked-up slices)\n", o.shards, a2a ? "all-to-all" : "exchange");
        else if (o.one_device) printf("table-sharded over %d shard contexts on GPU %d (staged host %s of the looked-up slices)\n", o.shards, o.device, a2a ? "all-to-all" : "exchange");
        else printf("table-sharded over %d GPUs (RCCL %s of the looked-up slices)\n", o.shards, a2a ? "all-to-all" : "all-gather");
    } else if (fr_ctx_create(model, o.device, &ctx) != FR_OK || fr_ctx_fill_tables(ctx, o.tables, 0xF1EE7) != FR_OK ||
               fr_ctx_fill_weights(ctx, o.weights, 99) != FR_OK || fr_ctx_set_fc_precision(ctx, o.precision) != FR_OK || !set_epilogues(ctx, model, o)) {
        fprintf(stderr, "set-up failed: %s\n", fr_last_error());
        return 1;
    }
    if (o.relu || o.bias_seed_given) printf("FC epilogue:%s%s\n", o.relu ? " ReLU on the hidden layers" : "", o.bias_seed_given ? " hashed biases on every layer" : "");
    if (o.hots > 0) {   // before the threads create their workers: a worker sizes its index buffers for the pooled rows at creation
        std::vector<int32_t> hots((size_t)fr_model_index_cols(model), o.hots);
        if (fr_ctx_set_pooling(ctx, hots.data(), (int)hots.size()) != FR_OK) {
            fprintf(stderr, "set-up failed: %s\n", fr_last_error());
            return 1;
        }
        if (o.pool == 1) {
            std::vector<int32_t> modes(hots.size(), FR_POOL_MEAN);
            if (fr_ctx_set_pooling_modes(ctx, modes.data(), (int)modes.size()) != FR_OK) {
                fprintf(stderr, "set-up failed: %s\n", fr_last_error());
                return 1;
            }
        }
        printf("pooled lookups: %d slots on each of %zu index columns, %d int32 per item\n", o.hots, hots.size(), fr_ctx_pooled_index_cols(ctx));
        if (o.csr) printf("offsets-form blocks: int32 offsets[batch x %zu + 1], indices[nnz]%s\n", hots.size(), o.pool == 2 ? ", float32 weights[nnz]" : "");
        if (o.pool > 0) printf("pooling: %s\n", o.pool == 1 ? "mean" : "weighted (float32 weights follow every block's index rows)");
    }
    if (o.requests > 0) {   // before the threads create their workers: a worker gets its request buffers at creation
        const int cols = fr_model_index_cols(model);
        if (o.shared_cols < (o.shared_dense ? 0 : 1) || o.shared_cols > cols - 1) {
            fprintf(stderr, "--requests with --shared-cols %d: the model has %d index columns, N = 1 .. %d (from 0 with --shared-dense)\n", o.shared_cols, cols, cols - 1);
            return 2;
        }
        std::vector<int32_t> shared((size_t)cols, 0);
        for (int c = 0; c < o.shared_cols; c++) shared[(size_t)c] = 1;
        int rs = 0, rc = 0, w = 0;
        if (fr_ctx_set_request_columns(ctx, shared.data(), cols, o.shared_dense ? 1 : 0) != FR_OK ||
            fr_ctx_request_words(ctx, o.hots > 0 ? FR_REQ_POOLED : FR_REQ_ONE_HOT, &rs, &rc, &w) != FR_OK) {
            fprintf(stderr, "set-up failed (--requests --shared-cols %d%s): %s\n", o.shared_cols, o.shared_dense ? " --shared-dense" : "", fr_last_error());
            return 2;
        }
        const size_t full = (size_t)o.batch * ((size_t)w + (size_t)model->dense_len) * 4;
        const size_t form = ((size_t)o.requests * (size_t)rs + (size_t)o.batch * (size_t)rc) * 4 +
                            (size_t)(o.shared_dense ? o.requests : o.batch) * (size_t)model->dense_len * 4;
        printf("request-form blocks: %d requests of %d candidates, %d request + %d candidate words%s; %zu bytes per block (%zu as full rows)\n", o.requests,
               o.batch / o.requests, rs, rc, o.shared_dense ? ", dense features shared" : "", form, full);
    }
    if (o.stream && o.reply && !g_engine && fr_ctx_set_small_block(ctx, o.small_block) != FR_OK) {
        fprintf(stderr, "set-up failed: %s\n", fr_last_error());
        return 1;
    }
    printf("model %s: %d tables, %.3f GB, record %d floats; batch %d, %d threads, ports %d..%d, %ld batches\n", model->name, model->n_tables,
           fr_model_table_bytes(model) / 1e9, model->record_len, o.batch, o.threads, o.port, o.port + o.threads - 1, o.total);
    fflush(stdout);
    std::thread updater;
    if (o.update_port > 0) {
        updater = std::thread(thread_update, o.update_port, g_engine ? engine.ctxs : std::vector<fr_ctx *>{ctx});
        printf("row updates on port %d\n", o.update_port);
    }
    fflush(stdout);
    std::vector<ThreadInfo> info(o.threads);
    std::vector<std::thread> th;
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < o.threads; i++) {
        info[i].port = o.port + i;  // PORT + i (cuda_server.c:541)
        info[i].ctx = ctx;
        th.emplace_back(thread_consume, &info[i], std::cref(o));
    }
    for (auto &t : th) t.join();
    if (updater.joinable()) {
        g_update_stop.store(true);
        updater.join();
    }
    const auto t_end = std::chrono::steady_clock::now();
    const double secs = std::chrono::duration<double>(t_end - t0).count();
    int rc = 0;
    long done = 0;
    double lat = 0;
    size_t nlat = 0;
    for (int i = 0; i < o.threads; i++) {
        if (info[i].status) {
            fprintf(stderr, "thread %d: %s\n", i, info[i].error.c_str());
            rc = 1;
        }
        done += info[i].batches;
        for (double v : info[i].recv_to_submit_us) lat += v, nlat++;
        if (info[i].batches > 0) {  // a thread whose connection came up after the last batch was taken has nothing to show
            printf("thread %d scores:", i);
            for (float v : info[i].first_scores) printf(" %f", v);
            printf("\n");
        } else {
            printf("thread %d took no batch\n", i);
        }
    }
    printf("processed %ld batches (%ld inferences) in %.3f s incl. connection set-up\n", done, done * o.batch, secs);
    if (const long long f = g_first_connection_ns.load()) {  // throughput without the wait for the sender to connect
        const double run_s = (std::chrono::duration_cast<std::chrono::nanoseconds>(t_end.time_since_epoch()).count() - f) * 1e-9;
        if (run_s > 0) printf("first connection -> last scores: %.3f s = %.2f M inferences/s over TCP\n", run_s, done * o.batch / run_s / 1e6);
    }
    if (nlat) printf("Average time from batch received to enqueued: %.3f us\n", lat / nlat);  // the reference's memcpy-time statistic (:565-591)
    if (o.latency) {
        // The reference's latency experiment (measure_network_cuda_cp_latency_single_node/cuda_server.c:1-15,227,548,728-737): the
        // sender is rate-limited so the server is never the bottleneck, and every batch's "received" and "on the device"
        // timestamps are differenced; here the second stamp also exists for "scores back in host memory".
        auto report = [&](const char *what, std::vector<double> v) {
            if (v.empty()) return;
            std::sort(v.begin(), v.end());
            double sum = 0;
            for (double x : v) sum += x;
            auto pct = [&](double p) { return v[(size_t)std::min<double>(v.size() - 1, p * v.size())]; };
            printf("latency %-34s n=%zu avg %.1f us  p50 %.1f  p90 %.1f  p99 %.1f  max %.1f\n", what, v.size(), sum / v.size(), pct(0.50), pct(0.90), pct(0.99),
                   v.back());
        };
        std::vector<double> a, b;
        for (int i = 0; i < o.threads; i++) {
            const size_t skip = std::min<size_t>(info[i].recv_to_submit_us.size(), 8);  // first batches include kernel/code-object warm-up
            a.insert(a.end(), info[i].recv_to_submit_us.begin() + skip, info[i].recv_to_submit_us.end());
            const size_t skip2 = std::min<size_t>(info[i].recv_to_scores_us.size(), 8);
            b.insert(b.end(), info[i].recv_to_scores_us.begin() + skip2, info[i].recv_to_scores_us.end());
        }
        for (size_t i = 0; i < info[0].recv_to_scores_us.size() && i < 10; i++)  // the reference prints every batch (:732); first ten here
            printf("i = %zu recv->enqueued = %.0f ns, recv->scores = %.0f ns\n", i, info[0].recv_to_submit_us[i] * 1e3, info[0].recv_to_scores_us[i] * 1e3);
        report("batch received -> enqueued", a);
        report("batch received -> scores on host", b);
    }
    if (g_engine) engine.shutdown();
    else fr_ctx_destroy(ctx);
    fr_model_free(model);
    return rc;
}
