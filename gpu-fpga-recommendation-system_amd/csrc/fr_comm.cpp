// Table-sharded mode behind the C-ABI: the exchange step on RCCL (include/fleetrec.h "table-sharded mode").
//
// Reference shape: the 3-node GPU server receives the three parts of every batch from three senders (CPU0, FPGA0, FPGA1) over
// three sockets before its GEMMs (GPU/final_network_cublasLt_3_nodes_no_FIFO_scatter/cuda_server.c:513-591).  Here the "senders" are
// the G GPUs that hold the table-ID shards: each gathers its slice of the record, ONE ncclAllGather over xGMI delivers all slices to
// everybody, each GPU runs the FC chain on its B/G items, and a second (tiny) all-gather hands every rank all B scores.
// EXCHANGE MODES (fr_comm_set_exchange): the all-gather above is the default; in all-to-all mode each rank receives from every rank only the
// rows of its own items (grouped ncclSend / ncclRecv; the host exchange copies only those rows) -- 1/G of the all-gather's bytes, the same
// readers (the receive buffer is the all-gather layout of a batch of n_r items), bit-identical scores.  The score exchange and the sharded fp8
// calibration are all-gathers in both modes.
// librccl.so is opened on first use (dlopen), so unsharded users never load it; every RCCL failure surfaces as FR_ERR_COMM.
//
// TWO TRANSPORTS under ONE protocol (round 6).  The step -- the uneven item split, the status word behind every score chunk, the
// communicator's reference counts, the bounded wait of fr_worker_sync, the three kinds of failure -- is written once (sharded_step,
// comm_wait_step).  What differs sits below it:
//   * RCCL: G GPU contexts; ncclAllGather on the worker's HIP stream; the step is ENQUEUED by fr_worker_submit_sharded.
//   * the in-process host exchange: G CPU contexts (device = -1) of one process driven by G host threads; the all-gather is a rendezvous of
//     those threads (HostGroup: publish, barrier, copy, barrier); the step RUNS on the worker's host stream (HostStream: one thread per
//     worker that executes the posted step in order -- what a HIP stream is to a GPU worker), so fr_worker_submit_sharded returns at once and
//     fr_worker_sync polls that stream with the same bounded loop.  Like an RCCL collective, the rendezvous itself waits without a bound and is
//     released by an abort; the bound lives in fr_worker_sync.
//   * the same host exchange, STAGED, for GPU shard contexts that share a device (fr_comm_init_all over contexts of which two sit on one GPU --
//     RCCL wants one device per rank): every all-gather is D2H into the worker's pinned staging, the rendezvous, H2D of all G parts; the step runs
//     on a host stream as a CPU worker's does (the rendezvous blocks), the kernels and copies on the worker's HIP stream.  It is how the WHOLE
//     step -- slice gathers in the chain's operand type, the uneven split on the device, NaN poisoning, status words through hipMemcpy2DAsync,
//     the bf16 / fp8 chains on all-gathered slices, the sharded fp8 calibration -- runs with G = 2 .. 8 ranks on a one-GPU box.
// The host exchange exists so that the protocol meets ranks 1 .. G-1 on machines without G GPUs (tests/test_cpu_backend.py, TSan build;
// tests/test_gpu_sharded.py on one GPU) and as the exchange of `fleetrec_server --shards G --device -1`.
#include <dlfcn.h>
#include <rccl/rccl.h>  // types and prototypes only: the functions are resolved through dlsym

#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <functional>
#include <mutex>
#include <new>
#include <thread>

#include "fr_internal.h"

namespace {
struct Rccl {
    void *handle = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclCommAbort) CommAbort = nullptr;  // optional: a rank that cannot take part in a collective aborts the communicator
    decltype(&ncclCommGetAsyncError) CommGetAsyncError = nullptr;  // optional: polled by the bounded wait of fr_comm_wait
    // optional as a set: the all-to-all exchange mode (fr_comm_set_exchange refuses FR_EXCHANGE_ALLTOALL over RCCL without them)
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
};
Rccl g_rccl;
std::once_flag g_rccl_once;
bool g_rccl_ok = false;
bool g_rccl_p2p = false;   // Send / Recv / GroupStart / GroupEnd all resolved
char g_rccl_why[256] = "symbol missing";

int rccl_load() {
    std::call_once(g_rccl_once, [] {
        const char *names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
        for (const char *n : names) {
            g_rccl.handle = dlopen(n, RTLD_NOW | RTLD_LOCAL);
            if (g_rccl.handle) break;
            const char *e = dlerror();  // dlerror() clears itself: read it once
            if (e) snprintf(g_rccl_why, sizeof(g_rccl_why), "%s", e);
        }
        if (!g_rccl.handle) return;
        snprintf(g_rccl_why, sizeof(g_rccl_why), "symbol missing");
#define FR_SYM(field, name)                                              \
    g_rccl.field = reinterpret_cast<decltype(g_rccl.field)>(dlsym(g_rccl.handle, name)); \
    if (!g_rccl.field) return;
        FR_SYM(GetUniqueId, "ncclGetUniqueId")
        FR_SYM(CommInitRank, "ncclCommInitRank")
        FR_SYM(CommInitAll, "ncclCommInitAll")
        FR_SYM(CommDestroy, "ncclCommDestroy")
        FR_SYM(AllGather, "ncclAllGather")
        FR_SYM(GetErrorString, "ncclGetErrorString")
#undef FR_SYM
        g_rccl.CommAbort = reinterpret_cast<decltype(g_rccl.CommAbort)>(dlsym(g_rccl.handle, "ncclCommAbort"));
        g_rccl.CommGetAsyncError = reinterpret_cast<decltype(g_rccl.CommGetAsyncError)>(dlsym(g_rccl.handle, "ncclCommGetAsyncError"));
        g_rccl.Send = reinterpret_cast<decltype(g_rccl.Send)>(dlsym(g_rccl.handle, "ncclSend"));
        g_rccl.Recv = reinterpret_cast<decltype(g_rccl.Recv)>(dlsym(g_rccl.handle, "ncclRecv"));
        g_rccl.GroupStart = reinterpret_cast<decltype(g_rccl.GroupStart)>(dlsym(g_rccl.handle, "ncclGroupStart"));
        g_rccl.GroupEnd = reinterpret_cast<decltype(g_rccl.GroupEnd)>(dlsym(g_rccl.handle, "ncclGroupEnd"));
        g_rccl_p2p = g_rccl.Send && g_rccl.Recv && g_rccl.GroupStart && g_rccl.GroupEnd;
        g_rccl_ok = true;
    });
    if (!g_rccl_ok) FR_FAIL(FR_ERR_COMM, "librccl.so could not be loaded (dlopen / dlsym): %s", g_rccl_why);
    return FR_OK;
}
}  // namespace


// ---- transport 2: the in-process host exchange --------------------------------------------------------------------------------------
namespace {
constexpr int FR_HOST_MAX_RANKS = 64;
// the uneven item split of a sharded step: rank q owns items [lo, lo + n) of a batch over G ranks
inline void item_range(int batch, int G, int q, int *lo, int *n) {
    const int base = batch / G, rem = batch % G;
    *lo = q * base + (q < rem ? q : rem);
    *n = base + (q < rem ? 1 : 0);
}

// One per fr_comm_init_all over CPU contexts (or over GPU contexts that share a device: the staged form), shared by its G handles.  all_gather: every rank publishes its send buffer and waits for the
// others (barrier 1), copies all G buffers into its own receive buffer, and waits until everybody has copied (barrier 2: only then may a
// send buffer be reused).  Barrier 1 ends early when the group is aborted; barrier 2 never does -- every rank that left barrier 1 is copying
// from its peers' buffers and will count itself in, and no buffer may go away under a peer's memcpy.  all_to_all: the same rendezvous, but
// each rank copies only the rows of its own items from every peer.  Every rank publishes the operation with its sizes: ranks that disagree
// (another operation, another size) break the group.
struct HostGroup {
    enum Op { ALL_GATHER = 0, ALL_TO_ALL = 1 };
    const int n;
    std::mutex m;
    std::condition_variable cv;
    const void *send[FR_HOST_MAX_RANKS] = {};
    size_t bytes[FR_HOST_MAX_RANKS] = {};
    size_t row[FR_HOST_MAX_RANKS] = {};
    int op[FR_HOST_MAX_RANKS] = {};
    int arrived = 0, copied = 0;
    uint64_t gen_arrive = 0, gen_copy = 0;
    bool broken = false;            // under m
    std::atomic<bool> broken_flag{false};   // the same, readable without the lock (the bounded wait's "asynchronous error" poll)
    std::atomic<int> refs;
    explicit HostGroup(int n_) : n(n_), refs(n_) {}
    void abort() {
        {
            std::lock_guard<std::mutex> lk(m);
            broken = true;
            broken_flag.store(true, std::memory_order_release);
        }
        cv.notify_all();
    }
    // -> FR_OK, or FR_ERR_COMM when the group was aborted before everybody had arrived / the ranks disagree about the size
    int all_gather(int rank, const void *sendbuf, void *recvbuf, size_t nbytes) { return exchange(rank, ALL_GATHER, sendbuf, recvbuf, nbytes, nbytes); }
    // every rank sends `batch` rows of row_bytes (nbytes = batch * row_bytes); rank r receives [G][n_r] rows: rows [lo_r, lo_r + n_r) of each
    // rank's buffer, in rank order.  -> as all_gather
    int all_to_all(int rank, const void *sendbuf, void *recvbuf, size_t nbytes, size_t row_bytes) { return exchange(rank, ALL_TO_ALL, sendbuf, recvbuf, nbytes, row_bytes); }

  private:
    int exchange(int rank, int op_, const void *sendbuf, void *recvbuf, size_t nbytes, size_t row_bytes) {
        const void *src[FR_HOST_MAX_RANKS];
        bool same = true;
        {
            std::unique_lock<std::mutex> lk(m);
            if (broken) return FR_ERR_COMM;
            send[rank] = sendbuf;
            bytes[rank] = nbytes;
            row[rank] = row_bytes;
            op[rank] = op_;
            const uint64_t g = gen_arrive;
            if (++arrived == n) {
                arrived = 0;
                gen_arrive++;
                cv.notify_all();
            } else {
                cv.wait(lk, [&] { return gen_arrive != g || broken; });
                if (gen_arrive == g) {   // aborted while waiting: this rank's arrival is withdrawn
                    arrived--;
                    return FR_ERR_COMM;
                }
            }
            for (int q = 0; q < n; q++) {
                src[q] = send[q];
                same &= bytes[q] == nbytes && row[q] == row_bytes && op[q] == op_;
            }
            if (!same) {   // every rank reads the same table and takes the same decision: nobody copies, everybody still passes barrier 2
                broken = true;
                broken_flag.store(true, std::memory_order_release);
            }
        }
        if (same && op_ == ALL_GATHER) {
            for (int q = 0; q < n; q++) memcpy(static_cast<char *>(recvbuf) + (size_t)q * nbytes, src[q], nbytes);
        } else if (same) {
            int lo, rows;
            item_range((int)(nbytes / row_bytes), n, rank, &lo, &rows);
            const size_t part = (size_t)rows * row_bytes;
            for (int q = 0; q < n && part; q++) memcpy(static_cast<char *>(recvbuf) + (size_t)q * part, static_cast<const char *>(src[q]) + (size_t)lo * row_bytes, part);
        }
        {
            std::unique_lock<std::mutex> lk(m);
            const uint64_t g = gen_copy;
            if (++copied == n) {
                copied = 0;
                gen_copy++;
                cv.notify_all();
            } else {
                cv.wait(lk, [&] { return gen_copy != g; });
            }
        }
        return same ? FR_OK : FR_ERR_COMM;
    }
};

// The host stream of a worker whose exchange is the host group (CPU workers; GPU workers of the staged form): one thread, one posted step at a
// time (a worker has at most one sharded step in flight).
struct HostStream {
    std::mutex m;
    std::condition_variable cv;
    std::function<int()> job;
    bool has_job = false, stop = false;
    std::atomic<bool> busy{false};
    int rc = FR_OK;           // of the last step; read after busy has gone false
    char text[512] = "";      // fr_last_error() of the stream thread after a failed step
    std::thread th;
    HostStream() : th([this] { loop(); }) {}
    ~HostStream() {
        {
            std::lock_guard<std::mutex> lk(m);
            stop = true;
        }
        cv.notify_all();
        th.join();
    }
    void post(std::function<int()> f) {
        {
            std::lock_guard<std::mutex> lk(m);
            job = std::move(f);
            has_job = true;
            busy.store(true, std::memory_order_release);
        }
        cv.notify_all();
    }
    bool done() const { return !busy.load(std::memory_order_acquire); }
    void wait() {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return !busy.load(std::memory_order_acquire); });
    }
    void loop() {
        for (;;) {
            std::function<int()> f;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return has_job || stop; });
                if (!has_job) return;
                f = std::move(job);
                has_job = false;
            }
            const int r = f();
            {
                std::lock_guard<std::mutex> lk(m);
                rc = r;
                snprintf(text, sizeof(text), "%s", r ? fr_last_error() : "");
                busy.store(false, std::memory_order_release);
            }
            cv.notify_all();
        }
    }
};
HostStream *host_stream(fr_worker *w) {
    if (!w->sh_host_stream) w->sh_host_stream = new HostStream();
    return static_cast<HostStream *>(w->sh_host_stream);
}
}  // namespace

#define FR_NCCL(call)                                                                                   \
    do {                                                                                                \
        ncclResult_t r_ = (call);                                                                       \
        if (r_ != ncclSuccess) FR_FAIL(FR_ERR_COMM, "%s failed: %s", #call, g_rccl.GetErrorString(r_)); \
    } while (0)

struct fr_comm {
    ncclComm_t comm = nullptr;   // transport 1: RCCL (GPU contexts)
    HostGroup *grp = nullptr;    // transport 2: the in-process host exchange (CPU contexts; staged: GPU contexts sharing a device); exactly one of the two is set
    int rank = 0, n_ranks = 1;
    fr_ctx *ctx = nullptr;
    // a collective step failed on this rank: the communicator was aborted, every later call returns FR_ERR_COMM (atomic: a CPU worker's step
    // runs on its host stream while fr_worker_sync polls)
    std::atomic<bool> broken{false};
    std::atomic<int> wait_ms{60000};  // bound of fr_comm_wait: how long fr_worker_sync lets a step's collectives take before it gives the peers up
    std::atomic<int> exchange{FR_EXCHANGE_ALLGATHER};   // fr_comm_set_exchange: how the slices travel (the score chunks are always all-gathered)
    std::atomic<uint64_t> x_received{0}, x_sent{0};     // fr_comm_exchange_bytes: slice bytes of the last step, peers only
    // one reference for the handle fr_comm_init_* gave out + one per worker with a sharded step in flight through this communicator
    // (fr_worker::sh_comm): fr_comm_destroy between a submit and its sync only drops the handle's reference, the communicator itself goes
    // when the last worker has synchronised (fr_comm_wait used to dereference a freed object in that sequence)
    std::atomic<int> refs{1};
};
constexpr int FR_COMM_MAX_RANKS = 64;   // fr_worker::h_sh_status holds 1 + FR_COMM_MAX_RANKS status words
static_assert(FR_HOST_MAX_RANKS == FR_COMM_MAX_RANKS, "one limit for both transports");

// Failure protocol of a collective step.  Three kinds of failure, three answers:
//  (1) argument / state errors found BEFORE anything was enqueued (worker busy, batch too large, tables not filled ...): returned as they
//      are, the communicator stays usable.  The ranks of a job are driven with the same arguments, so such an error is the same on every
//      rank; a caller that lets ONE rank skip a step has broken the contract and its peers run into (3).
//  (2) the local FC chain fails after the first collective: both collectives are still issued (the peers are on their way into them), the
//      rank's score chunk is poisoned with NaN and its STATUS WORD -- one float all-gathered behind every score chunk -- carries the code:
//      every rank's fr_worker_sync reads all G status words and returns FR_ERR_COMM naming the rank; nobody gets stale scores silently.
//      (RCCL: the failing rank's submit returns the chain's error too; host exchange: the step runs behind the submit, so the failing rank
//      learns it from its own fr_worker_sync like everybody else.)
//  (3) a real failure of the device / the transport on this rank (a HIP error, a collective that cannot be enqueued), or peers that do not
//      arrive: the rank ABORTS its communicator (comm_fail) and answers FR_ERR_COMM from then on; the peers' waits are BOUNDED (fr_comm_wait:
//      the step's stream is polled together with the transport's asynchronous-error state for at most wait_ms, then the waiting rank aborts
//      its own communicator and returns FR_ERR_COMM) -- a local ncclCommAbort does not by itself release a peer in another process; an abort
//      of the in-process host group does release every rank of it at once.
// Executed with G = 2, 3 and 8 ranks on the host exchange (tests/test_cpu_backend.py, also under ThreadSanitizer); over RCCL with one-rank
// communicators only -- the test boxes have one GPU.
static int comm_fail(fr_comm *comm, int rc) {
    if (comm && !comm->broken.exchange(true, std::memory_order_acq_rel)) {
        if (comm->grp) comm->grp->abort();
        if (comm->comm && g_rccl.CommAbort) {
            (void)g_rccl.CommAbort(comm->comm);
            comm->comm = nullptr;  // aborted communicators are already destroyed
        }
    }
    return rc;
}
static bool comm_is_broken(const fr_comm *comm) {
    return comm->broken.load(std::memory_order_acquire) || (comm->grp && comm->grp->broken_flag.load(std::memory_order_acquire));
}
#define FR_BROKEN_TEXT "the communicator was aborted by an earlier failure (on this rank, or on a peer of the in-process host exchange)"

static_assert(sizeof(ncclUniqueId) == 128, "fr_comm_unique_id hands out 128 bytes");

extern "C" int fr_comm_unique_id(void *id128) {
    if (!id128) FR_FAIL(FR_ERR_INVALID, "id128 is NULL");
    int rc = rccl_load();
    if (rc) return rc;
    ncclUniqueId id;
    FR_NCCL(g_rccl.GetUniqueId(&id));
    memcpy(id128, &id, sizeof(id));
    return FR_OK;
}

static int comm_check_ctx(const fr_ctx *ctx) {
    if (!ctx) FR_FAIL(FR_ERR_INVALID, "ctx is NULL");
    if (ctx->n_shards > FR_COMM_MAX_RANKS) FR_FAIL(FR_ERR_INVALID, "%d shards: the exchange serves at most %d ranks", ctx->n_shards, FR_COMM_MAX_RANKS);
    if (ctx->model.layout != FR_LAYOUT_SEMANTIC) FR_FAIL(FR_ERR_STATE, "the sharded exchange needs the SEMANTIC layout");
    return FR_OK;
}

extern "C" int fr_comm_init_rank(fr_ctx *ctx, const void *id128, fr_comm **out) {
    if (!out || !id128) FR_FAIL(FR_ERR_INVALID, "NULL argument");
    *out = nullptr;
    int rc = comm_check_ctx(ctx);
    if (rc) return rc;
    if (ctx->cpu) FR_FAIL(FR_ERR_STATE, "CPU contexts (device = -1) exchange in-process only: set the G shard contexts of one process up with fr_comm_init_all");
    rc = rccl_load();
    if (rc) return rc;
    FR_HIP(hipSetDevice(ctx->device));
    fr_comm *c = new (std::nothrow) fr_comm();
    if (!c) FR_FAIL(FR_ERR_OOM, "out of host memory");
    c->rank = ctx->shard_rank;
    c->n_ranks = ctx->n_shards;
    c->ctx = ctx;
    fr_ctx_ref(ctx);   // (dropped by comm_release: a communicator destroyed after its context touches no freed memory)
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    ncclResult_t r = g_rccl.CommInitRank(&c->comm, c->n_ranks, id, c->rank);
    if (r != ncclSuccess) {
        delete c;
        fr_ctx_unref(ctx);
        FR_FAIL(FR_ERR_COMM, "ncclCommInitRank(rank %d of %d) failed: %s", ctx->shard_rank, ctx->n_shards, g_rccl.GetErrorString(r));
    }
    *out = c;
    return FR_OK;
}

extern "C" int fr_comm_init_all(fr_ctx *const *ctxs, int n, fr_comm **out) {
    if (!ctxs || !out || n < 1 || n > FR_COMM_MAX_RANKS) FR_FAIL(FR_ERR_INVALID, "bad argument");
    for (int r = 0; r < n; r++) out[r] = nullptr;
    int rc;
    int devs[64];
    bool shared_device = false;
    for (int r = 0; r < n; r++) {
        rc = comm_check_ctx(ctxs[r]);
        if (rc) return rc;
        if (ctxs[r]->n_shards != n || ctxs[r]->shard_rank != r) FR_FAIL(FR_ERR_INVALID, "ctxs[%d] is shard %d of %d, expected %d of %d", r, ctxs[r]->shard_rank, ctxs[r]->n_shards, r, n);
        if (ctxs[r]->cpu != ctxs[0]->cpu) FR_FAIL(FR_ERR_INVALID, "ctxs[%d]: CPU and GPU shard contexts cannot share a communicator", r);
        devs[r] = ctxs[r]->device;
        if (!ctxs[r]->cpu)
            for (int q = 0; q < r; q++) shared_device |= devs[q] == devs[r];
    }
    // CPU contexts: the in-process host exchange.  GPU contexts of which two share a device (RCCL needs one device per rank): the same
    // exchange, staged through pinned host memory.  One device per rank: RCCL.
    const bool host = ctxs[0]->cpu || shared_device;
    ncclComm_t comms[64];
    HostGroup *grp = nullptr;
    if (host) {   // the in-process host exchange: nothing of RCCL is touched (or loaded)
        grp = new (std::nothrow) HostGroup(n);
        if (!grp) FR_FAIL(FR_ERR_OOM, "out of host memory");
    } else {
        rc = rccl_load();
        if (rc) return rc;
        FR_NCCL(g_rccl.CommInitAll(comms, n, devs));
    }
    for (int r = 0; r < n; r++) {
        fr_comm *c = new (std::nothrow) fr_comm();
        if (!c) {
            for (int q = 0; q < r; q++) {
                fr_comm_destroy(out[q]);
                out[q] = nullptr;
            }
            if (host) {
                if (grp->refs.fetch_sub(n - r, std::memory_order_acq_rel) == n - r) delete grp;   // the handles never made
            } else {
                for (int q = r; q < n; q++) (void)g_rccl.CommDestroy(comms[q]);
            }
            FR_FAIL(FR_ERR_OOM, "out of host memory");
        }
        if (host) c->grp = grp;
        else c->comm = comms[r];
        c->rank = r;
        c->n_ranks = n;
        c->ctx = ctxs[r];
        fr_ctx_ref(ctxs[r]);
        out[r] = c;
    }
    return FR_OK;
}

extern "C" int fr_comm_set_wait_ms(fr_comm *c, int wait_ms) {
    if (!c || wait_ms < 1) FR_FAIL(FR_ERR_INVALID, "bad argument");
    c->wait_ms.store(wait_ms, std::memory_order_relaxed);
    return FR_OK;
}

extern "C" int fr_comm_set_exchange(fr_comm *c, int exchange) {
    if (!c) FR_FAIL(FR_ERR_INVALID, "comm is NULL");
    if (exchange != FR_EXCHANGE_ALLGATHER && exchange != FR_EXCHANGE_ALLTOALL) FR_FAIL(FR_ERR_INVALID, "unknown exchange mode %d", exchange);
    if (comm_is_broken(c)) FR_FAIL(FR_ERR_COMM, FR_BROKEN_TEXT);
    // refs > 1: a worker holds this communicator for a step it has not synchronised yet
    if (c->refs.load(std::memory_order_acquire) > 1) FR_FAIL(FR_ERR_STATE, "a sharded step is in flight through this communicator: call fr_worker_sync first");
    if (exchange == FR_EXCHANGE_ALLTOALL && c->comm && !g_rccl_p2p)
        FR_FAIL(FR_ERR_COMM, "the all-to-all exchange needs ncclSend / ncclRecv / ncclGroupStart / ncclGroupEnd: librccl.so lacks at least one of them");
    c->exchange.store(exchange, std::memory_order_release);
    return FR_OK;
}

extern "C" int fr_comm_exchange(const fr_comm *c) {
    if (!c) FR_FAIL(FR_ERR_INVALID, "comm is NULL");
    return c->exchange.load(std::memory_order_acquire);
}

extern "C" int fr_comm_exchange_bytes(const fr_comm *c, uint64_t *received, uint64_t *sent) {
    if (!c || !received || !sent) FR_FAIL(FR_ERR_INVALID, "NULL argument");
    *received = c->x_received.load(std::memory_order_relaxed);
    *sent = c->x_sent.load(std::memory_order_relaxed);
    return FR_OK;
}

static void comm_release(fr_comm *c) {
    if (c->refs.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
    if (c->comm && g_rccl_ok) {
        if (c->ctx) (void)hipSetDevice(c->ctx->device);
        (void)g_rccl.CommDestroy(c->comm);
    }
    if (c->grp && c->grp->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) delete c->grp;   // the last of the G handles takes the group along
    fr_ctx *held = c->ctx;
    delete c;
    fr_ctx_unref(held);
}

extern "C" void fr_comm_destroy(fr_comm *c) {
    if (c) comm_release(c);
}

// fr_worker_sync leaves early (another path of the worker failed first): the step's reference goes without a wait
void fr_comm_forget(fr_worker *w) {
    fr_comm *comm = w->sh_comm;
    w->sh_comm = nullptr;
    if (comm) comm_release(comm);
}

bool fr_comm_step_on_host_stream(const fr_worker *w) { return w->sh_host_stream && !static_cast<const HostStream *>(w->sh_host_stream)->done(); }

// fr_worker_destroy of a worker with a host stream (CPU workers; GPU workers of a staged exchange): a step still running on the host stream is given its communicator's bound, then the exchange is
// aborted (which releases a step parked in a rendezvous); the stream thread is joined, the step's reference dropped.
void fr_comm_worker_release(fr_worker *w) {
    if (w->sh_host_stream) {
        HostStream *hs = static_cast<HostStream *>(w->sh_host_stream);
        fr_comm *comm = w->sh_comm;
        if (!hs->done() && comm) {
            struct timespec t0, t1;
            clock_gettime(CLOCK_MONOTONIC, &t0);
            while (!hs->done()) {
                clock_gettime(CLOCK_MONOTONIC, &t1);
                if ((t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6 > comm->wait_ms.load(std::memory_order_relaxed)) {
                    (void)comm_fail(comm, FR_ERR_COMM);
                    break;
                }
                struct timespec nap = {0, 200000};
                nanosleep(&nap, nullptr);
            }
        }
        hs->wait();
        delete hs;
        w->sh_host_stream = nullptr;
    }
    fr_comm_forget(w);
}

// ---- the few device operations of a step, on either back-end: a command on the worker's HIP stream, or the same thing done at once by the
// thread that runs the step (a CPU worker's step runs on its host stream: "enqueued" there means "done, in order") --------------------------
static int step_copy(fr_worker *w, void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    if (w->ctx->cpu) {
        memcpy(dst, src, bytes);
        return FR_OK;
    }
    FR_HIP(hipMemcpyAsync(dst, src, bytes, kind, w->stream));
    return FR_OK;
}
// the status word behind each of the G score chunks of d_score_all ([G][chunk + 1]) -> h_sh_status[1 .. G]: one strided copy
static int step_copy_status(fr_worker *w, int G, int chunk) {
    if (w->ctx->cpu) {
        for (int q = 0; q < G; q++) w->h_sh_status[1 + q] = w->d_score_all[(size_t)q * (chunk + 1) + chunk];
        return FR_OK;
    }
    FR_HIP(hipMemcpy2DAsync(w->h_sh_status + 1, sizeof(float), w->d_score_all + chunk, ((size_t)chunk + 1) * sizeof(float), sizeof(float), (size_t)G, hipMemcpyDeviceToHost, w->stream));
    return FR_OK;
}
static int step_fill_ff(fr_worker *w, void *dst, size_t bytes) {   // NaN in every float
    if (w->ctx->cpu) {
        memset(dst, 0xFF, bytes);
        return FR_OK;
    }
    FR_HIP(hipMemsetAsync(dst, 0xFF, bytes, w->stream));
    return FR_OK;
}
// ONE all-gather of `bytes` per rank through the communicator's transport
static int step_all_gather(fr_worker *w, fr_comm *comm, const void *send, void *recv, size_t bytes) {
    if (comm->grp) {
        const void *h_send = send;
        void *h_recv = recv;
        if (!w->ctx->cpu) {   // staged: this rank's part comes off the device first (everything the step enqueued so far has then run)
            FR_HIP(hipMemcpyAsync(w->h_stage_send, send, bytes, hipMemcpyDeviceToHost, w->stream));
            FR_HIP(hipStreamSynchronize(w->stream));
            h_send = w->h_stage_send;
            h_recv = w->h_stage_recv;
        }
        if (comm->grp->all_gather(comm->rank, h_send, h_recv, bytes) != FR_OK)
            FR_FAIL(FR_ERR_COMM, "host exchange: the all-gather of %zu bytes per rank was aborted (a peer failed, never arrived, or sent another size)", bytes);
        if (!w->ctx->cpu) FR_HIP(hipMemcpyAsync(recv, w->h_stage_recv, bytes * (size_t)comm->n_ranks, hipMemcpyHostToDevice, w->stream));
        return FR_OK;
    }
    ncclResult_t r = g_rccl.AllGather(send, recv, bytes, ncclChar, comm->comm, w->stream);
    if (r != ncclSuccess) FR_FAIL(FR_ERR_COMM, "ncclAllGather(%zu bytes per rank) failed: %s", bytes, g_rccl.GetErrorString(r));
    return FR_OK;
}
// ONE all-to-all of the item-major slices ([batch][row] bytes per rank): rank r receives [G][n_r][row], the rows of its own items from every
// rank in rank order -- the [n_shards][batch_total][P] layout of fr_worker_fc_from_slices(_lp) with batch_total = n_r, item0 = 0.  Rank q's
// rows for rank r are contiguous in q's slice, so neither side packs anything.
static int step_all_to_all(fr_worker *w, fr_comm *comm, const void *send, void *recv, int batch, size_t row) {
    const int G = comm->n_ranks, r = comm->rank;
    int lo_r, n_r;
    item_range(batch, G, r, &lo_r, &n_r);
    const size_t bytes = (size_t)batch * row, part = (size_t)n_r * row;
    if (comm->grp) {
        const void *h_send = send;
        void *h_recv = recv;
        if (!w->ctx->cpu) {   // staged: the whole slice comes off the device, only this rank's G parts go back
            FR_HIP(hipMemcpyAsync(w->h_stage_send, send, bytes, hipMemcpyDeviceToHost, w->stream));
            FR_HIP(hipStreamSynchronize(w->stream));
            h_send = w->h_stage_send;
            h_recv = w->h_stage_recv;
        }
        if (comm->grp->all_to_all(r, h_send, h_recv, bytes, row) != FR_OK)
            FR_FAIL(FR_ERR_COMM, "host exchange: the all-to-all of %zu bytes per rank was aborted (a peer failed, never arrived, or sent another size or mode)", bytes);
        if (!w->ctx->cpu && part) FR_HIP(hipMemcpyAsync(recv, w->h_stage_recv, part * (size_t)G, hipMemcpyHostToDevice, w->stream));
        return FR_OK;
    }
    // zero-count transfers are skipped on both sides: rank q sends n_r rows to r exactly when r expects n_r rows from q
    ncclResult_t r0 = g_rccl.GroupStart();
    if (r0 != ncclSuccess) FR_FAIL(FR_ERR_COMM, "ncclGroupStart failed: %s", g_rccl.GetErrorString(r0));
    ncclResult_t bad = ncclSuccess;
    for (int q = 0; q < G && bad == ncclSuccess; q++) {
        int lo_q, n_q;
        item_range(batch, G, q, &lo_q, &n_q);
        if (n_q > 0) bad = g_rccl.Send(static_cast<const char *>(send) + (size_t)lo_q * row, (size_t)n_q * row, ncclChar, q, comm->comm, w->stream);
        if (bad == ncclSuccess && part) bad = g_rccl.Recv(static_cast<char *>(recv) + (size_t)q * part, part, ncclChar, q, comm->comm, w->stream);
    }
    const ncclResult_t end = g_rccl.GroupEnd();   // the group is closed whatever happened inside it
    if (bad == ncclSuccess) bad = end;
    if (bad != ncclSuccess) FR_FAIL(FR_ERR_COMM, "all-to-all (ncclSend / ncclRecv, %zu bytes per rank) failed: %s", bytes, g_rccl.GetErrorString(bad));
    return FR_OK;
}
// -> 0 the step's stream is idle, 1 still working, < 0 the stream itself failed
static int step_query(fr_worker *w) {
    if (w->sh_host_stream && !static_cast<HostStream *>(w->sh_host_stream)->done()) return 1;   // the step is still being issued (host exchange, plain or staged)
    if (w->ctx->cpu) return 0;
    hipError_t q = hipStreamQuery(w->stream);
    if (q == hipSuccess) return 0;
    if (q == hipErrorNotReady) return 1;
    fr_set_error("sharded step: stream failed: %s", hipGetErrorString(q));
    return FR_ERR_HIP;
}
// the transport's asynchronous-error state (polled by the bounded wait): true = the exchange cannot complete any more
static bool step_async_error(fr_comm *comm) {
    if (comm->grp) {
        if (!comm->grp->broken_flag.load(std::memory_order_acquire)) return false;
        fr_set_error("sharded step: the in-process host exchange was aborted (by a peer rank, or by this rank's own step)");
        return true;
    }
    ncclResult_t ar = ncclSuccess;
    if (g_rccl.CommGetAsyncError && comm->comm && g_rccl.CommGetAsyncError(comm->comm, &ar) == ncclSuccess && ar != ncclSuccess && ar != ncclInProgress) {
        fr_set_error("sharded step: RCCL reported an asynchronous error: %s", g_rccl.GetErrorString(ar));
        return true;
    }
    return false;
}

// exchange buffers of a worker: slice [max_batch][F] and gathered [G][max_batch][F] sized for fp32 elements, score chunks
static int shard_buffers(fr_worker *w, int G, bool staged) {
    if (w->sh_ranks == G && w->d_slice && (!staged || w->ctx->cpu || w->h_stage_send)) return FR_OK;
    fr_ctx *c = w->ctx;
    const size_t slice = (size_t)w->max_batch * (size_t)c->slice_padded * sizeof(float);
    const size_t chunk = ((size_t)w->max_batch + G - 1) / G + 1;  // + the rank's status word (failure protocol, kind (2))
    if (G > FR_COMM_MAX_RANKS) FR_FAIL(FR_ERR_INVALID, "%d ranks: the status words of a sharded step hold %d", G, FR_COMM_MAX_RANKS);
    // (sh_ranks is set last: a call that failed half-way is run again, and every alloc releases what the first one made)
    const FrMem pinned = fr_mem_kind(c, FrMem::PINNED), device = fr_mem_kind(c, FrMem::DEVICE);
    FR_TRY(w->h_sh_status.grow(pinned, 1 + FR_COMM_MAX_RANKS, "status words"));   // [0] sent, [1 .. G] received
    FR_TRY(w->d_slice.alloc(device, slice, "exchange slice"));
    FR_TRY(w->d_gathered.alloc(device, slice * G, "exchange slices of all ranks"));
    FR_TRY(w->d_score_part.alloc(device, chunk, "exchange score chunk"));
    FR_TRY(w->d_score_all.alloc(device, chunk * G, "exchange score chunks of all ranks"));
    if (staged && !c->cpu) {   // the staged exchange of GPU contexts that share a device: one part out, G parts in, through pinned host memory
        const size_t part = slice > chunk * sizeof(float) ? slice : chunk * sizeof(float);
        FR_TRY(w->h_stage_send.alloc(FrMem::PINNED, part, "exchange staging (send)"));
        FR_TRY(w->h_stage_recv.alloc(FrMem::PINNED, part * G, "exchange staging (receive)"));
    }
    w->sh_ranks = G;
    return FR_OK;
}

// kind (1) of the failure protocol: nothing has been enqueued, the communicator is untouched
static int sharded_check_args(fr_worker *w, fr_comm *comm, int batch) {
    if (!w || !comm) FR_FAIL(FR_ERR_INVALID, "NULL argument");
    fr_ctx *c = w->ctx;
    if (comm->ctx != c) FR_FAIL(FR_ERR_INVALID, "the communicator belongs to another context");
    if (batch <= 0 || batch > w->max_batch) FR_FAIL(FR_ERR_INVALID, "batch %d outside (0, max_batch=%d]", batch, w->max_batch);
    if (!c->tables_filled) FR_FAIL(FR_ERR_STATE, "tables have not been filled or uploaded");
    if (!c->weights_set) FR_FAIL(FR_ERR_STATE, "FC weights have not been set");
    if (w->in_flight || w->sh_comm) FR_FAIL(FR_ERR_STATE, "a batch is already in flight on this worker: call fr_worker_sync first");
    return FR_OK;
}

// What the first line of a step gathers: the one-hot rows of fr_worker_submit_sharded (`pooled` false: batch, idx and dense alone count), or a pooled batch
// in the padded or the offsets (CSR) form (fr_worker_submit_sharded_pooled[_csr]).  The submit states batch, need_weights (a weighted step) and, in the
// offsets form, the pinned offsets with their nnz; sharded_prologue fills in where the gather reads the rest.
struct ShBatch {
    FrPooledBatch b;
    bool pooled = false;
};

// buffers + the request's H2D copies: a failure here is a device failure (kind (3)).  A CPU worker's "device" rows are its host rows.
// Index rows travel to the worker's device index buffer (one-hot: batch x index columns; pooled: batch x P; offsets form: the nnz flat entries -- the
// buffer holds max_batch x max(index columns, P)); a pooled step's weights and offsets are read by the gather in place, from the pinned buffers.
static int sharded_prologue(fr_worker *w, fr_comm *comm, ShBatch *what) {
    fr_ctx *c = w->ctx;
    FrPooledBatch &b = what->b;
    if (!c->cpu) FR_HIP(hipSetDevice(c->device));
    int rc = shard_buffers(w, comm->n_ranks, comm->grp != nullptr);
    if (rc) return rc;
    b.weights = b.need_weights ? w->h_pool_w.p : nullptr;
    b.idx = c->cpu ? w->h_idx : w->d_idx;
    b.dense = c->cpu ? w->h_dense : w->d_dense;
    if (c->cpu) return FR_OK;
    const size_t n_idx = !what->pooled ? (size_t)b.batch * idx_cols(c) : !b.offsets ? (size_t)b.batch * (size_t)c->pool_cols : (size_t)b.nnz;
    if (n_idx) rc = step_copy(w, w->d_idx, w->h_idx, n_idx * sizeof(int32_t), hipMemcpyHostToDevice);
    if (!rc && c->model.dense_len) rc = step_copy(w, w->d_dense, w->h_dense, (size_t)b.batch * c->model.dense_len * sizeof(float), hipMemcpyHostToDevice);
    return rc;
}

// the slice gather of a step: one-hot rows, or a pooled batch -- every form in the transport type, item-major
static int sharded_gather(fr_worker *w, const ShBatch &what, void *d_slice, int transport) {
    const FrPooledBatch &b = what.b;
    if (!what.pooled) return fr_worker_gather_slices(w, b.batch, b.idx, b.dense, d_slice, transport);
    if (b.offsets) return fr_worker_gather_slices_pooled_csr(w, b.batch, b.offsets, b.idx, b.nnz, b.weights, b.dense, d_slice, transport);
    return fr_worker_gather_slices_pooled(w, b.batch, b.idx, b.weights, b.dense, d_slice, transport);
}

// THE STEP, on either transport: slice gather -> all-gather (or all-to-all: `mode`) of the slices -> FC chain on this rank's items -> all-gather of the score
// chunks (each followed by its rank's status word) -> every rank's pinned score buffer.  A GPU worker's fr_worker_submit_sharded calls it
// inline (every line enqueues on the worker's stream); a host-exchange worker's (CPU, or staged GPU) posts it to the worker's host stream.  *enqueued is set once the
// second collective is on its way: from then on fr_worker_sync has something to wait for, whatever this function returns.
static int sharded_step(fr_worker *w, fr_comm *comm, int mode, ShBatch what, bool *enqueued) {
    *enqueued = false;
    const int batch = what.b.batch;
    int rc = sharded_prologue(w, comm, &what);        // from here on: whatever fails aborts the communicator (kind (3))
    if (rc) return comm_fail(comm, rc);
    fr_ctx *c = w->ctx;
    const int G = comm->n_ranks, r = comm->rank;
    const int transport = c->fc_precision;  // slices travel in the chain's own operand type: fp32, bf16 (half) or e4m3 (a quarter of the bytes)
    const size_t esz = transport == FR_FC_FP32 ? 4 : (transport == FR_FC_BF16 ? 2 : 1);
    rc = sharded_gather(w, what, w->d_slice, transport);
    if (rc) return comm_fail(comm, rc);
    const size_t row = (size_t)c->slice_padded * esz;
    const bool a2a = mode == FR_EXCHANGE_ALLTOALL;
    rc = a2a ? step_all_to_all(w, comm, w->d_slice, w->d_gathered, batch, row) : step_all_gather(w, comm, w->d_slice, w->d_gathered, (size_t)batch * row);
    if (rc) return comm_fail(comm, rc);
    const int base = batch / G, rem = batch % G, chunk = base + (rem ? 1 : 0);
    const int lo = r * base + (r < rem ? r : rem), n_mine = base + (r < rem ? 1 : 0);
    comm->x_received.store((uint64_t)(G - 1) * (uint64_t)(a2a ? n_mine : batch) * row, std::memory_order_relaxed);
    comm->x_sent.store((a2a ? (uint64_t)(batch - n_mine) : (uint64_t)(G - 1) * (uint64_t)batch) * row, std::memory_order_relaxed);
    int fc_rc = FR_OK;
    if (n_mine > 0) {
        w->in_flight = false;  // fr_worker_fc_from_slices_lp is a public entry point with its own state checks
        // all-to-all: d_gathered holds only this rank's items ([G][n_mine][P]), so they are items [0, n_mine) of a batch of n_mine
        fc_rc = a2a ? fr_worker_fc_from_slices_lp(w, n_mine, 0, n_mine, w->d_gathered, transport, w->d_score_part)
                    : fr_worker_fc_from_slices_lp(w, batch, lo, n_mine, w->d_gathered, transport, w->d_score_part);
        const int inject = FR_KNOB("SHARDED_INJECT_FC_FAIL", 0);   // experiments build only: the test of kind (2).  1 = every rank, 2 + q = rank q only
        if (!fc_rc && (inject == 1 || inject == 2 + r)) {
            fr_set_error("injected FC failure (FR_SHARDED_INJECT_FC_FAIL)");
            fc_rc = FR_ERR_STATE;
        }
        if (!fc_rc && w->sh_inject_fc_fail.load(std::memory_order_relaxed) > 0) {   // the product build's test hook (fleetrec_diag.h)
            w->sh_inject_fc_fail.fetch_sub(1, std::memory_order_relaxed);
            fr_set_error("injected FC failure (fr_worker_inject_fc_failure)");
            fc_rc = FR_ERR_STATE;
        }
    }
    // kind (2): the second collective is issued whatever the local FC chain returned -- the peers are already on their way into it -- but a
    // failed chain's chunk travels as NaN and its status word says so on every rank
    char fc_text[200] = "";
    if (fc_rc) {
        snprintf(fc_text, sizeof(fc_text), "%s", fr_last_error());
        if (step_fill_ff(w, w->d_score_part, (size_t)chunk * sizeof(float)) != FR_OK) return comm_fail(comm, FR_ERR_HIP);
    }
    w->h_sh_status[0] = (float)fc_rc;
    if (step_copy(w, w->d_score_part + chunk, w->h_sh_status, sizeof(float), hipMemcpyHostToDevice) != FR_OK) {
        fr_set_error("status word H2D failed");
        return comm_fail(comm, FR_ERR_HIP);
    }
    rc = step_all_gather(w, comm, w->d_score_part, w->d_score_all, ((size_t)chunk + 1) * sizeof(float));
    if (rc) return comm_fail(comm, rc);
    *enqueued = true;
    rc = FR_OK;
    rc = step_copy_status(w, G, chunk);           // all G status words ...
    for (int q = 0; q < G && rc == FR_OK; q++) {  // ... and every rank ends up with all B scores in its pinned score buffer
        const int qlo = q * base + (q < rem ? q : rem), qn = base + (q < rem ? 1 : 0);
        if (qn > 0) rc = step_copy(w, w->h_score + qlo, w->d_score_all + (size_t)q * (chunk + 1), (size_t)qn * sizeof(float), hipMemcpyDeviceToHost);
    }
    if (rc != FR_OK) return comm_fail(comm, FR_ERR_HIP);
    w->in_flight = true;
    if (fc_rc) FR_FAIL(fc_rc, "FC chain failed on this rank (its peers learn it from the status word): %s", fc_text);
    return FR_OK;
}

// the checked step, handed to its transport: enqueued inline on the worker's HIP stream (RCCL), or posted to the worker's host stream
static int sharded_submit(fr_worker *w, fr_comm *comm, const ShBatch &what) {
    w->sh_comm = comm;  // fr_worker_sync waits through fr_comm_wait and reads the G status words
    comm->refs.fetch_add(1, std::memory_order_acq_rel);   // (also what fr_comm_set_exchange reads as "a step in flight")
    const int mode = comm->exchange.load(std::memory_order_acquire);
    if (comm->grp) {   // the host exchange (CPU worker, or staged GPU worker): the step runs behind this call on the worker's host stream -- its rendezvous blocks
        host_stream(w)->post([w, comm, mode, what] {
            bool enqueued = false;
            return sharded_step(w, comm, mode, what, &enqueued);
        });
        return FR_OK;
    }
    bool enqueued = false;
    const int rc = sharded_step(w, comm, mode, what, &enqueued);
    if (!enqueued) fr_comm_forget(w);   // kind (3) before the second collective: the communicator is aborted, there is no step to wait for
    return rc;
}

static ShBatch sharded_batch(int batch, bool pooled, bool weighted) {
    ShBatch what{FrPooledBatch{batch}, pooled};
    what.b.need_weights = weighted;
    return what;
}

extern "C" int fr_worker_submit_sharded(fr_worker *w, fr_comm *comm, int batch) {
    if (comm && comm_is_broken(comm)) FR_FAIL(FR_ERR_COMM, FR_BROKEN_TEXT);
    int rc = sharded_check_args(w, comm, batch);  // kind (1): returned as it is
    if (rc) return rc;
    return sharded_submit(w, comm, sharded_batch(batch, false, false));
}

// kind (1) of a pooled step, sharded_check_args included: everything the slice gather would refuse is refused here, before anything is enqueued (inside
// the step a refusal would abort the communicator)
static int sharded_check_pooled(fr_worker *w, fr_comm *comm, int batch, bool weighted, bool csr) {
    if (comm && comm_is_broken(comm)) FR_FAIL(FR_ERR_COMM, FR_BROKEN_TEXT);
    int rc = sharded_check_args(w, comm, batch);
    if (rc) return rc;
    fr_ctx *c = w->ctx;
    if (c->pool_cols <= 0) return fr_pooling_unset(FR_NO_POOLING_SHARDED_STEP);
    if (weighted) rc = fr_pooled_weights_need_sum(c);
    if (rc) return rc;
    if (w->idx_cap < c->pool_cols || (weighted && (!w->h_pool_w || w->pool_w_cap < c->pool_cols)) || (csr && !w->h_pool_off))
        FR_FAIL(FR_ERR_STATE, "the worker lacks the pooled buffers (%d index columns per item, pooled rows have %d): create the worker after the context's pooling is set", w->idx_cap,
                c->pool_cols);
    return FR_OK;
}

extern "C" int fr_worker_submit_sharded_pooled(fr_worker *w, fr_comm *comm, int batch, int weighted) {
    const int rc = sharded_check_pooled(w, comm, batch, weighted != 0, false);
    if (rc) return rc;
    return sharded_submit(w, comm, sharded_batch(batch, true, weighted != 0));
}

extern "C" int fr_worker_submit_sharded_pooled_csr(fr_worker *w, fr_comm *comm, int batch, int weighted) {
    int rc = sharded_check_pooled(w, comm, batch, weighted != 0, true);
    if (rc) return rc;
    ShBatch what = sharded_batch(batch, true, weighted != 0);
    what.b.offsets = w->h_pool_off;
    rc = fr_pooled_host_offsets(w, batch, "fr_worker_submit_sharded_pooled_csr", &what.b.nnz);   // (fr_worker_submit_pooled_csr's rule)
    if (rc) return rc;
    return sharded_submit(w, comm, what);
}

extern "C" int fr_worker_inject_fc_failure(fr_worker *w, int steps) {
    if (!w || steps < 0) FR_FAIL(FR_ERR_INVALID, "bad argument");
    w->sh_inject_fc_fail.store(steps, std::memory_order_relaxed);
    return FR_OK;
}

// fr_worker_sync of a worker with a sharded step in flight: a BOUNDED wait (failure protocol, kind (3)), then the status words (kind (2)).
static int comm_wait_step(fr_worker *w, fr_comm *comm);
int fr_comm_wait(fr_worker *w) {
    fr_comm *comm = w->sh_comm;
    if (!comm) return FR_OK;
    const int rc = comm_wait_step(w, comm);
    w->sh_comm = nullptr;
    comm_release(comm);   // the step's reference; the last one destroys a communicator that fr_comm_destroy has already let go
    return rc;
}

// a host-exchange worker's step has left its host stream: what it returned (kind (3) failures surface here; a kind (2) return is told by the status words)
static int host_step_result(fr_worker *w, fr_comm *comm) {
    HostStream *hs = static_cast<HostStream *>(w->sh_host_stream);
    if (!hs) return FR_OK;
    hs->wait();
    if (hs->rc != FR_OK && comm->broken.load(std::memory_order_acquire)) {
        fr_set_error("%s", hs->text);
        return hs->rc;
    }
    return FR_OK;
}

static int comm_wait_step(fr_worker *w, fr_comm *comm) {
    const int G = comm->n_ranks;
    const bool host = comm->grp != nullptr;
    if (!host && comm->broken.load(std::memory_order_acquire)) FR_FAIL(FR_ERR_COMM, FR_BROKEN_TEXT);
    // poll instead of a blocking wait: a peer that never arrives must not hold this rank for ever
    const int wait_ms = comm->wait_ms.load(std::memory_order_relaxed);
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (unsigned spin = 0;; spin++) {
        const int q = step_query(w);
        if (q == 0) break;
        if (q < 0) return comm_fail(comm, q);
        if ((spin & 63) == 63) {
            bool give_up = step_async_error(comm);
            clock_gettime(CLOCK_MONOTONIC, &t1);
            const double ms = (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6;
            if (!give_up && ms > wait_ms) {
                fr_set_error("sharded step: the collectives did not complete within %d ms (a peer rank is missing): communicator aborted", wait_ms);
                give_up = true;
            }
            if (give_up) {
                char text[400];
                snprintf(text, sizeof(text), "%s", fr_last_error());
                (void)comm_fail(comm, FR_ERR_COMM);
                if (host) static_cast<HostStream *>(w->sh_host_stream)->wait();   // the abort has released the step: it leaves the stream before the worker's buffers may go
                fr_set_error("%s", text);
                return FR_ERR_COMM;
            }
            if (ms > 2.0) {  // long waits sleep between polls
                struct timespec nap = {0, 50000};
                nanosleep(&nap, nullptr);
            }
        }
    }
    if (host) {
        const int rc = host_step_result(w, comm);
        if (rc) return rc;
        if (comm->broken.load(std::memory_order_acquire)) FR_FAIL(FR_ERR_COMM, FR_BROKEN_TEXT);
    }
    for (int q = 0; q < G; q++)
        if (w->h_sh_status[1 + q] != 0.0f)
            FR_FAIL(FR_ERR_COMM, "shard rank %d reported a failed FC chain (status %d): the scores of its items are NaN", q, (int)w->h_sh_status[1 + q]);
    return FR_OK;
}

// fp8 chain on sharded contexts: every rank calibrates on the SAME all-gathered fp32 slices of the whole batch with the same
// (replicated) weights, so all ranks arrive at identical activation exponents without a further reduction.
static int sharded_calibrate(fr_worker *w, fr_comm *comm, ShBatch what) {
    const int batch = what.b.batch;
    int rc = sharded_prologue(w, comm, &what);
    if (rc) return comm_fail(comm, rc);
    fr_ctx *c = w->ctx;
    rc = sharded_gather(w, what, w->d_slice, FR_FC_FP32);   // (fp32: fr_worker_gather_only / fr_worker_gather_pooled[_weighted])
    if (rc) return comm_fail(comm, rc);
    rc = step_all_gather(w, comm, w->d_slice, w->d_gathered, (size_t)batch * c->slice_padded * sizeof(float));
    if (rc) return comm_fail(comm, rc);
    w->in_flight = false;
    return fr_worker_calibrate_fp8_slices(w, batch, 0, batch, reinterpret_cast<const float *>(w->d_gathered.p));
}

extern "C" int fr_worker_calibrate_fp8_sharded(fr_worker *w, fr_comm *comm, int batch) {
    if (w && w->ctx) FR_NOT_ON_CPU(w->ctx, "fr_worker_calibrate_fp8_sharded");
    if (comm && comm_is_broken(comm)) FR_FAIL(FR_ERR_COMM, FR_BROKEN_TEXT);
    int rc = sharded_check_args(w, comm, batch);
    if (rc) return rc;
    return sharded_calibrate(w, comm, sharded_batch(batch, false, false));
}

// The pooled sibling (padded form): the calibration sees the BAGS -- a SUM over a 16-slot bag can be many times a single row, and the X exponent
// leaves one binade of headroom, so an fp8 job calibrated on one-hot rows clips its pooled operand.
extern "C" int fr_worker_calibrate_fp8_sharded_pooled(fr_worker *w, fr_comm *comm, int batch, int weighted) {
    if (w && w->ctx) FR_NOT_ON_CPU(w->ctx, "fr_worker_calibrate_fp8_sharded_pooled");
    const int rc = sharded_check_pooled(w, comm, batch, weighted != 0, false);
    if (rc) return rc;
    return sharded_calibrate(w, comm, sharded_batch(batch, true, weighted != 0));
}
