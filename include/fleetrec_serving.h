/*
 * fleetrec_serving.h -- serving extensions: host-fed streaming with pinned staging blocks, replies, adaptive batching.
 *
 * None of this is needed to replace the reference's loop (fr_worker_submit + fr_worker_sync per batch does that, fleetrec.h); it is what
 * a server that feeds the GPU from sockets at the GPU's own rate uses (host/fleetrec_server.cpp --stream [--reply]).
 *
 * Part of the C-ABI of the MI355X-native FleetRec hot path; include/fleetrec.h is the boundary proper (the three spans of
 * thread_consume(), cuda_server.c:110-354,460-495, that SURVEY section 8(b) cuts).  Same conventions: plain C, opaque handles,
 * FR_OK or a negative fr_status, fr_last_error() for the text.  Citations are path:line under the reference tree (see fleetrec.h).
 */
#ifndef FLEETREC_SERVING_H
#define FLEETREC_SERVING_H

#include "fleetrec.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* n consecutive fr_worker_push_device calls in one: batch[i], d_idx[i], d_dense[i] (the array or any entry may be NULL for a model
 * without dense features), d_scores[i] for i = 0 .. n-1, in that order, stopping at the first error (its status is returned; the
 * batches before it stay pushed).  For callers whose per-call cost is comparable to a batch's share of a launch -- a language
 * binding feeding 256 batches of a 0.5 us share each -- so that the stream, not the caller, sets the pace (bench.py's one-stream
 * roofline legs).  Same buffer-lifetime rule as fr_worker_push_device.  The reference's loop is the n = 1 case (cuda_server.c:406-497). */
int fr_worker_push_device_list(fr_worker *w, int n, const int *batch, const int32_t *const *d_idx, const float *const *d_dense,
                               float *const *d_scores);
/* Host-fed streaming: like fr_worker_push_device for a batch that sits in (any) host memory.  The rows are copied into the worker's
 * pinned staging before the call returns (h_idx / h_dense may be reused at once); batches travel in blocks: ONE H2D copy on the worker's
 * copy stream (issued when the block is full, while the previous block's kernel still runs) + ONE launch whose output layer writes the
 * scores straight into pinned memory -- the worker's own stream carries nothing but kernels (round 5; rounds 2-4 issued H2D, launch and
 * D2H as three commands of that stream and lost 5 % to it: profiles/r05_host_fed_timeline.txt).  h_scores[0..batch) is valid after
 * fr_worker_sync (earlier deliveries happen -- a block's scores are copied out before its staging is reused, i.e. at the latest 4 blocks
 * later -- but fr_worker_sync is the only completion point the API defines).  Feed it from at most four streaming workers per context
 * (one worker stream per hardware queue).  The streaming counterpart of the per-batch recv -> H2D -> GEMMs -> D2H sequence of
 * cuda_server.c:425-495. */
int fr_worker_push_host(fr_worker *w, int batch, const int32_t *h_idx, const float *h_dense, float *h_scores);
/* The same without the copy into staging -- the reference's read() lands in pinned memory (cuda_server.c:136-160,437):
 * fr_worker_stage_acquire hands out where the NEXT pushed batch of this worker has to be written (*h_idx: batch x index_cols int32,
 * *h_dense: batch x dense_len floats or NULL; pinned, owned by the worker; it may first wait for the oldest block's scores and deliver
 * them, exactly as fr_worker_push_host does), the caller fills it (e.g. reads the socket into it), fr_worker_push_staged queues it
 * (batch <= the acquired size; h_scores as for fr_worker_push_host).  One slot at a time per worker; fr_worker_push_host between the
 * two calls is FR_ERR_STATE; fr_worker_sync drops a slot that was acquired and never pushed. */
int fr_worker_stage_acquire(fr_worker *w, int batch, int32_t **h_idx, float **h_dense);
int fr_worker_push_staged(fr_worker *w, int batch, float *h_scores);
/* Serving with replies (fleetrec_server --stream --reply): fr_worker_flush launches what is queued on the worker right now -- a
 * partially filled host block, queued device pushes -- without waiting (the latency knob under light load: call it when the request
 * source runs dry); fr_worker_host_poll delivers the scores of the host-fed blocks that have FINISHED (oldest first, no waiting) and
 * reports how many host-fed batches have been delivered since the worker was created: batches are delivered in push order, so the
 * caller knows exactly which h_scores buffers are valid. */
int fr_worker_flush(fr_worker *w);
/* Latency of nearly empty host-fed blocks, PER CONTEXT: a block that leaves with at most max_batches batches (0..8; default 0 = never) rides
 * the stage pipeline of fr_worker_submit -- its n batches follow each other through the five stage launches, n + 4 launches of ~10 us,
 * the whole chip per layer -- instead of the fused item-tile kernel (133 us for any number of batches up to a chip-full).  Such batches
 * get fr_worker_submit's scores bit for bit (the fused kernel sums in another order: equal to ~1e-6, not bit for bit).
 * fleetrec_server --stream --reply sets 8 (4 requests in flight per connection: 18 M inferences/s at 185 us request -> reply, against
 * 14 M at 245 us with five launches per batch; profiles/archive/r02_tcp_reply_small_blocks.txt). */
int fr_ctx_set_small_block(fr_ctx *ctx, int max_batches);
int fr_worker_host_poll(fr_worker *w, long long *delivered);
/* Host-fed batches queued in the block being filled (not launched yet) / launched and not delivered yet, and the number of launched
 * blocks not delivered yet (at most 4) -- what an adaptive batcher needs: flush when the request source is dry AND at most one block is
 * still in flight; while more are running, let the next block fill (any output pointer may be NULL). */
int fr_worker_host_pending(const fr_worker *w, int *queued, int *in_flight, int *blocks_in_flight);
/* Host-buffer STREAMING form: the same host-resident request stream handed to fr_worker_push_host (pinned staging blocks, one
 * H2D + one fused launch per block, scores written to pinned memory by the kernel, no per-batch synchronisation).  Only for models that stream through the fused
 * item-tile kernel.  Scores land in per-worker host rings (fr_driver_host_score_ring, same indexing as fr_driver_score_ring). */
int fr_driver_run_host_streaming(fr_driver *d, int batch, int64_t total_batches, const int32_t *const *h_idx_pool,
                                 const float *const *h_dense_pool, int n_pool, double *elapsed_s);
const float *fr_driver_host_score_ring(fr_driver *d, int thread, int slot, int *ring_len);

/* Exchange mode of a table-sharded communicator (fr_exchange, fleetrec.h): how fr_worker_submit_sharded ships the slices.  Set between
 * steps, the same mode on every rank of the communicator: FR_ERR_INVALID for an unknown mode, FR_ERR_STATE while a step is in flight
 * through this handle (submitted, not yet synchronised), FR_ERR_COMM on a broken communicator or -- ALLTOALL over RCCL -- a librccl.so
 * without ncclSend / ncclRecv / ncclGroupStart / ncclGroupEnd.  Ranks of a host exchange whose modes disagree break the group: every rank's
 * fr_worker_sync returns FR_ERR_COMM (over RCCL such a job does not match its collectives: the bounded wait of fr_worker_sync ends it). */
int fr_comm_set_exchange(fr_comm *c, int exchange);   /* between steps; every rank of the communicator sets the same mode */
int fr_comm_exchange(const fr_comm *c);               /* the current mode (FR_EXCHANGE_ALLGATHER after init) */

/* Multi-hot pooled lookups (additive in ABI 6).  Pooling is described per index COLUMN of the context's index mode: hots[c] (1 ..
 * FR_POOL_MAX_HOTS) slots for column c < fr_model_index_cols(model) -- FR_INDEX_PER_TABLE: a bag per table; FR_INDEX_PER_BANK: a bag of bank-row
 * indices per bank (every table of the bank is pooled with the same bag); FR_INDEX_PER_ITEM: one bag reused for every table.  The pooled
 * index row of an item is int32 idx[P], P = sum of hots, ordered by column, slot-minor: column c's slots are idx[prefix[c] + j], j < hots[c],
 * prefix = the exclusive prefix sum of hots.  A slot of -1 is EMPTY; any other negative value, or one >= the row count the one-hot gather checks,
 * is FR_ERR_INDEX_RANGE at fr_worker_sync (the slot reads row 0).  Every TABLE and COPY word of the record becomes the pooled value of its
 * column's bag: the first non-empty slot's row word as a bit copy, every further non-empty slot's word added to it in fp32, one add per lane,
 * in ascending slot order; an all-empty bag gives +0.0f.  DENSE words are copied as by the one-hot gather.  With every hots == 1 and no empty
 * slot the records are bit-identical to fr_worker_gather_only's.  Records are fp32 in the model's layout; the FC chain is the one
 * fr_worker_fc_only runs from records, in the context's precision.  Sharded contexts: pooling is stated at creation (fr_ctx_create_sharded_pooled, below), never by fr_ctx_set_pooling.  Streaming: the
 * fr_worker_push_pooled* entry points below; the fused kernels' producers and the host-fed path (fr_worker_push_host / push_staged) stay
 * one-hot.  An index or record buffer of 4000 MiB or more is FR_ERR_INVALID (32-bit buffer offsets). */
#define FR_POOL_MAX_HOTS 64
/* hots[n_cols], n_cols == fr_model_index_cols(fr_ctx_model(ctx)); hots == NULL clears.  Builds the pooled descriptors.
 * FR_ERR_STATE while a worker of the context has work in flight, or on a sharded context (its pooling is fixed at creation).  One-hot entry points are unaffected.
 * Like the other fr_ctx_set_* calls it is not to be raced against calls on the context's workers. */
int fr_ctx_set_pooling(fr_ctx *ctx, const int32_t *hots, int n_cols);
int fr_ctx_pooled_index_cols(const fr_ctx *ctx);          /* P; 0 when no pooling is set */
/* d_idx int32 [batch][P]; d_records as for fr_worker_gather_only.  Asynchronous; follow with fr_worker_sync. */
int fr_worker_gather_pooled(fr_worker *w, int batch, const int32_t *d_idx, const float *d_dense, float *d_records);
/* fr_worker_gather_pooled into the worker's record buffer, then the FC chain from those records. */
int fr_worker_submit_pooled_device(fr_worker *w, int batch, const int32_t *d_idx, const float *d_dense, float *d_scores);
/* Host form: the worker's pinned idx buffer holds [batch][P]; scores in fr_worker_score_ptr.  A worker created AFTER
 * fr_ctx_set_pooling sizes its pinned and device index buffers for max(index_cols, P); an older worker gets FR_ERR_STATE here. */
int fr_worker_submit_pooled(fr_worker *w, int batch);

/* Pooling modes and per-sample weights (additive in ABI 6).  Every index column has a pooling mode: FR_POOL_SUM (the default: the fold above)
 * or FR_POOL_MEAN.  A MEAN column's TABLE and COPY words are the SUM fold of the bag divided by n, the number of non-empty slots of the bag:
 * one IEEE fp32 division, correctly rounded, per lane, n converted exactly; n == 1 leaves the word the bit copy it is (no division), n == 0
 * gives +0.0f.  DENSE words are never divided.  MEAN takes effect through the unweighted pooled entry points above.
 * modes[n_cols], n_cols == fr_model_index_cols; modes == NULL makes every column SUM again, and so does every fr_ctx_set_pooling (also with
 * NULL).  FR_ERR_STATE when no pooling is set, on a sharded context (its modes are fixed at creation), or while a worker of the context has work in flight (the rule of
 * fr_ctx_set_pooling); FR_ERR_INVALID for a wrong n_cols or an unknown mode.  The pooled descriptors are rebuilt and uploaded again. */
#define FR_POOL_SUM 0
#define FR_POOL_MEAN 1
int fr_ctx_set_pooling_modes(fr_ctx *ctx, const int32_t *modes, int n_cols);
int fr_ctx_pooling_mode(const fr_ctx *ctx, int col);      /* the mode of index column col (FR_POOL_SUM when no pooling is set) */
/* Per-sample weights: float d_weights[batch][P], parallel to the pooled index rows -- the weight of a slot sits where the slot sits.  For a
 * non-empty slot the term is w * x: one fp32 multiply per lane, rounded to fp32, never fused with the add that follows.  The FIRST non-empty
 * slot's term becomes the accumulator (in the weighted fold the first word is NOT a bit copy); every further term is added in fp32, in
 * ascending slot order, one add per lane.  The weight of an empty slot is never read into arithmetic (it may be a NaN and does not show); an
 * all-empty bag gives +0.0f; DENSE words are copied unweighted; COPY words follow their source column's bag and weights.  Bits are pinned for
 * every result that is not a NaN (a NaN result is a NaN of unspecified payload); with every weight 1.0f the records equal the unweighted ones
 * bit for bit wherever no row word is a NaN.  Weights are legal only while every column's mode is FR_POOL_SUM: FR_ERR_STATE on a context
 * with a MEAN column.  d_weights == NULL is FR_ERR_INVALID.  Index-range errors, the 4000 MiB bound (the weight array is as large as the index
 * rows) and the behaviour on a sharded context are those of the unweighted calls, which behave exactly as before. */
int fr_worker_gather_pooled_weighted(fr_worker *w, int batch, const int32_t *d_idx, const float *d_weights, const float *d_dense, float *d_records);
int fr_worker_submit_pooled_weighted_device(fr_worker *w, int batch, const int32_t *d_idx, const float *d_weights, const float *d_dense, float *d_scores);
/* Host form: indices in fr_worker_idx_ptr, weights in fr_worker_pool_weights_ptr -- pinned float [max_batch][P] (host memory on the CPU
 * back-end), there on a worker created AFTER fr_ctx_set_pooling; NULL on an older worker, where the host form returns FR_ERR_STATE. */
float *fr_worker_pool_weights_ptr(fr_worker *w);
int fr_worker_submit_pooled_weighted(fr_worker *w, int batch);

/* Offsets-form (CSR) pooled lookups (additive in ABI 6): a second INPUT form of the pooled lookups above -- what a caller holding
 * `indices + offsets` (EmbeddingBag(offsets=...), a table-batched embedding) has.  Pooling is configured as above (fr_ctx_set_pooling, optionally
 * fr_ctx_set_pooling_modes); here hots[c] is the CAP of column c: the longest bag the column may carry.  C = fr_model_index_cols(model).  A context
 * may use the padded and the offsets entry points side by side.
 *   offsets  int32 [batch * C + 1], item-major, column-minor: bag (b, c) is indices[offsets[b * C + c] .. offsets[b * C + c + 1])
 *   indices  int32 [nnz];  weights (optional) float [nnz], parallel to indices.  Only 4-byte alignment of the three arrays is assumed.
 * An entry of -1 is an empty slot, as in the padded form.  Every TABLE and COPY word is the fold defined above over the bag's entries in
 * ascending position: SUM, MEAN over the non-empty entries, or (weights != NULL) the weighted sum with each product rounded on its own; an empty
 * bag (start == end, or only -1s) gives +0.0f; DENSE words are copied.  The records equal, BIT FOR BIT, those of the padded entry points on the same
 * context for the same bags padded with -1 up to hots[c] (weights padded with anything).
 * A bag is MALFORMED when start < 0, end < start, end > nnz, end - start > hots[c], or an entry is < -1 or >= the row count the one-hot gather
 * checks: FR_ERR_INDEX_RANGE at fr_worker_sync (sticky word, the worker is usable afterwards).  The malformed bag's own record words are
 * unspecified, every other bag's are as specified, and no byte outside offsets[0 .. batch * C], indices[0 .. nnz), weights[0 .. nnz), the tables
 * and the record buffer is read or written.
 * nnz == 0 is legal (indices / weights may then be NULL).  FR_ERR_INVALID: nnz < 0, offsets == NULL, indices == NULL with nnz > 0, or
 * (batch * C + 1) * 4, nnz * 4 or the record bytes reaching 4000 MiB (32-bit buffer offsets).  FR_ERR_STATE: weights on a context with a MEAN
 * column, no pooling set, a submit on a sharded context -- the rules of the padded calls.  weights == NULL means unweighted: one entry point per shape. */
int fr_worker_gather_pooled_csr(fr_worker *w, int batch, const int32_t *d_offsets, const int32_t *d_indices, int64_t nnz,
                                const float *d_weights /* NULL: unweighted */, const float *d_dense, float *d_records);
int fr_worker_submit_pooled_csr_device(fr_worker *w, int batch, const int32_t *d_offsets, const int32_t *d_indices, int64_t nnz,
                                       const float *d_weights, const float *d_dense, float *d_scores);
/* Host form: offsets in fr_worker_pool_offsets_ptr -- pinned int32 [max_batch * C + 1] (host memory on the CPU back-end), NULL on a worker created
 * before fr_ctx_set_pooling, where the host form returns FR_ERR_STATE; indices flat in fr_worker_idx_ptr (its max_batch x max(index cols, P) ints
 * always hold nnz <= batch x P), weights flat in fr_worker_pool_weights_ptr (read when weighted != 0).  nnz = offsets[batch * C], read on the host:
 * offsets[0] != 0 or nnz outside [0, batch x P] is FR_ERR_INVALID before anything is enqueued; the per-bag checks remain the gather's.  Order
 * against fr_worker_update_rows is that of the padded pooled calls. */
int32_t *fr_worker_pool_offsets_ptr(fr_worker *w);
int fr_worker_submit_pooled_csr(fr_worker *w, int batch, int weighted);

/* Streaming pushes of pooled lookups (additive in ABI 6): fr_worker_push_device for a pooled batch, in the padded and the offsets input form.
 * Nothing waits: the pooled gather writes the FC chain's first operand itself, in the chain's operand type, and the batch enters the stage
 * pipeline behind it -- its FC1 shares a launch with FC2 / FC3 / the output layer of the batches pushed before it.  A pooled push always rides the
 * stage pipeline, also on a context whose one-hot pushes go through the fused kernel (launch groups of 12 or more).
 *   d_weights NULL: the unweighted fold (SUM / MEAN by the context's modes); non-NULL: the weighted fold (FR_ERR_STATE on a context with a MEAN
 *   column).  Arguments, ranges and malformed bags: the rules of fr_worker_submit_pooled*_device / fr_worker_submit_pooled_csr_device.
 *   Scores: those of fr_worker_submit_pooled*_device for the same batch, BIT FOR BIT, in every precision (the same stage kernels over the same
 *   operand bytes).  fr_worker_sync is the only completion point; the buffer-lifetime rule of fr_worker_push_device applies -- d_idx / d_offsets /
 *   d_indices / d_weights / d_dense / d_scores stay valid, and d_scores distinct, for every batch still in the pipeline.
 *   One-hot and pooled pushes may alternate on one worker: batches fr_worker_push_device has queued for a fused launch are launched first (not
 *   waited for), a later one-hot push that goes fused drains the stage pipeline first.  Order against fr_worker_update_rows is the one stated
 *   there (a batch's gather is launched by its own push).  fr_ctx_set_pooling / fr_ctx_set_pooling_modes see pushed batches as work in flight.
 *   An index-range error (or a malformed bag) is FR_ERR_INDEX_RANGE at fr_worker_sync: sticky word, the worker is usable afterwards, every
 *   well-formed bag of every pushed batch is as specified.
 *   FR_ERR_STATE: no pooling set, a sharded context (fr_worker_submit_sharded_pooled is its step), a layout other than FR_LAYOUT_SEMANTIC, host-fed batches still queued in a block (flush
 *   first, as for fr_worker_update_rows).  The CPU back-end computes a push before it returns.
 *   Speed, not results: on a bf16 / fp8 chain two shapes of the gather keep the record round trip inside the push (one launch more, the same scores) --
 *   every bag of ONE slot, and a longest bag of 4 .. 7 slots unless every hots[c] is a multiple of 4 AND d_idx / d_weights are 16-byte aligned (the
 *   offsets form at those caps always: it assumes 4-byte alignment only).  Keep pooled index rows and weights 16-byte aligned.
 * fr_worker_push_pooled_device_list: n pushes in one call, stopping at the first error -- the pooled sibling of fr_worker_push_device_list
 * (padded form; the d_weights / d_dense arrays or any entry of them may be NULL). */
int fr_worker_push_pooled_device(fr_worker *w, int batch, const int32_t *d_idx, const float *d_weights /* NULL: unweighted */, const float *d_dense,
                                 float *d_scores);
int fr_worker_push_pooled_csr_device(fr_worker *w, int batch, const int32_t *d_offsets, const int32_t *d_indices, int64_t nnz,
                                     const float *d_weights /* NULL: unweighted */, const float *d_dense, float *d_scores);
int fr_worker_push_pooled_device_list(fr_worker *w, int n, const int *batch, const int32_t *const *d_idx, const float *const *d_weights,
                                      const float *const *d_dense, float *const *d_scores);

/* Pooled lookups on table-sharded contexts (additive in ABI 6).  A sharded context's pooling is fixed WHEN THE CONTEXT IS CREATED and cannot be changed
 * afterwards: every rank of a job must agree on the pooled row layout, exchange and worker buffers are sized once, and no rank may re-describe its bags
 * while a peer is inside a step.  fr_ctx_create_sharded_pooled is fr_ctx_create_sharded followed by the installation of the pooled descriptors, which
 * follow the shard's own words.  hots / modes (NULL: every column SUM) / n_cols have the length, range and meaning of fr_ctx_set_pooling[_modes]: the
 * GLOBAL index columns of the model's index mode, the same arrays on every rank (FR_ERR_INVALID for a wrong n_cols, a NULL hots, a value out of range:
 * no context is returned).  The pooled index row of an item is the whole [P] row on every rank, exactly as every rank receives the whole one-hot index
 * row; a shard reads only the bags of its own words.  n_shards == 1 gives a plain context with pooling set.  On the resulting context
 * fr_ctx_set_pooling / fr_ctx_set_pooling_modes keep returning FR_ERR_STATE when n_shards > 1, the getters answer, one-hot entry points are unaffected and
 * workers get the pooled buffer sizes.  The existing pooled entry points then behave as their one-hot siblings do on a shard: fr_worker_gather_pooled*
 * writes the shard's fp32 slice [batch][slice_padded] as fr_worker_gather_only does; fr_worker_submit_pooled* and fr_worker_push_pooled* stay
 * FR_ERR_STATE (the chain needs the all-gathered slices), with nothing enqueued.  A sharded context created WITHOUT pooling answers as before. */
int fr_ctx_create_sharded_pooled(const fr_model_desc *m, int device, int shard_rank, int n_shards, const int32_t *hots, const int32_t *modes /* NULL: every column SUM */,
                                 int n_cols, fr_ctx **out);
/* The pooled siblings of fr_worker_gather_slices: [batch][slice_padded] elements of `transport` (FR_FC_FP32, FR_FC_BF16, FR_FC_FP8 = e4m3 of x * 2^e of the
 * context's X exponent), item-major; every element is the pooled fold defined above (SUM, MEAN, weighted; the offsets form with its malformed-bag rules),
 * rounded with the one-hot slice gather's own rounding.  Legal on an unsharded context too, where the slice is the whole record.  Nothing past
 * batch x slice_padded elements is written.  Arguments, ranges, alignment and the 4000 MiB bounds: fr_worker_gather_pooled[_weighted] /
 * fr_worker_gather_pooled_csr (d_weights NULL: unweighted); transport: the rules of fr_worker_gather_slices (the CPU back-end: fp32 only, FR_ERR_STATE
 * otherwise).  Speed, not results: with a low-precision transport a longest bag of ONE slot, and one of 4 .. 7 slots in the narrow form (see the
 * streaming pushes), run through the neighbouring shape of the gather kernel that carries the store (fr_worker_last_kernel names it). */
int fr_worker_gather_slices_pooled(fr_worker *w, int batch, const int32_t *d_idx, const float *d_weights /* NULL: unweighted */, const float *d_dense, void *d_slice,
                                   int transport);
int fr_worker_gather_slices_pooled_csr(fr_worker *w, int batch, const int32_t *d_offsets, const int32_t *d_indices, int64_t nnz, const float *d_weights, const float *d_dense,
                                       void *d_slice, int transport);
/* fr_worker_submit_sharded with its first line replaced by the pooled slice gather: slice gather (pooled) -> exchange -> FC on this rank's items ->
 * score all-gather; both exchange modes, all three transports, the uneven item split, the status words, the bounded wait and the byte accounting of
 * fr_comm_exchange_bytes are those of fr_worker_submit_sharded.  Inputs are the host forms of the pooled calls: indices in fr_worker_idx_ptr ([batch][P];
 * the offsets form: flat), weights in fr_worker_pool_weights_ptr when weighted != 0, offsets in fr_worker_pool_offsets_ptr (offsets[0] != 0 or nnz =
 * offsets[batch * C] outside [0, batch x P]: FR_ERR_INVALID before anything is enqueued).  The index entries are copied to the worker's device index
 * buffer (sized at worker creation); the device reads the pinned WEIGHTS and OFFSETS IN PLACE, so all the worker's pinned buffers stay untouched until
 * fr_worker_sync has returned.  Errors found before anything is enqueued (kind (1) of the step's failure protocol, the communicator stays usable): no
 * pooling on the context, weighted with a MEAN column, a worker without the pooled buffers -- all FR_ERR_STATE.  An index-range error or a malformed bag is
 * reported as the one-hot step reports an out-of-range index: FR_ERR_INDEX_RANGE at fr_worker_sync of the rank(s) whose words read it; every rank's step
 * completes. */
int fr_worker_submit_sharded_pooled(fr_worker *w, fr_comm *comm, int batch, int weighted);
int fr_worker_submit_sharded_pooled_csr(fr_worker *w, fr_comm *comm, int batch, int weighted);
/* fr_worker_calibrate_fp8_sharded on a pooled batch (padded host form): the fp32 slices are pooled, so the activation exponents see the bags -- a SUM over
 * a 16-slot bag can be many times a single row, and a job calibrated on one-hot rows would clip its pooled operand at +-448.  A synchronous collective
 * (one thread per rank on the host exchange); identical exponents on every rank. */
int fr_worker_calibrate_fp8_sharded_pooled(fr_worker *w, fr_comm *comm, int batch, int weighted);

/* Sparse row updates of the embedding tables (additive in ABI 6): the write side of the lookups.  n listed rows of ONE table: row_ids int32 [n],
 * rows float [n][dim], dense -- row i of `rows` is the new content of table row row_ids[i].  Unlike fr_ctx_upload_table these are not set-up
 * calls: they run beside streams in flight, leave an operand-type bank image current (its listed rows are converted again in place, from the
 * fp32 arena, at the image's X exponent -- nothing is rebuilt) and touch neither tables_filled nor pooling or FC state.
 * fr_worker_update_rows: device pointers (host pointers on the CPU back-end, which computes before it returns), asynchronous on the worker's
 * stream; d_row_ids and d_rows (16-byte aligned) stay valid and untouched until fr_worker_sync(w) has returned.
 *   Order on the worker: every batch submitted or pushed on w BEFORE the call gathers the old rows, every batch submitted or pushed on w AFTER
 *   it the new ones -- one-hot and pooled entry points alike.  Batches fr_worker_push_device has queued for a fused launch are launched first
 *   (not waited for), as fr_worker_sync does before it waits; the stage pipeline needs no draining (a batch's gather is launched by its own
 *   push).  Host-fed batches still queued in a block (fr_worker_push_host / push_staged) make the call FR_ERR_STATE: flush first.
 *   Across workers and contexts there is no order until fr_worker_sync(w) has returned; from then on every batch submitted on any worker of
 *   the context sees the new rows.  A batch in flight on another worker meanwhile reads, per 16-byte row word, the old or the new word --
 *   each word whole, rows not atomic across words.  (Visibility is that of kernel boundaries; no cache-control instruction is involved.)
 *   Range: an id < 0 or >= the table's rows is FR_ERR_INDEX_RANGE at fr_worker_sync (the worker's sticky error word); that id writes nothing,
 *   every in-range id of the call is still written.  Rows at or past a bank's common range (the tail of a bank-interleaved table) are
 *   updatable as they are uploadable: no lookup reads them, fr_ctx_download_table does.
 *   Duplicates: an id listed twice ends up, per 16-byte word, as that word of ONE of its listed source rows -- which one is unspecified (the
 *   CPU back-end: the last); the bank image equals the conversion of whatever the fp32 arena ends up holding.
 *   Arguments: n == 0 is FR_OK and does nothing; n < 0, a NULL pointer with n > 0, a table out of range, n * dim / 4 >= 2^31: FR_ERR_INVALID;
 *   a table that is not resident on this shard: FR_ERR_STATE (fr_ctx_upload_table's text) -- resident tables of a sharded context are updatable.
 *   fr_worker_sync after an update alone (no batch) succeeds; fr_worker_last_kernel keeps naming the last batch's kernel.
 * fr_ctx_update_rows: the host form -- host arrays, synchronous: staged, the same launches on the context's set-up stream, waited for;
 * returns FR_ERR_INDEX_RANGE itself.  It may be called beside workers in flight (the cross-worker paragraph applies to it). */
int fr_worker_update_rows(fr_worker *w, int table, int n, const int32_t *d_row_ids, const float *d_rows);
int fr_ctx_update_rows(fr_ctx *ctx, int table, int n, const int32_t *h_row_ids, const float *h_rows);

/* Segmented top-K ranking of scores on the device (additive in ABI 6): a recommender's last step -- rank each request's candidates, return the best
 * k -- without fr_worker_sync, a D2H copy of every score and a host sort.
 * Segments: segment s is d_scores[off[s] .. off[s + 1]), off = d_seg_offsets int32 [n_seg + 1] (NULL: one segment [0, n)): one request's candidate
 * list inside a batch, or a span of several batches whose score buffers are contiguous.  Empty segments are legal; offsets need not start at 0 or end at n.
 * Rank order: a total order on bit patterns.  With u the score's 32 bits: key = 0 if (u & 0x7fffffff) > 0x7f800000 (every NaN), else ~u if the sign
 * bit is set, else u | 0x80000000.  A larger key ranks first; equal keys rank by LOWER POSITION first.  So NaNs rank last, behind -inf (key 0x007fffff),
 * in position order among themselves; +0 ranks above -0; the answer is unique for every input.
 * Outputs: d_top_idx[s][j] = the position INSIDE segment s of its j-th ranked score, d_top_scores[s][j] (the array may be NULL) = that score as a bit
 * copy; for j >= the segment's length -1 and -inf (0xff800000).  Nothing past [n_seg][k] is written.
 * Stream order: asynchronous on the worker's stream, behind everything submitted or pushed on w before the call -- batches fr_worker_push_device has
 * queued for a fused launch are launched first and the stage pipeline is drained by launches, neither waited for (the rule of fr_worker_update_rows;
 * host-fed batches still queued in a block make the call FR_ERR_STATE: flush first; so does a table-sharded step in flight).  fr_worker_sync is the
 * completion point; every buffer stays valid until then.  fr_worker_last_kernel keeps naming the last batch's kernel.
 * A segment is MALFORMED when off[s] < 0, off[s + 1] < off[s] or off[s + 1] > n: FR_ERR_INDEX_RANGE at fr_worker_sync (the sticky word, the worker is
 * usable afterwards); it is ranked as empty, every other segment is as specified, and no byte outside d_scores[0 .. n) and offsets[0 .. n_seg] is read.
 * FR_ERR_INVALID: k outside 1 .. FR_TOPK_MAX_K, n outside 1 .. 2^24, n_seg < 1 or > n + 1, a NULL d_scores or d_top_idx.  Nothing is enqueued on an
 * argument or state error.  A call over more than 16384 scores uses a scratch the worker allocates at the first such call; a later call that needs a
 * larger one waits for the worker's stream before it replaces it.  The CPU back-end computes before it returns, the same bits. */
#define FR_TOPK_MAX_K 256
int fr_worker_topk_device(fr_worker *w, int n, const float *d_scores, int n_seg, const int32_t *d_seg_offsets /* [n_seg + 1]; NULL: one segment [0, n) */,
                          int k, int32_t *d_top_idx /* [n_seg][k] */, float *d_top_scores /* [n_seg][k] or NULL */);
/* Host form: ranks the `batch` scores (fr_worker_score_ptr) of the host-form batch in flight on w -- fr_worker_submit, fr_worker_submit_pooled,
 * fr_worker_submit_pooled_weighted or fr_worker_submit_pooled_csr, not yet synchronised; FR_ERR_STATE when there is none, or after a sharded step;
 * FR_ERR_INVALID when batch is not that batch's size.  h_seg_offsets (NULL: one segment) is copied into pinned staging inside the call;
 * h_top_idx / h_top_scores (the latter may be NULL) receive the results in fr_worker_sync, the way fr_worker_push_host delivers h_scores, and stay
 * valid until then.  One host-form ranking may be in flight per worker (a second is FR_ERR_STATE).  The staging is allocated on first use and grows when
 * n_seg * k needs it; a grow waits for the worker's stream. */
int fr_worker_topk(fr_worker *w, int batch, int n_seg, const int32_t *h_seg_offsets /* NULL: one segment */,
                   int k, int32_t *h_top_idx, float *h_top_scores /* or NULL */);

/* Request-form batches (additive in ABI 6): the input side of the segments above.  A request is one user and N candidate items; without this its
 * batch arrives as N complete index rows, the user's columns (and dense features) repeated N times.  With a SPLIT set on the context a batch arrives
 * as request rows + candidate rows + segment offsets, and one small launch expands them on the device into the rows every existing lookup path takes.
 * The expanded rows are, bit for bit, the rows a host-side expansion would have produced; nothing downstream changes.
 * Split: C = fr_model_index_cols(model); shared[C] of 0/1 says which index columns are the request's -- tables, banks or the single per-item column.
 *   One-hot form (FR_REQ_ONE_HOT): the request row is int32 [Rs], the shared columns in ascending column order; the candidate row int32 [Rc], the
 *   others in ascending order; Rs + Rc = C.
 *   Pooled form (FR_REQ_POOLED): column c contributes hots[c] consecutive words, slot-minor, exactly as in the pooled row: request row [Rs'],
 *   candidate row [Rc'], Rs' + Rc' = P.  Per-sample weights have the same shape, as float, and take the same call.
 *   Dense form (FR_REQ_DENSE): when the context says dense_shared the request carries float [dense_len] once; otherwise dense rows stay per item.
 * Segments: seg_offsets int32 [n_req + 1] is the array fr_worker_topk* takes: request r owns items [off[r], off[r + 1]).  Well formed: off[0] == 0,
 *   non-decreasing, off[n_req] == batch.  Empty requests are legal.  NULL: n_req equal requests of batch / n_req items.
 * Expansion: row i of the output ([batch][C], [batch][P] or [batch][dense_len]) is the full row the existing entry points define: every word of a
 *   shared column from the request row of the request that owns item i, every other word from candidate row i.  Words are 32-BIT BIT COPIES, never
 *   interpreted: a -1 (empty slot), any negative value, a NaN weight, an out-of-range index arrive as they were, and the gather behind the expansion
 *   keeps reporting what it reports today.  Only 4-byte alignment of every array is assumed.
 * Malformed offsets (any of the three conditions violated): FR_ERR_INDEX_RANGE at fr_worker_sync (the worker's sticky word; the worker is usable
 *   afterwards).  The expanded rows of that call are unspecified but for this: every word written is a copy of some word of the request or
 *   candidate arrays passed in; no byte is read outside off[0 .. n_req], req[0 .. n_req x Rs), cand[0 .. batch x Rc); no byte is written outside
 *   out[0 .. batch x W) -- the owning request is always some r in [0, n_req), clamped, never trusted.
 * fr_ctx_set_request_columns: shared == NULL clears the split.  FR_ERR_INVALID: a wrong n_cols, a mask value other than 0/1, dense_shared other
 *   than 0/1 or 1 on a model without dense features, nothing shared at all (no shared column and no shared dense), nothing left per item (every
 *   column shared and no per-item dense).  FR_ERR_STATE: a worker of the context has work in flight (the rule of fr_ctx_set_pooling), a context
 *   with n_shards > 1.  The split survives fr_ctx_set_pooling / fr_ctx_set_pooling_modes: pooled widths always follow the current hots.  Every
 *   existing entry point behaves exactly as before, whether or not a split is set.
 * fr_ctx_request_words: the three widths of a form (any pointer may be NULL).  FR_ERR_STATE: no split set, the pooled form without pooling, the
 *   dense form without dense_shared.
 * fr_worker_expand_requests_device: the primitive.  Asynchronous on the worker's stream, fr_worker_sync is the completion point (the CPU back-end
 *   computes before it returns; malformed offsets wait in the sticky word, as the ranking's do).  It enqueues the one launch and nothing else: queued
 *   fused batches are not flushed and the stage pipeline is not drained -- it orders nothing behind earlier work.  The caller owns d_rows_out under
 *   the buffer-lifetime rule of fr_worker_push_device.  A following fr_worker_gather_only, submit_device, push_device, gather_pooled*,
 *   submit_pooled*_device or push_pooled_device* ON THE SAME WORKER with d_rows_out as its d_idx / d_weights / d_dense reads the expanded rows: that
 *   is the streaming form, no new push entry point is needed.
 *   FR_ERR_INVALID: a NULL worker, batch outside 1 .. max_batch, n_req outside 1 .. 2^24, an unknown form, a NULL d_req_rows or d_rows_out, a NULL
 *   d_cand_rows where the form has candidate words, NULL offsets with batch % n_req != 0, an array reaching the 4000 MiB bound of the pooled calls.
 *   FR_ERR_STATE: the cases of fr_ctx_request_words.  Nothing is enqueued on an argument or state error.  fr_worker_last_kernel keeps naming the last
 *   batch's kernel.
 * fr_worker_submit_requests: the host form.  Candidate rows packed [batch][Rc or Rc'] in fr_worker_idx_ptr, candidate weights in
 *   fr_worker_pool_weights_ptr (pooled weighted only), per-item dense in fr_worker_dense_ptr unless dense_shared; the request side packed
 *   [n_req][Rs or Rs'] / [n_req][dense_len] in the four buffers below; offsets always explicit.  On the host, before anything is enqueued: off[0] != 0,
 *   off[n_req] != batch or n_req outside 1 .. max_batch is FR_ERR_INVALID; the pair checks remain the kernel's.  The expansion reads the pinned arrays
 *   in place and writes worker-owned device buffers; the existing chain (fr_worker_submit_device's, or fr_worker_submit_pooled*_device's) then runs on
 *   them with the pinned score buffer as destination: up to three expansion launches plus the unchanged submit.  It counts as the host-form batch in
 *   flight, so fr_worker_topk(w, batch, n_req, the same offsets, k, ...) ranks every request's candidates.  One batch in flight per worker, as for
 *   fr_worker_submit.  The four buffers exist on a worker created AFTER fr_ctx_set_request_columns (pinned; host memory on the CPU back-end): on an
 *   older worker the accessors return NULL and the call returns FR_ERR_STATE; for the pooled forms the worker must also be created after
 *   fr_ctx_set_pooling, as today.  Pooled weighted on a context with a MEAN column: FR_ERR_STATE, as today. */
#define FR_REQ_ONE_HOT 0
#define FR_REQ_POOLED  1   /* pooled index rows AND per-sample weight rows (same shape, bit copies) */
#define FR_REQ_DENSE   2   /* request dense rows -> per-item dense rows; needs dense_shared */
int fr_ctx_set_request_columns(fr_ctx *ctx, const int32_t *shared /* [n_cols] 0/1; NULL clears */, int n_cols, int dense_shared);
int fr_ctx_request_words(const fr_ctx *ctx, int form, int *req_words, int *cand_words, int *row_words);
int fr_worker_expand_requests_device(fr_worker *w, int batch, int n_req, const int32_t *d_seg_offsets /* NULL: equal */, const void *d_req_rows,
                                     const void *d_cand_rows /* NULL for FR_REQ_DENSE */, int form, void *d_rows_out);
int32_t *fr_worker_request_idx_ptr(fr_worker *w);      /* pinned int32 [max_batch][max(Rs, Rs')] */
float *fr_worker_request_weights_ptr(fr_worker *w);    /* pinned float [max_batch][Rs'], NULL without pooling at creation */
float *fr_worker_request_dense_ptr(fr_worker *w);      /* pinned float [max_batch][dense_len], NULL unless dense_shared */
int32_t *fr_worker_request_offsets_ptr(fr_worker *w);  /* pinned int32 [max_batch + 1] */
int fr_worker_submit_requests(fr_worker *w, int batch, int n_req, int pooled /* 0 one-hot, 1 pooled, 2 pooled weighted */);

/* Keyed lookups (additive in ABI 6): the id -> row step in front of every lookup path.  Every entry point above takes int32 ROW NUMBERS; a serving host
 * holds 64-bit feature ids (hashed strings, item ids, user ids).  With a KEY SPACE set on an index column, one small launch turns int64 keys into the
 * int32 rows every existing path takes; nothing downstream changes.
 * Key spaces: every index column c < fr_model_index_cols(model) -- a table, a bank or the single per-item column -- has one.  R_c is the row count the
 *   one-hot gather checks for the column.
 *     FR_KEYS_ROWS (the default)  a key IS a row number: 0 <= k < 2^31 - 1 -> (int32) k; any other key -> FR_KEY_NO_ROW.
 *     FR_KEYS_HASHED              the hashing trick, no table and no state: row = (uint32) ((((mix64((uint64) k ^ seed)) >> 32) * (uint64) R_c) >> 32).
 *     FR_KEYS_MAPPED              an exact map in device memory: a present key -> its row, an absent key -> the column's miss_row.
 *   mix64 is the splitmix64 finaliser: z ^= z >> 30; z *= 0xbf58476d1ce4e5b9; z ^= z >> 27; z *= 0x94d049bb133111eb; z ^= z >> 31
 *   (mix64(5) = 13168350753275463132, mix64(4) = 13232826040865663252).
 *   FR_KEY_EMPTY (-1) is the empty slot of a pooled bag: it resolves to -1 in every mode and is never a map key.  FR_KEY_NO_ROW (0x7fffffff) is the row a
 *   key without a row becomes; every gather reports it as out of range, as it always has.  miss_row is a row in [0, R_c) (a shared "unknown" row), -1
 *   (an unknown id in a bag is an empty slot) or FR_KEY_NO_ROW (an unknown id is an index-range error at fr_worker_sync).
 * fr_ctx_set_key_space: MAPPED creates an EMPTY map for up to max_keys keys: slots = the smallest power of two >= 2 * max_keys (the load never exceeds
 *   0.5) of 16 bytes each, {int64 key; int32 row; int32 pad}; an empty slot holds key -1 and row miss_row; the home slot of a key is
 *   mix64(k ^ seed) & (slots - 1), probing is linear.  seed is the HASHED hash's and the MAPPED home slot's; max_keys and miss_row are read for MAPPED
 *   only.  Setting a column again replaces its key space (a MAPPED one starts empty again); ROWS drops it.
 *   FR_ERR_OOM: the map does not fit.  FR_ERR_INVALID: a column or mode out of range; for MAPPED a miss_row that is none of the three kinds, max_keys
 *   outside 1 .. 2^30.  FR_ERR_STATE: a worker of the context has work in flight (the rule of fr_ctx_set_pooling), a context with n_shards > 1.
 *   Key spaces belong to index columns: they survive fr_ctx_set_pooling / fr_ctx_set_pooling_modes / fr_ctx_set_request_columns.
 * fr_ctx_key_space reads one back (any output pointer may be NULL; n_keys: the keys in the map, 0 unless MAPPED); it synchronises the device, as
 *   fr_ctx_gather_merged_lookups does.
 * Writing a map: n pairs (keys[i], rows[i]) of ONE MAPPED column.  A put is an UPSERT: a present key gets the new row, an absent key is inserted.
 *   Legal rows are [0, R_c) and the column's own miss_row; putting miss_row "forgets" a key (it keeps its slot and resolves like an unknown one; it still
 *   counts in n_keys and is no miss for fr_worker_key_misses).  Not applied, and reported: a pair whose key is -1, a pair whose row is not legal, a NEW
 *   key when n_keys == max_keys -- every other pair of the call is still applied.  A key listed twice in one call ends up with one of its listed rows,
 *   which one is unspecified (the CPU back-end: the last); when such a key is new and takes the map's LAST place, its other occurrences may be reported
 *   as finding the map full.
 *   fr_worker_put_keys: device pointers (host pointers on the CPU back-end, which computes before it returns), asynchronous on the worker's stream;
 *   d_keys (8-byte aligned) and d_rows (4-byte aligned; FR_ERR_INVALID otherwise, in the host form too) stay valid until fr_worker_sync(w) has returned.  A pair that is not applied raises the worker's sticky word:
 *   FR_ERR_INDEX_RANGE at fr_worker_sync, fr_last_error() saying which of the three it was; the worker is usable afterwards.
 *   fr_ctx_put_keys: the host form -- host arrays, synchronous on the context's set-up stream, legal beside workers in flight; returns FR_ERR_INDEX_RANGE itself.
 *   Arguments (the rules of fr_worker_update_rows): n == 0 is FR_OK and does nothing; n < 0, a NULL pointer with n > 0, a column out of range:
 *   FR_ERR_INVALID; a column that is not MAPPED: FR_ERR_STATE.
 *   Order (the rules of fr_worker_update_rows): on one worker, keys resolved BEFORE the call see the old map, keys resolved AFTER it the new one; batches
 *   fr_worker_push_device has queued for a fused launch are launched first (not waited for); host-fed batches still queued in a block make the call
 *   FR_ERR_STATE (flush first).  Across workers there is no order until fr_worker_sync(w) has returned; a resolve in flight on another worker meanwhile
 *   yields, per key, the old row (miss_row if the key was absent) or the new row, never anything else: the key is claimed first (one 64-bit
 *   compare-and-swap), the row stored second, and an empty slot is pre-filled with miss_row.
 * fr_worker_resolve_keys_device: d_keys int64 [n_rows][W] (8-byte aligned, nothing more) -> d_idx_out int32 [n_rows][W].  W and the word -> column map:
 *     FR_KEY_ROWS_FULL        the rows fr_worker_submit_device (pooled = 0: W = C) / fr_worker_submit_pooled_device (pooled = 1: W = P) take; n_rows <= max_batch
 *     FR_KEY_ROWS_REQUEST     the request rows of fr_worker_expand_requests_device (FR_REQ_ONE_HOT: W = Rs / FR_REQ_POOLED: W = Rs'); n_rows <= 2^24
 *     FR_KEY_ROWS_CANDIDATE   its candidate rows (W = Rc / Rc'); n_rows <= max_batch
 *   (the widths of fr_ctx_request_words).  It enqueues ONE launch and nothing else -- the rule of fr_worker_expand_requests_device: queued fused batches are not
 *   flushed, the stage pipeline is not drained.  (The first resolve after the pooling or the split has changed uploads the word -> column tables first.)  A following
 *   fr_worker_gather_only, submit*_device, push*_device or fr_worker_expand_requests_device ON THE SAME WORKER with d_idx_out among its inputs reads the resolved
 *   rows: no new push entry point is needed; the buffer-lifetime rule of fr_worker_push_device applies.  No byte outside d_keys[0 .. n_rows x W), the maps and
 *   d_idx_out[0 .. n_rows x W) is read or written.  The CPU back-end computes before it returns, the same rows bit for bit.
 *   FR_ERR_INVALID: a NULL worker or pointer, an unknown rows_kind, pooled other than 0 / 1, n_rows outside its range, a key or row array reaching 4000 MiB.
 *   FR_ERR_STATE: REQUEST / CANDIDATE rows without a split, the pooled forms without pooling, a form of zero words, a context with n_shards > 1.
 * Host form: fr_worker_key_ptr is pinned int64 [max_batch][max(C, P)] (host memory on the CPU back-end), there on a worker created AFTER the context's first
 *   non-default key space, NULL before; fr_worker_submit_keyed runs the resolve over the pinned keys ([batch][C] or [batch][P]) in place into the worker's
 *   device index buffer and then the unchanged chain of fr_worker_submit_device / fr_worker_submit_pooled[_weighted]_device with the pinned score buffer as
 *   destination (dense rows in fr_worker_dense_ptr, weights in fr_worker_pool_weights_ptr, as for the plain host forms).  It counts as the host-form batch in
 *   flight: fr_worker_topk ranks it.  FR_ERR_STATE: a worker without the key buffer, and every state the plain host forms refuse.
 * fr_worker_key_misses: the MAPPED lookups of this worker that found no slot holding their key, since the worker was created or the counter was last reset;
 *   it synchronises the worker's stream (nothing is flushed).  The counter lives in device memory; a wave adds to it once, not a lane.
 * Out of scope: flat key arrays for the offsets (CSR) form; keyed forms of fr_worker_push_host and fr_worker_submit_requests; the TCP wire format of
 *   fleetrec_server; sharded contexts.  (Retiring keys and growing a map: "The life cycle of a key map" below.) */
#define FR_KEYS_ROWS   0
#define FR_KEYS_HASHED 1
#define FR_KEYS_MAPPED 2
#define FR_KEY_EMPTY  (-1)
#define FR_KEY_NO_ROW 0x7fffffff
#define FR_KEY_ROWS_FULL      0
#define FR_KEY_ROWS_REQUEST   1
#define FR_KEY_ROWS_CANDIDATE 2
int fr_ctx_set_key_space(fr_ctx *ctx, int col, int mode, uint64_t seed, int64_t max_keys, int32_t miss_row);
int fr_ctx_key_space(fr_ctx *ctx, int col, int *mode, uint64_t *seed, int64_t *max_keys, int64_t *n_keys, int32_t *miss_row);
int fr_ctx_put_keys(fr_ctx *ctx, int col, int n, const int64_t *h_keys, const int32_t *h_rows);
int fr_worker_put_keys(fr_worker *w, int col, int n, const int64_t *d_keys, const int32_t *d_rows);
int fr_worker_resolve_keys_device(fr_worker *w, int n_rows, int rows_kind, int pooled, const int64_t *d_keys, int32_t *d_idx_out);
int64_t *fr_worker_key_ptr(fr_worker *w);
int fr_worker_submit_keyed(fr_worker *w, int batch, int pooled /* 0 one-hot, 1 pooled, 2 pooled weighted */);
int fr_worker_key_misses(fr_worker *w, uint64_t *misses, int reset);

/* The life cycle of a key map (additive in ABI 6): retire ids, look at a map, and compact / grow / shrink / reseed it on the device.
 * For a MAPPED column a slot is OCCUPIED when its key is not -1, DEAD when it is occupied and its row equals the column's miss_row, LIVE when it is
 *   occupied and not dead.  Dead is exactly what putting miss_row ("forgetting") has always produced; a key put on purpose with a row equal to a
 *   miss_row that is a real row of the column is dead by the same definition: export does not list it and a rebuild drops it (it resolves to the same
 *   row before and after, as a miss afterwards).
 * Erase: n keys of ONE MAPPED column.  A present key's row becomes miss_row; the slot keeps its key (probe chains stay whole) and the key still counts in
 *   n_keys.  An ABSENT key writes nothing, claims nothing and is no error -- the difference from put(k, miss_row), which inserts.  A key of -1 is not
 *   applied and is reported: FR_ERR_INDEX_RANGE at fr_worker_sync (fr_ctx_erase_keys returns it itself), fr_last_error() naming the key erase and
 *   FR_KEY_EMPTY; every other key of the call is applied and the worker stays usable.  A later put of an erased key gives it a row again in the same
 *   slot, n_keys unchanged.  An erased key is no miss for fr_worker_key_misses, an absent one is.
 *   fr_worker_erase_keys: device pointer (host pointer on the CPU back-end, which computes before it returns), asynchronous on the worker's stream;
 *   d_keys (8-byte aligned, FR_ERR_INVALID otherwise, in the host form too) stays valid until fr_worker_sync(w) has returned.  fr_ctx_erase_keys: the host
 *   form, synchronous on the context's set-up stream, legal beside workers in flight.  Arguments and order are fr_worker_put_keys's: n == 0 is FR_OK;
 *   n < 0, a NULL pointer with n > 0, a column out of range: FR_ERR_INVALID; a column that is not MAPPED: FR_ERR_STATE; on one worker keys resolved BEFORE
 *   the call see the old rows, keys resolved AFTER it the erased ones; batches queued for a fused launch are launched first; host-fed batches still
 *   queued in a block make the call FR_ERR_STATE (flush first).  Across workers a resolve in flight sees, per key, the old row or miss_row, never anything
 *   else (one 4-byte store).  Erase and put of the same key on different unsynchronised workers: one of the two results, unspecified which.
 * fr_ctx_key_space_stats: slots = the slot count; occupied (= n_keys of fr_ctx_key_space when no put is in flight); live; probe_sum = the sum over the
 *   occupied slots of (slot - home(key)) & (slots - 1), so 1 + probe_sum / occupied is the mean number of probes of a present key.  probe_sum, unlike
 *   the longest displacement, does not depend on the order in which the keys were put.  Any output pointer may be NULL; it synchronises the device as
 *   fr_ctx_key_space does.  A column that is not MAPPED: FR_ERR_STATE.
 * fr_ctx_export_keys: the LIVE pairs into host arrays of cap elements each, in unspecified order; *n_out = their number.  cap < live: FR_ERR_INVALID with
 *   *n_out = live and nothing written (cap == 0 with NULL arrays is the size query).  Never a byte past cap elements of either array.  It synchronises
 *   the device first; a put or erase racing it from another thread makes the result unspecified.  A column that is not MAPPED: FR_ERR_STATE.
 * fr_ctx_rebuild_key_space replaces the column's map by a new one of fr_key_slots(max_keys) slots (the smallest power of two >= 2 * max_keys) with home
 *   slot mix64(k ^ seed) & (slots - 1), pre-filled with the UNCHANGED miss_row, holding exactly the live pairs of the old one: dead slots are dropped,
 *   n_keys becomes live, max_keys and seed become the arguments.  Afterwards every key resolves to the row it resolved to before; the one visible
 *   difference is that a dropped key is now a miss for fr_worker_key_misses.  It runs on the context's set-up stream, is synchronous, and the pairs
 *   never leave the device.  State: the rule of fr_ctx_set_key_space -- a worker of the context with work in flight, or a context with n_shards > 1:
 *   FR_ERR_STATE (a live, undrained rebuild is out of scope).  FR_ERR_INVALID: max_keys outside 1 .. 2^30 or below live; FR_ERR_STATE: a column that is
 *   not MAPPED; FR_ERR_OOM: old and new map coexist during the call.  In every error case the old map stays exactly as it was.  On success the old map
 *   is released before the call returns; workers created earlier keep working; other columns are untouched.
 * Out of scope: reusing dead slots in place; a rebuild beside workers in flight; sharded contexts; keyed CSR arrays; fleetrec_server's wire format. */
int fr_worker_erase_keys(fr_worker *w, int col, int n, const int64_t *d_keys);
int fr_ctx_erase_keys(fr_ctx *ctx, int col, int n, const int64_t *h_keys);
int fr_ctx_key_space_stats(fr_ctx *ctx, int col, int64_t *slots, int64_t *occupied, int64_t *live, int64_t *probe_sum);
int fr_ctx_export_keys(fr_ctx *ctx, int col, int64_t cap, int64_t *h_keys, int32_t *h_rows, int64_t *n_out);
int fr_ctx_rebuild_key_space(fr_ctx *ctx, int col, uint64_t seed, int64_t max_keys);

/* Row pools: admitting ids (additive in ABI 6).  Which row a new id gets is decided on the device: a MAPPED column is given a ROW POOL, a range of
 * its rows that the library hands out and takes back, and the whole life of an id runs in one stream on one worker, without a host copy of the map:
 *   fr_worker_admit_keys -> fr_worker_update_rows (ids = the rows just assigned) -> fr_worker_resolve_keys_device -> gather / submit -> fr_worker_erase_keys
 * Pool: the rows [first_row, first_row + n_rows) of the column, inside [0, R_c), not containing the column's miss_row; n_rows == 0 drops the pool.
 *   The FREE SET IS DERIVED FROM THE MAP AS IT STANDS: a pool row held by a live key is taken, every other pool row is free.  So the call works on a map
 *   restored from an export (set_key_space + put_keys + set_row_pool), on an empty map, and AGAIN on the same column, where it re-derives the free set:
 *   the way back after rows inside the range were put by hand, which fr_*_put_keys still allows and the pool does not learn of.  FR_ERR_INVALID: a
 *   range outside [0, R_c), one that contains miss_row, n_rows < 0, a column out of range; FR_ERR_STATE (the rules of fr_ctx_set_key_space): a column
 *   that is not MAPPED, a worker of the context with work in flight, n_shards > 1; FR_ERR_OOM: the bookkeeping (one bit per pool row) does not fit.  In
 *   every error case the column keeps the pool it had.  fr_ctx_rebuild_key_space keeps the pool (live keys keep their rows); fr_ctx_set_key_space on
 *   the column drops it (the map starts empty).  fr_ctx_row_pool: n_rows = 0 for a column without a pool; free_rows = the free rows; any output pointer
 *   may be NULL; it synchronises the device as fr_ctx_key_space does.
 * Admit, per key k of the call (a column without a pool: FR_ERR_STATE):
 *   k live (present, row != miss_row): rows_out[i] = its row; nothing is written, free_rows is unchanged.
 *   k absent or dead: one free pool row r is taken; an absent key claims a slot under the put's rules (n_keys against max_keys, bounded probe), a dead
 *     key keeps its slot and n_keys; the row is stored and rows_out[i] = r.  Which free row is taken is unspecified on the device; the CPU back-end
 *     takes the lowest-numbered one.
 *   Not applied, reported as FR_ERR_INDEX_RANGE at fr_worker_sync (fr_ctx_admit_keys returns it itself), fr_last_error() naming the key admit and the
 *     case, every other key applied, the worker usable afterwards: k == -1 (rows_out[i] = -1); no free row (status bit FR_KEYS_ERR_NO_FREE_ROW = 32;
 *     rows_out[i] = FR_KEY_NO_ROW; an absent key stays absent: nothing is claimed, n_keys is unchanged); a new key when n_keys == max_keys
 *     (rows_out[i] = FR_KEY_NO_ROW; the row goes back to the pool).
 *   A key listed several times in one call: every occurrence reports the SAME row and free_rows drops by one per distinct new key -- one occurrence is
 *     elected on the device and the others take its answer, so neither rows nor places in the map are taken for a moment by the duplicates.  The put's
 *     caveat remains between CALLS: when admits of one key race from unsynchronised workers while the pool is at its last row or the map at its last
 *     place, one of them may be reported as finding none.
 *   Arguments, order and the flush rule are fr_worker_put_keys's: n == 0 is FR_OK; d_keys 8-byte, d_rows_out 4-byte aligned; queued fused batches are
 *     launched first; host-fed blocks still queued: FR_ERR_STATE; both arrays stay valid until the sync.  While the call is in flight rows_out may hold
 *     values that are no answer.  fr_ctx_admit_keys: the host form, synchronous on the context's set-up stream, legal beside workers in flight.
 *   Composition: a following fr_worker_update_rows(w, table, n, d_rows_out, d_vectors) on the same worker writes the embeddings of exactly the admitted
 *     ids (FR_KEY_NO_ROW and -1 entries write nothing and are reported, by the range rule of the updates); a following resolve sees the new rows; a
 *     resolve in flight on another worker sees, per key, the old row (or miss_row) or the new row, never anything else.
 *   Racing admits of one column from unsynchronised workers are legal: distinct keys get distinct rows, the same key gets one row, free_rows ends exact.
 *   Admit racing erase of one column across unsynchronised workers: which rows are handed out is unspecified; no row outside the pool is ever handed
 *     out, no live row is handed out twice, and no byte outside the map, the pool's bookkeeping and the call's arrays is touched.
 * Erase on a column with a pool: fr_*_erase_keys keeps its contract word for word; in addition the row of each erased key goes back to the pool if it
 *   lies in the pool range -- once, however often the key is listed.  Absent keys and -1 behave as ever.
 * Out of scope: a combined admit-and-write call; eviction policy; pools on sharded contexts; reuse of dead SLOTS (fr_ctx_rebuild_key_space). */
int fr_ctx_set_row_pool(fr_ctx *ctx, int col, int32_t first_row, int32_t n_rows);   /* n_rows == 0 drops the pool */
int fr_ctx_row_pool(fr_ctx *ctx, int col, int32_t *first_row, int32_t *n_rows, int64_t *free_rows);
int fr_worker_admit_keys(fr_worker *w, int col, int n, const int64_t *d_keys, int32_t *d_rows_out);
int fr_ctx_admit_keys(fr_ctx *ctx, int col, int n, const int64_t *h_keys, int32_t *h_rows_out);

/* ---- per-layer epilogue: bias and ReLU between the FC layers ----
 * The reference's chain is four matrix products with nothing between them (alpha = 1, beta = 0, cuda_server.c:211-217), which no trained model
 * looks like.  A context holds, per layer l = 0..3 (W1, W2, W3, Wout), an optional bias vector b_l of fc[l + 1] fp32 values and, for the hidden
 * layers 0..2, an activation: FR_ACT_NONE (the default) or FR_ACT_RELU.  The chain then computes R_l = act(W_l R_(l-1) + b_l), in every kernel
 * that finishes a layer, on both back-ends.  A context that never sets one behaves, names its kernels and performs exactly as before.
 *   fp32:  the layer's sum over k is taken exactly as without an epilogue; v = sum + b[h] is ONE fp32 add after the WHOLE K sum (where the stage
 *          pipeline splits K in two, after the partials are combined, never per partial); then the activation.
 *   ReLU:  v > 0 ? v : +0.0f; a NaN stays a NaN (a corrupt feature still reaches the score); -0 and negatives become +0.
 *   bf16:  the same fp32 v; activation first, then the chain's ONE round-to-nearest-even to bf16 per hidden activation.  The bias is never rounded.
 *   fp8:   the sum in real units (the accumulator times 2^-(e_act[l] + e_w[l])), v = real + b[h] in fp32, the activation, then x 2^e_act[l + 1],
 *          the clamp to +-448 and round-to-nearest-even to e4m3 as before.
 *   output layer: score = sum + b_3[0], one fp32 add after the sum -- also where the output layer is folded into FC3's launch.  No activation
 *          there: a monotone transform does not change a ranking (sigmoid is out of scope).
 *   fp8 calibration (fr_worker_calibrate_fp8, _slices, _sharded, _sharded_pooled) runs the fp32 chain WITH the epilogues and takes max |.| of X
 *          and of the post-activation R1..R3.  The uncalibrated rms estimate does not know about biases: a context with biases should calibrate.
 * The epilogue belongs to the context: submit, submit_device, push_device, push_host / staged, the pooled, CSR, request-form and keyed forms,
 * fr_worker_fc_only, fr_worker_fc_layer_only / _repeat, fr_worker_fc_from_slices[_lp], fr_worker_submit_sharded[_pooled] and the drivers all honour
 * it without a new entry point.  FC weights are replicated on shards, and so are the epilogues: each shard context is set by its owner.
 * Two dispatch changes for a context WITH an epilogue, both for want of registers, both with bit-identical sums (DESIGN section 3.6 has the measured
 * cost).  (1) bf16: the persistent fused kernel is not run; streamed launches take the chunked bf16 fused kernel (records of 352 / 880 floats), other
 * records the stage pipeline (fr_ctx_stream_group reports 1 then, and fr_worker_push_host refuses as for any model that does not stream through a
 * fused kernel).  (2) fp32, records of 352 floats (Model-A), launches of the 32-item fused kernel (stream groups below 64, partial launches): the
 * one-workgroup-per-CU instantiation runs instead of the two-workgroups-per-CU one.
 * fr_ctx_set_epilogue: bias = fc[layer + 1] floats, or NULL with count 0 (no bias); act = FR_ACT_*.  The threading and in-flight rules of
 *   fr_ctx_set_weights (a blocking copy; no worker of the context may have work in flight).  (NULL, 0, FR_ACT_NONE) restores the layer as it was
 *   before, bit for bit.  It does not touch the fp8 exponents, the weight images, the chain width or the stream group setting.
 *   FR_ERR_INVALID: a bad layer, a count that is not the layer's width, an unknown activation, an activation on layer 3.
 * fr_ctx_epilogue reads back: bias_out may be NULL (else count = the layer's width; written only when a bias is set), *has_bias 0 / 1, *act. */
#define FR_ACT_NONE 0
#define FR_ACT_RELU 1
int fr_ctx_set_epilogue(fr_ctx *ctx, int layer, const float *bias, size_t count, int act);
int fr_ctx_epilogue(fr_ctx *ctx, int layer, float *bias_out, size_t count, int *has_bias, int *act);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
