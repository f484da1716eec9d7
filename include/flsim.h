/*
 * flsim.h -- C-ABI of libflsim.so, the MI355X (gfx950) engine for the federated-learning
 * simulation hot path of grossmanlev/FL-distributed-delay.
 *
 * The reference is pure Python; its "interface" for this path is the call sites below.  Each
 * entry point names the reference code it replaces.  All device pointers are raw HIP device
 * addresses (e.g. torch tensor data_ptr()), all work is enqueued on `stream` and is
 * asynchronous; no entry point allocates device memory or synchronises.  Status: 0 = OK,
 * 1 = invalid argument / the reference would raise, 2 = HIP error; flsim_last_error() gives the
 * message (thread-local).
 */
#ifndef FLSIM_H
#define FLSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* flsim_stream_t; /* == hipStream_t */

/* one simulated worker-step of a chunk: epoch t, worker i, dataset index k (main.py:138).
 * pad = the worker's batch size B (main.py:43-44 --batch_size; 0 = the default 128): a batch of
 * B samples spans ceil(B/128) consecutive records (128-sample groups) whose i is worker +
 * g * 2^20 for group g (the group's dropout key); sample slot j of group g is sample g*128 + j
 * of the worker's batch, drawn with the worker's key; slots past B are padding that adds no loss
 * and no gradient; the CrossEntropyLoss gradient is the mean over the B samples.  worker_loss of
 * a group = its summed loss / 128, so the worker's loss = sum over its groups * 128 / B. */
typedef struct WorkerRec {
    uint32_t t;
    uint32_t i;
    uint32_t k;
    uint32_t pad;
} WorkerRec;

const char* flsim_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * The one collective of a sharded server step: each rank computes its contiguous
 * block of the epoch's workers (main.py:137-178 split across GPUs) into a partial
 * [S_t | losses]; one all-reduce (sum, fp32, in place) over RCCL / xGMI then gives every rank the
 * sum that rule() (main.py:184) and Adam (main.py:188) consume, replicated.  The reference has no
 * collective (one process, main.py:137); this is its replacement for a caller that does not use
 * torch.distributed.  RCCL is bound at run time: the copy already loaded in the process (e.g.
 * torch's), else $FLSIM_RCCL_LIB, else librccl.so.1.
 *   flsim_comm_unique_id: rank 0 makes the id (ncclGetUniqueId) and ships it to the others;
 *   flsim_comm_create(nranks, rank, id): ncclCommInitRank; nranks = 1 with id = NULL is a local
 *     communicator that never touches RCCL (its all-reduce is the identity);
 *   flsim_allreduce_sum: ncclAllReduce(buf, buf, count, float32, sum) on `stream`.
 * ------------------------------------------------------------------------------------------- */
#define FLSIM_COMM_ID_BYTES 128
typedef struct flsim_comm flsim_comm;
int flsim_comm_unique_id(unsigned char* id /* FLSIM_COMM_ID_BYTES */);
int flsim_comm_create(int nranks, int rank, const unsigned char* id, flsim_comm** out);
int flsim_comm_size(const flsim_comm* comm);
int flsim_comm_rank(const flsim_comm* comm);
int flsim_allreduce_sum(flsim_comm* comm, float* buf, size_t count, flsim_stream_t stream);
int flsim_comm_destroy(flsim_comm* comm);

/* ---------------------------------------------------------------------------------------------
 * Schedule (host): replaces the integer scan of main.py:119-123 (state), :150-166 (slow worker
 * + pesky_worker_grads FIFO), :167-178 (fast worker + throttle), :180-181 (window decrement).
 * delays[i] != 0 marks a slow worker (reference: only i = n-1, delay = --delay);
 * FLSIM_DELAY_ZERO marks the reference's slow worker under --delay 0: it computes and pushes at
 * t = 0 (main.py:153-157), and the epoch t = 1 fails like main.py:158's t % 0.
 * ------------------------------------------------------------------------------------------- */
#define FLSIM_DELAY_ZERO ((int32_t)0x80000000)
typedef struct flsim_sched flsim_sched;
flsim_sched* flsim_sched_create(int32_t n, const int32_t* delays, int32_t throttle,
                                int32_t max_throttle);
void flsim_sched_destroy(flsim_sched* s);
/* computes[n], fast[n]: u8 flags; stale_worker[n], stale_src[n]: popped FIFO entries in append
 * order; info[4] = {c_t, s_t, pushed, t}.  Returns 1 where main.py would raise IndexError in
 * rule() (empty weight_ups). */
int flsim_sched_epoch(flsim_sched* s, uint8_t* computes, uint8_t* fast, int32_t* stale_worker,
                      int64_t* stale_src, int64_t* info);
void flsim_sched_state(const flsim_sched* s, int64_t* out3);

/* ---------------------------------------------------------------------------------------------
 * PerformantNet1 worker-batched forward/backward: replaces Worker.fwd_bkwd (agents.py:32-40)
 * for every worker of a chunk at once, on models.py:11-47, including the batch draw of
 * main.py:138-142 (synthetic CIFAR-shaped u8 pool, ToTensor + Normalize via `lut`).
 * Gradients of all chunks of an epoch accumulate (agents.py:35 in-place .grad accumulation)
 * into split-K slabs inside `gradstate`; flsim_pn1_end_epoch sums them into S_t (torch
 * named_parameters layout, P = flsim_pn1_param_count() floats).
 * `gradstate` (flsim_pn1_gradstate_bytes()) and `workspace` (flsim_pn1_workspace_bytes()) need no
 * initialisation by the caller: results do not depend on what the buffers held before
 * flsim_pn1_begin_epoch (any bytes, NaN patterns included), nor on earlier epochs and chunks run
 * on them.  The caller only keeps them alive and calls flsim_pn1_begin_epoch before the first
 * backward pass on a gradstate.  The same holds for the flsim_vgg11_* and flsim_vgg11_bn_* families.
 * ------------------------------------------------------------------------------------------- */
long flsim_pn1_param_count(void);
long flsim_pn1_gradstate_bytes(void);
long flsim_pn1_workspace_bytes(int max_samples);
int flsim_pn1_workspace_offset(int which, int samples, long* offset_bytes);
/* (debug / tests) the tensors that feed the split-bf16 GEMMs are stored split (HM + L parts,
 * DESIGN 6g): the workspace id of tensor `which`'s L part, or -1 when it is stored fp32 */
int flsim_pn1_workspace_split_part(int which);
/* (debug / tests) 1 when workspace tensor `which` is stored channel-slice-major, [samples][C/16]
 * [H][W][16] (the inputs of conv2-4: a1, d1, a3), 0 when pixel-major [samples][H][W][C] */
int flsim_pn1_workspace_slice_major(int which);
/* packs theta_t into the kernel layouts and zeroes the slabs (start of main.py:126 epoch) */
int flsim_pn1_begin_epoch(void* gradstate, const float* theta, flsim_stream_t stream);
/* workers: device array of n_chunk_workers WorkerRec; worker_loss: device float per worker
 * (agents.py:40 lossval); backward_pass 0 = forward + loss only (eval / debugging) */
int flsim_pn1_fwd_bwd_chunk(void* gradstate, void* workspace, int max_samples, const float* theta,
                            const uint8_t* pool, const int32_t* labels, const int32_t* list_a,
                            int len_a, const int32_t* list_b, int len_b, const float* lut,
                            const WorkerRec* workers, int n_chunk_workers, int n_workers_total,
                            uint64_t seed, int dropout, int backward_pass, float* worker_loss,
                            flsim_stream_t stream);
/* pipelined variant of flsim_pn1_fwd_bwd_chunk (backward_pass always 1), the engine side of the
 * same main.py:137-178 worker loop: the batch draw, forward and loss run on `stream`, the
 * backward on the gradstate's own backward stream after this forward and after the previous
 * call's backward, so one chunk's forward overlaps the previous chunk's backward.  Successive
 * calls must alternate two workspaces (a forward waits for the backward that last used its
 * workspace).  Every other flsim_pn1_* entry point on the gradstate first makes `stream` wait
 * for the outstanding backward work, so end_epoch / server_step / begin_epoch see all chunks. */
int flsim_pn1_fwd_bwd_chunk_async(void* gradstate, void* workspace, int max_samples,
                                  const float* theta, const uint8_t* pool, const int32_t* labels,
                                  const int32_t* list_a, int len_a, const int32_t* list_b,
                                  int len_b, const float* lut, const WorkerRec* workers,
                                  int n_chunk_workers, int n_workers_total, uint64_t seed,
                                  int dropout, float* worker_loss, flsim_stream_t stream);
/* pipelined form of flsim_pn1_fwd_bwd_input (backward_pass always 1; the facade's
 * Worker.fwd_bkwd, agents.py:32-40): worker_loss is ready on `stream` after the forward, and the
 * backward overlaps the next call's forward.  Same workspace alternation and join rule as
 * flsim_pn1_fwd_bwd_chunk_async. */
int flsim_pn1_fwd_bwd_input_async(void* gradstate, void* workspace, int max_samples,
                                  const float* theta, const float* x, const int64_t* y,
                                  int n_samples, const WorkerRec* workers, uint64_t seed,
                                  int dropout, float* worker_loss, flsim_stream_t stream);
/* The facade's deferred backward: Worker.fwd_bkwd (agents.py:32-40) with the backward of up to
 * 16,384 samples of calls batched into one pass.  All calls of an epoch use theta_t
 * (main.py:154,159,169), so a call runs only its forward + CrossEntropyLoss now (the loss is what
 * agents.py:40 returns) into workspace rows [row0, row0 + ceil(n/128)*128); x, y, workers and
 * worker_loss as for flsim_pn1_fwd_bwd_input.  row0 is a multiple of 128; max_samples <= 16384. */
int flsim_pn1_fwd_rows(void* gradstate, void* workspace, int max_samples, int row0,
                       const float* theta, const float* x, const int64_t* y, int n_samples,
                       const WorkerRec* workers, uint64_t seed, int dropout, float* worker_loss,
                       flsim_stream_t stream);
/* The deferred forward of 128-sample calls: flsim_pn1_load_rows stages a call's batch (x, y as
 * for flsim_pn1_fwd_rows) into rows [row0, row0 + ceil(n/128)*128) and returns; later
 * flsim_pn1_fwd_loaded_rows runs the forward + CrossEntropyLoss of staged rows
 * [row0, row0 + n_rows) as one batched pass, each 128-row group one whole batch (workers[g] its
 * dropout key, worker_loss[g] its mean loss, bit-identical to flsim_pn1_fwd_rows on that batch). */
int flsim_pn1_load_rows(void* gradstate, void* workspace, int max_samples, int row0,
                        const float* x, const int64_t* y, int n_samples, flsim_stream_t stream);
int flsim_pn1_fwd_loaded_rows(void* gradstate, void* workspace, int max_samples, int row0,
                              int n_rows, const float* theta, const WorkerRec* workers,
                              uint64_t seed, int dropout, float* worker_loss,
                              flsim_stream_t stream);
/* ...then one backward over rows [0, n_rows) (the same theta and dropout flag as their forwards)
 * adds every call's gradient to the epoch's slabs (agents.py:35 accumulation).  It runs on the
 * gradstate's backward stream after everything queued on `stream`, so the next chunk's forwards
 * (into a second workspace) overlap it; every other flsim_pn1_* entry point joins it first, and a
 * flsim_pn1_fwd_rows into the same workspace waits for it. */
int flsim_pn1_bwd_rows(void* gradstate, void* workspace, int max_samples, int n_rows,
                       const float* theta, int dropout, flsim_stream_t stream);
/* explicit batch variant (Worker.fwd_bkwd(inp, outp), agents.py:32): x NCHW fp32 [n][3][32][32],
 * y int64 [n], any n >= 1 (main.py:43-44 --batch_size; at most 16384): padded to whole groups of
 * 128 samples that add nothing; the gradient is CrossEntropyLoss's mean over the n samples
 * (agents.py:34-35).  workers[ceil(n/128)] give each group's dropout RNG key; worker_loss[g] =
 * group g's summed loss / 128 (so the batch loss = sum_g worker_loss[g] * 128 / n). */
int flsim_pn1_fwd_bwd_input(void* gradstate, void* workspace, int max_samples, const float* theta,
                            const float* x, const int64_t* y, int n_samples,
                            const WorkerRec* workers, uint64_t seed, int dropout,
                            int backward_pass, float* worker_loss, flsim_stream_t stream);
int flsim_pn1_end_epoch(void* gradstate, float* grad_out, flsim_stream_t stream);
/* the gradstate's buffer is about to be freed: drop the library's per-gradstate bookkeeping (the
 * slab rows written this epoch).  A backward pass on a gradstate with no flsim_pn1_begin_epoch
 * since creation or release fails with status 1. */
void flsim_pn1_release(void* gradstate);
/* eval of an explicit batch (util.py:31-45 print_test_accuracy's model(images), dropout off):
 * x NCHW fp32 [n_images][3][32][32] -> pred (device int32[n_images]) */
int flsim_pn1_eval_input(void* gradstate, void* workspace, int max_samples, const float* theta,
                         const float* x, int n_images, int32_t* pred, flsim_stream_t stream);
/* Evaluation: replaces util.print_test_accuracy (util.py:31-45) as called at main.py:196-210
 * after central.model.eval() (main.py:190: dropout off).  Forward of pool images
 * [first, first + n_images) (u8 NCHW 3x32x32, normalised through `lut`), predictions = argmax of
 * the logits (torch.max(outputs, 1): first maximum wins) into pred (device int32[n_images]).
 * Uses the gradstate's packed-weight area (re-packed from theta). */
int flsim_pn1_eval_pool(void* gradstate, void* workspace, int max_samples, const float* theta,
                        const uint8_t* pool, int first, int n_images, const float* lut,
                        int32_t* pred, flsim_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * VGG-11 worker-batched forward/backward (configs[4]'s larger CNN): replaces Worker.fwd_bkwd
 * (agents.py:32-40) when the central model is models.py:101-103 vgg11() (cfg 'A': 8 conv3x3
 * padding 1 + ReLU, 5 max-pools; classifier Dropout / Linear / ReLU twice + Linear,
 * models.py:50-98).  Same contract, argument meaning and errors as the flsim_pn1_* entry points
 * above; parameters flat in vgg11().named_parameters() order, P = flsim_vgg11_param_count()
 * = 9,750,922.  The classifier's dropouts use RNG sites 6 and 7 of the Philox spec.
 * ------------------------------------------------------------------------------------------- */
long flsim_vgg11_param_count(void);
long flsim_vgg11_gradstate_bytes(void);
long flsim_vgg11_workspace_bytes(int max_samples);
int flsim_vgg11_workspace_offset(int which, int samples, long* offset_bytes);
int flsim_vgg11_begin_epoch(void* gradstate, const float* theta, flsim_stream_t stream);
int flsim_vgg11_fwd_bwd_chunk(void* gradstate, void* workspace, int max_samples,
                              const float* theta, const uint8_t* pool, const int32_t* labels,
                              const int32_t* list_a, int len_a, const int32_t* list_b, int len_b,
                              const float* lut, const WorkerRec* workers, int n_chunk_workers,
                              int n_workers_total, uint64_t seed, int dropout, int backward_pass,
                              float* worker_loss, flsim_stream_t stream);
int flsim_vgg11_fwd_bwd_input(void* gradstate, void* workspace, int max_samples,
                              const float* theta, const float* x, const int64_t* y, int n_samples,
                              const WorkerRec* workers, uint64_t seed, int dropout,
                              int backward_pass, float* worker_loss, flsim_stream_t stream);
/* the facade's deferred fwd_bkwd for vgg11() (128-sample calls, agents.py:32-40): load_rows stages
 * a call's batch into workspace rows [row0, row0 + 128) as flsim_pn1_load_rows does; then
 * fwd_bwd_loaded_rows runs forward, CrossEntropyLoss and backward of the staged rows [0, n_rows) as
 * one batched chunk into the epoch's slabs (workers[g] / worker_loss[g]: one per 128-row call). */
int flsim_vgg11_load_rows(void* gradstate, void* workspace, int max_samples, int row0,
                          const float* x, const int64_t* y, int n_samples, flsim_stream_t stream);
int flsim_vgg11_fwd_bwd_loaded_rows(void* gradstate, void* workspace, int max_samples, int n_rows,
                                    const float* theta, const WorkerRec* workers, uint64_t seed,
                                    int dropout, float* worker_loss, flsim_stream_t stream);
/* vgg11_bn: the same two calls; each staged 128-row call is one BatchNorm batch, and bn_stats
 * [n_rows / 128][flsim_vgg11_bn_stats_per_worker()] receives the calls' statistics for
 * flsim_vgg11_bn_update_running (in call order, as nn.BatchNorm2d's per-call updates). */
int flsim_vgg11_bn_load_rows(void* gradstate, void* workspace, int max_samples, int row0,
                             const float* x, const int64_t* y, int n_samples,
                             flsim_stream_t stream);
int flsim_vgg11_bn_fwd_bwd_loaded_rows(void* gradstate, void* workspace, int max_samples,
                                       int n_rows, const float* theta, const WorkerRec* workers,
                                       uint64_t seed, int dropout, float* worker_loss,
                                       float* bn_stats, flsim_stream_t stream);
int flsim_vgg11_end_epoch(void* gradstate, float* grad_out, flsim_stream_t stream);
int flsim_vgg11_eval_input(void* gradstate, void* workspace, int max_samples, const float* theta,
                           const float* x, int n_images, int32_t* pred, flsim_stream_t stream);
int flsim_vgg11_eval_pool(void* gradstate, void* workspace, int max_samples, const float* theta,
                          const uint8_t* pool, int first, int n_images, const float* lut,
                          int32_t* pred, flsim_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * VGG-11 with BatchNorm (models.py:106-108 vgg11_bn(): Conv2d -> BatchNorm2d -> ReLU per conv,
 * models.py:88-89): replaces Worker.fwd_bkwd (agents.py:32-40) when the central model is
 * vgg11_bn().  Same contract as flsim_vgg11_*; parameters flat in vgg11_bn().named_parameters()
 * order (conv weight, conv bias, BatchNorm weight, BatchNorm bias per layer), P = 9,756,426.
 * Train mode: every simulated worker's 128 samples are one BatchNorm batch (one fwd_bkwd call);
 * bn_stats (device float[n_chunk_workers][flsim_vgg11_bn_stats_per_worker()] or nullptr)
 * receives each worker's per-layer [batch mean | unbiased batch variance], the inputs of the
 * running-buffer update nn.BatchNorm2d does on every call.  The running buffers are a device
 * float[5504]: [running_mean | running_var] of features.1, .5, .9, .12, .16, .19, .23, .26.
 * ------------------------------------------------------------------------------------------- */
long flsim_vgg11_bn_param_count(void);
long flsim_vgg11_bn_gradstate_bytes(void);
long flsim_vgg11_bn_workspace_bytes(int max_samples);
int flsim_vgg11_bn_workspace_offset(int which, int samples, long* offset_bytes);
int flsim_vgg11_bn_stats_per_worker(void);
int flsim_vgg11_bn_begin_epoch(void* gradstate, const float* theta, flsim_stream_t stream);
int flsim_vgg11_bn_fwd_bwd_chunk(void* gradstate, void* workspace, int max_samples,
                                 const float* theta, const uint8_t* pool, const int32_t* labels,
                                 const int32_t* list_a, int len_a, const int32_t* list_b,
                                 int len_b, const float* lut, const WorkerRec* workers,
                                 int n_chunk_workers, int n_workers_total, uint64_t seed,
                                 int dropout, int backward_pass, float* worker_loss,
                                 float* bn_stats, flsim_stream_t stream);
int flsim_vgg11_bn_fwd_bwd_input(void* gradstate, void* workspace, int max_samples,
                                 const float* theta, const float* x, const int64_t* y,
                                 int n_samples, const WorkerRec* workers, uint64_t seed,
                                 int dropout, int backward_pass, float* worker_loss,
                                 float* bn_stats, flsim_stream_t stream);
int flsim_vgg11_bn_end_epoch(void* gradstate, float* grad_out, flsim_stream_t stream);
/* vgg11_bn: explicit batches must be whole 128-sample groups (one BatchNorm batch each) */
int flsim_vgg11_bn_eval_input(void* gradstate, void* workspace, int max_samples,
                              const float* theta, const float* x, int n_images,
                              const float* running, int32_t* pred, flsim_stream_t stream);
/* util.py:31-45 in eval mode: BatchNorm normalises with the running buffers `running`. */
int flsim_vgg11_bn_eval_pool(void* gradstate, void* workspace, int max_samples,
                             const float* theta, const uint8_t* pool, int first, int n_images,
                             const float* lut, const float* running, int32_t* pred,
                             flsim_stream_t stream);
/* nn.BatchNorm2d's running update (momentum 0.1) for n_workers calls in worker order:
 * r = 0.1 * stat + 0.9 * r per call, stat from bn_stats[w] (w = 0 .. n_workers-1). */
int flsim_vgg11_bn_update_running(float* running, const float* bn_stats, int n_workers,
                                  flsim_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Server step: replaces Agg.rule = rule() (main.py:23-25, agents.py:43-45: per-tensor
 * torch.stack(weight_ups).mean(0)) + Central.update_model (agents.py:9-21: Adam step,
 * main.py:106).  Bit-exact with torch 2.10 CPU except sqrt rounding;
 * step = Adam step count after increment.
 *
 * flsim_rule describes weight_ups: the entries are S_t (every fast worker's aliased .grad,
 * main.py:172) or one of `arrays` (popped stale FIFO entries, main.py:161-165; NULL = zeros, the
 * torch-1.x semantics).
 *   prog == NULL : reference order, [S_t] * c followed by arrays[0 .. n_arrays) (the slow worker
 *                  is the last worker, main.py:150);
 *   prog != NULL : general order (heterogeneous-delay extension, SURVEY 8 a1: entries appended in
 *                  worker-index order): a device program from flsim_cascade_program, info = its
 *                  info words.
 * k is the divisor of the mean (= the entry count, main.py:24; the independent-entry semantics
 * passes S = the sum of k distinct entries with c = 1).
 * ------------------------------------------------------------------------------------------- */
#define FLSIM_MAX_ARRAYS 64
typedef struct flsim_rule {
    int32_t k;
    int32_t c;
    const int32_t* prog;
    int32_t info[4];
    int32_t n_arrays;
    const float* arrays[FLSIM_MAX_ARRAYS];
} flsim_rule;

/* host: the summation program of rule() over k entries whose non-S_t entries sit at positions
 * pos[0 .. n_events) (increasing) and hold arrays arr[] (indices into flsim_rule.arrays; at most
 * 64), in the device's macro-word form: prog[0 .. cap) receives (lo, hi) int32 pairs plus one
 * padding pair; info[4] = {pairs, pair index of the row_sum part, flags, level power}.
 * k <= 524288. */
int flsim_cascade_program(int k, const int32_t* pos, const int32_t* arr, int n_events,
                          int32_t* prog, int cap, int32_t* info);
/* host (testing): run a macro program on the host, out[e] = cascade sum for element e (x = S[e],
 * entry arrays ys[q][e]; tail[e] != 0 selects the row_sum part) */
int flsim_cascade_eval_host(const int32_t* prog, const int32_t* info, const float* S,
                            const float* const* ys, int n_arrays, const uint8_t* tail, long n,
                            float* out);

/* rule() + Adam from S_t in a buffer (world > 1 after the all-reduce; the FL.agents facade).
 * tensor_sizes: numel of each parameter tensor in named_parameters order (the cascade's column
 * rule is per tensor). */
int flsim_aggregate_adam_rule(const float* S, const flsim_rule* rule, float* p, float* m, float* v,
                              long P, const long* tensor_sizes, int n_tensors, long step, double lr,
                              double beta1, double beta2, double eps, flsim_stream_t stream);
/* the same, also writing S_t into S_out (nullable; 16-byte aligned) in the same pass: the slow
 * worker's FIFO entry at a tick (main.py:156,161) when S_t arrives in a buffer (world > 1, after
 * the all-reduce) */
int flsim_aggregate_adam_rule_push(const float* S, float* S_out, const flsim_rule* rule, float* p,
                                   float* m, float* v, long P, const long* tensor_sizes,
                                   int n_tensors, long step, double lr, double beta1, double beta2,
                                   double eps, flsim_stream_t stream);
/* convenience forms of the above: reference order with n_stale <= 8 stale entries; and the
 * independent-entry semantics (S = sum of k distinct entries, mean = S / k) */
int flsim_aggregate_adam(const float* S, int c, const float* const* stale, int n_stale,
                         float* p, float* m, float* v, long P, const long* tensor_sizes,
                         int n_tensors, long step, double lr, double beta1, double beta2,
                         double eps, flsim_stream_t stream);
int flsim_aggregate_adam_sum(const float* S, int k, float* p, float* m, float* v, long P,
                             const long* tensor_sizes, int n_tensors, long step, double lr,
                             double beta1, double beta2, double eps, flsim_stream_t stream);

/* Fused end of an epoch at world = 1: S_t = sum of the gradstate's slabs (what
 * flsim_<net>_end_epoch computes), written to S_out if non-NULL (the slow worker's FIFO entry at a
 * tick, main.py:156,161), then rule() + Adam -- one launch, S_t never round-trips through HBM. */
int flsim_pn1_server_step(void* gradstate, float* S_out, const flsim_rule* rule, float* p,
                          float* m, float* v, long step, double lr, double beta1, double beta2,
                          double eps, flsim_stream_t stream);
int flsim_vgg11_server_step(void* gradstate, float* S_out, const flsim_rule* rule, float* p,
                            float* m, float* v, long step, double lr, double beta1, double beta2,
                            double eps, flsim_stream_t stream);
int flsim_vgg11_bn_server_step(void* gradstate, float* S_out, const flsim_rule* rule, float* p,
                               float* m, float* v, long step, double lr, double beta1,
                               double beta2, double eps, flsim_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Server step with a chosen optimizer: Central(model, optim) (agents.py:4-8) takes any torch
 * optimizer; these entry points run rule() fused with torch.optim.SGD (momentum, dampening,
 * weight decay, nesterov), torch.optim.Adam with weight_decay (coupled L2) or torch.optim.AdamW
 * (decoupled), bit-exact with torch 2.10's CPU single-tensor path (Adam family: except sqrt
 * rounding, as above).  step = the optimizer's step count after increment; step 1 initialises
 * SGD's momentum buffer (buf = g).  m holds exp_avg (Adam family) or the momentum buffer (SGD
 * with momentum != 0), v exp_avg_sq.  Arrays a kind does not own are neither read nor written
 * and may be NULL: v for SGD, m and v for SGD with momentum == 0.
 * The hyper-parameters are checked before any pointer: an unknown kind, a negative lr,
 * weight_decay or momentum, and nesterov with momentum <= 0 or dampening != 0 (where torch
 * raises ValueError) return status 1.  The flsim_aggregate_adam* / flsim_*_server_step entry
 * points above are these with kind = FLSIM_OPT_ADAM and weight_decay = 0.
 *
 * FedAdagrad and FedYogi (Reddi et al. 2021, Adaptive Federated Optimization) are two more kinds:
 *   FLSIM_OPT_ADAGRAD  torch.optim.Adagrad (lr, lr_decay, weight_decay, eps), per element
 *                        g = fma(p, wd, g) if wd != 0;  sum = fma(g, g, sum);
 *                        p = p + (f32(-clr) * g) / (sqrt(sum) + eps),
 *                        clr = lr / (1 + (step - 1) * lr_decay) in double.
 *                      The accumulator `sum` lives in m; v is neither read nor written and may be
 *                      NULL.  initial_accumulator_value is what the caller fills m with before
 *                      step 1 (the library never initialises state).
 *   FLSIM_OPT_YOGI     Yogi (Zaheer et al. 2018) without bias correction (lr, beta1, beta2, eps,
 *                      weight_decay: coupled), per element
 *                        g = fma(p, wd, g) if wd != 0;  m = fma(1 - beta1, g - m, m);
 *                        g2 = g * g;  v = fma(f32(-(1 - beta2)) * sign(v - g2), g2, v);
 *                        p = p + (f32(-lr) * m) / (sqrt(v) + eps)
 *                      with sign(NaN) = 0; m = exp_avg, v = exp_avg_sq (the caller fills v with
 *                      its initial accumulator value before step 1).
 * Both take the correctly rounded sqrt, as the Adam kinds do.  Refused with status 1, with
 * torch's messages: lr_decay < 0 (Adagrad), eps < 0 (both), a beta outside [0, 1) (Yogi), and a
 * NaN in any of these.
 * ------------------------------------------------------------------------------------------- */
#define FLSIM_OPT_ADAM 0
#define FLSIM_OPT_ADAMW 1
#define FLSIM_OPT_SGD 2
#define FLSIM_OPT_ADAGRAD 3
#define FLSIM_OPT_YOGI 4
typedef struct flsim_optim {
    int32_t kind;     /* FLSIM_OPT_* */
    int32_t nesterov; /* SGD only */
    double lr;
    double beta1, beta2, eps; /* Adam family, Yogi; eps: Adagrad too */
    double weight_decay;
    double momentum, dampening; /* SGD only */
    double lr_decay; /* read only when kind == FLSIM_OPT_ADAGRAD (appended: a caller built against
                        the struct without it is unaffected for the kinds 0 .. 2) */
} flsim_optim;

int flsim_aggregate_optim_rule_push(const float* S, float* S_out, const flsim_rule* rule, float* p,
                                    float* m, float* v, long P, const long* tensor_sizes,
                                    int n_tensors, long step, const flsim_optim* optim,
                                    flsim_stream_t stream);
int flsim_pn1_server_step_optim(void* gradstate, float* S_out, const flsim_rule* rule, float* p,
                                float* m, float* v, long step, const flsim_optim* optim,
                                flsim_stream_t stream);
int flsim_vgg11_server_step_optim(void* gradstate, float* S_out, const flsim_rule* rule, float* p,
                                  float* m, float* v, long step, const flsim_optim* optim,
                                  flsim_stream_t stream);
int flsim_vgg11_bn_server_step_optim(void* gradstate, float* S_out, const flsim_rule* rule,
                                     float* p, float* m, float* v, long step,
                                     const flsim_optim* optim, flsim_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Staleness-weighted rule: Agg(rule) (agents.py:43-45) takes any rule; these entry points run
 *
 *   [torch.stack([x[i] * w for x, w in zip(ups_list, weights)]).sum(0) / W for i in ...]
 *
 * fused with the update, bit-exact with torch 2.10 CPU: w = 1.0 for every entry that is S_t,
 * wts->w[q] for arrays[q] (a popped FIFO entry discounted by its age), W = wts->divisor (the sum
 * of the weights, or the entry count).  Each weight and the divisor are rounded to fp32 once; a
 * stale value is multiplied by its weight in fp32 where it is loaded, the cascade sums the
 * products, one IEEE fp32 division follows.  A NULL array stays zero and still counts in the
 * divisor.  wts == NULL is the plain mean (the entry points above are these with wts = NULL).
 * Checked before any pointer, status 1: a weight that is not finite and >= 0; a divisor that is
 * not > 0 (message "ZeroDivisionError: ...") or not finite.  Then: wts->n != rule->n_arrays; an
 * array that is S_t itself (the S or S_out buffer) with a weight other than 1.0, and a fused step
 * with more than 16 arrays (message "NotImplementedError: ..."; the streaming step takes all 64).
 * ------------------------------------------------------------------------------------------- */
typedef struct flsim_rule_weights {
    int32_t n;                   /* == rule->n_arrays */
    double w[FLSIM_MAX_ARRAYS];  /* weight of arrays[q]; rounded to fp32 once */
    double divisor;              /* rounded to fp32 once; > 0 */
} flsim_rule_weights;

int flsim_aggregate_optim_wrule_push(const float* S, float* S_out, const flsim_rule* rule,
                                     const flsim_rule_weights* wts, float* p, float* m, float* v,
                                     long P, const long* tensor_sizes, int n_tensors, long step,
                                     const flsim_optim* optim, flsim_stream_t stream);
int flsim_pn1_server_step_wrule(void* gradstate, float* S_out, const flsim_rule* rule,
                                const flsim_rule_weights* wts, float* p, float* m, float* v,
                                long step, const flsim_optim* optim, flsim_stream_t stream);
int flsim_vgg11_server_step_wrule(void* gradstate, float* S_out, const flsim_rule* rule,
                                  const flsim_rule_weights* wts, float* p, float* m, float* v,
                                  long step, const flsim_optim* optim, flsim_stream_t stream);
int flsim_vgg11_bn_server_step_wrule(void* gradstate, float* S_out, const flsim_rule* rule,
                                     const flsim_rule_weights* wts, float* p, float* m, float* v,
                                     long step, const flsim_optim* optim, flsim_stream_t stream);
/* host (testing): flsim_cascade_eval_host with the weighted rule's arithmetic: entry array q
 * enters as ys[q][e] * (float)w[q], out[e] = sum / (float)divisor */
int flsim_cascade_eval_host_w(const int32_t* prog, const int32_t* info, const float* S,
                              const float* const* ys, const double* w, int n_arrays,
                              double divisor, const uint8_t* tail, long n, float* out);

/* ---------------------------------------------------------------------------------------------
 * Delay-compensated rule (DC-ASGD, Zheng et al. 2017): a popped FIFO entry x = S_src, pushed when
 * the model was theta_src and popped when it is theta_now, is corrected for the distance the model
 * has moved before it enters the average.  These entry points run
 *
 *   def compensate(x, theta_now, theta_src, lam):          # per parameter tensor, fp32
 *       return x + (x * x) * lam * (theta_now - theta_src)
 *   def compensated_rule(ups_list, snaps, theta_now, lam, weights=None, normalize="weights"):
 *       ys = [u if s is None else [compensate(u[i], theta_now[i], s[i], lam) ...]
 *             for u, s in zip(ups_list, snaps)]
 *       return rule(ys) if weights is None else weighted_rule(ys, weights, normalize)
 *
 * fused with the update, bit-exact with torch 2.10 CPU: five fp32 roundings per element (x*x,
 * times f32(lambda), theta_now - theta_src, their product, the add), no contraction; lambda is
 * rounded to fp32 once; theta_now is p before this step's update.  Compensation comes first, then
 * the staleness weight (wts; NULL: none), the cascade sum and the division.  comp->theta_src[q] is
 * the snapshot of arrays[q]; NULL leaves that array as it stands, and a NULL array stays zero.  An
 * entry that is S_t is never compensated.  theta_out (nullable, 16-byte aligned): the pre-update p
 * is also written there in the same pass -- the snapshot of the entry a tick pushes into S_out.
 * comp == NULL and theta_out == NULL is the weighted entry point above.
 * Note: under the reference's aliasing an entry is S_src, a sum over that epoch's workers, so
 * x * x grows with the square of the worker count; lambda has to be chosen with that in mind.
 * Checked before any pointer, status 1: a lambda that is not finite and >= 0; comp->n !=
 * rule->n_arrays.  Then: a snapshot for an array that is the S or S_out buffer; theta_out aliasing
 * p or a snapshot read in the same launch; a fused step with more than 16 arrays (message
 * "NotImplementedError: ..."; the streaming step takes all 64).
 * ------------------------------------------------------------------------------------------- */
typedef struct flsim_rule_comp {
    int32_t n;                                /* == rule->n_arrays */
    double lambda;                            /* rounded to fp32 once; finite, >= 0 */
    const float* theta_src[FLSIM_MAX_ARRAYS]; /* snapshot of arrays[q]; NULL = not compensated */
} flsim_rule_comp;

int flsim_aggregate_optim_crule_push(const float* S, float* S_out, float* theta_out,
                                     const flsim_rule* rule, const flsim_rule_weights* wts,
                                     const flsim_rule_comp* comp, float* p, float* m, float* v,
                                     long P, const long* tensor_sizes, int n_tensors, long step,
                                     const flsim_optim* optim, flsim_stream_t stream);
int flsim_pn1_server_step_crule(void* gradstate, float* S_out, float* theta_out,
                                const flsim_rule* rule, const flsim_rule_weights* wts,
                                const flsim_rule_comp* comp, float* p, float* m, float* v,
                                long step, const flsim_optim* optim, flsim_stream_t stream);
int flsim_vgg11_server_step_crule(void* gradstate, float* S_out, float* theta_out,
                                  const flsim_rule* rule, const flsim_rule_weights* wts,
                                  const flsim_rule_comp* comp, float* p, float* m, float* v,
                                  long step, const flsim_optim* optim, flsim_stream_t stream);
int flsim_vgg11_bn_server_step_crule(void* gradstate, float* S_out, float* theta_out,
                                     const flsim_rule* rule, const flsim_rule_weights* wts,
                                     const flsim_rule_comp* comp, float* p, float* m, float* v,
                                     long step, const flsim_optim* optim, flsim_stream_t stream);
/* host (testing): flsim_cascade_eval_host_w with the compensation in front: entry array q with a
 * snapshot theta_src[q] enters as compensate(ys[q][e], theta_now[e], theta_src[q][e], lambda),
 * then times (float)w[q] (w == NULL: 1.0).  theta_src == NULL: no array is compensated. */
int flsim_cascade_eval_host_c(const int32_t* prog, const int32_t* info, const float* S,
                              const float* const* ys, const double* w, int n_arrays,
                              double divisor, const float* theta_now,
                              const float* const* theta_src, double lambda, const uint8_t* tail,
                              long n, float* out);

/* ---------------------------------------------------------------------------------------------
 * Global-norm gradient clipping: Central.update_model (agents.py:9-21) sets p.grad and steps in one
 * call; these entry points run what a torch user writes between the two,
 *
 *   total_norm = torch.nn.utils.get_total_norm(grads, 2.0)        # the engine's: see below
 *   torch.nn.utils.clip_grads_with_norm_(parameters, max_norm, total_norm)
 *   optim.step()
 *
 * on g = the rule's output (any of the rules above), in three launches: the rule streams g into
 * clip->G and one fp64 sum of squares per block into clip->partials; a one-block launch adds the
 * partials in index order and writes out[0] = total_norm, out[1] = coef; the update of `optim`
 * then runs on g * coef.
 *   total_norm = (float)sqrt(sum_e (double)g_e * (double)g_e): accumulated in fp64 (a square of an
 *     fp32 value is exact there) in an order the launch geometry alone fixes (no atomics), so the
 *     same shape gives the same bits on every run.  It is the correctly rounded norm; torch's own
 *     get_total_norm accumulates in fp32 and is up to 1e-4 relative below it.
 *   coef = min(RN(1 / (total_norm + f32(1e-6))) * f32(max_norm), 1.0f) in fp32, as
 *     clip_grads_with_norm_ computes max_norm / (total_norm + 1e-6) (a reciprocal and a multiply)
 *     and clamps it; a NaN norm gives a NaN coefficient.  max_norm = inf only reports the norm.
 *   g' = g * coef: one fp32 multiply, always applied (as torch always multiplies).
 * Only norm_type 2; error_if_nonfinite stays False.  S_out and theta_out are written by the first
 * launch as the entry points above write them.  The library still never allocates: the caller
 * provides G (P floats), partials (at least the doubles the launch sequence writes; the bound
 * below holds for any layout of at most 4096 tensors) and out (2 floats), all 16-byte aligned;
 * nothing depends on what they held before.  clip == NULL is the delay-compensated entry point
 * above.
 * Checked before any pointer, status 1: max_norm NaN or <= 0.  Then: a NULL or misaligned G /
 * partials / out; n_partials too small; G overlapping S, S_out, theta_out, p, m, v, an entry array
 * or a snapshot.
 * ------------------------------------------------------------------------------------------- */
typedef struct flsim_clip {
    float max_norm;   /* > 0; +inf: report the norm only */
    float* G;         /* [P] the rule's output g (scratch between the launches) */
    double* partials; /* [n_partials] per-block sums of squares */
    long n_partials;
    float* out;       /* [2]: total_norm, coef */
} flsim_clip;

long flsim_clip_partials(long P);
int flsim_aggregate_optim_clip_push(const float* S, float* S_out, float* theta_out,
                                    const flsim_rule* rule, const flsim_rule_weights* wts,
                                    const flsim_rule_comp* comp, const flsim_clip* clip, float* p,
                                    float* m, float* v, long P, const long* tensor_sizes,
                                    int n_tensors, long step, const flsim_optim* optim,
                                    flsim_stream_t stream);
/* host (testing): the rule's g as the host twins above give it (w == NULL and theta_src == NULL:
 * the plain mean sum / divisor), then the norm, the coefficient and g' of the text above:
 * g_out[e] = g[e] * coef, norm_coef[0] = total_norm, norm_coef[1] = coef.  The squares are summed
 * in fp64 in element order.  max_norm is refused as the entry point refuses it. */
int flsim_cascade_eval_host_clip(const int32_t* prog, const int32_t* info, const float* S,
                                 const float* const* ys, const double* w, int n_arrays,
                                 double divisor, const float* theta_now,
                                 const float* const* theta_src, double lambda, const uint8_t* tail,
                                 long n, double max_norm, float* g_out, float* norm_coef);

/* ---------------------------------------------------------------------------------------------
 * Measurement (no reference counterpart): HIP events around every worker-batched GEMM launch on
 * its stream, for bench.py's live roofline figure.  read() fills flsim_probe_kernel_count()
 * entries per kernel id (launches, total ms, total algorithmic FLOPs) and resets the record.
 * ------------------------------------------------------------------------------------------- */
int flsim_probe_enable(int capacity);
int flsim_probe_read(int* launches, double* total_ms, double* total_flops);
int flsim_probe_disable(void);
int flsim_probe_kernel_count(void);
const char* flsim_probe_kernel_name(int kid);

/* ---------------------------------------------------------------------------------------------
 * Robust rules: Agg(rule) (agents.py:43-45) takes any rule; these entry points run the
 * coordinate-wise median and the trimmed mean (Yin et al. 2018) over bucket means of the workers
 * (Karimireddy et al. 2022) fused with the update.  The text (flsim/robust.py, plain torch):
 *
 *   def _robust(cols, kind, trim):             # cols: [k, numel] fp32, already bucket means
 *       k = cols.shape[0]
 *       s = cols.sort(0).values                # ascending; -inf < finite < +inf < NaN
 *       if kind == "median":
 *           return s[(k - 1) // 2].clone()     # lower median
 *       xs = s[trim:k - trim]                  # drop the `trim` lowest and the `trim` highest
 *       acc = xs[0].clone()
 *       for r in xs[1:]:                       # sequential fp32 adds, ascending order
 *           acc += r
 *       return acc / (k - 2 * trim)            # one IEEE fp32 division
 *
 * Per element e: x_j = entries[j][e] / (float)count[j] (one IEEE fp32 division: the mean of bucket
 * j from its sum), g = _robust over the k values x_j, then the update of `optim` on g -- every kind
 * of flsim_optim, the same arithmetic and the same correctly rounded sqrt as the entry points above.
 * The result equals the text as a number: the same 32 bits wherever the text's value is neither
 * zero nor NaN, a zero (of either sign) where it is a zero, a NaN where it is a NaN (torch's sort
 * is stable, so the sign of a -0 / +0 tie follows the input order there; the sorting network
 * orders -0 below +0).  The rule has no tensor structure, hence no tensor_sizes.
 *   g_out (nullable, 16-byte aligned): g is also written there in the same pass.  optim == NULL
 *     with g_out != NULL writes g only and touches none of p / m / v (clip must then be NULL).
 *   clip != NULL: the launch stores g to clip->G and one fp64 sum of squares per block to
 *     clip->partials (deterministic; at most flsim_clip_partials(P) of them); the finish and apply
 *     launches of the clipped entry point above follow unchanged.
 * Checked before any pointer, status 1: an unknown kind; k outside [1, FLSIM_MAX_ARRAYS]; trim < 0
 * or 2 * trim >= k; trim != 0 with the median; a count < 1; what flsim_optim and flsim_clip are
 * refused for above.  Then: a NULL or misaligned p (m, v where the kind owns them), a misaligned
 * g_out or entry, P out of range, the clip buffers as above, and an entry overlapping p, m, v,
 * g_out or clip->G.
 * ------------------------------------------------------------------------------------------- */
#define FLSIM_ROBUST_MEDIAN 0
#define FLSIM_ROBUST_TRIMMED_MEAN 1
typedef struct flsim_robust {
    int32_t kind, trim, k;                      /* 1 <= k <= FLSIM_MAX_ARRAYS; trimmed mean: 2*trim < k */
    const float* entries[FLSIM_MAX_ARRAYS];     /* bucket / class SUMS; NULL = an all-zero entry */
    int32_t count[FLSIM_MAX_ARRAYS];            /* >= 1: entry value = entries[j][e] / count[j] */
} flsim_robust;
int flsim_robust_optim_step(const flsim_robust* r, const flsim_clip* clip, float* g_out,
                            float* p, float* m, float* v, long P, long step,
                            const flsim_optim* optim, flsim_stream_t stream);
/* host (testing): g of the text above for host pointers, through the same sorting network and
 * select / sum code the kernel runs; refuses what the entry point refuses about r */
int flsim_robust_eval_host(const flsim_robust* r, long P, float* g_out);

/* ---------------------------------------------------------------------------------------------
 * Krum and Multi-Krum (Blanchard et al. 2017) over bucket means, fused with the update: the
 * entry closest to its neighbours (Krum, m = 1) or the mean of the m such entries (Multi-Krum).
 * Unlike the rules above it is not coordinate-wise: the distances are over all P elements.  The
 * text (flsim/robust.py, plain torch):
 *
 *   def krum_select(cols, f, m):                 # cols: [k, numel] fp32, already bucket means
 *       k = cols.shape[0]
 *       x = cols.double()
 *       d = torch.stack([((x[i] - x) ** 2).sum(1) for i in range(k)])      # fp64
 *       d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
 *       score = []
 *       for i in range(k):
 *           row = torch.cat([d[i, :i], d[i, i + 1:]]).sort().values[:k - f - 2]
 *           acc = row[0].clone()
 *           for r in row[1:]:                    # ascending, sequential fp64 adds
 *               acc += r
 *           score.append(acc)
 *       order = sorted(range(k), key=lambda i: (score[i].item(), i))       # ties: lowest index
 *       return d, torch.stack(score), sorted(order[:m])                    # selection in index order
 *   def _krum(cols, f, m):
 *       _, _, sel = krum_select(cols, f, m)
 *       acc = cols[sel[0]].clone()
 *       for j in sel[1:]:                        # sequential fp32 adds, ascending entry index
 *           acc += cols[j]
 *       return acc / m                           # one IEEE fp32 division
 *
 * Per element x_j = entries[j][e] / (float)count[j] as for flsim_robust; a NULL entry is all zero.
 * Three launches on `stream`, no host synchronisation: the distance launch reads the entries once
 * and writes, per block, one fp64 sum of ((double)x_i - (double)x_j)^2 for every pair i < j (the
 * direct difference, never the Gram form) to s->partials; a one-block launch adds the partials in
 * block order, writes s->dist (symmetric: a pair is computed once and mirrored; zero diagonal; a
 * NaN distance becomes +inf, so a poisoned entry is never preferred), s->score and s->sel; the
 * apply launch reads sel on the device, loads the m selected entries only, forms g as the text
 * does and runs the update of `optim` (every kind).  No atomics: the grid and the element-to-block
 * map depend on (P, k) alone, so the same shape gives the same bits on every run.
 *   dist, score: each within 2 (P + 2) 2^-53 (dist) and twice that (score) of the text, relative;
 *   sel equal to the text's wherever the text's scores are further apart than that; g then equal
 *   bit for bit.
 * g_out, optim == NULL and clip as for flsim_robust_optim_step (clip: the apply launch stores g to
 * clip->G with one fp64 sum of squares per 256 elements; the finish and apply launches of the
 * clipped entry point follow unchanged).  The library never allocates: the caller provides the
 * scratch, and nothing depends on what it held before.
 * Checked before any pointer, status 1: k outside [3, FLSIM_MAX_ARRAYS]; f < 0 or k < 2f + 3;
 * m outside [1, k - f]; a count < 1; what flsim_optim and flsim_clip are refused for.  Then: what
 * flsim_robust_optim_step refuses about p / m / v / g_out / P / clip and the entries; a NULL or
 * misaligned (16 bytes) scratch pointer; n_partials too small; an entry overlapping the scratch.
 * ------------------------------------------------------------------------------------------- */
typedef struct flsim_krum {
    int32_t f, m, k;                            /* k >= 2f+3, 1 <= m <= k-f, k <= FLSIM_MAX_ARRAYS */
    const float* entries[FLSIM_MAX_ARRAYS];     /* bucket / class SUMS; NULL = all zero */
    int32_t count[FLSIM_MAX_ARRAYS];            /* >= 1 */
} flsim_krum;
typedef struct flsim_krum_scratch {             /* caller-provided; the library never allocates */
    double* partials; long n_partials;          /* >= flsim_krum_partials(P, k) */
    double* dist;                               /* [k*k] out: the distance matrix */
    double* score;                              /* [k]   out */
    int32_t* sel;                               /* [m]   out: selected entries, ascending */
} flsim_krum_scratch;
/* the doubles the distance launch writes for P elements and k entries (0: k or P out of range) */
long flsim_krum_partials(long P, int k);
/* (tests) the distance launch's tile: the elements of every entry a block stages at a time */
long flsim_krum_tile_elems(int k);
int flsim_krum_optim_step(const flsim_krum* r, const flsim_krum_scratch* s, const flsim_clip* clip,
                          float* g_out, float* p, float* m, float* v, long P, long step,
                          const flsim_optim* optim, flsim_stream_t stream);
/* host (testing): dist [k*k], score [k], sel [m] and g (g_out nullable) of the text for host
 * pointers: the distances summed in element order, then the score / selection code the finish
 * kernel runs; refuses what the entry point refuses about r */
int flsim_krum_eval_host(const flsim_krum* r, long P, double* dist, double* score, int32_t* sel,
                         float* g_out);

/* ---------------------------------------------------------------------------------------------
 * Bulyan (El Mhamdi, Guerraoui and Rouault 2018) over bucket means, fused with the update: Krum's
 * selection repeated until theta = k - 2f entries are chosen, then per coordinate the mean of the
 * beta = theta - 2f = k - 4f values closest to the median of the chosen ones.  The text
 * (flsim/robust.py, plain torch; d is krum_select's matrix):
 *
 *   def bulyan_order(d, f):
 *       k = d.shape[0]; left = list(range(k)); order, win = [], []
 *       for _ in range(k - 2 * f):
 *           r = len(left)
 *           if r == 1:                                # (only when f == 0)
 *               order.append(left[0]); win.append(0.0); break
 *           n = max(r - f - 2, 1); sc = {}
 *           for i in left:                            # ascending (value, index), sequential fp64 adds
 *               row = sorted((d[i, j].item(), j) for j in left if j != i)[:n]
 *               sc[i] = sum of row's values in that order
 *           w = min(left, key=lambda i: (sc[i], i))   # ties: lowest index
 *           order.append(w); win.append(sc[w]); left.remove(w)
 *       return order, win
 *   def _bulyan_coord(s_cols, f):                     # [theta, numel] fp32, the selected means
 *       sort ascending (NaN last); med = s[(theta - 1) // 2]; the window starts as {median} and
 *       grows beta - 1 times by the closer of its two outer neighbours: right iff a right
 *       neighbour exists and (no left neighbour or (s[hi + 1] - med) < (med - s[lo - 1]) in fp32;
 *       a false compare, ties and NaN included, goes left); g = the window's values added in
 *       ascending order, sequential fp32 adds, / float(beta)
 *
 * Per element x_j = entries[j][e] / (float)count[j] as for flsim_robust; a NULL entry is all zero.
 * Three launches on `stream`, no host synchronisation, no atomics: the distance launch of
 * flsim_krum_optim_step (same kernel, same geometry, same sums) into s->partials; a one-block launch
 * adds the partials in Krum's fixed order, writes s->dist (the matrix flsim_krum_optim_step and
 * flsim_nnm_entries write, bit for bit), ranks every row's neighbours once and runs the theta
 * rounds, writing s->score (the winning scores in round order), s->order and s->sel; the apply
 * launch reads sel on the device, loads the theta selected entries only, sorts them per element,
 * forms g as the text does and runs the update of `optim` (every kind).
 *   dist: within 2 (P + 2) 2^-53 relative of the text; order, score and sel equal, score bit for
 *   bit, the text's bulyan_order applied to the device's own dist; g equals _bulyan_coord over the
 *   device's own sel as numbers (the same 32 bits wherever the text's value is neither zero nor
 *   NaN, a zero where it gives a zero, a NaN where it gives a NaN).
 * g_out, optim == NULL and clip as for flsim_krum_optim_step.  The library never allocates: the
 * caller provides the scratch, and nothing depends on what it held before.
 * Checked before any pointer, status 1: k outside [3, FLSIM_MAX_ARRAYS]; f < 0 or k < 4f + 3; a
 * count < 1; what flsim_optim and flsim_clip are refused for.  Then: what flsim_krum_optim_step
 * refuses about p / m / v / g_out / P / clip and the entries; a NULL or misaligned (16 bytes)
 * scratch pointer; n_partials too small; an entry overlapping the scratch.
 * ------------------------------------------------------------------------------------------- */
typedef struct flsim_bulyan {
    int32_t f, k;                               /* k >= 4f+3, f >= 0, k <= FLSIM_MAX_ARRAYS */
    const float* entries[FLSIM_MAX_ARRAYS];     /* bucket / class SUMS; NULL = all zero */
    int32_t count[FLSIM_MAX_ARRAYS];            /* >= 1 */
} flsim_bulyan;
typedef struct flsim_bulyan_scratch {           /* caller-provided; the library never allocates */
    double* partials; long n_partials;          /* >= flsim_bulyan_partials(P, k) */
    double* dist;                               /* [k*k]   out: the distance matrix */
    double* score;                              /* [theta] out: the winning scores, round order */
    int32_t* order;                             /* [theta] out: the winners, round order */
    int32_t* sel;                               /* [theta] out: the winners, ascending */
} flsim_bulyan_scratch;
/* the doubles the distance launch writes: flsim_krum_partials(P, k) (0: P or k out of range) */
long flsim_bulyan_partials(long P, int k);
int flsim_bulyan_optim_step(const flsim_bulyan* r, const flsim_bulyan_scratch* s,
                            const flsim_clip* clip, float* g_out, float* p, float* m, float* v,
                            long P, long step, const flsim_optim* optim, flsim_stream_t stream);
/* host (testing): dist [k*k], score, order, sel [theta] and g (g_out nullable) of the text for host
 * pointers: the distances summed in element order, then the selection code the finish kernel runs
 * and the window / sum code the apply kernel runs; refuses what the entry point refuses about r */
int flsim_bulyan_eval_host(const flsim_bulyan* r, long P, double* dist, double* score,
                           int32_t* order, int32_t* sel, float* g_out);

/* ---------------------------------------------------------------------------------------------
 * Geometric median over bucket means by smoothed Weiszfeld iterations ("RFA", Pillutla, Kakade and
 * Harchaoui 2022), fused with the update.  Breakdown point 1/2, no Byzantine count from the user;
 * where Krum selects, it re-weights the entries continuously by 1 / distance to the iterate.  The
 * text (flsim/robust.py, plain torch):
 *
 *   def _seqsum(v):                    # sequential fp64 adds, index order
 *   def _wsum(x, w):                   # z = sum_j w[j] * x[j]: fp64, index order, one multiply and one add
 *                                      # per term (two roundings, never an fma); terms with w[j] == 0 are
 *                                      # skipped (not read); the first term kept initialises the sum
 *   def geomed_steps(cols, alpha, iters, nu):     # cols [k, numel] fp32 (bucket means), alpha [k] fp64 > 0
 *       x = cols.double()
 *       alive = torch.isfinite(x).all(1)          # an entry with any NaN / inf element is dead
 *       a = torch.where(alive, alpha, 0.0)
 *       if not alive.any(): return all-NaN g, ...
 *       w = [a / _seqsum(a)]                      # w^(0): z_0 is the alpha-weighted mean of the live entries
 *       d2, obj = [], []
 *       for r in range(iters):
 *           z = _wsum(x, w[r])
 *           d2_r = ((x - z) ** 2).sum(1); d2_r[~alive] = inf
 *           d = d2_r.sqrt()
 *           obj.append(_seqsum(a * d over the live entries))      # sum_j alpha_j ||x_j - z_r||
 *           beta = a / torch.maximum(d, nu)       # smoothed Weiszfeld weight; dead: 0
 *           w.append(beta / _seqsum(beta))
 *           d2.append(d2_r)
 *       g = _wsum(x, w[iters]).float()            # one fp64 -> fp32 rounding
 *       return g, w, d2, obj
 *
 * alpha_j = 1 (weighted = 0) or count[j] (weighted = 1: RFA's sample-count weights).  No early
 * stopping: that would need a host synchronisation.  Per element x_j = entries[j][e] /
 * (float)count[j] as for flsim_robust; a NULL entry is all zero.
 * iters + 1 pairs of (distance launch, one-block finish launch), then one apply launch, all on
 * `stream`, no host synchronisation, no atomics: the grid and the element-to-block map depend on
 * (P, k) alone, so the same shape gives the same bits on every run.  A distance launch reads the
 * live entries once as coalesced rows, forms z[e] exactly as _wsum does (zero-weight entries are
 * not loaded) and adds ((double)x_j - z)^2 into k fp64 sums a thread, reduced once per block into
 * s->partials.  Pair 0 takes w^(0) of "every entry alive" from the host and also notes which
 * entries hold a NaN or an inf.  A finish launch adds the partials in a fixed order and writes
 * d2, obj and the next w with the scalar fp64 code of the text (correctly rounded sqrt, max,
 * divide, sequential sums).  A dead entry makes pair 0's z a NaN: its finish then marks the dead
 * entries in s->state, rewrites w^(0) from the live ones and sets a "redo" word, and every later
 * pair acts as iteration (its index - 1); a pair whose iteration number equals iters returns at
 * once (with no dead entry: the last pair).  Every entry dead: g is all NaN.  The apply launch forms
 * z with w^(iters), g = (float)z, and runs the update of `optim` (every kind).
 *   d2[r]: within 2 (P + 2) 2^-53 relative of the text's distances at the device's own w[r]
 *   (z is then bit-identical; the summation order differs); w[r + 1] and obj[r] equal, bit for bit,
 *   the text's scalar code applied to d2[r]; g equals _wsum(x, w[iters]).float() bit for bit.
 * g_out, optim == NULL and clip as for flsim_krum_optim_step (clip: the apply launch stores g to
 * clip->G with one fp64 sum of squares per 256 elements; the finish and apply launches of the
 * clipped entry point follow unchanged).  The library never allocates: the caller provides the
 * scratch, and nothing depends on what it held before.
 * Checked before any pointer, status 1: k outside [1, FLSIM_MAX_ARRAYS]; iters outside
 * [0, FLSIM_GEOMED_MAX_ITERS]; nu NaN, inf or <= 0; weighted not 0 or 1; a count < 1; what
 * flsim_optim and flsim_clip are refused for.  Then: what flsim_krum_optim_step refuses about
 * p / m / v / g_out / P / clip and the entries; a NULL or misaligned (16 bytes) scratch pointer;
 * n_partials too small; an entry overlapping the scratch.
 * ------------------------------------------------------------------------------------------- */
#define FLSIM_GEOMED_MAX_ITERS 32
typedef struct flsim_geomed {
    int32_t iters, weighted, k;               /* 0..32; 0: alpha = 1, 1: alpha = count; 1..FLSIM_MAX_ARRAYS */
    double nu;                                /* finite, > 0 */
    const float* entries[FLSIM_MAX_ARRAYS];   /* bucket / class SUMS; NULL = all zero */
    int32_t count[FLSIM_MAX_ARRAYS];          /* >= 1: x_j[e] = entries[j][e] / (float)count[j] */
} flsim_geomed;
typedef struct flsim_geomed_scratch {         /* caller-provided, 16-byte aligned, never pre-initialised */
    double* partials; long n_partials;        /* >= flsim_geomed_partials(P, k) */
    double* w;                                /* [(iters + 1) * k] out: w^(0) .. w^(iters) */
    double* d2;                               /* [iters * k]       out: squared distances; +inf for a dead entry */
    double* obj;                              /* [iters]           out */
    int32_t* state;                           /* [k + 4] out: dead flags, then the control words the launches share */
} flsim_geomed_scratch;
/* the doubles a distance launch writes for P elements and k entries (0: k or P out of range) */
long flsim_geomed_partials(long P, int k);
/* (tests) the distance launch's tile: the elements of every entry a block takes at a time */
long flsim_geomed_tile_elems(int k);
int flsim_geomed_optim_step(const flsim_geomed* r, const flsim_geomed_scratch* s, const flsim_clip* clip,
                            float* g_out, float* p, float* m, float* v, long P, long step,
                            const flsim_optim* optim, flsim_stream_t stream);
/* host (testing): w [(iters + 1) * k], d2 [iters * k], obj [iters] and g (g_out nullable) of the
 * text for host pointers: the distances summed in element order, then the scalar code the finish
 * kernel runs; refuses what the entry point refuses about r */
int flsim_geomed_eval_host(const flsim_geomed* r, long P, double* w, double* d2, double* obj, float* g_out);

/* ---------------------------------------------------------------------------------------------
 * Simulated Byzantine workers: the omniscient attacks IPM (inner-product manipulation, Xie et al.
 * 2020: every Byzantine worker sends -eps * mu) and ALIE ("A Little Is Enough", Baruch et al. 2019:
 * every Byzantine worker sends mu - z * sigma) mixed into the bucket SUMS a robust step then reads.
 * mu and sigma are the coordinate-wise mean and population standard deviation of the honest parts'
 * means of the entries, unweighted: the simulator holds bucket sums, not per-worker gradients, so
 * with one worker a bucket this is the papers' definition and with larger buckets the attacker sees
 * sigma at bucket granularity.  The text (flsim/robust.py, plain torch):
 *
 *   def attack_vector(sums, honest, kind, strength):
 *       y  = [sums[j].double() / honest[j] for j in range(len(sums)) if honest[j] >= 1]   # IEEE fp64 division
 *       kh = len(y)
 *       mu = _seqsum(y) / kh                               # index order
 *       if kind == "ipm":
 *           b = mu * (-strength)
 *       else:                                              # alie
 *           var = _seqsum([(t - mu) * (t - mu) for t in y]) / kh      # population variance
 *           b = mu - _sqrt_rn(var) * strength              # correctly rounded sqrt, multiply, subtract
 *       return b.float()                                   # one fp64 -> fp32 rounding
 *   def attack_flat(sums, honest, byz, kind, strength):    # -> (entries, counts, b)
 *       entries[j] = sums[j] + b * float(byz[j])           # fp32: a multiply, then an add
 *                    where honest[j] >= 1 and byz[j] >= 1; b * float(byz[j]) where honest[j] == 0;
 *                    sums[j] itself (same bits) where byz[j] == 0
 *       counts[j]  = honest[j] + byz[j]
 *
 * fp64 throughout, one rounding per operation, never an fma.  One launch on `stream`: no
 * allocation, no synchronisation, no atomics and no reduction across elements; the result is
 * purely element-wise, so its bits cannot depend on the launch geometry.  A thread issues the loads
 * of all honest entries for its elements before any arithmetic, forms y_j, mu, var and b in fp64
 * registers in the text's order (correctly rounded divisions and sqrt), rounds b to fp32 once and
 * stores.  An entry with honest[j] >= 1 is read; an entry with byz[j] >= 1 is written; an entry
 * with honest[j] == 0 is never read (its previous contents, any bytes, do not matter); an entry
 * with byz[j] == 0 is never written.  b_out (nullable) receives the crafted vector b.  The result
 * equals attack_flat "as numbers" in the sense of flsim_robust_optim_step: the same 32 bits
 * wherever the text's value is neither zero nor NaN, a zero where it gives a zero, a NaN where it
 * gives a NaN.  A NaN or an inf in an honest entry propagates into b exactly as the text propagates
 * it: there is no dead-entry logic here.  P need not be a multiple of anything.
 * Checked before any pointer, status 1: an unknown kind; k outside [1, FLSIM_MAX_ARRAYS]; a strength
 * that is NaN, inf or < 0; a negative honest or byz; honest[j] + byz[j] == 0; no entry with
 * honest >= 1 (the attacker has nothing to observe: "ValueError: ..."); no entry with byz >= 1.
 * Then: a NULL or misaligned (16 bytes) entry (every entry is read or written); a misaligned
 * b_out; P outside [1, 2^31); two entries, or an entry and b_out, that overlap.
 * ------------------------------------------------------------------------------------------- */
#define FLSIM_ATTACK_IPM 0
#define FLSIM_ATTACK_ALIE 1
typedef struct flsim_attack {
    int32_t kind, k;                      /* FLSIM_ATTACK_*; 1 <= k <= FLSIM_MAX_ARRAYS */
    double  strength;                     /* ipm: eps; alie: z; finite, >= 0 */
    float*  entries[FLSIM_MAX_ARRAYS];    /* in/out bucket SUMS, updated in place */
    int32_t honest[FLSIM_MAX_ARRAYS];     /* >= 0: the honest workers summed into the entry */
    int32_t byz[FLSIM_MAX_ARRAYS];        /* >= 0: its Byzantine workers; honest[j] + byz[j] >= 1 */
} flsim_attack;
/* (tests) the launch's tile: the elements of every entry a block takes at a time (0: k out of range) */
long flsim_attack_tile_elems(int k);
int flsim_attack_entries(const flsim_attack* a, float* b_out /* nullable, [P] */, long P,
                         flsim_stream_t stream);
/* host (testing): the same for host pointers, by the same element code; refuses what the entry
 * point refuses */
int flsim_attack_eval_host(const flsim_attack* a, float* b_out, long P);

/* ---------------------------------------------------------------------------------------------
 * The optimised attacks Min-Max and Min-Sum (Shejwalkar and Houmansadr, NDSS 2021, "Manipulating
 * the Byzantine"): every Byzantine worker sends b = mu + gamma * p, p a perturbation direction and
 * gamma the largest coefficient at which b stays no farther (squared 2-norm over the whole model)
 * from any honest entry than the honest entries are from each other (Min-Max: the largest
 * distance; Min-Sum: the largest row sum of distances).  The inputs, the honest parts' means y_j
 * and mu, the mix and the read / write contract are flsim_attack's.  The text (flsim/robust.py:
 * opt_attack_flat, opt_gamma), with e_i = mu - y_i over the kh honest entries in index order:
 *
 *   p      = -mu ("unit": unnormalised, gamma absorbs 1 / |mu|), -_sqrt_rn(var) ("std": var as
 *            ALIE's) or -sign(mu) ("sign": sign(0) = 0, a NaN stays)
 *   a_i    = sum_e e_i * e_i,  c_i = sum_e e_i * p,  q = sum_e p * p     (fp64, element order)
 *   dist   = the pairwise-distance stage's matrix (flsim_krum / flsim_nnm: NaN -> +inf, a zero
 *            diagonal) over the fp32 means sums_j / honest_j of the honest entries alone
 *   gamma  = 0 where q == 0; else
 *     minmax: D = max dist, r_i = max(D - a_i, 0), gamma_i = (sqrt(c_i c_i + q r_i) - c_i) / q,
 *             gamma = the smallest gamma_i (a NaN if any is one)
 *     minsum: S = max_i sum_j dist[i][j], A = sum a_i, C = sum c_i, Q = kh q, r = max(S - A, 0),
 *             gamma = (sqrt(C C + Q r) - C) / Q
 *   b      = (float)(mu + p * (gamma * strength))
 *
 * the closed form of the paper's bisection (every constraint is a convex quadratic in gamma that
 * holds at 0).  fp64, one rounding per operation, never an fma, IEEE division, correctly rounded
 * sqrt.  Four launches on `stream`; no allocation, no host synchronisation, no atomics; the grids
 * depend on (P, k) alone:
 *   1. stats: one streaming pass over the honest entries; a thread forms y_j, mu, p and the
 *      2 kh + 1 products of its elements and adds them in a fixed order; a block writes its sums
 *      to s->partials.
 *   2. distances: the launch of flsim_krum_optim_step over the honest entries (same kernel).
 *   3. finish, one block: the distance matrix (Krum's order) -> s->dist; the stats partials in a
 *      fixed order -> s->stats (a at [0, kh), c at [64, 64 + kh), q at [128]); gamma -> s->gamma,
 *      and gamma * strength -> the last word of s->partials.
 *   4. mix: flsim_attack's launch, which reads that word as a launch-uniform scalar.
 * dist, a_i and q are within 2 (P + 2) 2^-53 relative of the text's, c_i within that times
 * sqrt(a_i q) absolute; gamma is opt_gamma of the device's own a, c, q, dist bit for bit; b and
 * the entries equal the text evaluated with the device's gamma "as numbers".  A NaN or an inf in
 * an honest entry propagates as the text propagates it.
 * Checked before any pointer, status 1: an unknown kind, then an unknown dir, then as flsim_attack.
 * Then the entries, b_out and P as flsim_attack; a NULL or misaligned (16 bytes) scratch pointer;
 * n_partials too small; an entry or b_out that overlaps the scratch; scratch buffers that overlap
 * each other.
 * ------------------------------------------------------------------------------------------- */
#define FLSIM_ATTACK_MINMAX 2
#define FLSIM_ATTACK_MINSUM 3
#define FLSIM_ATTACK_DIR_UNIT 0
#define FLSIM_ATTACK_DIR_STD 1
#define FLSIM_ATTACK_DIR_SIGN 2
#define FLSIM_ATTACK_OPT_STATS (2 * FLSIM_MAX_ARRAYS + 1)
typedef struct flsim_attack_opt {
    int32_t kind, dir, k;                 /* FLSIM_ATTACK_MINMAX / _MINSUM; FLSIM_ATTACK_DIR_* */
    double  strength;                     /* scales gamma: 1 is the paper's attack; finite, >= 0 */
    float*  entries[FLSIM_MAX_ARRAYS];    /* in/out bucket SUMS, updated in place */
    int32_t honest[FLSIM_MAX_ARRAYS];     /* as flsim_attack */
    int32_t byz[FLSIM_MAX_ARRAYS];
} flsim_attack_opt;
typedef struct flsim_attack_opt_scratch {  /* caller-provided, 16-byte aligned, never pre-initialised */
    double* partials; long n_partials;     /* >= flsim_attack_opt_partials(P, k) */
    double* dist;                          /* [k*k] out: the first kh*kh hold the kh x kh matrix */
    double* stats;                         /* [FLSIM_ATTACK_OPT_STATS] out: a, c, q */
    double* gamma;                         /* [1] out */
} flsim_attack_opt_scratch;
/* the doubles the stats and distance launches write, for any number of honest entries <= k
 * (0: P or k out of range) */
long flsim_attack_opt_partials(long P, int k);
/* (tests) the STATS launch's tile over kh honest entries (0: out of range); the mix launch's is
 * flsim_attack_tile_elems(k) */
long flsim_attack_opt_tile_elems(int kh);
int flsim_attack_opt_entries(const flsim_attack_opt* a, const flsim_attack_opt_scratch* s,
                             float* b_out /* nullable, [P] */, long P, flsim_stream_t stream);
/* host (testing): the same for host pointers by the same element and scalar code, the sums in
 * element order; dist [kh*kh], stats [FLSIM_ATTACK_OPT_STATS], gamma [1]; refuses what the entry
 * point refuses about a, the entries, b_out and P */
int flsim_attack_opt_eval_host(const flsim_attack_opt* a, double* dist, double* stats,
                               double* gamma, float* b_out, long P);

/* ---------------------------------------------------------------------------------------------
 * Nearest-neighbour mixing (NNM; Allouah, Farhadkhani, Guerraoui, Gupta, Pinot and Stephan 2023,
 * "Fixing by Mixing"): a pre-aggregation stage in front of any robust rule.  Every entry is
 * replaced by the mean of its k - f nearest entries, itself included; the rule then reads the
 * mixed entries with count 1.  An in-place transform of the bucket SUMS, like flsim_attack.  The
 * text (flsim/robust.py, plain torch):
 *
 *   def nnm_neighbours(cols, f):                 # cols: [k, numel] fp32, already bucket means
 *       k = cols.shape[0]
 *       x = cols.double()
 *       d = torch.stack([((x[i] - x) ** 2).sum(1) for i in range(k)])      # fp64, exactly symmetric
 *       d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
 *       d.fill_diagonal_(0.0)                    # an entry is always its own nearest neighbour
 *       nbr = []
 *       for i in range(k):
 *           order = sorted(range(k), key=lambda j: (d[i, j].item(), j))    # ties: lowest index
 *           nbr.append(sorted(order[:k - f]))    # the k - f nearest, in index order
 *       return d, nbr
 *   def _nnm(cols, f):
 *       _, nbr = nnm_neighbours(cols, f)
 *       out = []
 *       for i in range(cols.shape[0]):
 *           acc = cols[nbr[i][0]].clone()
 *           for j in nbr[i][1:]:                 # sequential fp32 adds, ascending entry index
 *               acc += cols[j]
 *           out.append(acc / (cols.shape[0] - f))    # one IEEE fp32 division
 *       return torch.stack(out)
 *
 * x_j[e] = entries[j][e] / (float)count[j], as flsim_robust forms the bucket means.  The diagonal
 * is zero even for an entry that holds a NaN: such an entry keeps itself among its neighbours and
 * stays NaN, and the rule behind treats it as it treats any poisoned entry; every other row sees
 * it at +inf, hence last.
 *
 * Three launches on `stream`; no allocation, no host synchronisation, no atomics; the grids and
 * the element-to-block maps depend on (P, k) alone.
 *   1. distances: the launch of flsim_krum_optim_step (same kernel, same geometry, same sums)
 *      into s->partials; it pads to 4 .. 64 rows with zero rows, so k = 1 and 2 take it too.
 *      Reads every entry once.
 *   2. finish, one block: adds the partials in Krum's fixed order (NaN -> +inf, mirrored, zero
 *      diagonal), writes s->dist, runs the neighbour selection (each row: k - f scans for the
 *      smallest (value, j) above the last one taken) and writes s->nbr.
 *   3. mix, element-wise and in place: a thread issues the loads of all k entries for its
 *      elements before any arithmetic or store, forms every x_j, then every y_i in the text's
 *      order (ascending j over the bits of nbr[i], sequential fp32 adds, never an fma, one IEEE
 *      division by (float)(k - f)) and stores y_i to entries[i].  Every element is read and
 *      written by one thread only, so in place needs no ordering between blocks.  Reads and
 *      writes k P floats once each; nothing is written past P.  P need not be a multiple of
 *      anything.
 * s->partials, s->dist and s->nbr are never read before they are written: their previous contents,
 * any bytes, do not matter.
 *
 * dist is within 2 (P + 2) 2^-53 relative of the text's (Krum's bound, from the same launch; the
 * same inputs give the same bits on every call, and identical rows give bit-identical sums).  nbr
 * equals the text's wherever the text's row i has its (k - f)-th and (k - f + 1)-th smallest
 * distances further apart than that; exact ties are broken by the lower index on both sides.
 * Given equal nbr, the mixed entries equal _nnm "as numbers" in the sense of
 * flsim_robust_optim_step.
 * Checked before any pointer, status 1: k outside [1, FLSIM_MAX_ARRAYS]; f < 0 or 2 f >= k; a
 * count < 1.  Then: a NULL or misaligned (16 bytes) entry (every entry is read and written: no
 * NULL "all-zero" entries here); P outside [1, 2^31); a NULL or misaligned (16 bytes) scratch
 * pointer; n_partials too small; two entries that overlap; an entry that overlaps the scratch;
 * scratch buffers that overlap each other.
 * ------------------------------------------------------------------------------------------- */
typedef struct flsim_nnm {
    int32_t f, k;                          /* 1 <= k <= FLSIM_MAX_ARRAYS, 0 <= 2f < k */
    float*  entries[FLSIM_MAX_ARRAYS];     /* in: bucket SUMS; out: the mixed MEANS (count 1), in place */
    int32_t count[FLSIM_MAX_ARRAYS];       /* >= 1: x_j[e] = entries[j][e] / (float)count[j] */
} flsim_nnm;
typedef struct flsim_nnm_scratch {         /* caller-provided, 16-byte aligned, never pre-initialised */
    double* partials; long n_partials;     /* >= flsim_nnm_partials(P, k) */
    double* dist;                          /* [k*k] out */
    uint64_t* nbr;                         /* [k] out: bit j of nbr[i] = entry j is a neighbour of i */
} flsim_nnm_scratch;
/* the doubles the distance launch writes: flsim_krum_partials(P, k) (0: P or k out of range) */
long flsim_nnm_partials(long P, int k);
/* (tests) the MIX launch's tile: the elements of every entry a block takes at a time (0: k out of
 * range); the distance launch's tile is flsim_krum_tile_elems(k) */
long flsim_nnm_tile_elems(int k);
int flsim_nnm_entries(const flsim_nnm* a, const flsim_nnm_scratch* s, long P, flsim_stream_t stream);
/* host (testing): dist [k * k], nbr [k] and the mixed entries (out nullable, [k * P] row-major) of
 * the text for host pointers: the distances summed in element order, then the selection and the
 * element code the kernels run; a->entries are left unmodified; refuses what the entry point
 * refuses about a's fields, and a NULL entry */
int flsim_nnm_eval_host(const flsim_nnm* a, long P, double* dist, uint64_t* nbr, float* out);

/* ---------------------------------------------------------------------------------------------
 * Centered clipping with a carried center ("CClip", Karimireddy, He and Jaggi 2021), fused with
 * the update.  The clipping center c of an epoch is the previous epoch's aggregate (all zero on
 * the first step): every entry is pulled towards the iterate with weight min(1, tau / distance),
 * so an entry far from where the model now is counts by tau / distance instead of whole or not at
 * all.  The text (flsim/robust.py, plain torch; _seqsum and _wsum as for flsim_geomed):
 *
 *   def cclip_steps(cols, center, alpha, iters, tau):     # cols [k, numel] fp32 (bucket means),
 *       x = cols.double()                                 # center [numel] fp32 or None (fresh)
 *       alive = torch.isfinite(x).all(1)                  # an entry with any NaN / inf element is dead
 *       a = torch.where(alive, alpha, 0.0)
 *       lam = a / _seqsum(a) if alive.any() else zeros    # every entry dead: g is the center
 *       u, w = [1.0], [zeros(k)]                          # v_l = u[l] * c + sum_j w[l][j] * x_j
 *       for r in range(iters):
 *           z = _wsum([c; x], [u[r]; w[r]])               # the center first; c is None: no such term
 *           d2_r = ((x - z) ** 2).sum(1); d2_r[~alive] = inf
 *           q = tau / sqrt(d2_r)                          # correctly rounded sqrt; d = 0: +inf
 *           s_r = q where q < 1, 1 where q >= 1, q (a NaN) otherwise; s_r[~alive] = 0
 *           t = lam * s_r; om = 1 - _seqsum(t)
 *           u.append(u[r] * om); w.append(w[r] * om + t)  # a multiply, then an add
 *       g = _wsum([c; x], [u[iters]; w[iters]]).float()   # one fp64 -> fp32 rounding
 *       return g, u, w, d2, s                             # and the next step's center is g
 *
 * The iterate v_l = v_(l-1) + sum_j lam_j s_j (x_j - v_(l-1)) is never materialised: it is the
 * affine combination above, so an iteration is one streaming distance launch (z formed on the fly
 * from the k + 1 fp64 weights) and a one-block finish launch, and one apply launch at the end forms
 * g, stores it to `center` (unclipped) and runs the update: 2 * iters + 1 launches on `stream`, no
 * temporary of P elements, no host synchronisation, no atomics; the grid and the element-to-block
 * map depend on (P, k) alone.  alpha_j, x_j, NULL entries, g_out, optim == NULL and clip as for
 * flsim_geomed_optim_step.  Pair 0 has w = 0, so z = c (+0 when fresh) and a NaN or an inf in an
 * entry cannot reach z: it notes the dead entries in its mask and there is no redo pass; later
 * pairs do not load the dead entries.  The center is not loaded while its weight u is +-0, nor at
 * all when fresh = 1.
 *   d2[r]: within 2 (P + 2) 2^-53 relative of the text's distances at the device's own u[r], w[r];
 *   s[r], u[r + 1], w[r + 1] equal, bit for bit, the text's scalar code applied to d2[r]; g equals
 *   the text's at the device's u[iters], w[iters] bit for bit, and `center` holds the bits of g.
 * Checked before any pointer, status 1: k outside [1, FLSIM_MAX_ARRAYS]; iters outside
 * [1, FLSIM_CCLIP_MAX_ITERS]; tau NaN, inf or <= 0; weighted not 0 or 1; fresh not 0 or 1; a
 * count < 1; what flsim_optim and flsim_clip are refused for.  Then: what flsim_geomed_optim_step
 * refuses about p / m / v / g_out / P / clip, the entries and the scratch; a NULL or misaligned
 * (16 bytes) center; the center overlapping p / m / v / g_out, clip G, the scratch or an entry.
 * ------------------------------------------------------------------------------------------- */
#define FLSIM_CCLIP_MAX_ITERS 32
typedef struct flsim_cclip {
    int32_t iters, weighted, k, fresh;        /* 1..32; 0: alpha = 1, 1: alpha = count; 1..FLSIM_MAX_ARRAYS;
                                                 fresh 1: the center counts as all zero and is NOT read */
    double tau;                               /* the clipping radius: finite, > 0 */
    const float* entries[FLSIM_MAX_ARRAYS];   /* bucket / class SUMS; NULL = all zero */
    int32_t count[FLSIM_MAX_ARRAYS];          /* >= 1: x_j[e] = entries[j][e] / (float)count[j] */
    float* center;                            /* [P], 16-byte aligned, non-NULL: read (unless fresh), then
                                                 overwritten with g */
} flsim_cclip;
typedef struct flsim_cclip_scratch {          /* caller-provided, 16-byte aligned, never pre-initialised */
    double* partials; long n_partials;        /* >= flsim_cclip_partials(P, k) */
    double* u;                                /* [iters + 1]       out: the center's weight in v_0 .. v_iters */
    double* w;                                /* [(iters + 1) * k] out: the entries' weights */
    double* d2;                               /* [iters * k]       out: squared distances; +inf for a dead entry */
    double* s;                                /* [iters * k]       out: min(1, tau / distance); 0 for a dead entry */
    int32_t* state;                           /* [k + 4] out: dead flags, then control words */
} flsim_cclip_scratch;
/* the doubles a distance launch writes for P elements and k entries (0: k or P out of range) */
long flsim_cclip_partials(long P, int k);
/* (tests) the distance launch's tile: the elements of every entry a block takes at a time */
long flsim_cclip_tile_elems(int k);
int flsim_cclip_optim_step(const flsim_cclip* r, const flsim_cclip_scratch* s, const flsim_clip* clip,
                           float* g_out, float* p, float* m, float* v, long P, long step,
                           const flsim_optim* optim, flsim_stream_t stream);
/* host (testing): u [iters + 1], w [(iters + 1) * k], d2 [iters * k], s [iters * k], g (g_out
 * nullable) and the next center (center_out nullable, [P]: the bits of g) of the text for host
 * pointers: the distances summed in element order, then the scalar code the finish kernel runs.
 * r->center is read unless fresh (then it may be NULL) and is not written; refuses what the entry
 * point refuses about r's numbers */
int flsim_cclip_eval_host(const flsim_cclip* r, long P, double* u, double* w, double* d2, double* s,
                          float* g_out, float* center_out);

#ifdef __cplusplus
}
#endif

#endif /* FLSIM_H */
