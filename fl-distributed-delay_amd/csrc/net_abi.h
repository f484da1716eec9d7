// The entry-point layer the network engines share (pn1_net.hip: PerformantNet1; vgg_net.hip: vgg11,
// vgg11_bn): argument checks, the batch-fill launches, and the bodies of the per-network C-ABI
// contract (include/flsim.h) that are the same for every network, as templates over a network
// description N:
//   Grad, Ws                   gradient-state, workspace layouts (Ws: x0, y, e2, loss_s, dlog, dh2)
//   HEAD, BATCH_NORM           width of the last layer's input; per-group BatchNorm statistics
//   grad(gs), ws(p, samples)   the layouts over a buffer
//   params(), head_w(), head_b()   parameter total, offsets of the last Linear's weight and bias
//   head_scale(dropout)        scale of a dropout in front of the last Linear
//   pack(g, theta, st)         re-pack theta's conv weights
//   forward(g, w, theta, S, workers, seed, dropout, train, bn_stats, st)   up to the last ReLU
//   eval_coef(w, running, st)  (BATCH_NORM only) eval-mode BatchNorm coefficients
//   backward(gs, g, w, theta, S, dropout, st)   from the head's dlog / dh2
//   join(gs, st)               st waits for work outstanding on the gradstate's own streams
//   plan(g, gs)                the step plan of the epoch's slab sum
// bn_stats and running are null for a network without BatchNorm.
#pragma once
#include "net_kernels.h"
#include "slabstep.h"

namespace flsim {

constexpr int MAX_PASS_SAMPLES = 16384;   // one pass's samples: the kernels' 32-bit index budget

inline int whole_groups(int n_samples) {
    return ceil_div(n_samples, SAMPLES_PER_WORKER) * SAMPLES_PER_WORKER;
}

// ---- argument checks (each computes the pass's padded sample count where there is one) -------
inline int check_chunk(int n_chunk_workers, int max_samples, int len_a, int len_b, int* S) {
    FLSIM_REQUIRE(n_chunk_workers > 0, "empty chunk");
    *S = n_chunk_workers * SAMPLES_PER_WORKER;
    FLSIM_REQUIRE(*S <= max_samples, "chunk of %d samples exceeds workspace (%d)", *S, max_samples);
    FLSIM_REQUIRE(*S <= MAX_PASS_SAMPLES, "chunk of %d samples exceeds the 32-bit index budget",
                  *S);
    FLSIM_REQUIRE(len_a > 0 && len_b > 0, "empty class list");
    return 0;
}

// an explicit batch, padded to whole 128-sample groups; batch_norm: one BatchNorm batch per
// group, so only whole groups
inline int check_batch(int n_samples, int max_samples, bool batch_norm, int* S) {
    FLSIM_REQUIRE(n_samples > 0, "empty batch");
    FLSIM_REQUIRE(!batch_norm || n_samples % SAMPLES_PER_WORKER == 0,
                  "vgg11_bn batch of %d samples: must be a multiple of %d", n_samples,
                  SAMPLES_PER_WORKER);
    *S = whole_groups(n_samples);
    FLSIM_REQUIRE(*S <= max_samples, "batch of %d samples exceeds workspace (%d)", n_samples,
                  max_samples);
    FLSIM_REQUIRE(*S <= MAX_PASS_SAMPLES, "batch of %d samples exceeds the 32-bit index budget",
                  n_samples);
    return 0;
}

inline int check_row_range(int row0, int rows, int max_samples) {
    FLSIM_REQUIRE(row0 >= 0 && row0 % SAMPLES_PER_WORKER == 0,
                  "row0 %d is not a multiple of %d", row0, SAMPLES_PER_WORKER);
    FLSIM_REQUIRE((long)row0 + rows <= max_samples, "rows [%d, %d) exceed workspace (%d)", row0,
                  row0 + rows, max_samples);
    FLSIM_REQUIRE(max_samples <= MAX_PASS_SAMPLES,
                  "workspace of %d samples exceeds the 32-bit index budget", max_samples);
    return 0;
}

// an explicit batch staged into workspace rows [row0, row0 + S)
inline int check_batch_rows(int n_samples, int row0, int max_samples, int* S) {
    FLSIM_REQUIRE(n_samples > 0, "empty batch");
    *S = whole_groups(n_samples);
    return check_row_range(row0, *S, max_samples);
}

inline int check_row_count(int n_rows, int max_samples) {
    FLSIM_REQUIRE(n_rows > 0 && n_rows % SAMPLES_PER_WORKER == 0 && n_rows <= max_samples &&
                  n_rows <= MAX_PASS_SAMPLES, "bad row count %d (workspace %d)", n_rows,
                  max_samples);
    return 0;
}

inline int check_eval_samples(int max_samples) {
    FLSIM_REQUIRE(max_samples >= SAMPLES_PER_WORKER && max_samples % SAMPLES_PER_WORKER == 0,
                  "max_samples must be a positive multiple of %d", SAMPLES_PER_WORKER);
    return 0;
}

// workspace_offset: tensor `which` of a layout over `fake`
inline int tensor_offset(const void* const* tensors, int n, const char* fake, int which,
                         long* offset_bytes) {
    FLSIM_REQUIRE(offset_bytes, "null pointer");
    FLSIM_REQUIRE(which >= 0 && which < n, "bad workspace id %d", which);
    *offset_bytes = (long)((const char*)tensors[which] - fake);
    return 0;
}

// ---- batch fills: S blocks write x0 [S][32][32][4] and y [S] ---------------------------------
// where a chunk's samples are drawn from (main.py:154-169: each worker's two classes)
struct ChunkSrc {
    const uint8_t* pool;
    const int32_t* labels;
    const int32_t* list_a;
    int len_a;
    const int32_t* list_b;
    int len_b;
    const float* lut;
    int n_workers_total;
    bool complete() const { return pool && labels && list_a && list_b && lut; }
};

inline int fill_batch(const ChunkSrc& c, const WorkerRec* workers, uint64_t seed, float* x0,
                      int32_t* y, int S, hipStream_t st) {
    hipLaunchKernelGGL(k_fill_batch, dim3(S), dim3(256), 0, st, c.pool, c.labels, c.list_a, c.len_a,
                       c.list_b, c.len_b, workers, c.n_workers_total, seed, c.lut, x0, y);
    FLSIM_LAUNCH_CHECK();
    return 0;
}

// an explicit NCHW fp32 batch (labels: nullable)
inline int load_input(const float* x, const int64_t* labels, int n_samples, float* x0, int32_t* y,
                      int S, hipStream_t st) {
    hipLaunchKernelGGL(k_load_input, dim3(S), dim3(256), 0, st, x, labels, n_samples, x0, y);
    FLSIM_LAUNCH_CHECK();
    return 0;
}

inline int fill_seq(const uint8_t* pool, int first, int n, const float* lut, float* x0, int32_t* y,
                    int S, hipStream_t st) {
    hipLaunchKernelGGL(k_fill_seq, dim3(S), dim3(256), 0, st, pool, first, n, lut, x0, y);
    FLSIM_LAUNCH_CHECK();
    return 0;
}

// ---- the shared bodies -------------------------------------------------------------------------
// forward, last Linear + CrossEntropyLoss (main.py:107) of rows [0, S): worker_loss[g] = group g's
// loss; backward_pass: dlog and dh2 (the CE gradient times gscale) are written for the backward
template <class N>
static int forward_loss(const typename N::Grad& g, const typename N::Ws& w, const float* theta,
                        int S, const WorkerRec* workers, uint64_t seed, int dropout,
                        int backward_pass, float gscale, float* worker_loss, float* bn_stats,
                        hipStream_t st) {
    RC(N::forward(g, w, theta, S, workers, seed, dropout, 1, bn_stats, st));
    return head_and_loss<N::HEAD>(w.e2, theta + N::head_w(), theta + N::head_b(), w.y, w.loss_s,
                                  w.dlog, w.dh2, S, backward_pass, N::head_scale(dropout), gscale,
                                  worker_loss, st, workers);
}

template <class N>
static int run_chunk(void* gradstate, const typename N::Ws& w, const float* theta,
                     const WorkerRec* workers, int S, uint64_t seed, int dropout,
                     int backward_pass, float gscale, float* worker_loss, float* bn_stats,
                     hipStream_t st) {
    const typename N::Grad g = N::grad(gradstate);
    RC(forward_loss<N>(g, w, theta, S, workers, seed, dropout, backward_pass, gscale, worker_loss,
                       bn_stats, st));
    if (backward_pass) RC(N::backward(gradstate, g, w, theta, S, dropout, st));
    return 0;
}

template <class N>
static int net_fwd_bwd_chunk(void* gradstate, void* workspace, int max_samples, const float* theta,
                             const ChunkSrc& src, const WorkerRec* workers, int n_chunk_workers,
                             uint64_t seed, int dropout, int backward_pass, float* worker_loss,
                             float* bn_stats, hipStream_t stream) {
    FLSIM_REQUIRE(gradstate && workspace && theta && src.complete() && workers && worker_loss,
                  "null pointer");
    int S;
    RC(check_chunk(n_chunk_workers, max_samples, src.len_a, src.len_b, &S));
    RC(N::join(gradstate, stream));
    const typename N::Ws w = N::ws(workspace, max_samples);
    RC(fill_batch(src, workers, seed, w.x0, w.y, S, stream));
    return run_chunk<N>(gradstate, w, theta, workers, S, seed, dropout, backward_pass,
                        1.f / SAMPLES_PER_WORKER, worker_loss, bn_stats, stream);
}

// explicit batch (the Worker.fwd_bkwd(inp, outp) facade, agents.py:32-35): x NCHW fp32, y int64,
// any n_samples (main.py:43-44 --batch_size); the batch is padded to whole 128-sample groups
// (padding has zero loss and gradient) and the CE gradient is the mean over the n samples.
// workers[ceil(n/128)] give each group's dropout key; worker_loss[g] = group g's loss sum / 128.
template <class N>
static int net_fwd_bwd_input(void* gradstate, void* workspace, int max_samples, const float* theta,
                             const float* x, const int64_t* y, int n_samples,
                             const WorkerRec* workers, uint64_t seed, int dropout,
                             int backward_pass, float* worker_loss, float* bn_stats,
                             hipStream_t stream) {
    FLSIM_REQUIRE(gradstate && workspace && theta && x && y && workers && worker_loss,
                  "null pointer");
    int S;
    RC(check_batch(n_samples, max_samples, N::BATCH_NORM, &S));
    RC(N::join(gradstate, stream));
    const typename N::Ws w = N::ws(workspace, max_samples);
    RC(load_input(x, y, n_samples, w.x0, w.y, S, stream));
    return run_chunk<N>(gradstate, w, theta, workers, S, seed, dropout, backward_pass,
                        N::BATCH_NORM ? 1.f / SAMPLES_PER_WORKER : 1.f / (float)n_samples,
                        worker_loss, bn_stats, stream);
}

// Evaluation (util.py:31-45 print_test_accuracy after central.model.eval(), main.py:190: dropout
// off, BatchNorm on the running buffers): forward in pieces of at most max_samples, argmax of the
// logits into pred[n_images].  The input is pool images [first, first + n_images), or, with xin,
// an explicit NCHW fp32 batch.  Re-packs theta (the next begin_epoch packs again).
template <class N>
static int net_eval(void* gradstate, void* workspace, int max_samples, const float* theta,
                    const uint8_t* pool, int first, int n_images, const float* lut,
                    const float* xin, const float* running, int32_t* pred, hipStream_t stream) {
    FLSIM_REQUIRE(gradstate && workspace && theta && (xin || (pool && lut)) && pred,
                  "null pointer");
    FLSIM_REQUIRE(!N::BATCH_NORM || running, "null running buffers");
    FLSIM_REQUIRE(n_images > 0 && first >= 0, "bad image range");
    RC(check_eval_samples(max_samples));
    RC(N::join(gradstate, stream));
    const typename N::Grad g = N::grad(gradstate);
    const typename N::Ws w = N::ws(workspace, max_samples);
    RC(N::pack(g, theta, stream));
    if constexpr (N::BATCH_NORM) RC(N::eval_coef(w, running, stream));
    const int cap = max_samples < MAX_PASS_SAMPLES ? max_samples : MAX_PASS_SAMPLES;
    for (int c0 = 0; c0 < n_images; c0 += cap) {
        const int n = n_images - c0 < cap ? n_images - c0 : cap;
        const int S = whole_groups(n);
        if (xin)
            RC(load_input(xin + (long)c0 * 3072, nullptr, n, w.x0, w.y, S, stream));
        else
            RC(fill_seq(pool, first + c0, n, lut, w.x0, w.y, S, stream));
        RC(N::forward(g, w, theta, S, nullptr, 0, 0, 0, nullptr, stream));
        RC(head_predict<N::HEAD>(w.e2, theta + N::head_w(), theta + N::head_b(), w.y, w.loss_s, S,
                                 pred + c0, n, stream));
    }
    return 0;
}

// S_t (torch named_parameters layout, params() floats) = sum of the epoch's slabs (fixed order)
template <class N>
static int net_end_epoch(void* gradstate, float* grad_out, hipStream_t stream) {
    FLSIM_REQUIRE(gradstate && grad_out, "null pointer");
    RC(N::join(gradstate, stream));
    const typename N::Grad g = N::grad(gradstate);
    return slab_step_launch((float*)gradstate, N::plan(g, gradstate), g.cnt_off, g.part_off,
                            grad_out, nullptr, nullptr, nullptr, nullptr, nullptr, N::params(),
                            stream);
}

// the same reduction fused with rule() + the update rule of `optim` (include/flsim.h: SGD, Adam
// with weight decay, AdamW), world = 1
// wts (nullable): the staleness-weighted rule (include/flsim.h)
// comp (nullable), theta_out (nullable): delay compensation and the snapshot write; either one
// selects the compensated step, which runs in the weighted form (wts == NULL: weights 1.0 and the
// divisor k)
template <class N>
static int net_server_step_crule(void* gradstate, float* S_out, float* theta_out,
                                 const flsim_rule* rule, const flsim_rule_weights* wts,
                                 const flsim_rule_comp* comp, float* p, float* m, float* v,
                                 long step, const flsim_optim* optim, hipStream_t stream) {
    RC(check_optim(optim));
    RC(check_weights(wts));
    RC(check_comp(comp, rule));
    const bool cform = comp != nullptr || theta_out != nullptr;
    const int nstate = optim_n_state(optim);
    FLSIM_REQUIRE(gradstate && rule && p && (m || nstate < 1) && (v || nstate < 2),
                  "null pointer");
    RC(N::join(gradstate, stream));
    const typename N::Grad g = N::grad(gradstate);
    RuleProg R;
    RC(make_rule(rule, &R));
    OptLaunch ol;
    RC(make_opt_launch(optim, wts ? wts->divisor : (double)rule->k, step, &ol));
    float w[STEP_MAX_WARR];
    if (wts) RC(make_weights(rule, wts, S_out, nullptr, w, STEP_MAX_WARR));
    CompLaunch cl;
    if (cform) {
        FLSIM_REQUIRE(rule->n_arrays <= STEP_MAX_WARR, "NotImplementedError: compensated rule "
                      "with %d arrays in this step (max %d)", rule->n_arrays, STEP_MAX_WARR);
        if (!wts) unit_weights(rule->n_arrays, w);
        RC(make_comp(rule, comp, nullptr, S_out, theta_out, p, STEP_MAX_CARR, &cl));
    }
    return slab_step_launch_optim((float*)gradstate, N::plan(g, gradstate), g.cnt_off, g.part_off,
                                  S_out, &R, ol, p, m, v, N::params(), stream,
                                  (wts || cform) ? w : nullptr, cform ? &cl : nullptr);
}

template <class N>
static int net_server_step_wrule(void* gradstate, float* S_out, const flsim_rule* rule,
                                 const flsim_rule_weights* wts, float* p, float* m, float* v,
                                 long step, const flsim_optim* optim, hipStream_t stream) {
    return net_server_step_crule<N>(gradstate, S_out, nullptr, rule, wts, nullptr, p, m, v, step,
                                    optim, stream);
}

template <class N>
static int net_server_step_optim(void* gradstate, float* S_out, const flsim_rule* rule, float* p,
                                 float* m, float* v, long step, const flsim_optim* optim,
                                 hipStream_t stream) {
    return net_server_step_wrule<N>(gradstate, S_out, rule, nullptr, p, m, v, step, optim, stream);
}

// ... with Adam(lr, betas, eps)
template <class N>
static int net_server_step(void* gradstate, float* S_out, const flsim_rule* rule, float* p,
                           float* m, float* v, long step, double lr, double beta1, double beta2,
                           double eps, hipStream_t stream) {
    const flsim_optim o = adam_optim(lr, beta1, beta2, eps);
    return net_server_step_optim<N>(gradstate, S_out, rule, p, m, v, step, &o, stream);
}

}  // namespace flsim
