// Fused end of a server step (SURVEY 8 a6 + a8 + a9) over the weight-gradient slabs the networks'
// GEMMs accumulate during an epoch:
//
//   S_t = sum_z slab[z]                 agents.py:35 -- .grad accumulates over the epoch's workers
//   [S_out = S_t]                       main.py:156,161 -- the slow worker's FIFO entry (a tick)
//   g   = rule(weight_ups)              main.py:23-25  -- cascade mean over [S_t]*c + stale entries
//   Adam(p, m, v, g)                    agents.py:9-21 -- Central.update_model
//
// in ONE launch that streams every slab byte once.  A network describes its slabs as segments
// (one per parameter tensor: slab base, split count Z, slab row length n, where the tensor sits in
// the flat parameter vector, and the packed-conv layout that maps a slab column to torch's
// [co][ci][kh][kw]).  The planner cuts each segment into units of <= UNIT_FLOATS slab floats:
// 256 slab columns x a z-range.  A tile whose z-range is split over several units is finished by
// the unit that arrives last (counter per tile); its partials are handed over through sc1
// stores / loads (agent scope), the in-launch split-K recipe of cdna_hip_programming.md §5.
#pragma once
#include <stdint.h>

#include "cascade.h"
#include "common.h"
#include "flsim.h"

namespace flsim {

constexpr int STEP_MAX_SEG = 40;      // parameter tensors per network (vgg11_bn: 38)
constexpr int RULE_MAX_ARR = FLSIM_MAX_ARRAYS;   // weight_ups arrays besides S_t per launch
constexpr int RULE_INL_PROG = 192;    // program words carried in the kernel arguments
// arrays of a weighted rule in the fused step: its argument block (the segments take 2.5 KB of the
// 4 KB) has room for this many weights; the streaming step carries RULE_MAX_ARR
constexpr int STEP_MAX_WARR = 16;
// Delay compensation (the C kernels): the fused step takes a snapshot for each of its (at most
// STEP_MAX_WARR) arrays.  Its argument block has 8 bytes left, which theta_out takes, so the
// snapshot of R.arr[q] rides in the unused upper part of R.arr, at R.arr[STEP_SNAP0 + q]; the
// streaming step carries RULE_MAX_ARR snapshots in a field of its own.
constexpr int STEP_MAX_CARR = 16;
constexpr int STEP_SNAP0 = 32;
static_assert(STEP_MAX_CARR <= STEP_MAX_WARR && STEP_SNAP0 >= STEP_MAX_WARR &&
              STEP_SNAP0 + STEP_MAX_CARR <= RULE_MAX_ARR, "snapshots in the free part of R.arr");
constexpr long STEP_UNIT_FLOATS = 65536;

// host description of one parameter tensor's gradient slabs (offsets in floats)
struct SegSpec {
    long slab_off;     // slab [Z][n] at gradstate + slab_off
    int Z;
    long n;
    long toff, numel;  // the tensor in the flat named_parameters vector
    int CO, CI, CIP, KP;   // packed conv layout n = CO * KP, column = co*KP + khkw*CIP + ci; CO = 0: identity
    int group = -1;        // slab-row group whose rows in use this epoch are tracked (-1: all Z)
};

// planned segment (kernel argument)
struct SlabSeg {
    long slab_off;
    int Z, n, zc, nz, tiles, tpu, unit0, tile0, toff, numel;
    uint16_t CO, CI, CIP, KP;
    uint16_t wide;   // identity layout, 16-B aligned, no row_sum tail: 1024-element float4 tiles
    int16_t group;   // SegSpec::group
    int zlim;        // rows [0, zlim) hold this epoch's sums (set per launch; the rest are stale)
};

struct StepPlan {
    SlabSeg seg[STEP_MAX_SEG];
    int nseg, units, ctiles;
    long slab_floats;     // sum of Z * n (the slab bytes the step streams / 4)
    int u_wide, u_conv;   // first unit of the wide (class 1) and packed conv (class 2) segments
};

// wide (float4) tiles: identity layout, 16-B aligned, no row_sum tail, a real weight matrix
inline bool seg_wide(const SegSpec& s) {
    return s.CO == 0 && s.n % 4 == 0 && s.toff % 4 == 0 && s.numel % 32 == 0 && s.n >= 4096;
}

// Dispatch order of the units: small tensors first (biases, the head, conv1: few units, each a
// long serial z-reduction), then the wide segments (the linear layers: many short units) and the
// packed conv segments (uniform 256 KB streaming units) interleaved in proportion (the kernel
// maps block positions onto the two runs), so the units that carry most of the rule() program's
// arithmetic (the linear layers' elements) run beside the ones that carry most of the slab bytes.
inline int seg_class(const SegSpec& s) { return s.n < 4096 ? 0 : (seg_wide(s) ? 1 : 2); }

inline int plan_step(const SegSpec* s_in, int nseg, StepPlan* P) {
    if (nseg > STEP_MAX_SEG) return 1;
    SegSpec s[STEP_MAX_SEG];
    int k = 0;
    for (int pass = 0; pass < 3; ++pass)
        for (int i = 0; i < nseg; ++i)
            if (seg_class(s_in[i]) == pass) s[k++] = s_in[i];
    P->nseg = nseg;
    int u = 0, ct = 0;
    long sf = 0;
    P->u_wide = P->u_conv = -1;
    for (int i = 0; i < nseg; ++i) {
        SlabSeg& g = P->seg[i];
        if (P->u_wide < 0 && seg_class(s[i]) >= 1) P->u_wide = u;
        if (P->u_conv < 0 && seg_class(s[i]) == 2) P->u_conv = u;
        g.slab_off = s[i].slab_off;
        g.Z = s[i].Z;
        g.n = (int)s[i].n;
        g.toff = (int)s[i].toff;
        g.numel = (int)s[i].numel;
        g.CO = (uint16_t)s[i].CO;
        g.CI = (uint16_t)s[i].CI;
        g.CIP = (uint16_t)s[i].CIP;
        g.KP = (uint16_t)s[i].KP;
        g.wide = seg_wide(s[i]);
        g.group = (int16_t)s[i].group;
        g.zlim = g.Z;
        g.tiles = (int)((s[i].n + (g.wide ? 1023 : 255)) / (g.wide ? 1024 : 256));
        const long tile_f = (g.wide ? 1024L : 256L) * s[i].Z;
        // wide tiles: 64 KB units (one tile of a few rows per block: many blocks in flight)
        const long unit_f = g.wide ? STEP_UNIT_FLOATS / 4 : STEP_UNIT_FLOATS;
        int units;
        if (tile_f <= unit_f) {
            g.nz = 1;
            g.zc = g.Z;
            long tpu = unit_f / tile_f;
            if (tpu > (g.wide ? 1 : 4)) tpu = g.wide ? 1 : 4;   // short units, no serial tails
            g.tpu = (int)(tpu < g.tiles ? tpu : g.tiles);
            units = (g.tiles + g.tpu - 1) / g.tpu;
            g.tile0 = 0;
        } else {
            int nz = (int)((tile_f + unit_f - 1) / unit_f);
            g.zc = (g.Z + nz - 1) / nz;
            g.zc = (g.zc + 3) / 4 * 4;
            g.nz = (g.Z + g.zc - 1) / g.zc;
            g.tpu = 1;
            units = g.tiles * g.nz;
            g.tile0 = ct;
            ct += g.tiles;
        }
        g.unit0 = u;
        u += units;
        sf += (long)s[i].Z * s[i].n;
    }
    P->units = u;
    if (P->u_wide < 0) P->u_wide = u;
    if (P->u_conv < 0) P->u_conv = u;
    P->ctiles = ct;
    P->slab_floats = sf;
    return 0;
}

// Adam hyper-parameters + rule() divisor, prepared on the host (agents.py:9-21, main.py:106)
struct AdamConst {
    float w1, b2, w2, bc2s, rbc2s, eps, neg_ss, fk, rk;
    float lam;      // delay compensation's lambda (C kernels only); sits in what was padding, so
                    // no argument offset of the other kernels moves
};

// The update rule a launch applies (compile-time: the kinds differ in the arrays they stream).
//   OK_ADAM   torch.optim.Adam, no weight decay: p, m, v
//   OK_ADAMD  Adam with weight_decay (coupled L2) or AdamW (decoupled): p, m, v
//   OK_SGDM   torch.optim.SGD with momentum != 0: p and the momentum buffer in m; v untouched
//   OK_SGD    torch.optim.SGD with momentum == 0: p only; m and v untouched
//   OK_GOUT   no update (the clipped step's first launch, k_agg_stream only): g = rule() is stored
//             to G and its squares are summed per block; p is read by the C form alone
//   OK_ADAGRAD  torch.optim.Adagrad: p and the accumulator `sum` in m; v untouched
//   OK_YOGI     Yogi in the FedYogi form (no bias correction): p, m, v
enum OptKind { OK_ADAM = 0, OK_ADAMD = 1, OK_SGDM = 2, OK_SGD = 3, OK_GOUT = 4, OK_ADAGRAD = 5,
               OK_YOGI = 6 };
constexpr int opt_n_state(int ok) {
    return (ok <= OK_ADAMD || ok == OK_YOGI) ? 2 : ((ok == OK_SGDM || ok == OK_ADAGRAD) ? 1 : 0);
}
// the same count from a checked flsim_optim (check_optim), before its OptLaunch is made
inline int optim_n_state(const flsim_optim* o) {
    if (o->kind == FLSIM_OPT_ADAGRAD) return 1;
    return o->kind == FLSIM_OPT_SGD ? (o->momentum != 0.0 ? 1 : 0) : 2;
}

// what the kinds other than OK_ADAM need besides AdamConst (whose fk, rk every kind uses)
// OK_ADAGRAD reads AdamConst.eps and OptConst.wd / neg_lr / flags (OF_WD); OK_YOGI reads
// AdamConst.w1 / w2 / eps and the same three OptConst fields
enum { OF_DECOUPLED = 1, OF_WD = 2, OF_NESTEROV = 4, OF_FIRST = 8 };
struct OptConst {
    float wd;       // weight_decay; OK_ADAMD decoupled: f32(1 - lr * weight_decay)
    float mu;       // momentum
    float omd;      // f32(1 - dampening)
    float neg_lr;   // f32(-lr); OK_ADAGRAD: f32(-clr), clr = lr / (1 + (step - 1) * lr_decay)
    int flags;      // OF_*: decoupled decay, weight_decay != 0, nesterov, step 1 (buf = g)
};

// rule(): which program and which arrays (host side, see flsim_rule in include/flsim.h)
struct RuleProg {
    const int32_t* prog;            // device program, or nullptr: iprog
    int32_t iprog[RULE_INL_PROG];
    CascInfo info;
    int narr;
    const float* arr[RULE_MAX_ARR]; // nullptr entry = zeros (torch-1.x stale semantics)
    int distinct;                   // distinct non-null arrays (algorithmic bytes)
};

// gradstate extras the fused step needs: tile counters (zeroed with the slabs) and partials
inline long step_counter_floats(const StepPlan& P) { return (P.ctiles + 63) / 64 * 64; }
inline long step_partial_floats(const StepPlan& P) { return (long)P.units * 1024; }

// launch: S_out (nullable) receives S_t in the flat layout; rule == nullptr: reduce only (the
// network's end_epoch); else rule() + Adam on p, m, v
int slab_step_launch(float* gradstate, const StepPlan& plan, long cnt_off, long part_off,
                     float* S_out, const RuleProg* rule, const AdamConst* ac, float* p, float* m,
                     float* v, long P, hipStream_t stream);

// a validated flsim_optim in launch form: the kernel kind and its constants
struct OptLaunch {
    int ok;         // OptKind
    AdamConst ac;
    OptConst oc;
};
// the same with a chosen update rule; m / v may be null where the kind does not own them
// weights (nullable): the staleness-weighted rule, weights[q] (fp32) of rule->arr[q], at most
// STEP_MAX_WARR arrays; ol's divisor is then the weighted rule's
// comp (nullable): the delay-compensated step (on top of the weighted form: weights must be given);
// comp->snap[q] (nullable) = the snapshot of rule->arr[q], comp->theta_out (nullable) receives the
// pre-update p, comp->lam = f32(lambda)
struct CompLaunch {
    float lam;
    float* theta_out;
    const float* snap[RULE_MAX_ARR];
    int nsnap;                      // distinct non-null snapshots (algorithmic bytes)
};
int slab_step_launch_optim(float* gradstate, const StepPlan& plan, long cnt_off, long part_off,
                           float* S_out, const RuleProg* rule, const OptLaunch& ol, float* p,
                           float* m, float* v, long P, hipStream_t stream,
                           const float* weights = nullptr, const CompLaunch* comp = nullptr);

// host helpers shared with server.hip's C-ABI
int make_rule(const flsim_rule* r, RuleProg* out);
int make_adam_const(double divisor, long step, double lr, double beta1, double beta2, double eps,
                    AdamConst* ac);
// hyper-parameter checks (the cases where torch raises ValueError); before any pointer check
int check_optim(const flsim_optim* o);
int make_opt_launch(const flsim_optim* o, double divisor, long step, OptLaunch* ol);
// a weighted rule's weights and divisor (include/flsim.h); before any pointer check
int check_weights(const flsim_rule_weights* w);
// the weights in launch form (fp32); alias0 / alias1: buffers that are S_t (their weight must be 1)
int make_weights(const flsim_rule* r, const flsim_rule_weights* w, const float* alias0,
                 const float* alias1, float* out, int cap);
// delay compensation (include/flsim.h): lambda and the array count, before any pointer check
int check_comp(const flsim_rule_comp* c, const flsim_rule* r);
// the compensation in launch form.  S / S_out: the buffers that are S_t (never compensated); p:
// the parameters (theta_out must not alias them, nor a snapshot); cap: compensated arrays the step
// takes.  comp == nullptr: no snapshots (theta_out only)
int make_comp(const flsim_rule* r, const flsim_rule_comp* comp, const float* S, const float* S_out,
              float* theta_out, const float* p, int cap, CompLaunch* out);
// unit weights for a compensated rule without a discount (the C kernels exist in the weighted form)
inline void unit_weights(int n, float* w) {
    for (int q = 0; q < n; ++q) w[q] = 1.f;
}
inline flsim_optim adam_optim(double lr, double beta1, double beta2, double eps) {
    flsim_optim o{};
    o.kind = FLSIM_OPT_ADAM;
    o.lr = lr;
    o.beta1 = beta1;
    o.beta2 = beta2;
    o.eps = eps;
    return o;
}

}  // namespace flsim
