// VGG-11 (reference FL/models.py:50-103: VGG(make_layers(cfg['A'])), vgg11()) forward + backward
// for a chunk of simulated workers on gfx950 -- configs[4]'s "larger CNN" (SURVEY 8 f2).  Same
// engine structure as pn1_net.hip: every worker of an epoch runs on the central model theta_t
// (main.py:154,159,169), so a chunk of W workers is ONE batch of W*128 samples whose gradients
// add up along the weight-gradient GEMMs' reduction dimension (agents.py:35).
//
// Network on 3x32x32 input (models.py:80-98: conv3x3 padding 1 + ReLU, 'M' = 2x2 max-pool):
//   conv1 3->64 @32 +pool | conv2 64->128 @16 +pool | conv3 128->256 @8 | conv4 256->256 @8
//   +pool | conv5 256->512 @4 | conv6 512->512 @4 +pool | conv7 512->512 @2 | conv8 512->512 @2
//   +pool -> 512 features (models.py:75 flatten of a 1x1 map = channel order)
//   classifier (models.py:57-65): Dropout(.5) -> Linear(512,512) -> ReLU -> Dropout(.5) ->
//   Linear(512,512) -> ReLU -> Linear(512,10)
// Each conv + ReLU (+ pool) is one fused MFMA launch (pooled layers: GEMM rows in pool-window
// order, argmax kept for the backward); the classifier's first Dropout is fused into conv8's pool
// epilogue.  Activations NHWC fp32.
//
// vgg11_bn (models.py:106-108: Conv2d -> BatchNorm2d -> ReLU per conv, models.py:88-89) shares
// every launch above except the conv epilogue: the conv writes z = conv + bias, the per-worker
// batch statistics of z are reduced (bn_kernels.h), and one streaming pass applies the
// normalisation + ReLU (+ pool / dropout).  The backward turns the masked gradient of each
// BatchNorm output into dz in place before the conv's weight / data gradients.
#include "bn_kernels.h"
#include "net_abi.h"

namespace flsim {

// Philox sites of the classifier dropouts (models.py:58,61); the oracle uses the same
enum : uint32_t { SITE_VDROP1 = 6, SITE_VDROP2 = 7 };

struct VConv {
    int CI, CIP, CO, H;  // input channels (real / padded), output channels, spatial size (in = out)
    int KP;              // packed forward K = 9*CIP rounded up to 16
    int ZW;              // weight-gradient pixel splits: thousands of blocks per launch
};
static const VConv VG[8] = {
    {3, 4, 64, 32, 48, 2048},      {64, 64, 128, 16, 576, 512},
    {128, 128, 256, 8, 1152, 256}, {256, 256, 256, 8, 2304, 128},
    {256, 256, 512, 4, 2304, 64},  {512, 512, 512, 4, 4608, 32},
    {512, 512, 512, 2, 4608, 32},  {512, 512, 512, 2, 4608, 32},
};
constexpr int VFEAT = 512;   // classifier width
constexpr int VZL = 16;      // classifier weight-gradient splits
constexpr int VZH = 32;      // head weight-gradient splits

// vgg11_bn: per-call statistics of the 8 BatchNorms, [mean | unbiased var] per layer
// (the running-buffer layout: running_mean, running_var of features.1, .5, .9, ... in order)
constexpr int BN_RUN_OFF[8] = {0, 128, 384, 896, 1408, 2432, 3456, 4480};
constexpr int BN_NSTAT = 5504;

// flat parameter offsets in named_parameters order: features.{0,3,6,8,11,13,16,18}.{weight,bias},
// classifier.{1,4,6}.{weight,bias}; vgg11_bn: conv {weight, bias} then BatchNorm {weight, bias}
// per layer (features.{0,1}, {4,5}, {8,9}, {11,12}, {15,16}, {18,19}, {22,23}, {25,26})
struct VOff {
    long w[8], b[8], g[8], be[8], l1w, l1b, l2w, l2b, l3w, l3b, total;
};
static VOff voff(bool bn = false) {
    VOff o;
    long p = 0;
    for (int l = 0; l < 8; ++l) {
        o.w[l] = p;
        p += (long)VG[l].CO * VG[l].CI * 9;
        o.b[l] = p;
        p += VG[l].CO;
        o.g[l] = o.be[l] = -1;
        if (bn) {
            o.g[l] = p;
            p += VG[l].CO;
            o.be[l] = p;
            p += VG[l].CO;
        }
    }
    o.l1w = p; p += (long)VFEAT * VFEAT;
    o.l1b = p; p += VFEAT;
    o.l2w = p; p += (long)VFEAT * VFEAT;
    o.l2b = p; p += VFEAT;
    o.l3w = p; p += 10L * VFEAT;
    o.l3b = p; p += 10;
    o.total = p;
    return o;
}

// gradient state (floats): packed weights + weight-gradient slabs
struct VGrad {
    float* wf[8];
    float* wd[8];   // wd[0] unused (the input needs no gradient)
    float* sw[8];   // [ZW][CO][KP]
    float* sb[8];   // [ZW][CO]
    float *l1w, *l1b, *l2w, *l2b, *l3w, *l3b;
    float* bnacc[8];   // vgg11_bn: epoch sums of the BatchNorm [weight | bias] gradients
    float* slab_begin;
    long slab_floats, total_floats;
    StepPlan plan;  // the fused server step over the slabs (slabstep.h)
    long cnt_off, part_off;
};

// one segment per parameter tensor (named_parameters order), offsets from the gradstate base
static int vgg_segments(const VGrad& g, const float* base, bool bn, SegSpec* s) {
    const VOff o = voff(bn);
    int i = 0;
    for (int l = 0; l < 8; ++l) {
        const VConv& c = VG[l];
        s[i++] = SegSpec{g.sw[l] - base, c.ZW, (long)c.CO * c.KP, o.w[l], (long)c.CO * c.CI * 9,
                         c.CO, c.CI, c.CIP, c.KP};
        s[i++] = SegSpec{g.sb[l] - base, c.ZW, c.CO, o.b[l], c.CO, 0, 0, 1, 1};
        if (bn) {
            s[i++] = SegSpec{g.bnacc[l] - base, 1, c.CO, o.g[l], c.CO, 0, 0, 1, 1};
            s[i++] = SegSpec{g.bnacc[l] + c.CO - base, 1, c.CO, o.be[l], c.CO, 0, 0, 1, 1};
        }
    }
    s[i++] = SegSpec{g.l1w - base, VZL, (long)VFEAT * VFEAT, o.l1w, (long)VFEAT * VFEAT, 0, 0, 1, 1};
    s[i++] = SegSpec{g.l1b - base, VZL, VFEAT, o.l1b, VFEAT, 0, 0, 1, 1};
    s[i++] = SegSpec{g.l2w - base, VZL, (long)VFEAT * VFEAT, o.l2w, (long)VFEAT * VFEAT, 0, 0, 1, 1};
    s[i++] = SegSpec{g.l2b - base, VZL, VFEAT, o.l2b, VFEAT, 0, 0, 1, 1};
    s[i++] = SegSpec{g.l3w - base, VZH, 10L * VFEAT, o.l3w, 10L * VFEAT, 0, 0, 1, 1};
    s[i++] = SegSpec{g.l3b - base, VZH, 10, o.l3b, 10, 0, 0, 1, 1};
    return i;
}

static VGrad vgs_layout(float* base_in, bool bn = false) {
    VGrad g;
    // offsets only (sizes, plan) when base_in is null: lay out over a fake base, never dereferenced
    float* const base = base_in ? base_in : reinterpret_cast<float*>(4096);
    long o = 0;
    auto take = [&](long n) {
        float* p = base + o;
        o += (n + 63) / 64 * 64;
        return p;
    };
    for (int l = 0; l < 8; ++l) {
        g.wf[l] = take((long)VG[l].CO * VG[l].KP);
        g.wd[l] = l ? take((long)VG[l].CI * 9 * VG[l].CO) : nullptr;
    }
    const long slab0 = o;
    g.slab_begin = base + o;
    for (int l = 0; l < 8; ++l) {
        g.sw[l] = take((long)VG[l].ZW * VG[l].CO * VG[l].KP);
        g.sb[l] = take((long)VG[l].ZW * VG[l].CO);
    }
    g.l1w = take((long)VZL * VFEAT * VFEAT);
    g.l1b = take((long)VZL * VFEAT);
    g.l2w = take((long)VZL * VFEAT * VFEAT);
    g.l2b = take((long)VZL * VFEAT);
    g.l3w = take((long)VZH * 10 * VFEAT);
    g.l3b = take((long)VZH * 10);
    for (int l = 0; l < 8; ++l) g.bnacc[l] = bn ? take(2L * VG[l].CO) : nullptr;
    SegSpec specs[STEP_MAX_SEG];
    plan_step(specs, vgg_segments(g, base, bn, specs), &g.plan);
    g.cnt_off = o;
    take(step_counter_floats(g.plan));
    g.slab_floats = o - slab0;
    g.part_off = o;
    take(step_partial_floats(g.plan));
    g.total_floats = o;
    return g;
}

// workspace (per chunk of S samples).  Forward: x0, pooled maps d*, unpooled a*, f0 = dropped
// features, e1 = dropped relu(linear1), e2 = relu(linear2), argmax bytes i*.  Backward: dz of a
// conv output goes to ga (full-resolution maps after a pool scatter) or gb, pooled gradients to gy.
struct VWS {
    float *x0, *d1, *d2, *a3, *d4, *a5, *d6, *a7, *f0, *e1, *e2, *part, *dh1, *dh2;
    float *ga, *gb, *gy, *loss_s, *dlog;
    int32_t* y;
    uint8_t *i1, *i2, *i4, *i6, *i8;
    // vgg11_bn: z = conv + bias per layer, per-(worker, channel) mean / invstd, scratch
    float *z[8], *bmean[8], *binv[8], *pa, *pb, *cm, *ck, *dg, *db;
    long bytes;
};

static VWS vws_layout(char* base, int S, bool bn = false) {
    VWS w;
    long o = 0;
    auto take = [&](long bytes) {
        char* p = base ? base + o : nullptr;
        o += (bytes + 255) / 256 * 256;
        return p;
    };
    auto tf = [&](long per) { return (float*)take(per * (long)S * 4); };
    auto tb = [&](long per) { return (uint8_t*)take(per * (long)S); };
    w.x0 = tf(4096);
    w.d1 = tf(16 * 16 * 64);
    w.d2 = tf(8 * 8 * 128);
    w.a3 = tf(8 * 8 * 256);
    w.d4 = tf(4 * 4 * 256);
    w.a5 = tf(4 * 4 * 512);
    w.d6 = tf(2 * 2 * 512);
    w.a7 = tf(2 * 2 * 512);
    w.f0 = tf(VFEAT);
    w.e1 = tf(VFEAT);
    w.e2 = tf(VFEAT);
    w.part = tf(VFEAT);
    w.dh1 = tf(VFEAT);
    w.dh2 = tf(VFEAT);
    w.ga = tf(32 * 32 * 64);
    w.gb = tf(8 * 8 * 256);
    w.gy = tf(16 * 16 * 64);
    w.loss_s = tf(1);
    w.dlog = tf(16);
    w.y = (int32_t*)take(4L * S);
    w.i1 = tb(16 * 16 * 64);
    w.i2 = tb(8 * 8 * 128);
    w.i4 = tb(4 * 4 * 256);
    w.i6 = tb(2 * 2 * 512);
    w.i8 = tb(VFEAT);
    for (int l = 0; l < 8; ++l) w.z[l] = w.bmean[l] = w.binv[l] = nullptr;
    w.pa = w.pb = w.cm = w.ck = w.dg = w.db = nullptr;
    if (bn) {
        const int W = S / SAMPLES_PER_WORKER;
        for (int l = 0; l < 8; ++l) {
            w.z[l] = tf((long)VG[l].H * VG[l].H * VG[l].CO);
            w.bmean[l] = (float*)take(4L * (W > 0 ? W : 1) * VG[l].CO);
            w.binv[l] = (float*)take(4L * (W > 0 ? W : 1) * VG[l].CO);
        }
        w.pa = tf(256);     // W * NS * C = 256 * S floats at most (bn_kernels.h)
        w.pb = tf(256);
        w.cm = (float*)take(4L * (W > 0 ? W : 1) * 512);
        w.ck = (float*)take(4L * (W > 0 ? W : 1) * 512);
        w.dg = (float*)take(4L * (W > 0 ? W : 1) * 512);
        w.db = (float*)take(4L * (W > 0 ? W : 1) * 512);
    }
    w.bytes = o;
    return w;
}

static int vpack(const VGrad& g, const float* th, const VOff& o, hipStream_t st) {
    for (int l = 0; l < 8; ++l)
        RC(pack_conv(th + o.w[l], g.wf[l], g.wd[l], VG[l].CO, VG[l].CI, VG[l].CIP, VG[l].KP, st));
    return 0;
}

// vgg11_bn forward mode: train (batch statistics of every worker's 128 samples; per-call
// statistics for the running buffers into stats[worker][BN_NSTAT] unless null) or eval (the
// per-channel coefficients of the running buffers, vbn_eval_coef)
struct VBN {
    const VWS* w;
    int train;
    float* stats;
};

// conv (z = conv + bias) -> BatchNorm -> ReLU (-> 2x2 max-pool (-> dropout)) of layer l
template <int H, int CIP, int CO, int FM, int FN, int WM, int WN, bool POOL>
static int vbn_conv(const VBN& bn, int l, const float* X, int S, const VGrad& g, const float* th,
                    const VOff& o, float* out, uint8_t* idx, const WorkerRec* workers,
                    uint64_t seed, uint32_t site, int dropout, hipStream_t st, int kid,
                    int kreal) {
    const VWS& w = *bn.w;
    RC((conv_x6<H, H, CIP, 1, FM, FN, WM, WN>(X, S, g.wf[l], CO, VG[l].KP,
        EpiBias{w.z[l], th + o.b[l], S * H * H, CO}, st, kid, kreal)));
    if (bn.train)
        RC((bn_forward_stats<H, CO>(w.z[l], S, w.bmean[l], w.binv[l], w.pa, w.pb, bn.stats,
                                    BN_RUN_OFF[l], BN_NSTAT, st)));
    if constexpr (POOL)
        return bn_apply_pool<H, CO>(w.z[l], S, w.bmean[l], w.binv[l], th + o.g[l], th + o.be[l],
                                    bn.train, out, idx, workers, seed, site, THR_P50, SCALE_P50,
                                    dropout, st);
    else
        return bn_apply<H, CO>(w.z[l], S, w.bmean[l], w.binv[l], th + o.g[l], th + o.be[l],
                               bn.train, out, st);
}

// eval mode: mean / invstd of every BatchNorm from the running buffers
static int vbn_eval_coef(const VWS& w, const float* running, hipStream_t st) {
    for (int l = 0; l < 8; ++l) {
        const int C = VG[l].CO;
        hipLaunchKernelGGL(k_bn_eval_coef, dim3(ceil_div(C, 256)), dim3(256), 0, st,
                           running + BN_RUN_OFF[l], running + BN_RUN_OFF[l] + C, C, w.bmean[l],
                           w.binv[l]);
        FLSIM_LAUNCH_CHECK();
    }
    return 0;
}

// models.py:73-77 (features, flatten, classifier) up to the last ReLU; the head follows
template <bool BN>
static int vforward(const VGrad& g, const VWS& w, const float* th, const VOff& o, int S,
                    const WorkerRec* workers, uint64_t seed, int dropout, const VBN* bn,
                    hipStream_t st) {
    if constexpr (BN) {
        // features.{0-3}, {4-7}, {8-10}, {11-14}, {15-17}, {18-21}, {22-24}, {25-28}
        RC((vbn_conv<32, 4, 64, 2, 4, 4, 1, true>(*bn, 0, w.x0, S, g, th, o, w.d1, w.i1, workers,
                                                  seed, 0, 0, st, K_VF1, 27)));
        RC((vbn_conv<16, 64, 128, 4, 4, 4, 2, true>(*bn, 1, w.d1, S, g, th, o, w.d2, w.i2,
                                                    workers, seed, 0, 0, st, K_VF2, 576)));
        RC((vbn_conv<8, 128, 256, 4, 4, 4, 2, false>(*bn, 2, w.d2, S, g, th, o, w.a3, nullptr,
                                                     workers, seed, 0, 0, st, K_VF3, 1152)));
        RC((vbn_conv<8, 256, 256, 4, 4, 4, 2, true>(*bn, 3, w.a3, S, g, th, o, w.d4, w.i4,
                                                    workers, seed, 0, 0, st, K_VF4, 2304)));
        RC((vbn_conv<4, 256, 512, 4, 4, 4, 2, false>(*bn, 4, w.d4, S, g, th, o, w.a5, nullptr,
                                                     workers, seed, 0, 0, st, K_VF5, 2304)));
        RC((vbn_conv<4, 512, 512, 4, 4, 4, 2, true>(*bn, 5, w.a5, S, g, th, o, w.d6, w.i6,
                                                    workers, seed, 0, 0, st, K_VF6, 4608)));
        RC((vbn_conv<2, 512, 512, 4, 4, 4, 2, false>(*bn, 6, w.d6, S, g, th, o, w.a7, nullptr,
                                                     workers, seed, 0, 0, st, K_VF7, 4608)));
        // + classifier Dropout (models.py:58) on the flattened 1x1 pooled map
        RC((vbn_conv<2, 512, 512, 4, 4, 4, 2, true>(*bn, 7, w.a7, S, g, th, o, w.f0, w.i8,
                                                    workers, seed, SITE_VDROP1, dropout, st,
                                                    K_VF8, 4608)));
    } else {
        // conv1 + ReLU + pool (features.0-2)
        RC((conv_pool_fwd<32, 32, 4, 64, 1, 2, 4, 4, 1, false, true>(w.x0, S, g.wf[0], 48, w.d1, w.i1,
            th + o.b[0], workers, seed, 0, 0, 1.f, 0, st, K_VF1, 27)));
        // conv2 + ReLU + pool (features.3-5)
        RC((conv_pool_fwd<16, 16, 64, 128, 1, 4, 4, 4, 2, false, true>(w.d1, S, g.wf[1], 576, w.d2,
            w.i2, th + o.b[1], workers, seed, 0, 0, 1.f, 0, st, K_VF2, 576)));
        // conv3 + ReLU (features.6-7)
        RC((conv_x6<8, 8, 128, 1, 4, 4, 4, 2>(w.d2, S, g.wf[2], 256, 1152,
            EpiBiasRelu{w.a3, th + o.b[2], S * 64, 256}, st, K_VF3, 1152)));
        // conv4 + ReLU + pool (features.8-10)
        RC((conv_pool_fwd<8, 8, 256, 256, 1, 4, 4, 4, 2, false, true>(w.a3, S, g.wf[3], 2304, w.d4,
            w.i4, th + o.b[3], workers, seed, 0, 0, 1.f, 0, st, K_VF4, 2304)));
        // conv5 + ReLU (features.11-12)
        RC((conv_x6<4, 4, 256, 1, 4, 4, 4, 2>(w.d4, S, g.wf[4], 512, 2304,
            EpiBiasRelu{w.a5, th + o.b[4], S * 16, 512}, st, K_VF5, 2304)));
        // conv6 + ReLU + pool (features.13-15)
        RC((conv_pool_fwd<4, 4, 512, 512, 1, 4, 4, 4, 2, false, true>(w.a5, S, g.wf[5], 4608, w.d6,
            w.i6, th + o.b[5], workers, seed, 0, 0, 1.f, 0, st, K_VF6, 4608)));
        // conv7 + ReLU (features.16-17)
        RC((conv_x6<2, 2, 512, 1, 4, 4, 4, 2>(w.d6, S, g.wf[6], 512, 4608,
            EpiBiasRelu{w.a7, th + o.b[6], S * 4, 512}, st, K_VF7, 4608)));
        // conv8 + ReLU + pool (features.18-20) + classifier Dropout (models.py:58): the 1x1
        // pooled map is the flattened feature vector
        RC((conv_pool_fwd<2, 2, 512, 512, 1, 4, 4, 4, 2, false, true>(w.a7, S, g.wf[7], 4608, w.f0,
            w.i8, th + o.b[7], workers, seed, SITE_VDROP1, THR_P50, SCALE_P50, dropout, st,
            K_VF8, 4608)));
    }
    // Linear + ReLU + Dropout (models.py:59-61)
    RC((linear_fwd<4, 4, 2, 2, true>(w.f0, th + o.l1w, w.part, S, VFEAT, VFEAT, 1, st, K_VL1F)));
    RC(linear_finish(w.part, 1, th + o.l1b, w.e1, S, VFEAT, workers, seed, SITE_VDROP2, THR_P50,
                     SCALE_P50, dropout, st));
    // Linear + ReLU (models.py:62-63)
    RC((linear_fwd<4, 4, 2, 2, true>(w.e1, th + o.l2w, w.part, S, VFEAT, VFEAT, 1, st, K_VL2F)));
    RC(linear_finish(w.part, 1, th + o.l2b, w.e2, S, VFEAT, workers, seed, 0, 0, 1.f, 0, st));
    return 0;
}

// vgg11_bn: gradient wrt BatchNorm l's output (mask applied) -> dz in place
template <bool BN, int H, int C>
static int vbn_back(const VGrad& g, const VWS& w, const float* th, const VOff& o, int l,
                    float* dy, int S, hipStream_t st) {
    if constexpr (BN)
        return bn_backward<H, C>(dy, w.z[l], S, w.bmean[l], w.binv[l], th + o.g[l], w.pa, w.pb,
                                 w.cm, w.ck, w.dg, w.db, g.bnacc[l], st);
    return 0;
}

// backward from the head's dlog / dh2 (gradient wrt linear2's pre-activation)
template <bool BN>
static int vbackward(const VGrad& g, const VWS& w, const float* th, const VOff& o, int S,
                     int dropout, hipStream_t st) {
    const float s50 = dropout ? SCALE_P50 : 1.f;
    // Linear(512,10) weight / bias
    RC(head_wgrad<VFEAT>(w.dlog, w.e2, g.l3w, g.l3b, S, VZH, st));
    // Linear2: wgrad (input e1), dgrad through Dropout + ReLU of Linear1 (e1 is the dropped output)
    RC((linear_wgrad<4, 4, 2, 2, true>(w.dh2, w.e1, g.l2w, g.l2b, S, VFEAT, VFEAT, VZL, st, K_VL2W)));
    // (every data gradient on the fp32 MFMA, the classifier's too: the bf16 MFMA's truncating
    // sum biases per-channel sums)
    RC((linear_dgrad<4, 4, 2, 2>(w.dh2, th + o.l2w, w.dh1, w.e1, s50, S, VFEAT, VFEAT, st,
                                 K_VL2D)));
    // Linear1: wgrad (input f0 = dropped features), dgrad through the first Dropout and conv8's
    // pooled ReLU (f0 > 0), then the pool scatter -> dz8
    RC((linear_wgrad<4, 4, 2, 2, true>(w.dh1, w.f0, g.l1w, g.l1b, S, VFEAT, VFEAT, VZL, st, K_VL1W)));
    RC((linear_dgrad<4, 4, 2, 2>(w.dh1, th + o.l1w, w.gy, w.f0, s50, S, VFEAT, VFEAT, st,
                                 K_VL1D)));
    RC((pool_scatter<2, 2, 512, false>(w.gy, w.i8, w.ga, S, st)));
    RC((vbn_back<BN, 2, 512>(g, w, th, o, 7, w.ga, S, st)));
    // The conv weight gradients run on the fp32 MFMA (an fmaf chain): summed over a chunk's
    // pixels (4096 samples x up to 32 x 32), the bf16 MFMA's truncating accumulation leaves a
    // relative bias that grows past SURVEY 8(c)'s bound (measured on PerformantNet1's)
    // conv8: wgrad (input a7), dgrad -> dz7 = . * (a7 > 0)
    RC((conv_wgrad<2, 2, 512, 1, 4, 4, 4, 2, 0, false, false>(
        w.ga, w.a7, S, 512, 4608, g.sw[7], g.sb[7], VG[7].ZW, st, K_VWG8, 4608)));
    RC((conv_like<2, 2, 512, 1, 4, 4, 4, 2>(w.ga, S, g.wd[7], 512, 4608,
        EpiMask<true>{w.gb, w.a7, S * 4, 512}, st, K_VDG8, 4608)));
    RC((vbn_back<BN, 2, 512>(g, w, th, o, 6, w.gb, S, st)));
    // conv7: wgrad (input d6), dgrad -> gradient wrt d6 (d6 > 0), pool scatter -> dz6
    RC((conv_wgrad<2, 2, 512, 1, 4, 4, 4, 2, 0, false, false>(
        w.gb, w.d6, S, 512, 4608, g.sw[6], g.sb[6], VG[6].ZW, st, K_VWG7, 4608)));
    RC((conv_like<2, 2, 512, 1, 4, 4, 4, 2>(w.gb, S, g.wd[6], 512, 4608,
        EpiDropMask{w.gy, w.d6, 1.f, S * 4, 512}, st, K_VDG7, 4608)));
    RC((pool_scatter<4, 4, 512, false>(w.gy, w.i6, w.ga, S, st)));
    RC((vbn_back<BN, 4, 512>(g, w, th, o, 5, w.ga, S, st)));
    // conv6: wgrad (input a5), dgrad -> dz5 = . * (a5 > 0)
    RC((conv_wgrad<4, 4, 512, 1, 4, 4, 4, 2, 0, false, false>(
        w.ga, w.a5, S, 512, 4608, g.sw[5], g.sb[5], VG[5].ZW, st, K_VWG6, 4608)));
    RC((conv_like<4, 4, 512, 1, 4, 4, 4, 2>(w.ga, S, g.wd[5], 512, 4608,
        EpiMask<true>{w.gb, w.a5, S * 16, 512}, st, K_VDG6, 4608)));
    RC((vbn_back<BN, 4, 512>(g, w, th, o, 4, w.gb, S, st)));
    // conv5: wgrad (input d4), dgrad -> gradient wrt d4, pool scatter -> dz4
    RC((conv_wgrad<4, 4, 256, 1, 4, 4, 2, 2, 0, false, false>(
        w.gb, w.d4, S, 512, 2304, g.sw[4], g.sb[4], VG[4].ZW, st, K_VWG5, 2304)));
    RC((conv_like<4, 4, 512, 1, 4, 4, 4, 2>(w.gb, S, g.wd[4], 256, 4608,
        EpiDropMask{w.gy, w.d4, 1.f, S * 16, 256}, st, K_VDG5, 4608)));
    RC((pool_scatter<8, 8, 256, false>(w.gy, w.i4, w.ga, S, st)));
    RC((vbn_back<BN, 8, 256>(g, w, th, o, 3, w.ga, S, st)));
    // conv4: wgrad (input a3), dgrad -> dz3 = . * (a3 > 0)
    RC((conv_wgrad<8, 8, 256, 1, 4, 4, 2, 2, 0, false, false>(
        w.ga, w.a3, S, 256, 2304, g.sw[3], g.sb[3], VG[3].ZW, st, K_VWG4, 2304)));
    RC((conv_like<8, 8, 256, 1, 4, 4, 4, 2>(w.ga, S, g.wd[3], 256, 2304,
        EpiMask<true>{w.gb, w.a3, S * 64, 256}, st, K_VDG4, 2304)));
    RC((vbn_back<BN, 8, 256>(g, w, th, o, 2, w.gb, S, st)));
    // conv3: wgrad (input d2), dgrad -> gradient wrt d2, pool scatter -> dz2
    RC((conv_wgrad<8, 8, 128, 1, 4, 4, 2, 2, 0, false, false>(
        w.gb, w.d2, S, 256, 1152, g.sw[2], g.sb[2], VG[2].ZW, st, K_VWG3, 1152)));
    RC((conv_like<8, 8, 256, 1, 4, 4, 4, 2>(w.gb, S, g.wd[2], 128, 2304,
        EpiDropMask{w.gy, w.d2, 1.f, S * 64, 128}, st, K_VDG3, 2304)));
    RC((pool_scatter<16, 16, 128, false>(w.gy, w.i2, w.ga, S, st)));
    RC((vbn_back<BN, 16, 128>(g, w, th, o, 1, w.ga, S, st)));
    // conv2: wgrad (input d1), dgrad -> gradient wrt d1, pool scatter -> dz1
    RC((conv_wgrad<16, 16, 64, 1, 2, 4, 4, 2, 0, false, false>(
        w.ga, w.d1, S, 128, 576, g.sw[1], g.sb[1], VG[1].ZW, st, K_VWG2, 576)));
    RC((conv_like<16, 16, 128, 1, 2, 4, 4, 1>(w.ga, S, g.wd[1], 64, 1152,
        EpiDropMask{w.gy, w.d1, 1.f, S * 256, 64}, st, K_VDG2, 1152)));
    RC((pool_scatter<32, 32, 64, false>(w.gy, w.i1, w.ga, S, st)));
    RC((vbn_back<BN, 32, 64>(g, w, th, o, 0, w.ga, S, st)));
    // conv1: wgrad (input x0)
    RC((conv_wgrad<32, 32, 4, 1, 4, 3, 1, 1, 0, false, false>(
        w.ga, w.x0, S, 64, 48, g.sw[0], g.sb[0], VG[0].ZW, st, K_VWG1, 27)));
    return 0;
}

// ---- the network descriptions of net_abi.h: vgg11 (BN = false) and vgg11_bn -------------------
template <bool BN>
struct VggNet {
    using Grad = VGrad;
    using Ws = VWS;
    static constexpr int HEAD = VFEAT;
    static constexpr bool BATCH_NORM = BN;
    static VGrad grad(void* gradstate) { return vgs_layout((float*)gradstate, BN); }
    static VWS ws(void* workspace, int samples) { return vws_layout((char*)workspace, samples, BN); }
    static long params() { return voff(BN).total; }
    static long head_w() { return voff(BN).l3w; }
    static long head_b() { return voff(BN).l3b; }
    static float head_scale(int) { return 1.f; }      // no dropout after the last ReLU
    static int pack(const VGrad& g, const float* th, hipStream_t st) {
        return vpack(g, th, voff(BN), st);
    }
    static int forward(const VGrad& g, const VWS& w, const float* th, int S,
                       const WorkerRec* workers, uint64_t seed, int dropout, int train,
                       float* bn_stats, hipStream_t st) {
        const VBN bn{&w, train, bn_stats};
        return vforward<BN>(g, w, th, voff(BN), S, workers, seed, dropout, &bn, st);
    }
    static int eval_coef(const VWS& w, const float* running, hipStream_t st) {
        return vbn_eval_coef(w, running, st);
    }
    static int backward(void*, const VGrad& g, const VWS& w, const float* th, int S, int dropout,
                        hipStream_t st) {
        return vbackward<BN>(g, w, th, voff(BN), S, dropout, st);
    }
    static int join(void*, hipStream_t) { return 0; }      // every pass runs on the caller's stream
    static StepPlan plan(const VGrad& g, const void*) { return g.plan; }
};
using V11 = VggNet<false>;
using V11BN = VggNet<true>;

// ---- the C-ABI bodies that differ from PerformantNet1's ---------------------------------------
template <bool BN>
static int vgg_workspace_offset(int which, int samples, long* offset_bytes) {
    char* const fake = reinterpret_cast<char*>(4096);   // layout only; never dereferenced
    VWS w = vws_layout(fake, samples, BN);
    const void* p[] = {w.x0, w.d1, w.d2, w.a3, w.d4, w.a5, w.d6, w.a7, w.f0, w.e1, w.e2, w.dh1,
                       w.dh2, w.ga, w.gb, w.gy, w.loss_s, w.dlog, w.y, w.i1, w.i2, w.i4, w.i6,
                       w.i8,
                       w.z[0], w.z[1], w.z[2], w.z[3], w.z[4], w.z[5], w.z[6], w.z[7],
                       w.bmean[0], w.bmean[1], w.bmean[2], w.bmean[3], w.bmean[4], w.bmean[5],
                       w.bmean[6], w.bmean[7],
                       w.binv[0], w.binv[1], w.binv[2], w.binv[3], w.binv[4], w.binv[5],
                       w.binv[6], w.binv[7]};
    return tensor_offset(p, BN ? (int)(sizeof(p) / sizeof(p[0])) : 24, fake, which, offset_bytes);
}

template <bool BN>
static int vgg_begin_epoch(void* gradstate, const float* theta, hipStream_t stream) {
    FLSIM_REQUIRE(gradstate && theta, "null pointer");
    VGrad g = vgs_layout((float*)gradstate, BN);
    RC(vpack(g, theta, voff(BN), stream));
    FLSIM_CHECK_HIP(hipMemsetAsync(g.slab_begin, 0, g.slab_floats * 4, stream));
    return 0;
}

// The facade's deferred fwd_bkwd for vgg11 (Worker.fwd_bkwd of 128-sample batches, agents.py:32-40):
// a call stages its batch into workspace rows [row0, row0 + 128) (vgg_load_rows); the forward,
// loss and backward of the staged rows [0, n_rows) then run as ONE worker-batched pass
// (vgg_fwd_bwd_loaded_rows, the batched engine's own chunk), when a loss or the gradient is needed.
template <bool BN>
static int vgg_load_rows(void* gradstate, void* workspace, int max_samples, int row0,
                         const float* x, const int64_t* y, int n_samples, hipStream_t stream) {
    FLSIM_REQUIRE(gradstate && workspace && x && y, "null pointer");
    int S;
    RC(check_batch_rows(n_samples, row0, max_samples, &S));
    VWS w = vws_layout((char*)workspace, max_samples, BN);
    return load_input(x, y, n_samples, w.x0 + (long)row0 * 4096, w.y + row0, S, stream);
}

template <bool BN>
static int vgg_fwd_bwd_loaded_rows(void* gradstate, void* workspace, int max_samples, int n_rows,
                                   const float* theta, const WorkerRec* workers, uint64_t seed,
                                   int dropout, float* worker_loss, float* bn_stats,
                                   hipStream_t stream) {
    FLSIM_REQUIRE(gradstate && workspace && theta && workers && worker_loss, "null pointer");
    FLSIM_REQUIRE(!BN || bn_stats, "null bn_stats");
    RC(check_row_count(n_rows, max_samples));
    return run_chunk<VggNet<BN>>(gradstate, vws_layout((char*)workspace, max_samples, BN), theta,
                                 workers, n_rows, seed, dropout, 1, 1.f / SAMPLES_PER_WORKER,
                                 worker_loss, bn_stats, stream);
}

}  // namespace flsim

using namespace flsim;

// =============================================================================================
// C-ABI (declared in include/flsim.h): the flsim_pn1_* contract for vgg11() and vgg11_bn()
// =============================================================================================
extern "C" {

long flsim_vgg11_param_count(void) { return voff(false).total; }

long flsim_vgg11_gradstate_bytes(void) { return vgs_layout(nullptr, false).total_floats * 4; }

long flsim_vgg11_workspace_bytes(int max_samples) {
    return vws_layout(nullptr, max_samples, false).bytes;
}

int flsim_vgg11_workspace_offset(int which, int samples, long* offset_bytes) {
    return vgg_workspace_offset<false>(which, samples, offset_bytes);
}

int flsim_vgg11_begin_epoch(void* gradstate, const float* theta, hipStream_t stream) {
    return vgg_begin_epoch<false>(gradstate, theta, stream);
}

int flsim_vgg11_fwd_bwd_chunk(void* gradstate, void* workspace, int max_samples,
                              const float* theta, const uint8_t* pool, const int32_t* labels,
                              const int32_t* list_a, int len_a, const int32_t* list_b, int len_b,
                              const float* lut, const WorkerRec* workers, int n_chunk_workers,
                              int n_workers_total, uint64_t seed, int dropout, int backward_pass,
                              float* worker_loss, hipStream_t stream) {
    const ChunkSrc src{pool, labels, list_a, len_a, list_b, len_b, lut, n_workers_total};
    return net_fwd_bwd_chunk<V11>(gradstate, workspace, max_samples, theta, src, workers,
                                  n_chunk_workers, seed, dropout, backward_pass, worker_loss,
                                  nullptr, stream);
}

int flsim_vgg11_fwd_bwd_input(void* gradstate, void* workspace, int max_samples,
                              const float* theta, const float* x, const int64_t* y, int n_samples,
                              const WorkerRec* workers, uint64_t seed, int dropout,
                              int backward_pass, float* worker_loss, hipStream_t stream) {
    return net_fwd_bwd_input<V11>(gradstate, workspace, max_samples, theta, x, y, n_samples,
                                  workers, seed, dropout, backward_pass, worker_loss, nullptr,
                                  stream);
}

int flsim_vgg11_load_rows(void* gradstate, void* workspace, int max_samples, int row0,
                          const float* x, const int64_t* y, int n_samples, hipStream_t stream) {
    return vgg_load_rows<false>(gradstate, workspace, max_samples, row0, x, y, n_samples, stream);
}

int flsim_vgg11_fwd_bwd_loaded_rows(void* gradstate, void* workspace, int max_samples, int n_rows,
                                    const float* theta, const WorkerRec* workers, uint64_t seed,
                                    int dropout, float* worker_loss, hipStream_t stream) {
    return vgg_fwd_bwd_loaded_rows<false>(gradstate, workspace, max_samples, n_rows, theta,
                                          workers, seed, dropout, worker_loss, nullptr, stream);
}

int flsim_vgg11_bn_load_rows(void* gradstate, void* workspace, int max_samples, int row0,
                             const float* x, const int64_t* y, int n_samples, hipStream_t stream) {
    // one BatchNorm batch per 128-sample group, so only whole groups
    FLSIM_REQUIRE(n_samples % SAMPLES_PER_WORKER == 0,
                  "vgg11_bn batch of %d samples: must be a multiple of %d", n_samples,
                  SAMPLES_PER_WORKER);
    return vgg_load_rows<true>(gradstate, workspace, max_samples, row0, x, y, n_samples, stream);
}

int flsim_vgg11_bn_fwd_bwd_loaded_rows(void* gradstate, void* workspace, int max_samples,
                                       int n_rows, const float* theta, const WorkerRec* workers,
                                       uint64_t seed, int dropout, float* worker_loss,
                                       float* bn_stats, hipStream_t stream) {
    return vgg_fwd_bwd_loaded_rows<true>(gradstate, workspace, max_samples, n_rows, theta,
                                         workers, seed, dropout, worker_loss, bn_stats, stream);
}

int flsim_vgg11_eval_pool(void* gradstate, void* workspace, int max_samples, const float* theta,
                          const uint8_t* pool, int first, int n_images, const float* lut,
                          int32_t* pred, hipStream_t stream) {
    return net_eval<V11>(gradstate, workspace, max_samples, theta, pool, first, n_images, lut,
                         nullptr, nullptr, pred, stream);
}

int flsim_vgg11_eval_input(void* gradstate, void* workspace, int max_samples, const float* theta,
                           const float* x, int n_images, int32_t* pred, hipStream_t stream) {
    return net_eval<V11>(gradstate, workspace, max_samples, theta, nullptr, 0, n_images, nullptr,
                         x, nullptr, pred, stream);
}

int flsim_vgg11_end_epoch(void* gradstate, float* grad_out, hipStream_t stream) {
    return net_end_epoch<V11>(gradstate, grad_out, stream);
}

int flsim_vgg11_server_step(void* gradstate, float* S_out, const flsim_rule* rule, float* p,
                            float* m, float* v, long step, double lr, double beta1, double beta2,
                            double eps, hipStream_t stream) {
    return net_server_step<V11>(gradstate, S_out, rule, p, m, v, step, lr, beta1, beta2, eps,
                                stream);
}

int flsim_vgg11_server_step_optim(void* gradstate, float* S_out, const flsim_rule* rule, float* p,
                                  float* m, float* v, long step, const flsim_optim* optim,
                                  hipStream_t stream) {
    return net_server_step_optim<V11>(gradstate, S_out, rule, p, m, v, step, optim, stream);
}

int flsim_vgg11_server_step_wrule(void* gradstate, float* S_out, const flsim_rule* rule,
                                  const flsim_rule_weights* wts, float* p, float* m, float* v,
                                  long step, const flsim_optim* optim, hipStream_t stream) {
    return net_server_step_wrule<V11>(gradstate, S_out, rule, wts, p, m, v, step, optim, stream);
}

int flsim_vgg11_server_step_crule(void* gradstate, float* S_out, float* theta_out,
                                  const flsim_rule* rule, const flsim_rule_weights* wts,
                                  const flsim_rule_comp* comp, float* p, float* m, float* v,
                                  long step, const flsim_optim* optim, hipStream_t stream) {
    return net_server_step_crule<V11>(gradstate, S_out, theta_out, rule, wts, comp, p, m, v,
                                      step, optim, stream);
}

// ---- vgg11_bn -------------------------------------------------------------------------------
long flsim_vgg11_bn_param_count(void) { return voff(true).total; }

long flsim_vgg11_bn_gradstate_bytes(void) { return vgs_layout(nullptr, true).total_floats * 4; }

long flsim_vgg11_bn_workspace_bytes(int max_samples) {
    return vws_layout(nullptr, max_samples, true).bytes;
}

int flsim_vgg11_bn_workspace_offset(int which, int samples, long* offset_bytes) {
    return vgg_workspace_offset<true>(which, samples, offset_bytes);
}

int flsim_vgg11_bn_stats_per_worker(void) { return BN_NSTAT; }

int flsim_vgg11_bn_begin_epoch(void* gradstate, const float* theta, hipStream_t stream) {
    return vgg_begin_epoch<true>(gradstate, theta, stream);
}

int flsim_vgg11_bn_fwd_bwd_chunk(void* gradstate, void* workspace, int max_samples,
                                 const float* theta, const uint8_t* pool, const int32_t* labels,
                                 const int32_t* list_a, int len_a, const int32_t* list_b,
                                 int len_b, const float* lut, const WorkerRec* workers,
                                 int n_chunk_workers, int n_workers_total, uint64_t seed,
                                 int dropout, int backward_pass, float* worker_loss,
                                 float* bn_stats, hipStream_t stream) {
    const ChunkSrc src{pool, labels, list_a, len_a, list_b, len_b, lut, n_workers_total};
    return net_fwd_bwd_chunk<V11BN>(gradstate, workspace, max_samples, theta, src, workers,
                                    n_chunk_workers, seed, dropout, backward_pass, worker_loss,
                                    bn_stats, stream);
}

int flsim_vgg11_bn_fwd_bwd_input(void* gradstate, void* workspace, int max_samples,
                                 const float* theta, const float* x, const int64_t* y,
                                 int n_samples, const WorkerRec* workers, uint64_t seed,
                                 int dropout, int backward_pass, float* worker_loss,
                                 float* bn_stats, hipStream_t stream) {
    return net_fwd_bwd_input<V11BN>(gradstate, workspace, max_samples, theta, x, y, n_samples,
                                    workers, seed, dropout, backward_pass, worker_loss, bn_stats,
                                    stream);
}

int flsim_vgg11_bn_eval_pool(void* gradstate, void* workspace, int max_samples,
                             const float* theta, const uint8_t* pool, int first, int n_images,
                             const float* lut, const float* running, int32_t* pred,
                             hipStream_t stream) {
    return net_eval<V11BN>(gradstate, workspace, max_samples, theta, pool, first, n_images, lut,
                           nullptr, running, pred, stream);
}

int flsim_vgg11_bn_eval_input(void* gradstate, void* workspace, int max_samples,
                              const float* theta, const float* x, int n_images,
                              const float* running, int32_t* pred, hipStream_t stream) {
    return net_eval<V11BN>(gradstate, workspace, max_samples, theta, nullptr, 0, n_images,
                           nullptr, x, running, pred, stream);
}

int flsim_vgg11_bn_end_epoch(void* gradstate, float* grad_out, hipStream_t stream) {
    return net_end_epoch<V11BN>(gradstate, grad_out, stream);
}

int flsim_vgg11_bn_server_step(void* gradstate, float* S_out, const flsim_rule* rule, float* p,
                               float* m, float* v, long step, double lr, double beta1,
                               double beta2, double eps, hipStream_t stream) {
    return net_server_step<V11BN>(gradstate, S_out, rule, p, m, v, step, lr, beta1, beta2, eps,
                                  stream);
}

int flsim_vgg11_bn_server_step_optim(void* gradstate, float* S_out, const flsim_rule* rule,
                                     float* p, float* m, float* v, long step,
                                     const flsim_optim* optim, hipStream_t stream) {
    return net_server_step_optim<V11BN>(gradstate, S_out, rule, p, m, v, step, optim, stream);
}

int flsim_vgg11_bn_server_step_wrule(void* gradstate, float* S_out, const flsim_rule* rule,
                                     const flsim_rule_weights* wts, float* p, float* m, float* v,
                                     long step, const flsim_optim* optim, hipStream_t stream) {
    return net_server_step_wrule<V11BN>(gradstate, S_out, rule, wts, p, m, v, step, optim,
                                        stream);
}

int flsim_vgg11_bn_server_step_crule(void* gradstate, float* S_out, float* theta_out,
                                     const flsim_rule* rule, const flsim_rule_weights* wts,
                                     const flsim_rule_comp* comp, float* p, float* m, float* v,
                                     long step, const flsim_optim* optim, hipStream_t stream) {
    return net_server_step_crule<V11BN>(gradstate, S_out, theta_out, rule, wts, comp, p, m, v,
                                        step, optim, stream);
}

int flsim_vgg11_bn_update_running(float* running, const float* bn_stats, int n_workers,
                                  hipStream_t stream) {
    FLSIM_REQUIRE(running && (bn_stats || n_workers == 0), "null pointer");
    FLSIM_REQUIRE(n_workers >= 0, "negative worker count");
    if (n_workers == 0) return 0;
    hipLaunchKernelGGL(k_bn_running, dim3(ceil_div(BN_NSTAT, 256)), dim3(256), 0, stream, running,
                       bn_stats, n_workers, BN_NSTAT);
    FLSIM_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

