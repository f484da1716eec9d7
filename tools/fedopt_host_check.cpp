// Stand-alone host check of the host code FedAdagrad and FedYogi add (csrc/server.hip: check_optim
// and make_opt_launch for FLSIM_OPT_ADAGRAD / FLSIM_OPT_YOGI), meant to be built with the host
// sanitizers and run on a CPU-only machine, as tools/clip_host_check.cpp is for clipping.  Nothing
// here launches a kernel: the entry points are only driven into their refusals, which come before
// any pointer check or launch.
//
//   cd fl-distributed-delay_amd && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 \
//       -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I../include -I../tools -Icsrc -x hip \
//       csrc/server.hip csrc/probe.cpp ../tools/fedopt_host_check.cpp \
//       -fsanitize=address,undefined -o /tmp/fedopt_host_check && /tmp/fedopt_host_check
//
// Three parts: every refusal of check_optim for the new kinds (and that the old kinds never read
// lr_decay); the constant mapping of make_opt_launch onto the AdamConst / OptConst fields the
// argument blocks already carry, with lr_decay at steps up to 10^6; and the two element updates
// restated on the host from those launch constants (what opt_update<OK_ADAGRAD / OK_YOGI> does,
// fmaf and sqrtf being correctly rounded here) against the rule text evaluated from the
// hyper-parameters as torch evaluates it, on exactly sized heap buffers.

#include <vector>

#include "host_check.h"
#include "slabstep.h"

using namespace flsim;

static flsim_optim optim(int kind) {
    flsim_optim o{};
    o.kind = kind;
    o.lr = 1e-2;
    o.beta1 = 0.9;
    o.beta2 = 0.99;
    o.eps = kind == FLSIM_OPT_ADAGRAD ? 1e-10 : 1e-3;
    return o;
}

// ---- the device's element updates, restated from the launch constants ---------------------------
static void adagrad_launch(const OptLaunch& L, float g, float& p, float& sum) {
    if (L.oc.flags & OF_WD) g = fmaf(p, L.oc.wd, g);
    const float s = fmaf(g, g, sum);
    volatile float num = L.oc.neg_lr * g;
    volatile float den = sqrtf(s) + L.ac.eps;
    volatile float q = num / den;
    p = p + q;
    sum = s;
}
static void yogi_launch(const OptLaunch& L, float g, float& p, float& m, float& v) {
    if (L.oc.flags & OF_WD) g = fmaf(p, L.oc.wd, g);
    volatile float dm = g - m;
    const float mi = fmaf(L.ac.w1, dm, m);
    volatile float g2 = g * g;
    volatile float d = v - g2;
    const float sg = (float)(d > 0.f) - (float)(d < 0.f);
    volatile float c = -L.ac.w2 * sg;
    const float vi = fmaf(c, g2, v);
    volatile float num = L.oc.neg_lr * mi;
    volatile float den = sqrtf(vi) + L.ac.eps;
    volatile float q = num / den;
    p = p + q;
    m = mi;
    v = vi;
}

// ---- the rule text, from the hyper-parameters as torch evaluates it ------------------------------
// add(x, alpha=a) = fma(x, f32(a), y); addcmul_(a, b, value=c) = fma(f32(c) * a, b, x);
// addcdiv_(a, b, value=c) = x + (f32(c) * a) / b; lerp_(g, w) = fma(f32(w), g - m, m)
static void adagrad_text(const flsim_optim& o, long step, float g, float& p, float& sum) {
    if (o.weight_decay != 0.0) g = fmaf(p, (float)o.weight_decay, g);
    const double clr = o.lr / (1.0 + (double)(step - 1) * o.lr_decay);
    volatile float one_g = 1.0f * g;
    sum = fmaf(one_g, g, sum);
    volatile float std_ = sqrtf(sum);
    volatile float den = std_ + (float)o.eps;
    volatile float num = (float)(-clr) * g;
    volatile float q = num / den;
    p = p + q;
}
static void yogi_text(const flsim_optim& o, float g, float& p, float& m, float& v) {
    if (o.weight_decay != 0.0) g = fmaf(p, (float)o.weight_decay, g);
    volatile float dm = g - m;
    m = fmaf((float)(1.0 - o.beta1), dm, m);
    volatile float g2 = g * g;
    volatile float d = v - g2;
    const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);      // torch.sign: 0 for a NaN
    volatile float c = (float)(-(1.0 - o.beta2)) * sg;
    v = fmaf(c, g2, v);
    volatile float std_ = sqrtf(v);
    volatile float den = std_ + (float)o.eps;
    volatile float num = (float)(-o.lr) * m;
    volatile float q = num / den;
    p = p + q;
}

int main() {
    auto refused = [&](const flsim_optim& o, const char* what) {
        EXPECT(check_optim(&o) == 1);
        EXPECT(strstr(flsim_last_error(), what) != nullptr);
        OptLaunch ol;
        EXPECT(make_opt_launch(&o, 5.0, 1, &ol) == 1);
        // the entry point: the same refusal before any pointer check
        EXPECT(flsim_aggregate_optim_clip_push(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                               nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, 1,
                                               &o, nullptr) == 1);
        EXPECT(strstr(flsim_last_error(), what) != nullptr);
        EXPECT(strstr(flsim_last_error(), "null pointer") == nullptr);
    };
    // ---- check_optim: every refusal --------------------------------------------------------------
    for (int kind : {FLSIM_OPT_ADAGRAD, FLSIM_OPT_YOGI}) {
        for (double bad : {-1e-10, -1.0, (double)NAN, -(double)INFINITY}) {
            flsim_optim o = optim(kind);
            o.eps = bad;
            refused(o, "Invalid epsilon value");
            o = optim(kind);
            o.lr = bad;
            refused(o, "Invalid learning rate");
            o = optim(kind);
            o.weight_decay = bad;
            refused(o, "Invalid weight_decay value");
        }
        flsim_optim ok = optim(kind);
        ok.eps = 0.0;
        EXPECT(check_optim(&ok) == 0);
    }
    for (double bad : {-1e-3, -1.0, (double)NAN, -(double)INFINITY}) {
        flsim_optim o = optim(FLSIM_OPT_ADAGRAD);
        o.lr_decay = bad;
        refused(o, "Invalid lr_decay value");
        // lr_decay is read for Adagrad only: the other kinds accept whatever the field holds
        for (int kind : {FLSIM_OPT_ADAM, FLSIM_OPT_ADAMW, FLSIM_OPT_SGD, FLSIM_OPT_YOGI}) {
            flsim_optim x = optim(kind);
            x.lr_decay = bad;
            EXPECT(check_optim(&x) == 0);
        }
    }
    for (double bad : {1.0, 1.5, -0.1, (double)NAN, (double)INFINITY}) {
        flsim_optim o = optim(FLSIM_OPT_YOGI);
        o.beta1 = bad;
        refused(o, "Invalid beta parameter at index 0");
        o = optim(FLSIM_OPT_YOGI);
        o.beta2 = bad;
        refused(o, "Invalid beta parameter at index 1");
        // Adagrad reads no beta
        flsim_optim a = optim(FLSIM_OPT_ADAGRAD);
        a.beta1 = a.beta2 = bad;
        EXPECT(check_optim(&a) == 0);
    }
    {
        flsim_optim o = optim(FLSIM_OPT_YOGI);
        o.beta1 = o.beta2 = 0.0;
        EXPECT(check_optim(&o) == 0);
        for (int kind : {7, 5, -1}) {
            o = optim(kind);
            refused(o, "unknown optimizer kind");
        }
        EXPECT(check_optim(nullptr) == 1);
        // a valid optimizer reaches the pointer check
        o = optim(FLSIM_OPT_ADAGRAD);
        EXPECT(flsim_aggregate_optim_rule_push(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                               0, nullptr, 0, 1, &o, nullptr) == 1);
        EXPECT(strstr(flsim_last_error(), "null pointer") != nullptr);
        OptLaunch ol;
        EXPECT(make_opt_launch(&o, 5.0, 0, &ol) == 1);          // step must be >= 1
        EXPECT(make_opt_launch(&o, 0.0, 1, &ol) == 1);          // divisor out of range
        EXPECT(optim_n_state(&o) == 1);
        o = optim(FLSIM_OPT_YOGI);
        EXPECT(optim_n_state(&o) == 2);
        static_assert(opt_n_state(OK_ADAGRAD) == 1 && opt_n_state(OK_YOGI) == 2 &&
                      opt_n_state(OK_ADAM) == 2 && opt_n_state(OK_ADAMD) == 2 &&
                      opt_n_state(OK_SGDM) == 1 && opt_n_state(OK_SGD) == 0 &&
                      opt_n_state(OK_GOUT) == 0, "state arrays per kind");
    }
    // ---- make_opt_launch: the constant mapping ---------------------------------------------------
    for (double lr_decay : {0.0, 1e-4, 0.05, 3.0})
        for (long step : {1L, 2L, 3L, 1000L, 999999L, 1000000L})
            for (double wd : {0.0, 5e-4}) {
                flsim_optim o = optim(FLSIM_OPT_ADAGRAD);
                o.lr = 0.037;
                o.lr_decay = lr_decay;
                o.weight_decay = wd;
                OptLaunch ol;
                EXPECT(make_opt_launch(&o, 513.0, step, &ol) == 0);
                EXPECT(ol.ok == OK_ADAGRAD);
                const double clr = o.lr / (1.0 + (double)(step - 1) * lr_decay);
                EXPECT(bits(ol.oc.neg_lr) == bits((float)(-clr)));
                EXPECT(ol.oc.neg_lr < 0.f && (step > 1 || bits(ol.oc.neg_lr) == bits(-0.037f)));
                EXPECT(bits(ol.ac.eps) == bits(1e-10f));
                EXPECT(bits(ol.oc.wd) == bits((float)wd));
                EXPECT(ol.oc.flags == (wd != 0.0 ? OF_WD : 0));
                EXPECT(ol.ac.fk == 513.f && bits(ol.ac.rk) == bits(1.f / 513.f));
            }
    for (double b1 : {0.0, 0.9, 0.5})
        for (double b2 : {0.0, 0.99, 0.999})
            for (double wd : {0.0, 1e-3}) {
                flsim_optim o = optim(FLSIM_OPT_YOGI);
                o.beta1 = b1;
                o.beta2 = b2;
                o.weight_decay = wd;
                o.lr_decay = -7.0;                              // never read
                OptLaunch ol;
                EXPECT(make_opt_launch(&o, 6.0, 1000000, &ol) == 0);
                EXPECT(ol.ok == OK_YOGI);
                EXPECT(bits(ol.ac.w1) == bits((float)(1.0 - b1)));
                EXPECT(bits(ol.ac.w2) == bits((float)(1.0 - b2)));
                // the device's exact negation of w2 is torch's f32(-(1 - beta2))
                EXPECT(bits(-ol.ac.w2) == bits((float)(-(1.0 - b2))));
                EXPECT(bits(ol.oc.neg_lr) == bits((float)(-o.lr)));
                EXPECT(bits(ol.ac.eps) == bits(1e-3f));
                EXPECT(ol.oc.flags == (wd != 0.0 ? OF_WD : 0) && bits(ol.oc.wd) == bits((float)wd));
            }
    // ---- the element updates on exactly sized heap buffers -----------------------------------------
    const long n = 4099;
    uint32_t seed = 2021;
    auto rnd = [&]() {
        seed = seed * 1664525u + 1013904223u;
        return (float)((int)(seed >> 8) - (1 << 23)) * 0x1p-23f;     // [-1, 1)
    };
    std::vector<float> g(n), p0(n), m0(n), v0(n);
    for (long e = 0; e < n; ++e) {
        g[e] = 1e-2f * rnd();
        if (e % 17 == 0) g[e] = 0.f;
        if (e % 17 == 1) g[e] = -0.f;
        if (e % 17 == 2) g[e] = e % 2 ? 3e-39f : -3e-39f;
        if (e % 17 == 3) g[e] = 1e30f;
        p0[e] = rnd();
        m0[e] = 1e-3f * rnd();
        v0[e] = 1e-4f * fabsf(rnd());
        if (e % 17 >= 5 && e % 17 <= 7) v0[e] = g[e] * g[e];    // Yogi's sign 0
        if (e % 34 == 3) v0[e] = INFINITY;                      // ... and -+0 * inf = NaN
    }
    for (double wd : {0.0, 5e-4})
        for (long step : {1L, 3L, 1000000L}) {
            flsim_optim o = optim(FLSIM_OPT_ADAGRAD);
            o.lr_decay = 0.05;
            o.weight_decay = wd;
            OptLaunch ol;
            EXPECT(make_opt_launch(&o, 1.0, step, &ol) == 0);
            std::vector<float> pa(p0), sa(n), pb(p0), sb(n);
            for (long e = 0; e < n; ++e) sa[e] = sb[e] = fabsf(m0[e]);
            long diff = 0, moved = 0;
            for (long e = 0; e < n; ++e) {
                adagrad_launch(ol, g[e], pa[e], sa[e]);
                adagrad_text(o, step, g[e], pb[e], sb[e]);
                diff += !same_bits(pa[e], pb[e]) || !same_bits(sa[e], sb[e]);
                moved += bits(pa[e]) != bits(p0[e]);
            }
            EXPECT(diff == 0);
            EXPECT(moved > n / 2 || step == 1000000L);
        }
    for (double wd : {0.0, 5e-4})
        for (double b1 : {0.9, 0.0}) {
            flsim_optim o = optim(FLSIM_OPT_YOGI);
            o.beta1 = b1;
            o.weight_decay = wd;
            OptLaunch ol;
            EXPECT(make_opt_launch(&o, 1.0, 2, &ol) == 0);
            std::vector<float> pa(p0), ma(m0), va(v0), pb(p0), mb(m0), vb(v0);
            long diff = 0, nans = 0, signs[3] = {0, 0, 0};
            for (long e = 0; e < n; ++e) {
                const float d = v0[e] - g[e] * g[e];
                if (wd == 0.0) signs[d > 0.f ? 2 : (d < 0.f ? 0 : 1)]++;
                yogi_launch(ol, g[e], pa[e], ma[e], va[e]);
                yogi_text(o, g[e], pb[e], mb[e], vb[e]);
                diff += !same_bits(pa[e], pb[e]) || !same_bits(ma[e], mb[e]) || !same_bits(va[e], vb[e]);
                nans += va[e] != va[e];
            }
            EXPECT(diff == 0);
            EXPECT(nans >= n / 34 - 1);                         // g^2 = inf on v = inf
            if (wd == 0.0) EXPECT(signs[0] > n / 10 && signs[1] > n / 10 && signs[2] > n / 10);
        }
    printf(fails ? "%d checks FAILED\n" : "all checks passed\n", fails);
    return fails != 0;
}
