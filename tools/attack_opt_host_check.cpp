// Stand-alone host check of the optimised attacks' host code (csrc/server.hip: check_attack_opt,
// flsim_attack_opt_partials, flsim_attack_opt_tile_elems, flsim_attack_opt_eval_host;
// csrc/attack_opt.h: the element code and the scalar solve the kernels share with the twin), meant
// to be built with the host sanitizers and run on a CPU-only machine, as
// tools/attack_host_check.cpp is for IPM and ALIE.  Nothing here launches a kernel: the entry point
// is only driven into its refusals, which come before any launch.
//
//   cd fl-distributed-delay_amd && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 \
//       -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I../include -I../tools -Icsrc -x hip \
//       csrc/server.hip csrc/probe.cpp ../tools/attack_opt_host_check.cpp \
//       -fsanitize=address,undefined -o /tmp/attack_opt_host_check && /tmp/attack_opt_host_check
//
// The twin runs on exactly-sized heap buffers (ASan sees any over-read or over-write; a write-only
// entry starts from NaNs) for every k in 1 .. 64 over random honest / mixed / fully Byzantine
// splits, both kinds and the three directions, and is compared with the text restated here in
// plain C: a, c, q bit for bit (the same operations in the same order), dist within the pairwise
// stage's bound, gamma bit for bit the closed form on the twin's own sums, b and the entries as
// numbers; and the budget is checked at b itself.

#include <vector>

#include "host_check.h"

struct Text {
    std::vector<double> a, c, dist, mu, p;
    double q, gamma;
};

static double root(double c, double q, double r) {
    if (r < 0.0) r = 0.0;
    volatile double cc = c * c, qr = q * r;
    volatile double s = sqrt(cc + qr);
    volatile double n = s - c;
    return n / q;
}

// the text over the kh honest entries (x[i][e], counts hc[i]) in plain C
static Text text(const std::vector<std::vector<float>>& x, const std::vector<int>& hc, long P,
                 int kind, int dir) {
    const int kh = (int)x.size();
    Text t;
    t.a.assign(kh, 0.0);
    t.c.assign(kh, 0.0);
    t.dist.assign((size_t)kh * kh, 0.0);
    t.mu.resize(P);
    t.p.resize(P);
    t.q = 0.0;
    std::vector<double> y(kh);
    for (long e = 0; e < P; ++e) {
        volatile double s = 0.0;
        for (int i = 0; i < kh; ++i) {
            volatile double v = (double)x[i][e] / (double)hc[i];
            y[i] = v;
            s = i == 0 ? (double)v : s + v;
        }
        volatile double mu = s / (double)kh;
        double p;
        if (dir == FLSIM_ATTACK_DIR_UNIT) {
            p = -mu;
        } else if (dir == FLSIM_ATTACK_DIR_SIGN) {
            p = mu > 0.0 ? -1.0 : mu < 0.0 ? 1.0 : -mu;
        } else {
            volatile double v = 0.0;
            for (int i = 0; i < kh; ++i) {
                volatile double d = y[i] - mu;
                volatile double dd = d * d;
                v = i == 0 ? (double)dd : v + dd;
            }
            volatile double var = v / (double)kh;
            p = -sqrt(var);
        }
        t.mu[e] = mu;
        t.p[e] = p;
        volatile double pp = p * p;
        t.q = t.q + pp;
        for (int i = 0; i < kh; ++i) {
            volatile double d = mu - y[i];
            volatile double dd = d * d, dp = d * p;
            t.a[i] = t.a[i] + dd;
            t.c[i] = t.c[i] + dp;
        }
    }
    for (int i = 0; i < kh; ++i)
        for (int j = i + 1; j < kh; ++j) {
            double s = 0.0;
            for (long e = 0; e < P; ++e) {
                volatile float xi = x[i][e] / (float)hc[i], xj = x[j][e] / (float)hc[j];
                const double d = (double)xi - (double)xj;
                s += d * d;
            }
            if (s != s) s = INFINITY;
            t.dist[(size_t)i * kh + j] = t.dist[(size_t)j * kh + i] = s;
        }
    (void)kind;
    return t;
}

// the closed form on given sums
static double gamma_of(int kind, const double* a, const double* c, double q, const double* dist,
                       int kh) {
    if (q == 0.0) return 0.0;
    if (kind == FLSIM_ATTACK_MINMAX) {
        double D = dist[0];
        for (int i = 0; i < kh * kh; ++i) D = dist[i] > D ? dist[i] : D;
        double g = 0.0;
        bool nan = false;
        for (int i = 0; i < kh; ++i) {
            const double gi = root(c[i], q, D - a[i]);
            nan |= gi != gi;
            if (i == 0 || gi < g) g = gi;
        }
        return nan ? (double)NAN : g;
    }
    double S = 0.0, A = 0.0, C = 0.0;
    for (int i = 0; i < kh; ++i) {
        volatile double s = dist[(size_t)i * kh];
        for (int j = 1; j < kh; ++j) s = s + dist[(size_t)i * kh + j];
        S = i == 0 || s > S ? (double)s : S;
        A = i == 0 ? a[i] : A + a[i];
        C = i == 0 ? c[i] : C + c[i];
    }
    return root(C, (double)kh * q, S - A);
}

static long cases = 0;

static void twin_case(int k, long P, int kind, int dir, double strength, float bad, bool with_b) {
    std::vector<int> honest(k), byz(k);
    bool any_h = false, any_b = false;
    for (int j = 0; j < k; ++j) {
        const int what = k == 1 ? 0 : (int)(uniform() * 3);     // mixed, honest-only, Byzantine
        honest[j] = what == 2 ? 0 : 1 + (int)(uniform() * 4);
        byz[j] = what == 1 ? 0 : 1 + (int)(uniform() * 3);
        any_h |= honest[j] > 0;
        any_b |= byz[j] > 0;
    }
    if (!any_h) honest[0] = 2;
    if (!any_b) byz[k - 1] = 1;
    std::vector<std::vector<float>> ent(k), before(k), hx;
    std::vector<int> hc;
    flsim_attack_opt a;
    memset(&a, 0, sizeof(a));
    a.kind = kind;
    a.dir = dir;
    a.k = k;
    a.strength = strength;
    int bad_entry = -1;
    for (int j = 0; j < k; ++j) {
        ent[j].resize(P);
        for (long e = 0; e < P; ++e)
            ent[j][e] = honest[j] ? (normal() * 0.5f + 1.f) * (float)honest[j] : NAN;
        if (honest[j] && bad != 0.f && bad_entry < 0) {
            bad_entry = j;
            for (long e = 3 % P; e < P; e += 7) ent[j][e] = bad;
        }
        before[j] = ent[j];
        if (honest[j]) {
            hx.push_back(ent[j]);
            hc.push_back(honest[j]);
        }
        a.entries[j] = ent[j].data();
        a.honest[j] = honest[j];
        a.byz[j] = byz[j];
    }
    const int kh = (int)hc.size();
    std::vector<float> b(P, -7.f);
    std::vector<double> dist((size_t)kh * kh, -1.0), stats(FLSIM_ATTACK_OPT_STATS, -1.0);
    double gamma = -1.0;
    EXPECT(flsim_attack_opt_eval_host(&a, dist.data(), stats.data(), &gamma,
                                      with_b ? b.data() : nullptr, P) == 0);
    const Text t = text(hx, hc, P, kind, dir);
    bool ok = true;
    const double rel = 2.0 * (double)(P + 2) * ldexp(1.0, -53);
    for (int i = 0; i < kh; ++i) {
        ok &= same_bits(stats[i], t.a[i]) || (stats[i] == 0.0 && t.a[i] == 0.0);
        ok &= same_bits(stats[64 + i], t.c[i]) || (stats[64 + i] == 0.0 && t.c[i] == 0.0);
        for (int j = 0; j < kh; ++j) {
            const double d = dist[(size_t)i * kh + j], r = t.dist[(size_t)i * kh + j];
            ok &= r == INFINITY ? d == r : fabs(d - r) <= rel * r;
        }
    }
    ok &= same_bits(stats[128], t.q) || (stats[128] == 0.0 && t.q == 0.0);
    EXPECT(ok);
    EXPECT(same_bits(gamma, gamma_of(kind, stats.data(), stats.data() + 64, stats[128],
                                     dist.data(), kh)));
    ok = true;
    volatile double coef = gamma * strength;
    for (long e = 0; e < P; ++e) {
        volatile double pc = t.p[e] * coef;
        volatile double b64 = t.mu[e] + pc;
        const float bt = (float)b64;
        if (with_b) ok &= same_number(b[e], bt);
        for (int j = 0; j < k; ++j) {
            if (byz[j] == 0) {
                ok &= bits(ent[j][e]) == bits(before[j][e]);
                continue;
            }
            volatile float m = bt * (float)byz[j];
            volatile float want = honest[j] ? before[j][e] + m : (float)m;
            ok &= same_number(ent[j][e], want);
        }
    }
    EXPECT(ok);
    if (bad == 0.f && kh >= 2 && strength == 1.0 && P == 257) {
        // the budget at the fp64 b: the largest (Min-Max) or the summed (Min-Sum) squared distance
        // to the honest y_i against D or S, to 1e-6 relative (the distances are over the fp32
        // means, the constraint over the fp64 y_i: they differ by the fp32 roundings of the means)
        double worst = 0.0, total = 0.0;
        for (int i = 0; i < kh; ++i) {
            double s = 0.0;
            for (long e = 0; e < P; ++e) {
                const double d = t.mu[e] + t.p[e] * gamma - (double)hx[i][e] / (double)hc[i];
                s += d * d;
            }
            worst = s > worst ? s : worst;
            total += s;
        }
        double D = 0.0, S = 0.0;
        for (int i = 0; i < kh; ++i) {
            double s = 0.0;
            for (int j = 0; j < kh; ++j) {
                s += dist[(size_t)i * kh + j];
                D = dist[(size_t)i * kh + j] > D ? dist[(size_t)i * kh + j] : D;
            }
            S = s > S ? s : S;
        }
        const double got = kind == FLSIM_ATTACK_MINMAX ? worst : total;
        const double lim = kind == FLSIM_ATTACK_MINMAX ? D : S;
        EXPECT(fabs(got - lim) <= 1e-6 * lim);
    }
    ++cases;
}

// the entry point's refusals on made-up addresses (never read: every refusal precedes any launch)
static void refusals() {
    const uintptr_t B = 0x1000000;
    flsim_attack_opt r;
    memset(&r, 0, sizeof(r));
    r.kind = FLSIM_ATTACK_MINMAX;
    r.dir = FLSIM_ATTACK_DIR_STD;
    r.k = 3;
    r.strength = 1.0;
    const int h[3] = {2, 1, 0}, c[3] = {0, 1, 2};
    for (int j = 0; j < 3; ++j) {
        r.entries[j] = (float*)(B * (2 + j));
        r.honest[j] = h[j];
        r.byz[j] = c[j];
    }
    flsim_attack_opt_scratch s;
    s.partials = (double*)(B * 6);
    s.n_partials = 1 << 20;
    s.dist = (double*)(B * 7);
    s.stats = (double*)(B * 8);
    s.gamma = (double*)(B * 9);
    float* bo = (float*)(B * 1);
    const long P = 64;
#define REFUSED(expr, msg)                                                       \
    do {                                                                         \
        EXPECT((expr) == 1);                                                     \
        EXPECT(strstr(flsim_last_error(), msg) != nullptr);                      \
    } while (0)
#define BOTH(q, b, n, msg)                                                                      \
    do {                                                                                        \
        REFUSED(flsim_attack_opt_entries(q, &s, b, n, nullptr), msg);                           \
        REFUSED(flsim_attack_opt_eval_host(q, s.dist, s.stats, s.gamma, b, n), msg);            \
    } while (0)
    BOTH(nullptr, bo, P, "null attack");
    flsim_attack_opt q = r;
    q.kind = FLSIM_ATTACK_ALIE;
    q.dir = 7;
    BOTH(&q, bo, P, "Invalid attack kind 1");
    q = r;
    q.dir = 3;
    q.k = 0;
    BOTH(&q, bo, P, "Invalid attack direction 3");
    q = r;
    q.k = 65;
    BOTH(&q, bo, P, "k = 65 entries");
    q = r;
    q.strength = NAN;
    BOTH(&q, nullptr, 0, "Invalid attack strength");
    q = r;
    q.honest[1] = -1;
    BOTH(&q, bo, P, "Invalid honest count -1 of entry 1");
    q = r;
    q.honest[0] = q.honest[1] = 0;
    q.byz[0] = 1;
    BOTH(&q, bo, P, "ValueError: no entry holds an honest worker");
    q = r;
    q.byz[1] = q.byz[2] = 0;
    q.honest[2] = 1;
    BOTH(&q, bo, P, "no entry holds a Byzantine worker");
    q = r;
    q.entries[1] = nullptr;
    BOTH(&q, bo, P, "null entry 1");
    BOTH(&r, bo + 1, P, "b_out must be 16-byte aligned");
    BOTH(&r, bo, 1L << 31, "out of range");
    q = r;
    q.entries[1] = q.entries[0] + (P - 4);
    BOTH(&q, bo, P, "entries 0 and 1 overlap");
    // the scratch (the entry point alone)
    REFUSED(flsim_attack_opt_entries(&r, nullptr, bo, P, nullptr), "null attack scratch");
    flsim_attack_opt_scratch t = s;
    t.gamma = (double*)(B * 9 + 8);
    REFUSED(flsim_attack_opt_entries(&r, &t, bo, P, nullptr), "16-byte aligned");
    t = s;
    t.n_partials = 5;
    REFUSED(flsim_attack_opt_entries(&r, &t, bo, P, nullptr), "n_partials = 5");
    t = s;
    t.stats = (double*)r.entries[2];
    REFUSED(flsim_attack_opt_entries(&r, &t, bo, P, nullptr), "entry 2 overlaps the attack scratch");
    t = s;
    t.gamma = (double*)bo;
    REFUSED(flsim_attack_opt_entries(&r, &t, bo, P, nullptr), "b_out overlaps the attack scratch");
    t = s;
    t.gamma = s.stats + 128;
    REFUSED(flsim_attack_opt_entries(&r, &t, bo, P, nullptr), "scratch buffers overlap");
    for (int k = 1; k <= 64; ++k) {
        const long E = flsim_attack_opt_tile_elems(k);
        EXPECT(E >= 256 && E % 256 == 0);
        EXPECT(flsim_attack_opt_partials(5596090, k) > flsim_krum_partials(5596090, k));
    }
    EXPECT(flsim_attack_opt_tile_elems(0) == 0 && flsim_attack_opt_partials(8, 65) == 0);
}

int main() {
    const long Ps[] = {1, 2, 7, 257};
    const int kinds[] = {FLSIM_ATTACK_MINMAX, FLSIM_ATTACK_MINSUM};
    for (int k = 1; k <= 64; ++k)
        for (long P : Ps)
            for (int kind : kinds)
                for (int dir = 0; dir < 3; ++dir)
                    twin_case(k, P, kind, dir, (k + dir) % 2 ? 1.0 : 0.6180339887, 0.f,
                              (k + P) % 3 != 0);
    const float bads[] = {NAN, INFINITY, -INFINITY};
    for (int k : {1, 2, 5, 9, 33, 64})
        for (int kind : kinds)
            for (int dir = 0; dir < 3; ++dir) {
                twin_case(k, 255, kind, dir, 0.0, 0.f, true);                 // strength 0
                for (float bad : bads) twin_case(k, 255, kind, dir, 1.5, bad, true);
            }
    printf("host twin: %ld cases checked against the text for k = 1 .. 64\n", cases);
    refusals();
    if (fails) {
        printf("%d checks FAILED\n", fails);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
