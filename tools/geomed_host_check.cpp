// Stand-alone host check of the geometric median's host code (csrc/server.hip: check_geomed, the
// pointer checks of flsim_geomed_optim_step, flsim_geomed_partials, flsim_geomed_eval_host;
// csrc/geomed.h: the scalar code the finish kernel shares with the twin), meant to be built with the
// host sanitizers and run on a CPU-only machine, as tools/krum_host_check.cpp is for Krum.  Nothing
// here launches a kernel: the entry point is only driven into its refusals, which come before any
// launch.
//
//   cd fl-distributed-delay_amd && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 \
//       -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I../include -I../tools -Icsrc -x hip \
//       csrc/server.hip csrc/probe.cpp ../tools/geomed_host_check.cpp \
//       -fsanitize=address,undefined -o /tmp/geomed_host_check && /tmp/geomed_host_check
//
// The twin runs on exactly-sized heap buffers (ASan sees any over-read or over-write) for every k
// in 1 .. 64 and is compared, bit for bit, with the text restated here in plain C in the twin's
// summation order: one fp32 division per value, z by one fp64 multiply and one add per term in
// index order (zero weights skipped), fp64 sums of (x - z)^2 by one fma per element, sqrt, the
// sequential sums and the divisions.

#include <vector>

#include "host_check.h"

// the text in plain C; x: the bucket means [k][P]
static void text(const std::vector<std::vector<float>>& x, const std::vector<double>& alpha, long P,
                 int iters, double nu, std::vector<double>& w, std::vector<double>& d2,
                 std::vector<double>& obj, std::vector<float>& g) {
    const int k = (int)x.size();
    std::vector<int> alive(k, 1);
    std::vector<double> a(k);
    for (int j = 0; j < k; ++j) {
        for (long e = 0; e < P; ++e) alive[j] &= (int)isfinite(x[j][e]);
        a[j] = alive[j] ? alpha[j] : 0.0;
    }
    auto wsum = [&](const double* wt, long e) {
        volatile double z = 0.0;
        bool have = false;
        for (int j = 0; j < k; ++j) {
            if (wt[j] == 0.0) continue;
            volatile double t = (double)x[j][e] * wt[j];
            z = have ? z + t : (double)t;
            have = true;
        }
        return (double)z;
    };
    w.assign((size_t)(iters + 1) * k, 0.0);
    d2.assign((size_t)iters * k, 0.0);
    obj.assign(iters, 0.0);
    volatile double s = a[0];
    for (int j = 1; j < k; ++j) s = s + a[j];
    for (int j = 0; j < k; ++j) w[j] = a[j] / s;
    std::vector<double> beta(k);
    for (int r = 0; r < iters; ++r) {
        double* d = &d2[(size_t)r * k];
        for (long e = 0; e < P; ++e) {
            const double z = wsum(&w[(size_t)r * k], e);
            for (int j = 0; j < k; ++j) {
                const double df = (double)x[j][e] - z;
                d[j] = fma(df, df, d[j]);
            }
        }
        volatile double so = 0.0, sb = 0.0;
        bool any = false;
        for (int j = 0; j < k; ++j) {
            if (!alive[j]) {
                d[j] = INFINITY;
                beta[j] = 0.0;
            } else {
                const double dist = sqrt(d[j]);
                volatile double t = a[j] * dist;
                so = any ? so + t : (double)t;
                any = true;
                beta[j] = a[j] / (dist < nu ? nu : dist);
            }
            sb = j == 0 ? beta[j] : sb + beta[j];
        }
        obj[r] = any ? (double)so : (double)NAN;
        for (int j = 0; j < k; ++j) w[(size_t)(r + 1) * k + j] = beta[j] / sb;
    }
    g.resize(P);
    for (long e = 0; e < P; ++e) g[e] = (float)wsum(&w[(size_t)iters * k], e);
}

static long cases = 0;

// one case of the twin against the text; dead: entry to poison (-1: none; -2: all), with `bad`
static void twin_case(int k, long P, int iters, int weighted, double nu, int null_entry, int dead,
                      float bad) {
    std::vector<std::vector<float>> sums(k), x(k);
    std::vector<double> alpha(k);
    flsim_geomed r;
    memset(&r, 0, sizeof(r));
    r.iters = iters;
    r.weighted = weighted;
    r.k = k;
    r.nu = nu;
    for (int j = 0; j < k; ++j) {
        r.count[j] = 1 + (int)(uniform() * 4);
        alpha[j] = weighted ? (double)r.count[j] : 1.0;
        sums[j].resize(P);
        x[j].resize(P);
        for (long e = 0; e < P; ++e) {
            float v = j == null_entry ? 0.f : normal() * (float)r.count[j];
            if ((dead == j || dead == -2) && e % 7 == 3 % P) v = bad;
            sums[j][e] = v;
            volatile float num = v, den = (float)r.count[j];
            x[j][e] = num / den;
        }
        r.entries[j] = j == null_entry ? nullptr : sums[j].data();
    }
    // exactly sized outputs on the heap
    std::vector<double> w((size_t)(iters + 1) * k, -7.0), d2((size_t)iters * k, -7.0),
        obj(iters, -7.0);
    std::vector<float> g(P, -7.f);
    EXPECT(flsim_geomed_eval_host(&r, P, w.data(), iters ? d2.data() : nullptr,
                                  iters ? obj.data() : nullptr, g.data()) == 0);
    std::vector<double> wt, dt, ot;
    std::vector<float> gt;
    text(x, alpha, P, iters, nu, wt, dt, ot, gt);
    bool ok = true;
    for (size_t i = 0; i < w.size(); ++i) ok &= same_bits(w[i], wt[i]);
    for (size_t i = 0; i < d2.size(); ++i) ok &= same_bits(d2[i], dt[i]);
    for (size_t i = 0; i < obj.size(); ++i) ok &= same_bits(obj[i], ot[i]);
    for (long e = 0; e < P; ++e) ok &= same_bits(g[e], gt[e]);
    EXPECT(ok);
    if (dead >= 0) {
        for (int it = 0; it <= iters; ++it) EXPECT(w[(size_t)it * k + dead] == 0.0);
        for (int it = 0; it < iters; ++it) EXPECT(isinf(d2[(size_t)it * k + dead]));
        if (k > 1)
            for (long e = 0; e < P; ++e) EXPECT(isfinite(g[e]));
    }
    if (dead == -2)
        for (long e = 0; e < P; ++e) EXPECT(g[e] != g[e]);
    ++cases;
}

static flsim_optim sgd() {
    flsim_optim o;
    memset(&o, 0, sizeof(o));
    o.kind = FLSIM_OPT_SGD;
    o.lr = 0.1;
    return o;
}

// the entry point's refusals on made-up addresses (never read: every refusal precedes any launch)
static void refusals() {
    const uintptr_t B = 0x1000000;
    float* p = (float*)(B * 1);
    flsim_geomed r;
    memset(&r, 0, sizeof(r));
    r.iters = 3;
    r.k = 3;
    r.nu = 1e-6;
    for (int j = 0; j < 3; ++j) {
        r.entries[j] = (const float*)(B * (8 + j));
        r.count[j] = j + 1;
    }
    flsim_geomed_scratch s;
    s.partials = (double*)(B * 11);
    s.n_partials = 1 << 20;
    s.w = (double*)(B * 12);
    s.d2 = (double*)(B * 13);
    s.obj = (double*)(B * 14);
    s.state = (int32_t*)(B * 15);
    const flsim_optim o = sgd();
    const long P = 64;
#define REFUSED(expr, msg)                                                       \
    do {                                                                         \
        EXPECT((expr) == 1);                                                     \
        EXPECT(strstr(flsim_last_error(), msg) != nullptr);                      \
    } while (0)
    {
        flsim_geomed q = r;
        q.k = 0;
        REFUSED(flsim_geomed_optim_step(&q, &s, nullptr, nullptr, p, nullptr, nullptr, P, 1, &o, nullptr), "k = 0 entries");
        q.k = 65;
        REFUSED(flsim_geomed_optim_step(&q, &s, nullptr, nullptr, p, nullptr, nullptr, P, 1, &o, nullptr), "k = 65 entries");
        q = r;
        q.iters = -1;
        REFUSED(flsim_geomed_optim_step(&q, &s, nullptr, nullptr, p, nullptr, nullptr, P, 1, &o, nullptr), "Invalid iters = -1");
        q.iters = 33;
        REFUSED(flsim_geomed_optim_step(&q, &s, nullptr, nullptr, p, nullptr, nullptr, P, 1, &o, nullptr), "Invalid iters = 33");
        q = r;
        const double bad_nu[] = {0.0, -1.0, NAN, INFINITY, -INFINITY};
        for (double nu : bad_nu) {
            q.nu = nu;
            REFUSED(flsim_geomed_optim_step(&q, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, P, 1, &o, nullptr), "Invalid nu");
            REFUSED(flsim_geomed_eval_host(&q, 4, nullptr, nullptr, nullptr, nullptr), "Invalid nu");
        }
        q = r;
        q.weighted = 2;
        REFUSED(flsim_geomed_optim_step(&q, &s, nullptr, nullptr, p, nullptr, nullptr, P, 1, &o, nullptr), "Invalid weighted = 2");
        q = r;
        q.count[1] = 0;
        REFUSED(flsim_geomed_optim_step(&q, &s, nullptr, nullptr, p, nullptr, nullptr, P, 1, &o, nullptr), "Invalid count 0 of entry 1");
    }
    REFUSED(flsim_geomed_optim_step(nullptr, &s, nullptr, nullptr, p, nullptr, nullptr, P, 1, &o, nullptr), "null geometric-median rule");
    REFUSED(flsim_geomed_optim_step(&r, &s, nullptr, nullptr, p, nullptr, nullptr, P, 1, nullptr, nullptr), "null optimizer");
    REFUSED(flsim_geomed_optim_step(&r, &s, nullptr, nullptr, nullptr, nullptr, nullptr, P, 1, &o, nullptr), "null pointer");
    REFUSED(flsim_geomed_optim_step(&r, &s, nullptr, nullptr, p + 1, nullptr, nullptr, P, 1, &o, nullptr), "16-byte aligned");
    REFUSED(flsim_geomed_optim_step(&r, &s, nullptr, nullptr, p, nullptr, nullptr, 0, 1, &o, nullptr), "out of range");
    REFUSED(flsim_geomed_optim_step(&r, nullptr, nullptr, nullptr, p, nullptr, nullptr, P, 1, &o, nullptr), "null geometric-median scratch");
    {
        flsim_geomed_scratch q = s;
        q.w = nullptr;
        REFUSED(flsim_geomed_optim_step(&r, &q, nullptr, nullptr, p, nullptr, nullptr, P, 1, &o, nullptr), "null geometric-median scratch");
        q = s;
        q.state = (int32_t*)(B * 15 + 4);
        REFUSED(flsim_geomed_optim_step(&r, &q, nullptr, nullptr, p, nullptr, nullptr, P, 1, &o, nullptr), "scratch must be 16-byte aligned");
        q = s;
        q.n_partials = 3;
        REFUSED(flsim_geomed_optim_step(&r, &q, nullptr, nullptr, p, nullptr, nullptr, P, 1, &o, nullptr), "this step writes 4");
        q = s;
        q.w = (double*)(B * 11 + 16);
        REFUSED(flsim_geomed_optim_step(&r, &q, nullptr, nullptr, p, nullptr, nullptr, P, 1, &o, nullptr), "scratch buffers overlap");
        q = s;
        q.obj = (double*)(B * 1 + 16);
        REFUSED(flsim_geomed_optim_step(&r, &q, nullptr, nullptr, p, nullptr, nullptr, P, 1, &o, nullptr), "scratch overlaps p/m/v/g_out");
    }
    {
        flsim_geomed q = r;
        q.entries[1] = (const float*)(B * 9 + 2);
        REFUSED(flsim_geomed_optim_step(&q, &s, nullptr, nullptr, p, nullptr, nullptr, P, 1, &o, nullptr), "entry 1 must be 4-byte aligned");
        q = r;
        q.entries[2] = p + (P - 1);
        REFUSED(flsim_geomed_optim_step(&q, &s, nullptr, nullptr, p, nullptr, nullptr, P, 1, &o, nullptr), "entry 2 overlaps");
        q = r;
        q.entries[0] = (const float*)(B * 12 + 8);
        REFUSED(flsim_geomed_optim_step(&q, &s, nullptr, nullptr, p, nullptr, nullptr, P, 1, &o, nullptr), "entry 0 overlaps the geometric-median scratch");
    }
    for (int k = 1; k <= 64; ++k) {
        const long E = flsim_geomed_tile_elems(k);
        EXPECT(E >= 256 && E % 256 == 0);
        const long sizes[] = {1, E - 1, E, E + 1, 3 * E + 5, 5596090, (1L << 31) - 1};
        for (long n : sizes) {
            const long need = flsim_geomed_partials(n, k);
            EXPECT(need >= k + 1 && need % (k + 1) == 0);
        }
        EXPECT(flsim_geomed_partials(E, k) < flsim_geomed_partials(E + 1, k));
    }
    EXPECT(flsim_geomed_partials(0, 8) == 0 && flsim_geomed_partials(8, 65) == 0);
    EXPECT(flsim_geomed_tile_elems(0) == 0 && flsim_geomed_tile_elems(65) == 0);
    {
        float one[4] = {1.f, 2.f, 3.f, 4.f};
        flsim_geomed q = r;
        for (int j = 0; j < 3; ++j) q.entries[j] = one;
        double w[12], d2[9], obj[3];
        REFUSED(flsim_geomed_eval_host(&q, 0, w, d2, obj, nullptr), "out of range");
        REFUSED(flsim_geomed_eval_host(&q, 4, nullptr, d2, obj, nullptr), "null pointer");
        REFUSED(flsim_geomed_eval_host(&q, 4, w, nullptr, obj, nullptr), "null pointer");
        REFUSED(flsim_geomed_eval_host(nullptr, 4, w, d2, obj, nullptr), "null geometric-median rule");
        EXPECT(flsim_geomed_eval_host(&q, 4, w, d2, obj, nullptr) == 0);
    }
}

int main() {
    const long Ps[] = {1, 2, 7, 257};
    const int its[] = {0, 1, 3, 8};
    for (int k = 1; k <= 64; ++k)
        for (long P : Ps)
            for (int iters : its)
                for (int weighted = 0; weighted < 2; ++weighted)
                    twin_case(k, P, iters, weighted, 1e-6, -1, -1, 0.f);
    const float bads[] = {NAN, INFINITY, -INFINITY};
    for (int k : {1, 2, 5, 9, 33, 64}) {
        twin_case(k, 255, 3, 1, 1e-6, k / 2, -1, 0.f);               // a NULL entry
        twin_case(k, 255, 3, 0, 2.5, -1, -1, 0.f);                   // a large floor
        for (float bad : bads)
            for (int iters : {0, 3}) {
                if (k > 1) twin_case(k, 255, iters, 0, 1e-6, -1, k / 2, bad);
                twin_case(k, 255, iters, 1, 1e-6, -1, -2, bad);      // every entry dead
            }
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
