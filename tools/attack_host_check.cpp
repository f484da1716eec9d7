// Stand-alone host check of the simulated Byzantine workers' host code (csrc/server.hip:
// check_attack, check_attack_pointers, flsim_attack_tile_elems, flsim_attack_eval_host;
// csrc/attack.h: the element code the kernel shares with the twin), meant to be built with the host
// sanitizers and run on a CPU-only machine, as tools/geomed_host_check.cpp is for the geometric
// median.  Nothing here launches a kernel: the entry point is only driven into its refusals, which
// come before any launch.
//
//   cd fl-distributed-delay_amd && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 \
//       -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I../include -I../tools -Icsrc -x hip \
//       csrc/server.hip csrc/probe.cpp ../tools/attack_host_check.cpp \
//       -fsanitize=address,undefined -o /tmp/attack_host_check && /tmp/attack_host_check
//
// The twin runs on exactly-sized heap buffers (ASan sees any over-read or over-write; a write-only
// entry starts from NaNs, which would show in every result if it were read) for every k in 1 .. 64
// over random honest / mixed / fully Byzantine splits, and is compared, as numbers, with the text
// restated here in plain C: fp64 divisions, sequential sums in index order, sqrt, one fp64 -> fp32
// rounding, then a separate fp32 multiply and add.

#include <vector>

#include "host_check.h"

// the text's attack_vector for one element in plain C
static float text_b(const std::vector<float>& x, const std::vector<int>& honest, int kind,
                    double strength) {
    std::vector<double> y;
    for (size_t j = 0; j < x.size(); ++j)
        if (honest[j] >= 1) {
            volatile double q = (double)x[j] / (double)honest[j];
            y.push_back((double)q);
        }
    const double kh = (double)y.size();
    volatile double s = y[0];
    for (size_t j = 1; j < y.size(); ++j) s = s + y[j];
    volatile double mu = s / kh;
    if (kind == FLSIM_ATTACK_IPM) {
        volatile double b = mu * (-strength);
        return (float)b;
    }
    volatile double v = 0.0;
    for (size_t j = 0; j < y.size(); ++j) {
        volatile double d = y[j] - mu;
        volatile double t = d * d;
        v = j == 0 ? (double)t : v + t;
    }
    volatile double var = v / kh;
    volatile double p = sqrt(var) * strength;
    volatile double b = mu - p;
    return (float)b;
}

static long cases = 0;

// one case of the twin against the text.  bad: a value put into one honest entry (0: none)
static void twin_case(int k, long P, int kind, double strength, float bad, bool with_b) {
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
    // exactly sized heap buffers; a write-only entry starts from a NaN pattern
    std::vector<std::vector<float>> ent(k), before(k);
    flsim_attack a;
    memset(&a, 0, sizeof(a));
    a.kind = kind;
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
        a.entries[j] = ent[j].data();
        a.honest[j] = honest[j];
        a.byz[j] = byz[j];
    }
    std::vector<float> b(P, -7.f);
    EXPECT(flsim_attack_eval_host(&a, with_b ? b.data() : nullptr, P) == 0);
    bool ok = true;
    std::vector<float> x(k);
    for (long e = 0; e < P; ++e) {
        for (int j = 0; j < k; ++j) x[j] = before[j][e];
        const float bt = text_b(x, honest, kind, strength);
        if (with_b) ok &= same_number(b[e], bt);
        for (int j = 0; j < k; ++j) {
            if (byz[j] == 0) {
                ok &= bits(ent[j][e]) == bits(before[j][e]);
                continue;
            }
            volatile float t = bt * (float)byz[j];
            volatile float want = honest[j] ? before[j][e] + t : (float)t;
            ok &= same_number(ent[j][e], want);
        }
    }
    EXPECT(ok);
    ++cases;
}

// the entry point's refusals on made-up addresses (never read: every refusal precedes any launch)
static void refusals() {
    const uintptr_t B = 0x1000000;
    flsim_attack r;
    memset(&r, 0, sizeof(r));
    r.kind = FLSIM_ATTACK_ALIE;
    r.k = 3;
    r.strength = 1.0;
    const int h[3] = {2, 1, 0}, c[3] = {0, 1, 2};
    for (int j = 0; j < 3; ++j) {
        r.entries[j] = (float*)(B * (2 + j));
        r.honest[j] = h[j];
        r.byz[j] = c[j];
    }
    float* bo = (float*)(B * 1);
    const long P = 64;
#define REFUSED(expr, msg)                                                       \
    do {                                                                         \
        EXPECT((expr) == 1);                                                     \
        EXPECT(strstr(flsim_last_error(), msg) != nullptr);                      \
    } while (0)
#define BOTH(q, b, n, msg)                                                       \
    do {                                                                         \
        REFUSED(flsim_attack_entries(q, b, n, nullptr), msg);                    \
        REFUSED(flsim_attack_eval_host(q, b, n), msg);                           \
    } while (0)
    BOTH(nullptr, bo, P, "null attack");
    {
        flsim_attack q = r;
        q.kind = 2;
        BOTH(&q, bo, P, "Invalid attack kind 2");
        q = r;
        q.k = 0;
        BOTH(&q, bo, P, "k = 0 entries");
        q.k = 65;
        BOTH(&q, bo, P, "k = 65 entries");
        q = r;
        const double bad_s[] = {-1.0, NAN, INFINITY, -INFINITY};
        for (double s : bad_s) {
            q.strength = s;
            BOTH(&q, nullptr, 0, "Invalid attack strength");
        }
        q = r;
        q.honest[1] = -1;
        BOTH(&q, bo, P, "Invalid honest count -1 of entry 1");
        q = r;
        q.byz[2] = -2;
        BOTH(&q, bo, P, "Invalid Byzantine count -2 of entry 2");
        q = r;
        q.honest[1] = q.byz[1] = 0;
        BOTH(&q, bo, P, "entry 1 holds no worker");
        q = r;
        q.honest[0] = q.honest[1] = 0;
        q.byz[0] = 1;
        BOTH(&q, bo, P, "ValueError: no entry holds an honest worker");
        q = r;
        q.byz[1] = q.byz[2] = 0;
        q.honest[2] = 1;
        BOTH(&q, bo, P, "no entry holds a Byzantine worker");
        // the fields come before the pointers
        q = r;
        q.kind = 9;
        q.entries[0] = nullptr;
        BOTH(&q, bo + 1, 0, "Invalid attack kind 9");
        q = r;
        q.entries[1] = nullptr;
        BOTH(&q, bo, P, "null entry 1");
        q = r;
        q.entries[2] = (float*)(B * 4 + 4);
        BOTH(&q, bo, P, "entry 2 must be 16-byte aligned");
        BOTH(&r, bo + 1, P, "b_out must be 16-byte aligned");
        BOTH(&r, bo, 0, "out of range");
        BOTH(&r, bo, 1L << 31, "out of range");
        q = r;
        q.entries[1] = q.entries[0] + (P - 4);
        BOTH(&q, bo, P, "entries 0 and 1 overlap");
        BOTH(&r, r.entries[2] + (P - 4), P, "entry 2 overlaps b_out");
    }
    for (int k = 1; k <= 64; ++k) {
        const long E = flsim_attack_tile_elems(k);
        EXPECT(E >= 256 && E % 256 == 0);
    }
    EXPECT(flsim_attack_tile_elems(0) == 0 && flsim_attack_tile_elems(65) == 0);
}

int main() {
    const long Ps[] = {1, 2, 7, 257};
    for (int k = 1; k <= 64; ++k)
        for (long P : Ps)
            for (int kind = 0; kind < 2; ++kind) {
                twin_case(k, P, kind, kind ? 0.8416212335729143 : 1.3, 0.f, true);
                twin_case(k, P, kind, kind ? 2.5 : 4.0, 0.f, false);
            }
    const float bads[] = {NAN, INFINITY, -INFINITY};
    for (int k : {1, 2, 5, 9, 33, 64})
        for (int kind = 0; kind < 2; ++kind) {
            twin_case(k, 255, kind, 0.0, 0.f, true);                 // strength 0
            for (float bad : bads) twin_case(k, 255, kind, 1.5, bad, true);
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
