// Stand-alone host check of the weighted rule's host code (csrc/server.hip: check_weights,
// make_weights, flsim_cascade_eval_host_w), meant to be built with the host sanitizers and run on
// a CPU-only machine.  Nothing here launches a kernel: the weighted entry point is only driven
// into its refusals, which come before any launch.
//
//   cd fl-distributed-delay_amd && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 \
//       -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I../include -I../tools -Icsrc -x hip \
//       csrc/server.hip csrc/probe.cpp ../tools/wrule_host_check.cpp -fsanitize=address,undefined \
//       -o /tmp/wrule_host_check && /tmp/wrule_host_check
//
// It also answers the division question of DESIGN 6: div_const's arithmetic (q0 = a * RN(1/b),
// one fma correction) restated on the host against the IEEE quotient, over adversarial numerators
// for integer and non-integer divisors.  It prints the count of differing words per divisor.

#include <vector>

#include "host_check.h"

static float div_const_host(float a, float b, float rb) {
    const float q0 = a * rb;
    const float r = fmaf(-q0, b, a);
    const float q = fmaf(r, rb, q0);
    const float aq = fabsf(q0);
    return (aq >= 0x1p-124f && aq <= 0x1p+124f) ? q : a / b;
}

int main() {
    // ---- the host twin on exactly-sized caller buffers (ASan sees any over-read) --------------
    const int k = 40, nev = 5, narr = 4;
    const int32_t pos[nev] = {0, 3, 4, 20, 39}, arr[nev] = {1, 0, 0, 2, 3};
    const int cap = 2 * (72 + 40 * (nev + 8));
    std::vector<int32_t> prog(cap);
    int32_t info[4];
    EXPECT(flsim_cascade_program(k, pos, arr, nev, prog.data(), cap, info) == 0);
    const long n = 71;
    std::vector<float> S(n), out(n), outp(n);
    std::vector<std::vector<float>> ys(narr, std::vector<float>(n));
    std::vector<uint8_t> tail(n);
    uint32_t seed = 12345;
    auto rnd = [&]() {
        seed = seed * 1664525u + 1013904223u;
        return (float)((int)(seed >> 8) - (1 << 23)) * 0x1p-30f;
    };
    for (long e = 0; e < n; ++e) {
        S[e] = e % 13 == 3 ? 1e30f : (e % 13 == 2 ? 3e-39f : rnd());
        for (auto& y : ys) y[e] = e % 11 == 5 ? -1e30f : rnd();
        tail[e] = e >= 64;
    }
    const float* yp[narr] = {ys[0].data(), ys[1].data(), nullptr, ys[3].data()};
    std::vector<double> w = {pow(51.0, -0.5), 1.0 / 3.0, 1e-3, 1.0};
    const double W = 35.0 + w[1] + 2 * w[0] + w[2] + w[3];
    EXPECT(flsim_cascade_eval_host_w(prog.data(), info, S.data(), yp, w.data(), narr, W,
                                     tail.data(), n, out.data()) == 0);
    // all weights 1.0 and the divisor k: the plain cascade sum divided by k
    std::vector<double> ones(narr, 1.0);
    EXPECT(flsim_cascade_eval_host_w(prog.data(), info, S.data(), yp, ones.data(), narr, k,
                                     tail.data(), n, out.data()) == 0);
    EXPECT(flsim_cascade_eval_host(prog.data(), info, S.data(), yp, narr, tail.data(), n,
                                   outp.data()) == 0);
    for (long e = 0; e < n; ++e) EXPECT(bits(out[e]) == bits(outp[e] / (float)k));
    // refusals of the twin
    std::vector<double> bad = w;
    bad[1] = -1.0;
    EXPECT(flsim_cascade_eval_host_w(prog.data(), info, S.data(), yp, bad.data(), narr, W,
                                     tail.data(), n, out.data()) == 1);
    bad[1] = NAN;
    EXPECT(flsim_cascade_eval_host_w(prog.data(), info, S.data(), yp, bad.data(), narr, W,
                                     tail.data(), n, out.data()) == 1);
    EXPECT(flsim_cascade_eval_host_w(prog.data(), info, S.data(), yp, w.data(), narr, 0.0,
                                     tail.data(), n, out.data()) == 1);
    EXPECT(strstr(flsim_last_error(), "ZeroDivisionError") != nullptr);

    // ---- the weights copy of the entry point: a heap struct, every refusal before a launch ------
    auto* wts = new flsim_rule_weights();
    auto* rule = new flsim_rule();
    flsim_optim o{};
    o.kind = FLSIM_OPT_SGD;
    o.lr = 0.1;
    const long sizes[1] = {64};
    float* fakeS = reinterpret_cast<float*>(0x10000);
    float* fakeP = reinterpret_cast<float*>(0x20000);
    rule->k = 5;
    rule->c = 4;
    rule->n_arrays = 1;
    rule->arrays[0] = fakeS;
    wts->n = 1;
    wts->w[0] = 0.5;
    wts->divisor = 4.5;
    EXPECT(flsim_aggregate_optim_wrule_push(fakeS, nullptr, rule, wts, fakeP, nullptr, nullptr, 64,
                                            sizes, 1, 1, &o, nullptr) == 1);
    EXPECT(strstr(flsim_last_error(), "NotImplementedError") != nullptr);
    wts->n = FLSIM_MAX_ARRAYS + 1;
    EXPECT(flsim_aggregate_optim_wrule_push(nullptr, nullptr, nullptr, wts, nullptr, nullptr,
                                            nullptr, 64, sizes, 1, 1, &o, nullptr) == 1);
    wts->n = FLSIM_MAX_ARRAYS;
    for (int q = 0; q < FLSIM_MAX_ARRAYS; ++q) wts->w[q] = 0.25;
    wts->w[FLSIM_MAX_ARRAYS - 1] = -0.25;
    EXPECT(flsim_aggregate_optim_wrule_push(nullptr, nullptr, nullptr, wts, nullptr, nullptr,
                                            nullptr, 64, sizes, 1, 1, &o, nullptr) == 1);
    EXPECT(strstr(flsim_last_error(), "Invalid weight") != nullptr);
    wts->w[FLSIM_MAX_ARRAYS - 1] = 0.25;
    wts->divisor = 0.0;
    EXPECT(flsim_aggregate_optim_wrule_push(nullptr, nullptr, nullptr, wts, nullptr, nullptr,
                                            nullptr, 64, sizes, 1, 1, &o, nullptr) == 1);
    EXPECT(strstr(flsim_last_error(), "ZeroDivisionError") != nullptr);
    delete wts;
    delete rule;

    // ---- div_const against the IEEE quotient ------------------------------------------------------
    const double divs[] = {5.0, 513.0, 40.0, 512.0 + pow(3.0, -0.5), 4.0 + pow(51.0, -0.5),
                           36.0 + 1.0 / 3.0 + 1e-3, 2.5773502691896257, 0.14002800840280097,
                           1.0 / 3.0, 16777215.0 / 8388608.0};
    for (double d : divs) {
        const float b = (float)d;
        volatile float one = 1.f, vb = b;
        const float rb = one / vb;
        long diff = 0, tot = 0;
        // numerators: every quotient neighbourhood q * b for q over a spread of significands, the
        // products perturbed by a few ulps (the halfway cases of the division), and a random sweep
        for (uint32_t mant = 0; mant < (1u << 23); mant += 4099) {
            float q;
            const uint32_t qb = 0x3f800000u | mant;
            memcpy(&q, &qb, 4);
            const float a0 = q * b;
            for (int du = -3; du <= 3; ++du) {
                const uint32_t ab = bits(a0) + (uint32_t)du;
                float a;
                memcpy(&a, &ab, 4);
                for (float sc : {1.f, 0x1p-60f, 0x1p+60f, -1.f}) {
                    const float x = a * sc;
                    diff += bits(div_const_host(x, b, rb)) != bits(x / b);
                    ++tot;
                }
            }
        }
        for (int i = 0; i < 2000000; ++i) {
            seed = seed * 1664525u + 1013904223u;
            const uint32_t ab = (seed >> 9) | 0x3f800000u;
            float a;
            memcpy(&a, &ab, 4);
            diff += bits(div_const_host(a, b, rb)) != bits(a / b);
            ++tot;
        }
        printf("divisor %.17g: %ld of %ld quotients differ from IEEE\n", d, diff, tot);
    }
    printf(fails ? "%d checks FAILED\n" : "all checks passed\n", fails);
    return fails != 0;
}
