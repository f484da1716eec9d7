// Stand-alone host check of delay compensation's host code (csrc/server.hip: check_comp, make_comp,
// flsim_cascade_eval_host_c), meant to be built with the host sanitizers and run on a CPU-only
// machine, as tools/wrule_host_check.cpp is for the weighted rule.  Nothing here launches a
// kernel: the compensated entry point is only driven into its refusals, which come before any
// launch.
//
//   cd fl-distributed-delay_amd && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 \
//       -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I../include -I../tools -Icsrc -x hip \
//       csrc/server.hip csrc/probe.cpp ../tools/crule_host_check.cpp -fsanitize=address,undefined \
//       -o /tmp/crule_host_check && /tmp/crule_host_check
//
// The twin runs on exactly-sized caller buffers (ASan sees any over-read of a snapshot) and is
// compared with the five-rounding text restated here in plain C.

#include <vector>

#include "host_check.h"

// the text, one rounding per line (volatile: no contraction whatever the flags)
static float compensate_text(float x, float now, float src, float lam) {
    volatile float xx = x * x;
    volatile float h = xx * lam;
    volatile float d = now - src;
    volatile float hd = h * d;
    return x + hd;
}

int main() {
    // ---- the host twin ------------------------------------------------------------------------
    const int k = 40, nev = 5, narr = 4;
    const int32_t pos[nev] = {0, 3, 4, 20, 39}, arr[nev] = {1, 0, 0, 2, 3};
    const int cap = 2 * (72 + 40 * (nev + 8));
    std::vector<int32_t> prog(cap);
    int32_t info[4];
    EXPECT(flsim_cascade_program(k, pos, arr, nev, prog.data(), cap, info) == 0);
    const long n = 71;
    std::vector<float> S(n), now(n), out(n), outw(n);
    std::vector<std::vector<float>> ys(narr, std::vector<float>(n)),
        ts(narr, std::vector<float>(n)), yc(narr, std::vector<float>(n));
    std::vector<uint8_t> tail(n);
    uint32_t seed = 12345;
    auto rnd = [&]() {
        seed = seed * 1664525u + 1013904223u;
        return (float)((int)(seed >> 8) - (1 << 23)) * 0x1p-30f;
    };
    const double lambda = 2.0;
    for (long e = 0; e < n; ++e) {
        S[e] = e % 13 == 3 ? 1e30f : (e % 13 == 2 ? 3e-39f : rnd());
        now[e] = rnd();
        for (int q = 0; q < narr; ++q) {
            ys[q][e] = e % 11 == 5 ? -1e15f : (e % 11 == 6 ? 3e-39f : 300.f * rnd());
            ts[q][e] = e % 5 == 0 ? now[e] : now[e] + 0.125f * rnd();
            yc[q][e] = compensate_text(ys[q][e], now[e], ts[q][e], (float)lambda);
        }
        tail[e] = e >= 64;
    }
    // array 2 is a zero entry (its snapshot is ignored), array 3 has no snapshot
    const float* yp[narr] = {ys[0].data(), ys[1].data(), nullptr, ys[3].data()};
    const float* tp[narr] = {ts[0].data(), ts[1].data(), ts[2].data(), nullptr};
    const float* ycp[narr] = {yc[0].data(), yc[1].data(), nullptr, ys[3].data()};
    std::vector<double> w = {pow(51.0, -0.5), 1.0 / 3.0, 1e-3, 1.0};
    const double W = 35.0 + w[1] + 2 * w[0] + w[2] + w[3];
    // compensated twin == weighted twin over arrays compensated by the text
    EXPECT(flsim_cascade_eval_host_c(prog.data(), info, S.data(), yp, w.data(), narr, W,
                                     now.data(), tp, lambda, tail.data(), n, out.data()) == 0);
    EXPECT(flsim_cascade_eval_host_w(prog.data(), info, S.data(), ycp, w.data(), narr, W,
                                     tail.data(), n, outw.data()) == 0);
    long diff = 0, moved = 0;
    for (long e = 0; e < n; ++e) diff += bits(out[e]) != bits(outw[e]);
    EXPECT(diff == 0);
    // no weights (w == NULL: 1.0 each, divisor k), and no snapshots at all: the weighted twin
    std::vector<double> ones(narr, 1.0);
    EXPECT(flsim_cascade_eval_host_c(prog.data(), info, S.data(), yp, nullptr, narr, k, now.data(),
                                     tp, lambda, tail.data(), n, out.data()) == 0);
    EXPECT(flsim_cascade_eval_host_w(prog.data(), info, S.data(), ycp, ones.data(), narr, k,
                                     tail.data(), n, outw.data()) == 0);
    for (long e = 0; e < n; ++e) EXPECT(bits(out[e]) == bits(outw[e]));
    EXPECT(flsim_cascade_eval_host_c(prog.data(), info, S.data(), yp, ones.data(), narr, k,
                                     nullptr, nullptr, lambda, tail.data(), n, out.data()) == 0);
    EXPECT(flsim_cascade_eval_host_w(prog.data(), info, S.data(), yp, ones.data(), narr, k,
                                     tail.data(), n, outw.data()) == 0);
    for (long e = 0; e < n; ++e) {
        EXPECT(bits(out[e]) == bits(outw[e]));
        moved += bits(yc[0][e]) != bits(ys[0][e]);
    }
    EXPECT(moved > n / 2);                          // the compensation acts on these inputs
    // refusals of the twin
    EXPECT(flsim_cascade_eval_host_c(prog.data(), info, S.data(), yp, w.data(), narr, W,
                                     now.data(), tp, -1.0, tail.data(), n, out.data()) == 1);
    EXPECT(flsim_cascade_eval_host_c(prog.data(), info, S.data(), yp, w.data(), narr, W,
                                     now.data(), tp, NAN, tail.data(), n, out.data()) == 1);
    EXPECT(flsim_cascade_eval_host_c(prog.data(), info, S.data(), yp, w.data(), narr, W, nullptr,
                                     tp, lambda, tail.data(), n, out.data()) == 1);

    // ---- the entry point's checks and its launch-form copy: heap structs, every refusal before a
    // launch (made-up device addresses are never read on the host) ---------------------------------
    auto* comp = new flsim_rule_comp();
    auto* rule = new flsim_rule();
    flsim_optim o{};
    o.kind = FLSIM_OPT_SGD;
    o.lr = 0.1;
    const long sizes[1] = {64};
    float* fS = reinterpret_cast<float*>(0x10000);
    float* fP = reinterpret_cast<float*>(0x20000);
    float* fY = reinterpret_cast<float*>(0x30000);
    float* fT = reinterpret_cast<float*>(0x40000);
    float* fO = reinterpret_cast<float*>(0x50000);
    auto call = [&](const float* S_, float* S_out, float* theta_out, float* p_) {
        return flsim_aggregate_optim_crule_push(S_, S_out, theta_out, rule, nullptr, comp, p_,
                                                nullptr, nullptr, 64, sizes, 1, 1, &o, nullptr);
    };
    rule->k = 5;
    rule->c = 4;
    rule->n_arrays = 1;
    rule->arrays[0] = fY;
    comp->n = 1;
    comp->theta_src[0] = fT;
    for (double bad : {-0.5, (double)NAN, (double)INFINITY}) {
        comp->lambda = bad;
        EXPECT(call(nullptr, nullptr, nullptr, nullptr) == 1);
        EXPECT(strstr(flsim_last_error(), "lambda") != nullptr);
    }
    comp->lambda = 2.0;
    comp->n = FLSIM_MAX_ARRAYS;
    EXPECT(call(nullptr, nullptr, nullptr, nullptr) == 1);
    EXPECT(strstr(flsim_last_error(), "snapshots for") != nullptr);
    comp->n = 1;
    EXPECT(call(nullptr, nullptr, nullptr, nullptr) == 1);
    EXPECT(strstr(flsim_last_error(), "null pointer") != nullptr);
    rule->arrays[0] = fS;                           // a snapshot for S_t itself
    EXPECT(call(fS, nullptr, nullptr, fP) == 1);
    EXPECT(strstr(flsim_last_error(), "S_t itself") != nullptr);
    rule->arrays[0] = fY;
    EXPECT(call(fS, nullptr, fP, fP) == 1);
    EXPECT(strstr(flsim_last_error(), "theta_out aliases p") != nullptr);
    EXPECT(call(fS, nullptr, fT, fP) == 1);
    EXPECT(strstr(flsim_last_error(), "theta_out aliases the snapshot") != nullptr);
    comp->theta_src[0] = fT + 1;
    EXPECT(call(fS, nullptr, fO, fP) == 1);
    EXPECT(strstr(flsim_last_error(), "16-byte aligned") != nullptr);
    // all FLSIM_MAX_ARRAYS slots in use (a general-order rule: its program is a device pointer,
    // only its info is looked at): the copy into the launch form stays inside both structs
    rule->c = -1;
    rule->prog = reinterpret_cast<const int32_t*>(0x70000);
    rule->info[0] = 10;
    rule->info[1] = 5;
    rule->info[2] = 0;
    rule->info[3] = 4;
    rule->k = 4 + FLSIM_MAX_ARRAYS;
    rule->n_arrays = comp->n = FLSIM_MAX_ARRAYS;
    for (int q = 0; q < FLSIM_MAX_ARRAYS; ++q) {
        rule->arrays[q] = fY + 64 * q;
        comp->theta_src[q] = fT + 64 * q;
    }
    comp->theta_src[FLSIM_MAX_ARRAYS - 1] = fO;
    EXPECT(call(fS, nullptr, fO, fP) == 1);
    EXPECT(strstr(flsim_last_error(), "theta_out aliases the snapshot of array 63") != nullptr);
    delete comp;
    delete rule;
    printf(fails ? "%d checks FAILED\n" : "all checks passed\n", fails);
    return fails != 0;
}
