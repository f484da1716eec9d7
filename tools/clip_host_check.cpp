// Stand-alone host check of gradient clipping's host code (csrc/server.hip: check_clip, the clip
// buffer checks of flsim_aggregate_optim_clip_push, flsim_clip_partials,
// flsim_cascade_eval_host_clip), meant to be built with the host sanitizers and run on a CPU-only
// machine, as tools/crule_host_check.cpp is for delay compensation.  Nothing here launches a
// kernel: the clipped entry point is only driven into its refusals, which come before any launch.
//
//   cd fl-distributed-delay_amd && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 \
//       -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I../include -I../tools -Icsrc -x hip \
//       csrc/server.hip csrc/probe.cpp ../tools/clip_host_check.cpp -fsanitize=address,undefined \
//       -o /tmp/clip_host_check && /tmp/clip_host_check
//
// The twin runs on exactly-sized caller buffers (ASan sees any over-read or over-write) and is
// compared with the text restated here in plain C: the fp64 sum of squares, one fp32 add of
// f32(1e-6), the reciprocal, the multiply, the NaN-keeping clamp, one fp32 multiply per element.

#include <vector>

#include "host_check.h"

// the text, one rounding per line (volatile: no contraction whatever the flags)
static float coef_text(float t, float max_norm) {
    volatile float den = t + 1e-6f;
    volatile float rcp = 1.0f / den;
    volatile float c = rcp * max_norm;
    return c > 1.0f ? 1.0f : c;         // a NaN stays
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
    std::vector<float> S(n), now(n), g(n), out(n);
    std::vector<std::vector<float>> ys(narr, std::vector<float>(n)),
        ts(narr, std::vector<float>(n));
    std::vector<uint8_t> tail(n);
    uint32_t seed = 12345;
    auto rnd = [&]() {
        seed = seed * 1664525u + 1013904223u;
        return (float)((int)(seed >> 8) - (1 << 23)) * 0x1p-30f;
    };
    for (long e = 0; e < n; ++e) {
        S[e] = e % 13 == 2 ? 3e-39f : rnd();
        now[e] = rnd();
        for (int q = 0; q < narr; ++q) {
            ys[q][e] = e % 11 == 6 ? 3e-39f : 300.f * rnd();
            ts[q][e] = e % 5 == 0 ? now[e] : now[e] + 0.125f * rnd();
        }
        tail[e] = e >= 64;
    }
    const float* yp[narr] = {ys[0].data(), ys[1].data(), nullptr, ys[3].data()};
    const float* tp[narr] = {ts[0].data(), ts[1].data(), ts[2].data(), nullptr};
    std::vector<double> w = {pow(51.0, -0.5), 1.0 / 3.0, 1e-3, 1.0};
    const double W = 35.0 + w[1] + 2 * w[0] + w[2] + w[3];
    float nc[2];
    // the three forms: compensated + weighted, weighted, plain (w == NULL, theta_src == NULL)
    for (int form = 0; form < 3; ++form) {
        const double* wp = form < 2 ? w.data() : nullptr;
        const float* const* tpp = form == 0 ? tp : nullptr;
        const double div = form < 2 ? W : (double)k;
        if (form < 2)
            EXPECT(flsim_cascade_eval_host_c(prog.data(), info, S.data(), yp, wp, narr, div,
                                             now.data(), tpp, 2.0, tail.data(), n, g.data()) == 0);
        else {
            EXPECT(flsim_cascade_eval_host(prog.data(), info, S.data(), yp, narr, tail.data(), n,
                                           g.data()) == 0);
            for (long e = 0; e < n; ++e) g[e] = g[e] / (float)k;
        }
        double tot = 0.0;
        for (long e = 0; e < n; ++e) tot += (double)g[e] * (double)g[e];
        const float t = (float)sqrt(tot);
        for (double mn : {0.5 * t, (double)t, 2.0 * t, (double)INFINITY}) {
            EXPECT(flsim_cascade_eval_host_clip(prog.data(), info, S.data(), yp, wp, narr, div,
                                                now.data(), tpp, 2.0, tail.data(), n, mn,
                                                out.data(), nc) == 0);
            const float c = coef_text(t, (float)mn);
            EXPECT(bits(nc[0]) == bits(t));
            EXPECT(bits(nc[1]) == bits(c));
            EXPECT(mn < 2.0 * t || c == 1.0f);
            long diff = 0;
            for (long e = 0; e < n; ++e) {
                volatile float r = g[e] * c;
                diff += bits(out[e]) != bits(r);
            }
            EXPECT(diff == 0);
        }
    }
    // a NaN gradient: NaN norm, NaN coefficient (fminf would have dropped it)
    S[7] = NAN;
    EXPECT(flsim_cascade_eval_host_clip(prog.data(), info, S.data(), yp, nullptr, narr, k,
                                        nullptr, nullptr, 0.0, tail.data(), n, 1.0, out.data(),
                                        nc) == 0);
    EXPECT(nc[0] != nc[0] && nc[1] != nc[1]);
    // refusals of the twin: max_norm first, then the pointers
    for (double bad : {0.0, -1.0, (double)NAN, -(double)INFINITY}) {
        EXPECT(flsim_cascade_eval_host_clip(nullptr, nullptr, nullptr, nullptr, nullptr, 0, k,
                                            nullptr, nullptr, 0.0, nullptr, n, bad, nullptr,
                                            nullptr) == 1);
        EXPECT(strstr(flsim_last_error(), "max_norm") != nullptr);
    }
    EXPECT(flsim_cascade_eval_host_clip(prog.data(), info, S.data(), yp, nullptr, narr, k,
                                        nullptr, nullptr, 0.0, tail.data(), n, 1.0, nullptr,
                                        nc) == 1);
    EXPECT(strstr(flsim_last_error(), "null pointer") != nullptr);
    EXPECT(flsim_clip_partials(5596090) >= 5596090 / 1024 + 8 * 18);
    EXPECT(flsim_clip_partials(-1) == 0);

    // ---- the entry point's checks: heap structs, every refusal before a launch (made-up device
    // addresses are never read on the host) --------------------------------------------------------
    auto* clip = new flsim_clip();
    auto* rule = new flsim_rule();
    auto* comp = new flsim_rule_comp();
    flsim_optim o{};
    o.kind = FLSIM_OPT_SGD;
    o.lr = 0.1;
    const long sizes[1] = {64};
    float* fS = reinterpret_cast<float*>(0x10000);
    float* fP = reinterpret_cast<float*>(0x20000);
    float* fY = reinterpret_cast<float*>(0x30000);
    float* fT = reinterpret_cast<float*>(0x40000);
    float* fG = reinterpret_cast<float*>(0x50000);
    double* fD = reinterpret_cast<double*>(0x60000);
    float* fO = reinterpret_cast<float*>(0x70000);
    auto call = [&](const float* S_, float* S_out, float* theta_out, float* p_,
                    const flsim_rule_comp* c_) {
        return flsim_aggregate_optim_clip_push(S_, S_out, theta_out, rule, nullptr, c_, clip, p_,
                                               nullptr, nullptr, 64, sizes, 1, 1, &o, nullptr);
    };
    auto refused = [&](int rc, const char* what) {
        EXPECT(rc == 1);
        EXPECT(strstr(flsim_last_error(), what) != nullptr);
    };
    rule->k = 5;
    rule->c = 4;
    rule->n_arrays = 1;
    rule->arrays[0] = fY;
    comp->n = 1;
    comp->lambda = 2.0;
    comp->theta_src[0] = fT;
    clip->G = fG;
    clip->partials = fD;
    clip->n_partials = 1 << 20;
    clip->out = fO;
    for (float bad : {0.f, -1.f, NAN, -INFINITY}) {
        clip->max_norm = bad;
        refused(call(nullptr, nullptr, nullptr, nullptr, nullptr), "max_norm");
    }
    clip->max_norm = INFINITY;
    refused(call(nullptr, nullptr, nullptr, nullptr, nullptr), "null pointer");
    clip->max_norm = 1.f;
    clip->G = nullptr;
    refused(call(fS, nullptr, nullptr, fP, nullptr), "null clip buffer");
    clip->G = fG + 1;
    refused(call(fS, nullptr, nullptr, fP, nullptr), "16-byte aligned");
    clip->G = fG;
    clip->partials = fD + 1;
    refused(call(fS, nullptr, nullptr, fP, nullptr), "16-byte aligned");
    clip->partials = fD;
    clip->n_partials = 4;
    refused(call(fS, nullptr, nullptr, fP, nullptr), "n_partials");
    clip->n_partials = 1 << 20;
    for (float* over : {fS, fP, fS + 32, fS - 60, fY + 60, fT - 4}) {
        clip->G = over;
        refused(call(fS, nullptr, nullptr, fP, comp), "overlaps");
    }
    clip->G = fG;
    refused(call(fS, fG + 60, nullptr, fP, nullptr), "overlaps");
    refused(call(fS, nullptr, fG - 60, fP, nullptr), "overlaps");
    // adjacent to S: no overlap, the next refusal is reached
    clip->G = fS + 64;
    clip->n_partials = 0;
    refused(call(fS, nullptr, nullptr, fP, nullptr), "n_partials");
    delete clip;
    delete rule;
    delete comp;
    printf(fails ? "%d checks FAILED\n" : "all checks passed\n", fails);
    return fails != 0;
}
