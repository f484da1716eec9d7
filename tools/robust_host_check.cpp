// Stand-alone host check of the robust rules' host code (csrc/server.hip: check_robust, the pointer
// checks of flsim_robust_optim_step, flsim_robust_eval_host; csrc/robust.h: the sorting network and
// select / sum the kernel shares with the twin), meant to be built with the host sanitizers and run
// on a CPU-only machine, as tools/clip_host_check.cpp is for clipping.  Nothing here launches a
// kernel: the entry point is only driven into its refusals, which come before any launch.
//
//   cd fl-distributed-delay_amd && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 \
//       -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I../include -I../tools -Icsrc -x hip \
//       csrc/server.hip csrc/probe.cpp ../tools/robust_host_check.cpp \
//       -fsanitize=address,undefined -o /tmp/robust_host_check && /tmp/robust_host_check
//
// The twin runs on exactly-sized heap buffers (ASan sees any over-read or over-write) for every k
// in 1 .. 64 and is compared with the text restated here in plain C: one fp32 division per value,
// a stable sort that puts NaN last, the lower median, or sequential fp32 adds in ascending order
// and one division.

#include <algorithm>
#include <vector>

#include "host_check.h"

// the text for one element (volatile: one rounding per operation whatever the flags)
static float text(std::vector<float> x, int kind, int trim) {
    const int k = (int)x.size();
    std::stable_sort(x.begin(), x.end(), [](float a, float b) {
        return (a == a) && (b != b || a < b);              // ascending, NaN last
    });
    if (kind == FLSIM_ROBUST_MEDIAN) return x[(k - 1) / 2];
    volatile float acc = x[trim];
    for (int j = trim + 1; j < k - trim; ++j) acc = acc + x[j];
    volatile float n = (float)(k - 2 * trim);
    return acc / n;
}

int main() {
    // ---- the host twin, every k in 1 .. 64 ----------------------------------------------------------
    uint32_t seed = 2024;
    auto rnd = [&]() {
        seed = seed * 1664525u + 1013904223u;
        return (float)((int)(seed >> 8) - (1 << 23)) * 0x1p-20f;
    };
    const int cnts[3] = {1, 3, 128};
    long checked = 0;
    for (int k = 1; k <= FLSIM_MAX_ARRAYS; ++k) {
        const long P = 1 + (k * 7) % 37;
        auto* r = new flsim_robust();
        std::vector<float*> ent(k, nullptr);
        for (int j = 0; j < k; ++j) {
            r->count[j] = cnts[(j + k) % 3];
            if (k > 2 && j == k / 2) continue;              // one NULL entry: all zeros
            ent[j] = new float[P];
            for (long e = 0; e < P; ++e) {
                float x = rnd();
                if (e % 9 == 4 && j % 3 == 0) x = NAN;
                if (e % 9 == 5) x = j % 2 ? INFINITY : -INFINITY;
                if (e % 9 == 6) x = j % 2 ? 0.f : -0.f;
                if (e % 9 == 7 && j > 0) x = ent[0] ? ent[0][e] : 1.f;      // duplicates
                ent[j][e] = x;
            }
            r->entries[j] = ent[j];
        }
        r->k = k;
        float* out = new float[P];
        for (int kind = 0; kind < 2; ++kind)
            for (int trim = 0; 2 * trim < k && (kind == 1 || trim == 0); ++trim) {
                r->kind = kind;
                r->trim = trim;
                EXPECT(flsim_robust_eval_host(r, P, out) == 0);
                for (long e = 0; e < P; ++e) {
                    std::vector<float> x(k);
                    for (int j = 0; j < k; ++j) {
                        volatile float s = ent[j] ? ent[j][e] : 0.f, c = (float)r->count[j];
                        x[j] = s / c;
                    }
                    const float ref = text(x, kind, trim);
                    if (!same_number(out[e], ref)) {
                        printf("FAIL k=%d kind=%d trim=%d e=%ld got %a want %a\n", k, kind, trim, e,
                               (double)out[e], (double)ref);
                        ++fails;
                    }
                    ++checked;
                }
            }
        delete[] out;
        for (float* p : ent) delete[] p;
        delete r;
    }
    printf("host twin: %ld values checked against the text for k = 1 .. %d\n", checked,
           FLSIM_MAX_ARRAYS);

    // ---- the entry point's checks: heap structs, every refusal before a launch (made-up device
    // addresses are never read on the host) --------------------------------------------------------
    auto* r = new flsim_robust();
    auto* clip = new flsim_clip();
    flsim_optim o{};
    o.kind = FLSIM_OPT_SGD;
    o.lr = 0.1;
    const long P = 64;
    float* fP = reinterpret_cast<float*>(0x20000);
    float* fM = reinterpret_cast<float*>(0x30000);
    float* fV = reinterpret_cast<float*>(0x40000);
    float* fG = reinterpret_cast<float*>(0x50000);
    double* fD = reinterpret_cast<double*>(0x60000);
    float* fO = reinterpret_cast<float*>(0x70000);
    float* fE = reinterpret_cast<float*>(0x80000);
    float* fX = reinterpret_cast<float*>(0x90000);
    auto reset = [&]() {
        memset(r, 0, sizeof(*r));
        r->kind = FLSIM_ROBUST_TRIMMED_MEAN;
        r->trim = 1;
        r->k = 3;
        for (int j = 0; j < 3; ++j) {
            r->entries[j] = fE + 0x1000 * j;
            r->count[j] = cnts[j];
        }
        clip->max_norm = 1.f;
        clip->G = fG;
        clip->partials = fD;
        clip->n_partials = 1 << 20;
        clip->out = fO;
        o = flsim_optim{};
        o.kind = FLSIM_OPT_SGD;
        o.lr = 0.1;
    };
    auto call = [&](const flsim_clip* c, float* g_out, float* p, float* m, float* v, long n,
                    long step, const flsim_optim* op) {
        return flsim_robust_optim_step(r, c, g_out, p, m, v, n, step, op, nullptr);
    };
    auto refused = [&](int rc, const char* what) {
        EXPECT(rc == 1);
        EXPECT(strstr(flsim_last_error(), what) != nullptr);
    };
    reset();
    refused(flsim_robust_optim_step(nullptr, nullptr, nullptr, fP, nullptr, nullptr, P, 1, &o,
                                    nullptr), "null robust rule");
    // hyper-parameters first: every pointer is NULL in these calls
    for (int kind : {-1, 2, 77}) {
        reset();
        r->kind = kind;
        refused(call(nullptr, nullptr, nullptr, nullptr, nullptr, P, 1, &o), "unknown robust rule");
    }
    for (int k : {0, -3, FLSIM_MAX_ARRAYS + 1, 1 << 30}) {
        reset();
        r->k = k;
        refused(call(nullptr, nullptr, nullptr, nullptr, nullptr, P, 1, &o), "entries (1 .. 64)");
    }
    for (int trim : {-1, 2, 40, 0x7FFFFFFF}) {
        reset();
        r->trim = trim;
        refused(call(nullptr, nullptr, nullptr, nullptr, nullptr, P, 1, &o), "Invalid trim");
    }
    reset();
    r->k = 2;                                               // 2 * trim == k
    refused(call(nullptr, nullptr, nullptr, nullptr, nullptr, P, 1, &o), "Invalid trim");
    reset();
    r->kind = FLSIM_ROBUST_MEDIAN;
    refused(call(nullptr, nullptr, nullptr, nullptr, nullptr, P, 1, &o), "takes no trim");
    for (int c : {0, -1, (int)0x80000000}) {
        reset();
        r->count[2] = c;
        refused(call(nullptr, nullptr, nullptr, nullptr, nullptr, P, 1, &o), "Invalid count");
    }
    reset();
    o.lr = -1.0;
    refused(call(nullptr, nullptr, nullptr, nullptr, nullptr, P, 1, &o), "Invalid learning rate");
    reset();
    o.kind = 9;
    refused(call(nullptr, nullptr, nullptr, nullptr, nullptr, P, 1, &o), "unknown optimizer kind");
    reset();
    o.nesterov = 1;
    refused(call(nullptr, nullptr, nullptr, nullptr, nullptr, P, 1, &o), "Nesterov");
    for (float bad : {0.f, -1.f, NAN, -INFINITY}) {
        reset();
        clip->max_norm = bad;
        refused(call(clip, nullptr, nullptr, nullptr, nullptr, P, 1, &o), "max_norm");
    }
    reset();
    refused(call(nullptr, nullptr, fP, nullptr, nullptr, P, 1, nullptr), "null optimizer");
    refused(call(clip, fX, fP, nullptr, nullptr, P, 1, nullptr), "null optimizer");
    // then the pointers
    refused(call(nullptr, nullptr, nullptr, nullptr, nullptr, P, 1, &o), "null pointer");
    o.momentum = 0.9;
    refused(call(nullptr, nullptr, fP, nullptr, nullptr, P, 1, &o), "null pointer");
    o.kind = FLSIM_OPT_ADAM;
    refused(call(nullptr, nullptr, fP, fM, nullptr, P, 1, &o), "null pointer");
    refused(call(nullptr, nullptr, fP, fM, fV, P, 0, &o), "step must be >= 1");
    refused(call(nullptr, nullptr, fP + 1, fM, fV, P, 1, &o), "16-byte aligned");
    refused(call(nullptr, nullptr, fP, fM + 2, fV, P, 1, &o), "16-byte aligned");
    refused(call(nullptr, nullptr, fP, fM, fV + 3, P, 1, &o), "16-byte aligned");
    refused(call(nullptr, fX + 1, fP, fM, fV, P, 1, &o), "16-byte aligned");
    for (long n : {0L, -5L, 1L << 31})
        refused(call(nullptr, nullptr, fP, fM, fV, n, 1, &o), "out of range");
    refused(call(nullptr, fP + 32, fP, fM, fV, P, 1, &o), "overlap each other");
    refused(call(nullptr, nullptr, fP, fM, fM + 60, P, 1, &o), "overlap each other");
    r->entries[1] = reinterpret_cast<const float*>(0x81002);
    refused(call(nullptr, nullptr, fP, fM, fV, P, 1, &o), "4-byte aligned");
    for (const float* over : {(const float*)fP, (const float*)(fP + 63), (const float*)(fP - 63),
                              (const float*)fM, (const float*)(fV + 8), (const float*)fX}) {
        reset();
        o.kind = FLSIM_OPT_ADAM;
        r->entries[2] = over;
        refused(call(nullptr, fX, fP, fM, fV, P, 1, &o), "entry 2 overlaps");
    }
    reset();
    r->entries[0] = fG + 60;
    refused(call(clip, nullptr, fP, nullptr, nullptr, P, 1, &o), "entry 0 overlaps clip G");
    reset();
    clip->G = nullptr;
    refused(call(clip, nullptr, fP, nullptr, nullptr, P, 1, &o), "null clip buffer");
    reset();
    clip->partials = fD + 1;
    refused(call(clip, nullptr, fP, nullptr, nullptr, P, 1, &o), "16-byte aligned");
    reset();
    clip->G = fP + 32;
    refused(call(clip, nullptr, fP, nullptr, nullptr, P, 1, &o), "clip G overlaps");
    // adjacent buffers do not overlap: the next refusal (too few partials) is reached
    reset();
    r->entries[0] = fP - 64;
    r->entries[1] = fP + 64;
    clip->n_partials = 0;
    refused(call(clip, nullptr, fP, nullptr, nullptr, P, 1, &o), "n_partials");
    // the twin's own refusals
    reset();
    float one[1] = {1.f};
    r->k = 0;
    EXPECT(flsim_robust_eval_host(r, 1, one) == 1);
    reset();
    EXPECT(flsim_robust_eval_host(r, 1, nullptr) == 1);
    EXPECT(flsim_robust_eval_host(r, 0, one) == 1);
    EXPECT(flsim_robust_eval_host(nullptr, 1, one) == 1);
    // the partials bound covers the robust step's one partial per 256-thread block
    for (long n : {1L, 255L, 257L, 5596090L, (1L << 31) - 1})
        EXPECT(flsim_clip_partials(n) >= (n + 255) / 256);
    delete r;
    delete clip;
    printf(fails ? "%d checks FAILED\n" : "all checks passed\n", fails);
    return fails != 0;
}
