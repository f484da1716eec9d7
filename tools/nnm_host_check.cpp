// Stand-alone host check of nearest-neighbour mixing's host code (csrc/server.hip: check_nnm, the
// pointer checks of flsim_nnm_entries, flsim_nnm_partials, flsim_nnm_tile_elems,
// flsim_nnm_eval_host; csrc/nnm.h: the selection and the element code the kernels share with the
// twin), meant to be built with the host sanitizers and run on a CPU-only machine, as
// tools/attack_host_check.cpp is for the attack.  Nothing here launches a kernel: the entry point
// is only driven into its refusals, which come before any launch.
//
//   cd fl-distributed-delay_amd && hipcc -O1 -g -std=c++17 --offload-arch=gfx950 \
//       -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -I../include -I../tools -Icsrc -x hip \
//       csrc/server.hip csrc/probe.cpp ../tools/nnm_host_check.cpp \
//       -fsanitize=address,undefined -o /tmp/nnm_host_check && /tmp/nnm_host_check
//
// The twin runs on exactly-sized heap buffers (ASan sees any over-read or over-write) for every k
// in 1 .. 64 and f in {0, 1, (k - 1) / 2}, with duplicate entries and a poisoned one mixed in, and
// is compared with the text restated here in plain C: the distances the twin's own way (fp64 fma
// in element order; both are checked symmetric with a zero diagonal), the neighbours by sorting
// (distance, index) pairs, the mixed values by sequential fp32 adds and one division.

#include <algorithm>
#include <utility>
#include <vector>

#include "host_check.h"

int main() {
    long cases = 0;
    for (int k = 1; k <= 64; ++k) {
        const long P = 5 + k % 7;
        const int fs[3] = {0, 1, (k - 1) / 2};
        for (int fi = 0; fi < 3; ++fi) {
            const int f = fs[fi];
            if (2 * f >= k || (fi > 0 && f == fs[fi - 1])) continue;
            flsim_nnm a;
            memset(&a, 0, sizeof a);
            a.f = f;
            a.k = k;
            std::vector<float*> ent(k);
            for (int j = 0; j < k; ++j) {
                a.count[j] = 1 + j % 5;
                ent[j] = (float*)malloc(sizeof(float) * P);        // exactly sized
                for (long e = 0; e < P; ++e)
                    ent[j][e] = normal() * (1.f + 0.25f * j) * (float)a.count[j];
                a.entries[j] = ent[j];
            }
            if (k >= 4) {           // a duplicate of entry 0 and a poisoned entry
                memcpy(ent[2], ent[0], sizeof(float) * P);
                a.count[2] = a.count[0];
                ent[k - 1][P / 2] = (fi & 1) ? NAN : INFINITY;
            }
            std::vector<std::vector<float>> before(k);
            for (int j = 0; j < k; ++j) before[j].assign(ent[j], ent[j] + P);
            double* dist = (double*)malloc(sizeof(double) * k * k);
            uint64_t* nbr = (uint64_t*)malloc(sizeof(uint64_t) * k);
            float* out = (float*)malloc(sizeof(float) * k * P);
            EXPECT(flsim_nnm_eval_host(&a, P, dist, nbr, out) == 0);
            for (int j = 0; j < k; ++j)
                EXPECT(memcmp(before[j].data(), ent[j], sizeof(float) * P) == 0);
            // the text in plain C
            std::vector<std::vector<float>> x(k, std::vector<float>(P));
            for (int j = 0; j < k; ++j)
                for (long e = 0; e < P; ++e) {
                    volatile float q = ent[j][e] / (float)a.count[j];
                    x[j][e] = q;
                }
            for (int i = 0; i < k; ++i) {
                EXPECT(dist[i * k + i] == 0.0);
                std::vector<std::pair<double, int>> row(k);
                for (int j = 0; j < k; ++j) {
                    double d = 0.0;
                    if (j != i) {
                        const int lo = i < j ? i : j, hi = i < j ? j : i;
                        for (long e = 0; e < P; ++e) {
                            const double t = (double)x[lo][e] - (double)x[hi][e];
                            d = fma(t, t, d);
                        }
                        if (d != d) d = INFINITY;
                    }
                    EXPECT(dist[i * k + j] == d && dist[j * k + i] == d);
                    row[j] = std::make_pair(d, j);
                }
                std::sort(row.begin(), row.end());
                uint64_t mask = 0;
                for (int r = 0; r < k - f; ++r) mask |= 1ull << row[r].second;
                EXPECT(nbr[i] == mask);
                for (long e = 0; e < P; ++e) {
                    volatile float acc = 0.f;
                    bool have = false;
                    for (int j = 0; j < k; ++j)
                        if ((mask >> j) & 1) {
                            acc = have ? acc + x[j][e] : x[j][e];
                            have = true;
                        }
                    volatile float fn = (float)(k - f);
                    volatile float y = acc / fn;
                    EXPECT(same_number(out[(long)i * P + e], y));
                }
                ++cases;
            }
            // out is optional
            EXPECT(flsim_nnm_eval_host(&a, P, dist, nbr, nullptr) == 0);
            free(out);
            free(nbr);
            free(dist);
            for (int j = 0; j < k; ++j) free(ent[j]);
        }
    }
    // the sizing and the refusals (device entry point: made-up addresses, never read)
    EXPECT(flsim_nnm_partials(64, 3) == 16 && flsim_nnm_partials(0, 3) == 0);
    EXPECT(flsim_nnm_partials(1L << 22, 64) == flsim_krum_partials(1L << 22, 64));
    EXPECT(flsim_nnm_tile_elems(9) == flsim_attack_tile_elems(9) && flsim_nnm_tile_elems(65) == 0);
    flsim_nnm a;
    memset(&a, 0, sizeof a);
    flsim_nnm_scratch s;
    auto reset = [&] {
        a.f = 1;
        a.k = 3;
        for (int j = 0; j < 3; ++j) {
            a.count[j] = 1 + j;
            a.entries[j] = (float*)(uintptr_t)(0x4000000ul * (j + 1));
        }
        s.partials = (double*)(uintptr_t)0x1000000ul;
        s.n_partials = 16;
        s.dist = (double*)(uintptr_t)0x2000000ul;
        s.nbr = (uint64_t*)(uintptr_t)0x3000000ul;
    };
    const long P = 64;
    reset();
    EXPECT(refused(flsim_nnm_entries(nullptr, &s, P, nullptr), "null NNM"));
    a.k = 0;
    EXPECT(refused(flsim_nnm_entries(&a, &s, P, nullptr), "NNM over k = 0 entries"));
    a.k = 65;
    EXPECT(refused(flsim_nnm_entries(&a, &s, P, nullptr), "NNM over k = 65 entries"));
    reset();
    a.f = 2;
    EXPECT(refused(flsim_nnm_entries(&a, &s, P, nullptr), "Invalid NNM f = 2 for k = 3"));
    a.f = -1;
    EXPECT(refused(flsim_nnm_entries(&a, &s, P, nullptr), "Invalid NNM f = -1"));
    reset();
    a.count[1] = 0;
    EXPECT(refused(flsim_nnm_entries(&a, &s, P, nullptr), "Invalid count 0 of entry 1"));
    reset();
    a.entries[1] = nullptr;
    EXPECT(refused(flsim_nnm_entries(&a, &s, P, nullptr), "null entry 1"));
    reset();
    a.entries[2] = (float*)((uintptr_t)a.entries[2] + 4);
    EXPECT(refused(flsim_nnm_entries(&a, &s, P, nullptr), "entry 2 must be 16-byte aligned"));
    reset();
    EXPECT(refused(flsim_nnm_entries(&a, &s, 0, nullptr), "out of range"));
    EXPECT(refused(flsim_nnm_entries(&a, &s, 1L << 31, nullptr), "out of range"));
    EXPECT(refused(flsim_nnm_entries(&a, nullptr, P, nullptr), "null NNM scratch"));
    s.nbr = nullptr;
    EXPECT(refused(flsim_nnm_entries(&a, &s, P, nullptr), "null NNM scratch"));
    reset();
    s.dist = (double*)((uintptr_t)s.dist + 8);
    EXPECT(refused(flsim_nnm_entries(&a, &s, P, nullptr), "NNM scratch must be 16-byte aligned"));
    reset();
    s.n_partials = 15;
    EXPECT(refused(flsim_nnm_entries(&a, &s, P, nullptr), "NNM n_partials = 15"));
    reset();
    a.entries[1] = a.entries[0] + (P - 4);
    EXPECT(refused(flsim_nnm_entries(&a, &s, P, nullptr), "entries 0 and 1 overlap"));
    reset();
    s.dist = (double*)(a.entries[2] + (P - 4));
    EXPECT(refused(flsim_nnm_entries(&a, &s, P, nullptr), "entry 2 overlaps the NNM scratch"));
    reset();
    s.nbr = (uint64_t*)(s.partials + 14);
    EXPECT(refused(flsim_nnm_entries(&a, &s, P, nullptr), "NNM scratch buffers overlap"));
    reset();
    a.entries[0] = nullptr;
    double d9[9];
    uint64_t n3[3];
    EXPECT(refused(flsim_nnm_eval_host(&a, P, d9, n3, nullptr), "null entry 0"));
    printf("%ld rows checked, %d failures\n", cases, fails);
    return fails ? 1 : 0;
}
