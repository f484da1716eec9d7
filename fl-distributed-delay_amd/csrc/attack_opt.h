// The optimised attacks Min-Max and Min-Sum of Shejwalkar and Houmansadr (NDSS 2021) on the
// bucketed entries (include/flsim.h: flsim_attack_opt): the geometry of the stats launch
// (server.hip: k_attack_opt_stats), the arithmetic of one element, and the scalar solve for gamma,
// each as ONE host + device function, so the kernels and the host twin
// (flsim_attack_opt_eval_host) run the same code.  The mix launch is k_attack's (csrc/attack.h).
//
// Geometry of the stats launch: that of k_attack, over the kh honest entries alone (compacted on
// the host, padded to KPAD = 4 .. 64).  A thread keeps 2 * KPAD + 1 fp64 sums, so the unroll is
// smaller than k_attack's; the grid is min(tiles, attack_opt_max_blocks) and a block grid-strides
// over the tiles.  A block writes 2 * kh + 1 doubles, slot-major (partials[slot][block]): slot i
// is a_i, slot kh + i is c_i, slot 2 * kh is q.
#pragma once
#include <stdint.h>

#include "attack.h"
#include "common.h"
#include "flsim.h"

namespace flsim {

// k_attack's KIND for the mix of the optimised attacks: ATTACK_CRAFT_OPT + FLSIM_ATTACK_DIR_*
// (Min-Max and Min-Sum differ in gamma alone)
constexpr int ATTACK_CRAFT_OPT = 2;

inline int attack_opt_kpad(int kh) { return attack_kpad(kh); }
constexpr int attack_opt_unroll(int kpad) { return kpad <= 8 ? 4 : kpad == 16 ? 2 : 1; }
constexpr int attack_opt_tile_elems(int kpad) { return 256 * attack_opt_unroll(kpad); }
constexpr int attack_opt_max_blocks(int kpad) { return attack_max_blocks(kpad); }
inline long attack_opt_tiles(long P, int kpad) {
    const long E = attack_opt_tile_elems(kpad);
    return (P + E - 1) / E;
}
inline long attack_opt_blocks(long P, int kpad) {
    const long t = attack_opt_tiles(P, kpad);
    return t < attack_opt_max_blocks(kpad) ? t : attack_opt_max_blocks(kpad);
}
// the doubles the stats launch writes for (P, kh)
inline long attack_opt_stats_partials(long P, int kh) {
    return attack_opt_blocks(P, attack_opt_kpad(kh)) * (2 * kh + 1);
}

// y_j and mu of one element, attack_craft's first lines text for text (csrc/attack.h; called
// from there instead, ALIE's and IPM's kernels come out with other registers at KPAD >= 16, and
// they are to stay instruction-identical): y[j] is set for the entries of hmask alone
template <int KPAD>
__host__ __device__ __forceinline__ double attack_mean(const float* x, const double* hon,
                                                        uint64_t hmask, int k, double kh,
                                                        double (&y)[KPAD]) {
#pragma clang fp contract(off)
    constexpr int GRP = KPAD < 8 ? KPAD : 8;
    double s = 0.0;
    bool have = false;
#pragma unroll
    for (int j0 = 0; j0 < KPAD; j0 += GRP) {
        if (j0 < k) {
#pragma unroll
            for (int j = j0; j < j0 + GRP; ++j) {
                if ((hmask >> j) & 1) {
                    y[j] = (double)x[j] / hon[j];
                    s = have ? s + y[j] : y[j];
                    have = true;
                }
            }
        }
    }
    return s / kh;
}

// mu and the direction p of one element (the text's opt_attack_parts): y and mu as
// attack_mean; unit: p = -mu; std: p = -sqrt(_seqsum((y - mu) * (y - mu)) / kh), the correctly
// rounded sqrt; sign: p = -sign(mu), sign(0) = 0 and a NaN stays.  fp64, contraction off.
template <int KPAD, int DIR>
__host__ __device__ __forceinline__ void attack_opt_dir(const float* x, const double* hon,
                                                        uint64_t hmask, int k, double kh,
                                                        double (&y)[KPAD], double& mu, double& p) {
#pragma clang fp contract(off)
    constexpr int GRP = KPAD < 8 ? KPAD : 8;
    mu = attack_mean<KPAD>(x, hon, hmask, k, kh, y);
    if constexpr (DIR == FLSIM_ATTACK_DIR_UNIT) {
        p = -mu;
    } else if constexpr (DIR == FLSIM_ATTACK_DIR_SIGN) {
        p = mu > 0.0 ? -1.0 : mu < 0.0 ? 1.0 : -mu;
    } else {
        double v = 0.0;
        bool have = false;
#pragma unroll
        for (int j0 = 0; j0 < KPAD; j0 += GRP) {
            if (j0 < k) {
#pragma unroll
                for (int j = j0; j < j0 + GRP; ++j) {
                    if ((hmask >> j) & 1) {
                        const double d = y[j] - mu;
                        const double t = d * d;
                        v = have ? v + t : t;
                        have = true;
                    }
                }
            }
        }
        const double var = v / kh;
        p = -__builtin_sqrt(var);
    }
}

// The crafted value of one element: b = (float)(mu + p * coef), coef = gamma * strength (one
// multiply, launch-uniform): a multiply and an add, then one fp64 -> fp32 rounding.
template <int KPAD, int DIR>
__host__ __device__ __forceinline__ float attack_opt_craft(const float* x, const double* hon,
                                                           uint64_t hmask, int k, double kh,
                                                           double coef) {
#pragma clang fp contract(off)
    double y[KPAD], mu, p;
    attack_opt_dir<KPAD, DIR>(x, hon, hmask, k, kh, y, mu, p);
    const double t = p * coef;
    return (float)(mu + t);
}

// One element's 2 * kh + 1 products added to the caller's sums: with e_i = mu - y_i,
// a[i] += e_i * e_i, c[i] += e_i * p, q += p * p (a product, then an add: never an fma).  Every
// entry i < k is honest here (the table is compacted).  live == false (an element past P): the
// sums gain 0.
template <int KPAD, int DIR>
__host__ __device__ __forceinline__ void attack_opt_stats_elem(const float* x, const double* hon,
                                                                int k, double kh, bool live,
                                                                double (&a)[KPAD],
                                                                double (&c)[KPAD], double& q) {
#pragma clang fp contract(off)
    constexpr int GRP = KPAD < 8 ? KPAD : 8;
    const uint64_t hmask = k >= 64 ? ~0ull : (1ull << k) - 1;
    double y[KPAD], mu, p;
    attack_opt_dir<KPAD, DIR>(x, hon, hmask, k, kh, y, mu, p);
    const double pp = p * p;
    q = q + (live ? pp : 0.0);
#pragma unroll
    for (int j0 = 0; j0 < KPAD; j0 += GRP) {
        if (j0 < k) {
#pragma unroll
            for (int j = j0; j < j0 + GRP; ++j) {
                if (j < k) {
                    const double e = mu - y[j];
                    const double ee = e * e, ep = e * p;
                    a[j] = a[j] + (live ? ee : 0.0);
                    c[j] = c[j] + (live ? ep : 0.0);
                }
            }
        }
    }
}

// gamma of one constraint: the larger root of q g^2 + 2 c g - r = 0 with r clamped at 0
__host__ __device__ inline double attack_opt_root(double c, double q, double r) {
#pragma clang fp contract(off)
    if (r < 0.0) r = 0.0;
    const double cc = c * c, qr = q * r;
    return (__builtin_sqrt(cc + qr) - c) / q;
}

// The text's opt_gamma on the kh x kh matrix `dist` and the sums a, c, q.  Worker `lane` of
// `nlanes` takes the rows lane, lane + nlanes, ...: row i's largest distance -> rmax[i], its
// sum in index order (the first term initialises) -> rsum[i]; sync(); worker 0 then runs the
// scalar code and returns gamma (the other workers' return value is not used).  fp64, contraction
// off, IEEE division and the correctly rounded sqrt.
template <class Sync>
__host__ __device__ inline double attack_opt_gamma(int kind, const double* a, const double* c,
                                                   double q, const double* dist, int kh,
                                                   double* rmax, double* rsum, int lane,
                                                   int nlanes, Sync sync) {
#pragma clang fp contract(off)
    for (int i = lane; i < kh; i += nlanes) {
        const double* row = dist + (long)i * kh;
        double m = row[0], s = row[0];
        for (int j = 1; j < kh; ++j) {
            m = row[j] > m ? row[j] : m;
            s = s + row[j];
        }
        rmax[i] = m;
        rsum[i] = s;
    }
    sync();
    if (lane != 0) return 0.0;
    if (q == 0.0) return 0.0;
    if (kind == FLSIM_ATTACK_MINMAX) {
        double D = rmax[0];
        for (int i = 1; i < kh; ++i) D = rmax[i] > D ? rmax[i] : D;
        double g = 0.0;
        bool nan = false;
        for (int i = 0; i < kh; ++i) {
            const double gi = attack_opt_root(c[i], q, D - a[i]);
            nan |= gi != gi;
            if (i == 0 || gi < g) g = gi;
        }
        return nan ? (double)__builtin_nanf("") : g;
    }
    double S = rsum[0], A = a[0], C = c[0];
    for (int i = 1; i < kh; ++i) {
        S = rsum[i] > S ? rsum[i] : S;
        A = A + a[i];
        C = C + c[i];
    }
    const double Q = (double)kh * q;
    return attack_opt_root(C, Q, S - A);
}

}  // namespace flsim
