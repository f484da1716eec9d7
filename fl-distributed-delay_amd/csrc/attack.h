// Simulated Byzantine workers (include/flsim.h: flsim_attack): the omniscient attacks IPM (Xie et
// al. 2020) and ALIE (Baruch et al. 2019) on the bucketed entries.  The geometry of the launch
// (server.hip: k_attack), and the arithmetic of one element as ONE host + device function, so the
// kernel and the host twin (flsim_attack_eval_host) run the same code.
//
// Geometry: that of the geometric median's distance launch (csrc/geomed.h).  The k entries are
// padded to KPAD = 4 .. 64; a tile is E = 256 * U elements of every entry (thread t of the
// block's 256 owns the elements u * 256 + t, u < U); the grid is min(tiles, attack_max_blocks) and
// a block grid-strides over the tiles.  Nothing is summed across elements, so the bits do not
// depend on any of it.
#pragma once
#include <stdint.h>

#include "common.h"
#include "flsim.h"
#include "geomed.h"

namespace flsim {

inline int attack_kpad(int k) { return geomed_kpad(k); }
constexpr int attack_unroll(int kpad) { return geomed_unroll(kpad); }
constexpr int attack_tile_elems(int kpad) { return 256 * attack_unroll(kpad); }
constexpr int attack_max_blocks(int kpad) { return geomed_max_blocks(kpad); }
inline long attack_tiles(long P, int kpad) {
    const long E = attack_tile_elems(kpad);
    return (P + E - 1) / E;
}
inline long attack_blocks(long P, int kpad) {
    const long t = attack_tiles(P, kpad);
    return t < attack_max_blocks(kpad) ? t : attack_max_blocks(kpad);
}

// The crafted value b of one element, the text's attack_vector (flsim/robust.py):
//   y_j = (double)x[j] / hon[j] over the entries of hmask (honest[j] >= 1), index order;
//   mu = _seqsum(y) / kh;  ipm: b = mu * (-strength);
//   alie: var = _seqsum((y - mu) * (y - mu)) / kh, b = mu - sqrt(var) * strength;  (float)b.
// fp64, one rounding per operation (contraction off: never an fma), IEEE divisions, the correctly
// rounded sqrt; the first honest entry initialises each sum.  x: KPAD values (those outside hmask
// are not looked at); hon: (double)honest[j]; kh: the number of honest entries, >= 1.  hmask and k
// are uniform over the launch: every branch below is one.
template <int KPAD, int KIND>
__host__ __device__ __forceinline__ float attack_craft(const float* x, const double* hon,
                                                        uint64_t hmask, int k, double kh,
                                                        double strength) {
#pragma clang fp contract(off)
    constexpr int GRP = KPAD < 8 ? KPAD : 8;
    double y[KPAD];
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
    const double mu = s / kh;
    if constexpr (KIND == FLSIM_ATTACK_IPM) {
        return (float)(mu * (-strength));
    } else {
        double v = 0.0;
        have = false;
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
        const double p = __builtin_sqrt(var) * strength;
        return (float)(mu - p);
    }
}

// entries[j] of the text's attack_flat for an entry with byz[j] >= 1: H + b * (float)byz (fp32:
// a multiply, then an add), or the product alone where the entry has no honest part
__host__ __device__ __forceinline__ float attack_mix(float h, bool has_honest, float b,
                                                      float byz) {
#pragma clang fp contract(off)
    const float t = b * byz;
    return has_honest ? h + t : t;
}

}  // namespace flsim
