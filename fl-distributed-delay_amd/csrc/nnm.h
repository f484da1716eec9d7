// Nearest-neighbour mixing (include/flsim.h: flsim_nnm; Allouah et al. 2023): the geometry of the
// mix launch (server.hip: k_nnm_mix), shared with the host, and the neighbour selection and the
// arithmetic of one mixed element as ONE host + device function each, so the kernels (k_nnm_finish,
// k_nnm_mix) and the host twin (flsim_nnm_eval_host) run the same code.  The distance launch is
// Krum's, with Krum's geometry (csrc/krum.h).
//
// Geometry of the mix: that of the attack's launch (csrc/attack.h).  The k entries are padded to
// KPAD = 4 .. 64; a tile is E = 256 * U elements of every entry (thread t of the block's 256 owns
// the elements u * 256 + t, u < U); the grid is min(tiles, nnm_max_blocks) and a block grid-strides
// over the tiles.  Nothing is summed across elements, so the bits do not depend on any of it.
#pragma once
#include <stdint.h>

#include "attack.h"
#include "common.h"
#include "flsim.h"

namespace flsim {

inline int nnm_kpad(int k) { return attack_kpad(k); }
constexpr int nnm_unroll(int kpad) { return attack_unroll(kpad); }
constexpr int nnm_tile_elems(int kpad) { return 256 * nnm_unroll(kpad); }
constexpr int nnm_max_blocks(int kpad) { return attack_max_blocks(kpad); }
inline long nnm_tiles(long P, int kpad) {
    const long E = nnm_tile_elems(kpad);
    return (P + E - 1) / E;
}
inline long nnm_blocks(long P, int kpad) {
    const long t = nnm_tiles(P, kpad);
    return t < nnm_max_blocks(kpad) ? t : nnm_max_blocks(kpad);
}

// The text's neighbour selection (flsim/robust.py: nnm_neighbours) from the k x k distance matrix
// `dist` (symmetric, zero diagonal, no NaN: a NaN distance has become +inf): bit j of nbr[i] is
// set for the k - f entries j of lowest (dist[i][j], j).  The diagonal is zero, so an entry is at
// the head of its own row (only exact duplicates at a lower index come before it), even one that
// holds a NaN; every other row sees such an entry at +inf, hence last.
// Worker `lane` of `nlanes` takes the rows lane, lane + nlanes, ... (the host: one lane; the
// kernel: its threads).  No array is indexed at run time but the caller's: each step of a row is
// one scan for the smallest (value, j) above the last one taken, as krum_score_select.
__host__ __device__ inline void nnm_select(const double* dist, uint64_t* nbr, int k, int f,
                                           int lane, int nlanes) {
    const int n = k - f;
    for (int i = lane; i < k; i += nlanes) {
        const double* row = dist + (long)i * k;
        double lv = -1.0;                       // every distance is >= 0
        int lj = -1;
        uint64_t mask = 0;
        for (int r = 0; r < n; ++r) {
            double bv = 0.0;
            int bj = -1;
            for (int j = 0; j < k; ++j) {
                const double v = row[j];
                const bool after = v > lv || (v == lv && j > lj);
                const bool take = after && (bj < 0 || v < bv);
                bv = take ? v : bv;
                bj = take ? j : bj;
            }
            mask |= 1ull << (bj & 63);
            lv = bv;
            lj = bj;
        }
        nbr[i] = mask;
    }
}

// One element of one mixed entry, the text's _nnm: the bucket means x[j] of the neighbours (the
// bits of `mask`, ascending j) added by sequential fp32 adds, the first one initialising the sum
// (contraction off: never an fma), then one IEEE fp32 division by fn = (float)(k - f).  x: KPAD
// values (those outside the mask are not looked at).  mask and k are uniform over the launch:
// every branch below is one, taken once for the U elements a thread owns (the host: U = 1).  x is
// only ever indexed by the unrolled u and j, so it stays in registers.
template <int KPAD, int U>
__host__ __device__ __forceinline__ void nnm_mix_elem(const float (&x)[U][KPAD], uint64_t mask,
                                                      int k, float fn, float (&y)[U]) {
#pragma clang fp contract(off)
    constexpr int GRP = KPAD < 8 ? KPAD : 8;
    float acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = 0.f;
    bool have = false;
#pragma unroll
    for (int j0 = 0; j0 < KPAD; j0 += GRP) {
        if (j0 < k && ((mask >> j0) & ((1ull << GRP) - 1))) {
#pragma unroll
            for (int j = j0; j < j0 + GRP; ++j) {
                if ((mask >> j) & 1) {
#pragma unroll
                    for (int u = 0; u < U; ++u) acc[u] = have ? acc[u] + x[u][j] : x[u][j];
                    have = true;
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
#if defined(__HIP_DEVICE_COMPILE__)
        y[u] = __fdiv_rn(acc[u], fn);
#else
        volatile float s = acc[u], d = fn;
        y[u] = s / d;
#endif
    }
}

}  // namespace flsim
