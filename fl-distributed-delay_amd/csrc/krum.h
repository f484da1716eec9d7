// Krum / Multi-Krum (include/flsim.h: flsim_krum; Blanchard et al. 2017): the geometry of the
// all-pairs distance launch (server.hip: k_krum_dist), shared by the host code that sizes the
// caller's partials, and the score / selection code as ONE host + device function, so the finish
// kernel (k_krum_finish) and the host twin (flsim_krum_eval_host) run the same code.
//
// Geometry.  The k entries are padded to KPAD = 4 .. 64 rows (the rows past k are zero); a tile is
// E = KRUM_TILE_FLOATS / KPAD elements of every row.  The (i, j) pairs are cut into 4 x 4 blocks
// (ti, tj), ti <= tj, numbered row by row over the upper triangle: NPB = NB (NB + 1) / 2 of them,
// NB = KPAD / 4.  A block of the grid writes NPB * 16 doubles, slot krum_slot(i, j), stored
// slot-major (partials[slot][block]); only the
// slots with i < j < k are ever read.  The grid is min(tiles, krum_max_blocks) and tile t belongs
// to block t % grid: both depend on (P, k) alone.
#pragma once
#include <stdint.h>

#include "common.h"
#include "flsim.h"

namespace flsim {

constexpr int KRUM_TILE_FLOATS = 8192;
// the grid's cap: the blocks 256 CUs hold at once at the kernel's registers (three of 256 threads,
// two of KPAD = 64's 448); each block's sums are read back by the one-block finish launch, so the
// cap also bounds that launch
constexpr int krum_max_blocks(int kpad) { return kpad == 64 ? 512 : 768; }

inline int krum_kpad(int k) {
    int kp = 4;
    while (kp < k) kp <<= 1;
    return kp;
}
constexpr int krum_tile_elems(int kpad) { return KRUM_TILE_FLOATS / kpad; }
constexpr int krum_npb(int kpad) { return (kpad / 4) * (kpad / 4 + 1) / 2; }
inline long krum_tiles(long P, int kpad) {
    const long E = krum_tile_elems(kpad);
    return (P + E - 1) / E;
}
inline long krum_blocks(long P, int kpad) {
    const long t = krum_tiles(P, kpad);
    return t < krum_max_blocks(kpad) ? t : krum_max_blocks(kpad);
}

// the number of 4 x 4 block (ti, tj), ti <= tj < nb, and the slot of pair (i, j), i <= j
__host__ __device__ inline int krum_pb(int ti, int tj, int nb) {
    return ti * nb - ti * (ti - 1) / 2 + (tj - ti);
}
__host__ __device__ inline int krum_slot(int i, int j, int nb) {
    return krum_pb(i >> 2, j >> 2, nb) * 16 + (i & 3) * 4 + (j & 3);
}

// The rule text's score and selection from the k x k distance matrix `dist` (symmetric, no NaN:
// a NaN distance has become +inf):
//   score[i] = the sum of the k - f - 2 smallest dist[i][j], j != i, added in ascending order
//              (equal values: ascending j, which gives the same sum);
//   sel[0 .. m) = the m entries of lowest (score, index), in ascending index order.
// Worker `lane` of `nlanes` takes the rows lane, lane + nlanes, ...; sync() separates the three
// phases (the host: one lane and a no-op; the kernel: its threads and __syncthreads).  No array
// is indexed at run time but the caller's: each step of a row is one scan for the smallest
// (value, j) above the last one taken.  rank: k words of the caller's.
template <class Sync>
__host__ __device__ inline void krum_score_select(const double* dist, double* score, int32_t* rank,
                                                  int32_t* sel, int k, int f, int m, int lane,
                                                  int nlanes, Sync sync) {
    const int n = k - f - 2;
    for (int i = lane; i < k; i += nlanes) {
        const double* row = dist + (long)i * k;
        double acc = 0.0, lv = -1.0;            // every distance is >= 0
        int lj = -1;
        for (int r = 0; r < n; ++r) {
            double bv = 0.0;
            int bj = -1;
            for (int j = 0; j < k; ++j) {
                const double v = row[j];
                const bool after = v > lv || (v == lv && j > lj);
                const bool take = j != i && after && (bj < 0 || v < bv);
                bv = take ? v : bv;
                bj = take ? j : bj;
            }
            acc = r == 0 ? bv : acc + bv;
            lv = bv;
            lj = bj;
        }
        score[i] = acc;
    }
    sync();
    for (int i = lane; i < k; i += nlanes) {
        const double s = score[i];
        int below = 0;
        for (int l = 0; l < k; ++l) below += (score[l] < s || (score[l] == s && l < i)) ? 1 : 0;
        rank[i] = below;
    }
    sync();
    for (int i = lane; i < k; i += nlanes) {
        if (rank[i] >= m) continue;
        int pos = 0;
        for (int l = 0; l < i; ++l) pos += rank[l] < m ? 1 : 0;
        sel[pos] = i;
    }
}

}  // namespace flsim
