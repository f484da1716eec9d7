// Geometric median by smoothed Weiszfeld iterations ("RFA", Pillutla, Kakade and Harchaoui 2022;
// include/flsim.h: flsim_geomed): the geometry of the distance launch (server.hip: k_geomed_dist),
// shared by the host code that sizes the caller's partials, and the scalar fp64 code of one
// iteration as ONE host + device function, so the finish kernel (k_geomed_finish) and the host
// twin (flsim_geomed_eval_host) run the same code.
//
// Geometry.  The k entries are padded to KPAD = 4 .. 64 accumulators a thread; a tile is
// E = 256 * U elements of every entry (thread t of the block's 256 owns the elements
// u * 256 + t, u < U, of a tile: a wave's load is one coalesced 256-byte row).  The grid is
// min(tiles, geomed_max_blocks) and tile t belongs to block t % grid: both depend on (P, k) alone.
// A block writes k doubles (slot j: its sum of (x_j - z)^2) and, in slot k, the 64 bits of its
// "entry j held a NaN or an inf" mask, stored slot-major (partials[slot][block]).
#pragma once
#include <stdint.h>

#include "common.h"
#include "flsim.h"

namespace flsim {

inline int geomed_kpad(int k) {
    int kp = 4;
    while (kp < k) kp <<= 1;
    return kp;
}
// elements a thread owns per tile: k * U loads are in flight, and U independent chains form z
constexpr int geomed_unroll(int kpad) { return kpad <= 16 ? 4 : kpad == 32 ? 2 : 1; }
constexpr int geomed_tile_elems(int kpad) { return 256 * geomed_unroll(kpad); }
// the grid's cap: about the blocks 256 CUs hold at once at the kernel's registers; each block's
// sums are read back by the one-block finish launch, so the cap also bounds that launch
constexpr int geomed_max_blocks(int kpad) { return kpad <= 8 ? 2048 : kpad <= 32 ? 1024 : 512; }
inline long geomed_tiles(long P, int kpad) {
    const long E = geomed_tile_elems(kpad);
    return (P + E - 1) / E;
}
inline long geomed_blocks(long P, int kpad) {
    const long t = geomed_tiles(P, kpad);
    return t < geomed_max_blocks(kpad) ? t : geomed_max_blocks(kpad);
}

// the words of flsim_geomed_scratch.state after the k dead flags
enum { GEOMED_ST_REDO = 0, GEOMED_ST_NDEAD = 1, GEOMED_ST_WORDS = 4 };

// alpha_j of the text with the dead entries' set to zero
__host__ __device__ inline double geomed_alpha(int weighted, int32_t count, int32_t dead) {
    return dead ? 0.0 : (weighted ? (double)count : 1.0);
}

// _seqsum: sequential fp64 adds in index order
__host__ __device__ inline double geomed_seqsum(const double* v, int k) {
    double s = v[0];
    for (int j = 1; j < k; ++j) s = s + v[j];
    return s;
}

// w^(0) = a / _seqsum(a): the alpha-weighted mean of the live entries (every entry dead: 0 / 0, a
// NaN, as the text's formula gives)
__host__ __device__ inline void geomed_w0(const double* a, int k, double* w) {
    const double s = geomed_seqsum(a, k);
    for (int j = 0; j < k; ++j) w[j] = a[j] / s;
}

// a weight takes part in _wsum unless it is +-0 (a NaN weight does)
__host__ __device__ inline bool geomed_nonzero(double w) {
    return (__builtin_bit_cast(uint64_t, w) << 1) != 0;
}

// One iteration's scalar code, the text's lines from d2_r[~alive] = inf to w.append(...):
//   d = sqrt(d2) (correctly rounded); obj = _seqsum(a * d over the live entries) (none: NaN);
//   beta = a / max(d, nu) (dead: 0); w_next = beta / _seqsum(beta).
// d2 is rewritten in place: +inf for a dead entry.  a: geomed_alpha.  Worker `lane` of `nlanes`
// takes the entries lane, lane + nlanes, ...; sync() separates the three phases (the host: one
// lane and a no-op; the kernel: its threads and __syncthreads); the two sequential sums are
// worker 0's.  term: k words of the caller's; sums[0] = obj, sums[1] = _seqsum(beta).
template <class Sync>
__host__ __device__ inline void geomed_iterate(double* d2, const double* a, const int32_t* dead,
                                               int k, double nu, double* term, double* sums,
                                               double* w_next, int lane, int nlanes, Sync sync) {
    for (int j = lane; j < k; j += nlanes) {
        double beta = 0.0, t = 0.0;
        if (dead[j]) {
            d2[j] = (double)__builtin_inff();
        } else {
            const double d = __builtin_sqrt(d2[j]);
            t = a[j] * d;
            beta = a[j] / (d < nu ? nu : d);    // torch.maximum: a NaN d stays
        }
        term[j] = t;
        w_next[j] = beta;
    }
    sync();
    if (lane == 0) {
        double so = 0.0;
        bool any = false;
        for (int j = 0; j < k; ++j) {
            if (dead[j]) continue;
            so = any ? so + term[j] : term[j];
            any = true;
        }
        sums[0] = any ? so : (double)__builtin_nanf("");
        sums[1] = geomed_seqsum(w_next, k);
    }
    sync();
    for (int j = lane; j < k; j += nlanes) w_next[j] = w_next[j] / sums[1];
}

}  // namespace flsim
