// Centered clipping with a carried center ("CClip", Karimireddy, He and Jaggi 2021;
// include/flsim.h: flsim_cclip): the scalar fp64 code of one iteration as ONE host + device
// function, so the finish kernel (server.hip: k_cclip_finish) and the host twin
// (flsim_cclip_eval_host) run the same code.  The geometry of the distance launch (k_cclip_dist) is
// the geometric median's (csrc/geomed.h: geomed_kpad, geomed_unroll, geomed_tile_elems,
// geomed_max_blocks), and so are alpha (geomed_alpha) and the sequential sum (geomed_seqsum).
#pragma once
#include <stdint.h>

#include "common.h"
#include "flsim.h"
#include "geomed.h"

namespace flsim {

// the words of flsim_cclip_scratch.state after the k dead flags
enum { CCLIP_ST_NDEAD = 0, CCLIP_ST_WORDS = 4 };

// the words of cclip_iterate's sums
enum { CCLIP_SUM_ALPHA = 0, CCLIP_SUM_OM = 1, CCLIP_SUM_U = 2, CCLIP_SUM_WORDS = 3 };

// s of the text from a squared distance: q = tau / sqrt(d2) (correctly rounded; d = 0: +inf);
// q where q < 1, 1 where q >= 1, and q itself where it is a NaN (torch.minimum: a NaN stays)
__host__ __device__ inline double cclip_scale(double d2, double tau) {
    const double d = __builtin_sqrt(d2);
    const double q = tau / d;
    return q < 1.0 ? q : (q >= 1.0 ? 1.0 : q);
}

// One iteration's scalar code, the text's lines from d2_r[~alive] = inf to w.append(...):
//   s = cclip_scale(d2) (dead: 0); lam = a / _seqsum(a) (no entry alive: 0, not 0 / 0);
//   t = lam * s; om = 1 - _seqsum(t); u_next = u * om; w_next = w * om + t (a multiply, an add).
// d2 is rewritten in place: +inf for a dead entry.  a: geomed_alpha, so _seqsum(a) is 0 exactly
// when no entry is alive.  Worker `lane` of `nlanes` takes the entries lane, lane + nlanes, ...;
// sync() separates the phases (the host: one lane and a no-op; the kernel: its threads and
// __syncthreads); the sequential sums are worker 0's.  term: k words of the caller's;
// sums[CCLIP_SUM_U] = u_next.
template <class Sync>
__host__ __device__ inline void cclip_iterate(double* d2, const double* a, const int32_t* dead,
                                              int k, double tau, double u, const double* w,
                                              double* s, double* term, double* sums,
                                              double* w_next, int lane, int nlanes, Sync sync) {
#pragma clang fp contract(off)
    if (lane == 0) sums[CCLIP_SUM_ALPHA] = geomed_seqsum(a, k);
    sync();
    const double asum = sums[CCLIP_SUM_ALPHA];
    for (int j = lane; j < k; j += nlanes) {
        double sj = 0.0;
        if (dead[j]) d2[j] = (double)__builtin_inff();
        else sj = cclip_scale(d2[j], tau);
        const double lam = asum > 0.0 ? a[j] / asum : 0.0;
        s[j] = sj;
        term[j] = lam * sj;
    }
    sync();
    if (lane == 0) {
        const double om = 1.0 - geomed_seqsum(term, k);
        sums[CCLIP_SUM_OM] = om;
        sums[CCLIP_SUM_U] = u * om;
    }
    sync();
    const double om = sums[CCLIP_SUM_OM];
    for (int j = lane; j < k; j += nlanes) {
        const double t = w[j] * om;
        w_next[j] = t + term[j];
    }
}

}  // namespace flsim
