// Bulyan (include/flsim.h: flsim_bulyan; El Mhamdi, Guerraoui and Rouault 2018) over Krum's
// distance matrix: the repeated selection as ONE host + device function, so the finish kernel
// (server.hip: k_bulyan_finish) and the host twin (flsim_bulyan_eval_host) run the same code, and
// the coordinate-wise window around the median over the selected entries as ONE host + device
// template, shared by the apply kernel (k_bulyan_apply) and the twin.
#pragma once
#include <stdint.h>

#include "common.h"
#include "flsim.h"
#include "robust.h"

namespace flsim {

// The rule text's selection from the k x k distance matrix `dist` (symmetric, zero diagonal, no
// NaN): theta = k - 2f rounds; in a round with r entries left the score of a remaining i is the
// sum of its n = max(r - f - 2, 1) smallest distances to the other remaining entries, added in
// ascending (value, index) order; the lowest (score, index) wins and leaves.  r == 1: the one
// left wins with score 0.
//   order[0 .. theta) = the winners in round order, win[0 .. theta) = their scores,
//   sel[0 .. theta)   = the winners in ascending index order.
// The neighbour order of a row does not change as entries leave, so every row is ranked once
// (nbr[i * k + p] = the p-th nearest j != i by (value, index)) and a round walks the row's order,
// skips the entries that have left and adds the first n it meets: about theta * k steps a row
// where a scan per neighbour would take theta * n * k.  The entries that have left are a 64-bit
// mask every worker keeps for itself.  (With one entry left the walk meets nobody: score 0.)
// Worker `lane` of `nlanes` takes the rows lane, lane + nlanes, ...; sync() separates the phases
// (the host: one lane and a no-op; the kernel: its threads and __syncthreads).  No array is
// indexed at run time but the caller's: nbr [k * k] bytes, score [k] (work), win, order, sel.
template <class Sync>
__host__ __device__ inline void bulyan_order(const double* dist, uint8_t* nbr, double* score,
                                             double* win, int32_t* order, int32_t* sel, int k,
                                             int f, int lane, int nlanes, Sync sync) {
    const int theta = k - 2 * f;
    for (int idx = lane; idx < k * k; idx += nlanes) {
        const int i = idx / k, j = idx - i * k;
        if (j == i) continue;
        const double* row = dist + (long)i * k;
        const double v = row[j];
        int below = 0;
        for (int l = 0; l < k; ++l)
            below += (l != i && (row[l] < v || (row[l] == v && l < j))) ? 1 : 0;
        nbr[(long)i * k + below] = (uint8_t)j;
    }
    sync();
    uint64_t gone = 0;
    for (int round = 0; round < theta; ++round) {
        const int r = k - round;
        const int n = r - f - 2 > 1 ? r - f - 2 : 1;
        for (int i = lane; i < k; i += nlanes) {
            if ((gone >> i) & 1) continue;
            const double* row = dist + (long)i * k;
            const uint8_t* nb = nbr + (long)i * k;
            double acc = 0.0;
            int cnt = 0;
            for (int p = 0; p < k - 1 && cnt < n; ++p) {
                const int j = nb[p];
                if ((gone >> j) & 1) continue;
                acc = cnt == 0 ? row[j] : acc + row[j];
                ++cnt;
            }
            score[i] = acc;
        }
        sync();
        for (int i = lane; i < k; i += nlanes) {
            if ((gone >> i) & 1) continue;
            const double s = score[i];
            int below = 0;
            for (int l = 0; l < k; ++l)
                below += (!((gone >> l) & 1) && (score[l] < s || (score[l] == s && l < i))) ? 1 : 0;
            if (below == 0) {
                order[round] = i;
                win[round] = s;
            }
        }
        sync();
        gone |= (uint64_t)1 << (order[round] & 63);
    }
    for (int i = lane; i < k; i += nlanes) {
        if (!((gone >> i) & 1)) continue;
        int pos = 0;
        for (int l = 0; l < i; ++l) pos += (int)((gone >> l) & 1);
        sel[pos] = i;
    }
}

// t[i] = t[i + S] where the launch-uniform `shift` has bit S, the slots shifted in are ROBUST_PAD;
// stage after stage this is t[i] = a[i + shift] with every index a compile-time constant
template <int KPAD, int S = 1>
__host__ __device__ __forceinline__ void bulyan_shift(uint32_t (&t)[KPAD], int shift) {
    const bool on = (shift & S) != 0;
#pragma unroll
    for (int i = 0; i < KPAD; ++i) {
        const uint32_t up = i + S < KPAD ? t[i + S < KPAD ? i + S : i] : ROBUST_PAD;
        t[i] = on ? up : t[i];
    }
    if constexpr (S < KPAD) bulyan_shift<KPAD, 2 * S>(t, shift);
}

// The rule text's coordinate from the keys of an element's theta selected values (slots past theta:
// ROBUST_PAD): sort, med = s[(theta - 1) / 2], the window of beta values the text grows around the
// median, and their sum added in ascending order starting from the window's first value -- the
// caller divides it by (float)beta, one IEEE division.
// The text grows the window beta - 1 times by the closer outer neighbour (right iff strictly
// closer in fp32; a false compare goes left).  That is a merge of the left neighbours (distance
// med - s, not decreasing away from the median) with the right ones (s - med, likewise): a window
// of beta slots cannot hold both slot p and slot p + beta, and of such a pair around the median
// the merge reaches the right one first iff (s[p + beta] - med) < (med - s[p]).  So slot p < mid
// is inside iff p > mid - beta and (slot p + beta does not exist or that compare is false): one
// compare a slot against the slots shifted by beta.  Wherever a NaN comes up (a NaN value, inf -
// inf) the compare is false, as in the text, and the values a side's differences are NaN for are
// the ones furthest from the median on that side, so the merge order stays the text's.
template <int KPAD>
__host__ __device__ __forceinline__ float bulyan_window_sum(uint32_t (&a)[KPAD], int theta,
                                                            int beta) {
    robust_sort<KPAD>(a);
    const int mid = (theta - 1) / 2;
    uint32_t t[KPAD];
    float s[KPAD];
#pragma unroll
    for (int j = 0; j < KPAD; ++j) {
        t[j] = a[j];
        s[j] = robust_unkey(a[j]);
    }
    bulyan_shift<KPAD>(t, beta);
    float med = 0.f;
#pragma unroll
    for (int j = 0; j < KPAD; ++j) med = j == mid ? s[j] : med;
    int lo = mid;                       // the window's first slot: mid - (the left slots inside)
#pragma unroll
    for (int j = 0; j < KPAD; ++j) {
        const bool right_first = (robust_unkey(t[j]) - med) < (med - s[j]);
        const bool in = j < mid && j > mid - beta && (j + beta >= theta || !right_first);
        lo -= in ? 1 : 0;
    }
    const int hi = lo + beta;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < KPAD; ++j) acc = j == lo ? s[j] : ((j > lo && j < hi) ? acc + s[j] : acc);
    return acc;
}

}  // namespace flsim
