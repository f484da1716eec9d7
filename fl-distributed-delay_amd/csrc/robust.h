// Robust rules (include/flsim.h: flsim_robust): the coordinate-wise median and the trimmed mean
// over k <= 64 values per element, as ONE host + device template, so the kernel (server.hip:
// k_robust) and the host twin (flsim_robust_eval_host) run the same code.
//
// The k values of an element live in registers: a fully unrolled bitonic sorting network over
// KPAD = 2 .. 64 slots whose indices are all compile-time (template recursion, no loop: a
// runtime-indexed register array would go to scratch).  The network sorts integer keys:
//   NaN is canonicalised to 0x7FC00000; the bits map to a monotonic uint32 (all bits of a negative
//   value flipped, only the sign bit of a non-negative one), so -inf < finite < +inf < NaN as
//   torch.sort orders them and a comparator is one integer min / max pair; the slots past k hold
//   0xFFFFFFFF, above every key, and are never selected.
// The runtime k, kind and trim are launch-uniform: select / sum is a predicated, fully unrolled
// walk over the sorted slots (sequential fp32 adds in ascending order, as the rule text adds).
#pragma once
#include <stdint.h>

#include <utility>

#include "common.h"
#include "flsim.h"

namespace flsim {

constexpr uint32_t ROBUST_PAD = 0xFFFFFFFFu;

// the padded size of the network for k entries
inline int robust_kpad(int k) {
    int kp = 2;
    while (kp < k) kp <<= 1;
    return kp;
}

__host__ __device__ __forceinline__ uint32_t robust_key(float x) {
    uint32_t b = __builtin_bit_cast(uint32_t, x);
    b = (b & 0x7FFFFFFFu) > 0x7F800000u ? 0x7FC00000u : b;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__host__ __device__ __forceinline__ float robust_unkey(uint32_t key) {
    const uint32_t b = (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key;
    return __builtin_bit_cast(float, b);
}

// one comparator: slots I < L end up ascending (UP) or descending
template <int KPAD, int I, int L, bool UP>
__host__ __device__ __forceinline__ void robust_cs(uint32_t (&a)[KPAD]) {
    if constexpr (L > I) {
        const uint32_t x = a[I], y = a[L];
        const uint32_t lo = x < y ? x : y, hi = x < y ? y : x;
        a[I] = UP ? lo : hi;
        a[L] = UP ? hi : lo;
    }
}

// one layer of the bitonic network: partner distance J inside blocks of K
template <int KPAD, int K, int J, int... I>
__host__ __device__ __forceinline__ void robust_layer(uint32_t (&a)[KPAD],
                                                      std::integer_sequence<int, I...>) {
    (robust_cs<KPAD, I, (I ^ J), (I & K) == 0>(a), ...);
}

template <int KPAD, int K, int J>
__host__ __device__ __forceinline__ void robust_merge(uint32_t (&a)[KPAD]) {
    robust_layer<KPAD, K, J>(a, std::make_integer_sequence<int, KPAD>{});
    if constexpr (J > 1) robust_merge<KPAD, K, J / 2>(a);
}

// ascending sort of the KPAD slots
template <int KPAD, int K = 2>
__host__ __device__ __forceinline__ void robust_sort(uint32_t (&a)[KPAD]) {
    robust_merge<KPAD, K, K / 2>(a);
    if constexpr (K < KPAD) robust_sort<KPAD, 2 * K>(a);
}

// The rule text from the keys of an element's k values (slots past k: ROBUST_PAD): sort, then the
// lower median s[(k - 1) / 2], or the sum of s[trim .. k - trim) added in ascending order starting
// from s[trim] -- the caller divides that by (float)(k - 2 * trim), one IEEE division.
template <int KPAD>
__host__ __device__ __forceinline__ float robust_select(uint32_t (&a)[KPAD], int kind, int trim,
                                                        int k) {
    robust_sort<KPAD>(a);
    float acc = 0.f;
    if (kind == FLSIM_ROBUST_MEDIAN) {
        const int mid = (k - 1) / 2;
#pragma unroll
        for (int j = 0; j < KPAD; ++j) acc = j == mid ? robust_unkey(a[j]) : acc;
    } else {
        const int hi = k - trim;
#pragma unroll
        for (int j = 0; j < KPAD; ++j) {
            const float s = robust_unkey(a[j]);
            acc = j == trim ? s : ((j > trim && j < hi) ? acc + s : acc);
        }
    }
    return acc;
}

}  // namespace flsim
