// What the stand-alone host check programs (tools/*_host_check.cpp) share: the library's error
// slot, bit views and the two meanings of "equal", EXPECT and its failure count, a seeded normal
// generator, and the test of a refusal.  Each program includes it once; -I../tools on its build line.
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "flsim.h"

// the library's error slot lives with the network engines (csrc/pn1_net.hip), which these programs
// do not link: the same few lines
namespace flsim {
static thread_local char g_err[512];
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char* last_error() { return g_err; }
}  // namespace flsim
extern "C" const char* flsim_last_error(void) { return flsim::last_error(); }

static inline uint32_t bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}
static inline uint64_t bits(double x) {
    uint64_t u;
    memcpy(&u, &x, 8);
    return u;
}
// equal bit for bit, or both NaN
static inline bool same_bits(double a, double b) { return (a != a && b != b) || bits(a) == bits(b); }
static inline bool same_bits(float a, float b) { return (a != a && b != b) || bits(a) == bits(b); }
// equal as numbers: both NaN, both zero (+0 and -0 are one number), or the same bits
static inline bool same_number(float a, float b) {
    return (a != a && b != b) || (a == 0.f && b == 0.f) || bits(a) == bits(b);
}

static int fails = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAIL %s:%d %s [%s]\n", __FILE__, __LINE__, #cond, flsim_last_error()); \
            ++fails;                                                       \
        }                                                                  \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static inline double uniform() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng_state >> 11) / (double)(1ull << 53);
}
static inline float normal() {
    const double u = uniform() + 1e-300, v = uniform();
    return (float)(sqrt(-2.0 * log(u)) * cos(6.283185307179586 * v));
}

static inline bool refused(int rc, const char* what) {
    return rc == 1 && strstr(flsim_last_error(), what) != nullptr;
}
