// Stand-alone host check of the forward convolutions' tap-class row map (csrc/rowmap.h), meant to be
// built with the host sanitizers and run on a CPU-only machine before the kernels that index by
// the map run at all: a wrong map becomes out-of-range stores that nothing bounds-checks.
//
//   c++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Ifl-distributed-delay_amd/csrc tools/fwd_classes_host_check.cpp \
//       -o /tmp/fwd_classes_host_check && /tmp/fwd_classes_host_check
//
// For PerformantNet1's conv2-6 (3x3, padding 2), both tile heights of each and S = 128, 256, 384
// it walks every block of the grid and every virtual row of its tile, pad rows included:
//   - every block finds a tile, no two blocks the same one, and every class is whole tiles;
//   - the valid rows map onto 0 .. M - 1 exactly once each, pad rows to ROW_PAD, and a tile's
//     valid rows are its first RowTile::valid rows;
//   - no tap outside the class's tap rectangle is valid for any row of the class (the loaders'
//     tapmask rule, restated here), and every tap of the rectangle is valid for some row of it;
//   - the k sequence of the class is the one the kernels are specified to run, step i = real
//     k-step 9 (i / nt) + 3 (kh0 + j / nw) + kw0 + j % nw, j = i % nt, and stays on its last
//     step when asked for more;
//   - every XCD (block % 8) holds floor or ceil of an eighth of every class, and classes with
//     more taps come first within an XCD;
//   - issued over canonical k-steps, summed over the valid rows, is the squared ratio expected
//     from the geometry, as exact integers.

#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "rowmap.h"

using namespace flsim;

static int fails = 0;
#define EXPECT(cond)                                              \
    do {                                                          \
        if (!(cond)) {                                            \
            if (fails < 20) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
            ++fails;                                              \
        }                                                         \
    } while (0)

struct Geo {
    const char* name;
    int IH, win, CI, bm_large, bm_small;
    int num, den;      // expected k-step ratio per dimension
    int ncls;
};

static void check(const Geo& g, int S, int bm) {
    const int pad = 2, IW = g.IH;
    RowClasses rm;
    EXPECT(row_classes_build(rm, g.IH, IW, pad, g.win, S, bm));
    EXPECT(rm.ncls == g.ncls);
    const int OH = g.IH + 2 * pad - 2;
    const int PH = OH / 2;
    const long M = (long)S * (g.win ? 4 * PH * PH : OH * OH);
    std::vector<unsigned char> seen(M, 0);
    std::vector<std::vector<unsigned char>> tile_seen(rm.ncls);
    std::vector<int> tapuse(rm.ncls, 0);
    int total = 0;
    for (int k = 0; k < rm.ncls; ++k) {
        const RowClass& rc = rm.c[k];
        EXPECT(rc.tiles * bm >= rc.rows && (rc.tiles - 1) * bm < rc.rows);
        EXPECT(rc.rows == S * rc.hh * rc.ww * (g.win ? 4 : 1));
        if (k > 0) EXPECT(rc.nh * rc.nw <= rm.c[k - 1].nh * rm.c[k - 1].nw);
        tile_seen[k].assign(rc.tiles, 0);
        total += rc.tiles;
        // the k sequence
        const int slices = g.CI / 16, nt = rc.nh * rc.nw;
        EXPECT(rm.ksteps(k, slices) == slices * nt);
        EXPECT(rm.ksteps(k, slices) % 3 == 0 || g.CI > 96);      // conv2-4: KB = 3 stages
        RowKSeq seq;
        seq.init(rc, slices);
        int last = -1;
        for (int i = 0; i < slices * nt; ++i) {
            const int j = i % nt;
            const int want = 9 * (i / nt) + 3 * (rc.kh0 + j / rc.nw) + rc.kw0 + j % rc.nw;
            last = seq.next();
            EXPECT(last == want);
            EXPECT(last < 9 * slices);
        }
        for (int i = 0; i < 4; ++i) EXPECT(seq.next() == last);
    }
    EXPECT(total == rm.tiles);
    // blocks -> tiles, XCD shares
    std::vector<std::vector<int>> share(rm.ncls, std::vector<int>(8, 0));
    std::vector<int> xcd_last_cls(8, -1);
    long issued = 0, pads = 0;
    for (int b = 0; b < rm.tiles; ++b) {
        const RowTile t = rm.locate(b);
        EXPECT(t.cls >= 0 && t.cls < rm.ncls);
        const RowClass& rc = rm.c[t.cls];
        EXPECT(t.v0 % bm == 0 && t.v0 / bm < rc.tiles);
        EXPECT(t.valid > 0 && t.valid <= bm);
        if (t.v0 / bm >= rc.tiles) continue;
        EXPECT(!tile_seen[t.cls][t.v0 / bm]);
        tile_seen[t.cls][t.v0 / bm] = 1;
        ++share[t.cls][b & 7];
        EXPECT(t.cls >= xcd_last_cls[b & 7]);      // classes in table order within an XCD
        xcd_last_cls[b & 7] = t.cls;
        for (int r = 0; r < bm; ++r) {
            const int m = rm.row(t.cls, t.v0 + r);
            if (r >= t.valid) {
                EXPECT(m == ROW_PAD);
                ++pads;
                continue;
            }
            EXPECT(m >= 0 && m < M);
            if (m < 0 || m >= M) continue;
            EXPECT(!seen[m]);
            seen[m] = 1;
            issued += rc.nh * rc.nw;
            // canonical row -> (oh, ow), the loaders' rule
            int oh, ow;
            if (g.win) {
                const int rem = m % (4 * PH * PH), qq = rem >> 2, ph = qq / PH;
                oh = 2 * ph + ((rem >> 1) & 1);
                ow = 2 * (qq - ph * PH) + (rem & 1);
                // a window's four rows stay together, in order
                EXPECT((r & 3) == (m & 3));
                if (r & 3) EXPECT(m == rm.row(t.cls, t.v0 + r - 1) + 1);
            } else {
                const int rem = m % (OH * OH);
                oh = rem / OH;
                ow = rem - oh * OH;
            }
            for (int tp = 0; tp < 9; ++tp) {
                const int kh = tp / 3, kw = tp % 3;
                const int ih = oh + kh - pad, iw = ow + kw - pad;
                const bool valid = ih >= 0 && ih < g.IH && iw >= 0 && iw < IW;
                const bool in_rect = kh >= rc.kh0 && kh < rc.kh0 + rc.nh && kw >= rc.kw0 &&
                                     kw < rc.kw0 + rc.nw;
                if (valid) EXPECT(in_rect);
                if (valid) tapuse[t.cls] |= 1 << tp;
            }
        }
    }
    EXPECT(rm.locate(rm.tiles).valid == 0);
    for (long m = 0; m < M; ++m) EXPECT(seen[m]);
    for (int k = 0; k < rm.ncls; ++k) {
        const RowClass& rc = rm.c[k];
        for (int t = 0; t < rc.tiles; ++t) EXPECT(tile_seen[k][t]);
        for (int x = 0; x < 8; ++x)
            EXPECT(share[k][x] == rc.tiles / 8 || share[k][x] == rc.tiles / 8 + 1);
        int n = 0;
        for (int tp = 0; tp < 9; ++tp) n += (tapuse[k] >> tp) & 1;
        EXPECT(n == rc.nh * rc.nw);                // the rectangle is tight
    }
    for (int x = 0; x < 8; ++x) {
        int n = 0;
        for (int k = 0; k < rm.ncls; ++k) n += share[k][x];
        EXPECT(n == rm.tiles / 8 + (x < rm.tiles % 8 ? 1 : 0));
    }
    // issued / canonical == (num / den)^2, exactly
    EXPECT(issued * g.den * g.den == M * 9 * g.num * g.num);
    printf("%-6s S %3d BM %3d: %2d classes, M %8ld rows in %5d tiles (canonical %5ld), "
           "%6ld pad rows, k-steps %ld / %ld = (%d/%d)^2, with pad tiles %.4f\n",
           g.name, S, bm, rm.ncls, M, rm.tiles, (M + bm - 1) / bm, pads, issued, M * 9, g.num,
           g.den, [&] {
               double s = 0;
               for (int k = 0; k < rm.ncls; ++k)
                   s += (double)rm.c[k].tiles * rm.c[k].nh * rm.c[k].nw;
               return s / (9.0 * ((M + bm - 1) / bm));
           }());
}

int main() {
    const Geo geos[5] = {
        {"conv2", 34, 1, 48, 256, 128, 52, 54, 9},
        {"conv3", 18, 0, 48, 512, 128, 54, 60, 25},
        {"conv4", 20, 1, 96, 512, 128, 31, 33, 9},
        {"conv5", 11, 0, 96, 256, 128, 33, 39, 25},
        {"conv6", 13, 1, 192, 256, 128, 20, 21, 4},
    };
    const int Ss[3] = {128, 256, 384};
    for (const Geo& g : geos)
        for (int S : Ss) {
            check(g, S, g.bm_large);
            check(g, S, g.bm_small);
        }
    if (fails) {
        printf("%d FAILED\n", fails);
        return 1;
    }
    printf("fwd_classes_host_check: all passed\n");
    return 0;
}
