// Row maps of the implicit-GEMM convolutions: which output pixel a tile row stands for.
//
// Canonical order is what the loaders and epilogues index by: m = (img, oh, ow), or in pool-window
// order m = ((img * PH + ph) * PW + pw) * 4 + 2 dy + dx.  RowIdentity is that order.  RowClasses
// re-orders the rows of a padded 3x3 convolution by TAP CLASS: every spatial dimension is cut into
// segments of outputs (or pool windows) that see the same contiguous range of filter taps inside
// the input, a class is a pair of segments (a rectangle of pixels / windows per image with a tap
// rectangle), and the virtual row order is class, image, row-major inside the rectangle, then the
// four window positions.  Every class is padded to whole block tiles, so all rows of a block share
// one tap rectangle and the block can leave out the k-steps of the other taps (exact zeros) as a
// block: (CI / 16) * nh * nw k-steps instead of (CI / 16) * 9.
//
// Tiles are dealt to the eight XCDs class by class (blockIdx % 8 is the XCD, as the GEMM kernels
// assume): every XCD takes a contiguous eighth of every class, the remainders rotating on so that
// the XCD totals differ by at most one tile, and within an XCD the classes run in the order of
// the table, most taps first.
//
// Host and device code; the table builder and the maps use nothing of HIP
// (tools/fwd_classes_host_check.cpp walks them on the CPU).
#pragma once
#include <climits>

#if defined(__HIPCC__)
#define FLSIM_RM_HD __host__ __device__
#else
#define FLSIM_RM_HD
#endif

namespace flsim {

constexpr int ROW_PAD = INT_MAX;       // canonical row of a pad row: past every M

// the block's share of the map: where its tile lies and which k-steps it runs
struct RowTile {
    int cls;          // class index (RowClasses::c)
    int v0;           // first virtual row of the tile inside its class
    int valid;        // valid rows of the tile: the first `valid` rows, the others are pad
};

// canonical order: tile t holds rows [t * BM, t * BM + BM)
struct RowIdentity {
    static constexpr bool CLASSES = false;
};

struct RowClass {
    int tiles;                  // block tiles of the class (rows padded up)
    int rows;                   // valid rows: S * hh * ww (* 4 in window order)
    short h0, w0, hh, ww;       // the rectangle, in pixels or windows
    short kh0, nh, kw0, nw;     // the tap rectangle
    unsigned long long taps;    // the nh * nw taps 3 kh + kw in ascending order, 4 bits each
};

struct RowClasses {
    static constexpr bool CLASSES = true;
    static constexpr int MAXC = 25;
    int ncls;
    int bm;            // rows per block tile
    int win;           // rows in pool-window order
    int gh, gw;        // per image: output pixels OH x OW, or windows PH x PW
    int tiles;         // sum of the classes' tiles = the grid
    RowClass c[MAXC];

    // k-steps a block of class k runs for `slices` 16-channel slices
    FLSIM_RM_HD int ksteps(int k, int slices) const { return slices * c[k].nh * c[k].nw; }

    // block b of the grid -> its tile
    FLSIM_RM_HD RowTile locate(int b) const {
        const int x = b & 7;
        int i = b >> 3, off = 0;
        RowTile t{0, 0, 0};
        for (int k = 0; k < ncls; ++k) {
            const int T = c[k].tiles, q = T >> 3, r = T & 7;
            const int j = (x - off) & 7;
            const int n = q + (j < r ? 1 : 0);
            if (i < n) {
                t.cls = k;
                t.v0 = (j * q + (j < r ? j : r) + i) * bm;
                const int left = c[k].rows - t.v0;
                t.valid = left < bm ? left : bm;
                return t;
            }
            i -= n;
            off = (off + r) & 7;
        }
        return t;       // b >= tiles: an empty tile
    }

    // virtual row v of class k -> canonical row, ROW_PAD for a pad row
    FLSIM_RM_HD int row(int k, int v) const {
        const RowClass& rc = c[k];
        if (v >= rc.rows) return ROW_PAD;
        const unsigned u = win ? (unsigned)v >> 2 : (unsigned)v;
        const unsigned hw = (unsigned)(rc.hh * rc.ww);
        const unsigned img = u / hw;
        const unsigned rem = u - img * hw;
        const unsigned rh = rem / (unsigned)rc.ww;
        const unsigned rw = rem - rh * (unsigned)rc.ww;
        const unsigned p = (img * gh + rc.h0 + rh) * gw + rc.w0 + rw;
        return (int)(win ? p * 4 + ((unsigned)v & 3) : p);
    }
};

// The block-uniform k sequence of a class: step i is real k-step
// 9 * (i / nt) + tap(i % nt), carried incrementally (scalar adds and selects, no division).
// next() returns the current k-step and moves on; after the last step it stays there, so the
// pipelines' loads past the end of K re-read the last k-step.
struct RowKSeq {
    unsigned long long taps;
    int nt, j, base, left;
    FLSIM_RM_HD void init(const RowClass& rc, int slices) {
        taps = rc.taps;
        nt = rc.nh * rc.nw;
        j = 0;
        base = 0;
        left = slices * nt;
    }
    FLSIM_RM_HD int next() {
        const int ks = base + (int)((taps >> (4 * j)) & 15);
        if (left > 1) {
            --left;
            ++j;
            if (j == nt) {
                j = 0;
                base += 9;
            }
        }
        return ks;
    }
};

// valid taps of output coordinate o along one dimension, as a bit mask (bit t: input o + t - pad
// is inside [0, in)): the loaders' tapmask rule
inline int row_taps_1d(int o, int in, int pad) {
    int m = 0;
    for (int t = 0; t < 3; ++t)
        if (o + t - pad >= 0 && o + t - pad < in) m |= 1 << t;
    return m;
}

struct RowSeg {
    int o0, n, t0, nt;     // units [o0, o0 + n), taps [t0, t0 + nt)
};

// segments of one dimension: `units` outputs (win = 0) or pool windows of two outputs (win = 1)
// over `in` inputs; consecutive units with the same tap range (the union over a window's two
// outputs) share a segment.  At most 5.  Returns the count.
inline int row_segments(int units, int in, int pad, int win, RowSeg (&seg)[8]) {
    int ns = 0;
    for (int u = 0; u < units; ++u) {
        const int m = win ? row_taps_1d(2 * u, in, pad) | row_taps_1d(2 * u + 1, in, pad)
                          : row_taps_1d(u, in, pad);
        int t0 = 0, nt = 0;
        while (t0 < 3 && !((m >> t0) & 1)) ++t0;
        while (t0 + nt < 3 && ((m >> (t0 + nt)) & 1)) ++nt;
        if (nt == 0) { t0 = 0; }                        // an output that sees no input at all
        if (ns > 0 && seg[ns - 1].t0 == t0 && seg[ns - 1].nt == nt) {
            ++seg[ns - 1].n;
        } else {
            if (ns == 8) return -1;
            seg[ns++] = RowSeg{u, 1, t0, nt};
        }
    }
    return ns;
}

// The table of a 3x3 convolution over IH x IW inputs with padding `pad` and S images:
// win = 0: OH x OW = (IH + 2 pad - 2) x (IW + 2 pad - 2) output pixels per image;
// win = 1: (OH / 2) x (OW / 2) pool windows (the floor-mode border is not computed).
// Classes with the most taps come first.  Returns false if the geometry does not fit the table.
inline bool row_classes_build(RowClasses& rm, int IH, int IW, int pad, int win, int S, int bm) {
    const int OH = IH + 2 * pad - 2, OW = IW + 2 * pad - 2;
    rm.win = win;
    rm.bm = bm;
    rm.gh = win ? OH / 2 : OH;
    rm.gw = win ? OW / 2 : OW;
    RowSeg sh[8], sw[8];
    const int nsh = row_segments(rm.gh, IH, pad, win, sh);
    const int nsw = row_segments(rm.gw, IW, pad, win, sw);
    if (nsh < 0 || nsw < 0 || nsh * nsw > RowClasses::MAXC) return false;
    rm.ncls = 0;
    rm.tiles = 0;
    for (int want = 9; want >= 0; --want)               // most taps first, then row-major
        for (int a = 0; a < nsh; ++a)
            for (int b = 0; b < nsw; ++b) {
                if (sh[a].nt * sw[b].nt != want) continue;
                RowClass rc{};
                rc.h0 = (short)sh[a].o0;
                rc.hh = (short)sh[a].n;
                rc.w0 = (short)sw[b].o0;
                rc.ww = (short)sw[b].n;
                rc.kh0 = (short)sh[a].t0;
                rc.nh = (short)sh[a].nt;
                rc.kw0 = (short)sw[b].t0;
                rc.nw = (short)sw[b].nt;
                rc.rows = S * rc.hh * rc.ww * (win ? 4 : 1);
                rc.tiles = (rc.rows + bm - 1) / bm;
                rc.taps = 0;
                int n = 0;
                for (int kh = rc.kh0; kh < rc.kh0 + rc.nh; ++kh)
                    for (int kw = rc.kw0; kw < rc.kw0 + rc.nw; ++kw)
                        rc.taps |= (unsigned long long)(3 * kh + kw) << (4 * n++);
                rm.tiles += rc.tiles;
                rm.c[rm.ncls++] = rc;
            }
    return true;
}

// executed k-depth summed over the valid rows: sum over classes of rows * taps (* CI * N * 2 are
// the launch's FLOPs)
inline double row_classes_row_taps(const RowClasses& rm) {
    double s = 0;
    for (int k = 0; k < rm.ncls; ++k) s += (double)rm.c[k].rows * rm.c[k].nh * rm.c[k].nw;
    return s;
}

}  // namespace flsim
