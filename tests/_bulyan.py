"""Helpers of the Bulyan tests (tests/test_cpu_bulyan.py, tests/test_gpu_bulyan.py): the case grid,
the rule text (flsim/robust.py: bulyan_order, _bulyan_coord, bulyan_flat) as the reference, the host
twin, and the input condition.  The inputs, the distance bound and the comparisons are those of
tests/_krum.py.

Everything after the distances is compared stage by stage at the implementation's own outputs and
has no tolerance: order, the winning scores (bit for bit) and sel against bulyan_order run on the
implementation's own dist, g against _bulyan_coord over its own sel.  End to end (against the text
computed from scratch) the inputs keep, in every round of the text, the winner's score either
bit-equal to a rival's (an exact tie: both sides break it by the lower index) or at least 1000
score bounds below it, so no round can depend on the rounding of the distances; a score is a sum
of non-negative distances, each within dist_bound(P), and its bound is twice that, as Krum's.
"""
import ctypes

import numpy as np
import torch

import _krum as K

KS = (3, 4, 7, 8, 9, 16, 17, 32, 33, 64)
QNAN = K.QNAN


def fs(k):
    """f in {0, 1, (k - 3) // 4} with k >= 4f + 3."""
    return sorted(f for f in {0, 1, (k - 3) // 4} if f >= 0 and k >= 4 * f + 3)


GRID = [(k, f) for k in KS for f in fs(k)]


def text(entries, counts, f):
    """The rule text over bucket sums and counts -> (g, dist, order, win, sel) as numpy / lists."""
    from flsim.robust import bulyan_flat
    ent = [None if e is None else torch.from_numpy(np.ascontiguousarray(e)) for e in entries]
    g, d, order, win, sel = bulyan_flat(ent, counts, f)
    return (g.numpy().copy(), d.numpy().copy(), [int(j) for j in order], win.numpy().copy(),
            [int(j) for j in sel])


def order_of(dist, f):
    """bulyan_order on a given [k, k] fp64 matrix -> (order, win, sel)."""
    from flsim.robust import bulyan_order
    order, win = bulyan_order(torch.from_numpy(np.ascontiguousarray(dist, np.float64)), f)
    return [int(j) for j in order], win.numpy().copy(), sorted(int(j) for j in order)


def coord(entries, counts, sel, f):
    """_bulyan_coord over the means of the entries `sel` -> g."""
    from flsim.robust import _bulyan_coord
    P = next(len(e) for e in entries if e is not None)
    cols = torch.stack([torch.zeros(P) if entries[j] is None else
                        torch.from_numpy(np.ascontiguousarray(entries[j], np.float32)) / counts[j]
                        for j in sel])
    return _bulyan_coord(cols, f).numpy().copy()


def min_round_gap(dist, f):
    """Over the rounds of the text on `dist`: the smallest relative gap between the winner's score
    and a rival's that is not bit-equal to it (inf: no such rival anywhere)."""
    d = np.asarray(dist, np.float64)
    k = d.shape[0]
    left = list(range(k))
    gap = float("inf")
    for _ in range(k - 2 * f):
        r = len(left)
        if r == 1:
            break
        n = max(r - f - 2, 1)
        sc = {}
        for i in left:
            row = sorted((d[i, j], j) for j in left if j != i)[:n]
            acc = np.float64(row[0][0])
            for v, _ in row[1:]:
                acc = acc + np.float64(v)
            sc[i] = acc
        w = min(left, key=lambda i: (sc[i], i))
        for i in left:
            if i != w and sc[i] != sc[w] and np.isfinite(sc[w]):
                gap = min(gap, float((sc[i] - sc[w]) / sc[w]) if sc[w] > 0 else float("inf"))
        left.remove(w)
    return gap


def gap_bar(P):
    """1000 score bounds: a score is within 2 * dist_bound(P) of the text's, relatively."""
    return 1000 * 2 * K.dist_bound(P)


def c_bulyan(entries, counts, f, ptrs=None):
    """flsim_bulyan over host arrays (or the raw addresses `ptrs`).  Returns (struct, keep-alive)."""
    from flsim._lib import FlsimBulyan
    r = FlsimBulyan()
    r.f, r.k = int(f), len(counts)
    keep = []
    for j, c in enumerate(counts[:64]):
        r.count[j] = int(c)
        if ptrs is not None:
            r.entries[j] = ptrs[j]
        elif entries[j] is not None:
            a = np.ascontiguousarray(entries[j], np.float32)
            keep.append(a)
            r.entries[j] = a.ctypes.data
    return r, keep


def host_twin(entries, counts, f, r=None):
    """flsim_bulyan_eval_host on exactly sized host arrays -> (g, dist, order, win, sel)."""
    from flsim._lib import check, lib
    keep = None
    if r is None:
        r, keep = c_bulyan(entries, counts, f)
    k = len(counts)
    th = k - 2 * f
    P = next(len(e) for e in entries if e is not None)
    g = np.empty(P, np.float32)
    g.view(np.uint32)[:] = QNAN
    d = np.full((k, k), np.nan)
    win = np.full(th, np.nan)
    order = np.full(th, -1, np.int32)
    sel = np.full(th, -1, np.int32)
    vp = ctypes.c_void_p
    check(lib().flsim_bulyan_eval_host(ctypes.byref(r), P, d.ctypes.data_as(vp),
                                       win.ctypes.data_as(vp), order.ctypes.data_as(vp),
                                       sel.ctypes.data_as(vp), g.ctypes.data_as(vp)))
    del keep
    return g, d, [int(j) for j in order], win, [int(j) for j in sel]


def g_differs(got, ref):
    """Words where g differs from the text's as numbers: the same bits, a NaN where it has a NaN, a
    zero (of either sign) where it has a zero."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    same = np.where(np.isnan(ref), np.isnan(got),
                    np.where(ref == 0, got == 0, K.bits(got) == K.bits(ref)))
    return int((~same).sum())


def stage_check(got, entries, counts, f, P, what):
    """The stages of one result (g, dist, order, win, sel) at its own outputs: order, win (bit for
    bit) and sel against bulyan_order on its own dist; g against _bulyan_coord on its own sel, as
    _krum.g_mismatches compares."""
    g, d, order, win, sel = got
    k = len(counts)
    assert np.array_equal(d.view(np.uint64), d.T.copy().view(np.uint64)), what
    assert (np.diag(d) == 0).all() and not np.isnan(d).any(), what
    o_t, w_t, s_t = order_of(d, f)
    assert order == o_t and sel == s_t and len(sel) == k - 2 * f, (what, order, o_t)
    assert np.array_equal(np.asarray(win).view(np.uint64), w_t.view(np.uint64)), what
    bad = K.g_mismatches(g, coord(entries, counts, sel, f))
    assert bad == 0, (what, bad)
