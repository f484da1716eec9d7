"""Helpers of the nearest-neighbour-mixing tests (tests/test_cpu_nnm.py, tests/test_gpu_nnm.py):
seeded bucket sums with their counts, the text (flsim/robust.py: nnm_flat) as the reference, the
host twin, and the comparison against the text:

  dist   within 2 (P + 2) 2^-53 relative (fp64 sums of P non-negative terms in any order, each term
         one rounding of the difference's square; Krum's bound, the launch is Krum's);
  nbr    equal -- after ASSERTING that the text's own cut, the gap between the (k - f)-th and the
         (k - f + 1)-th smallest distance of every row, is more than 1000 times that bound wide (or
         an exact tie, which both sides break by the lower index): a property of the inputs, so the
         comparison never depends on a rounding and no case is ever skipped;
  mixed  equal as numbers (tests/_attack.py: mismatches): every operation is one IEEE fp32 operation
         on both sides, in the same order.
"""
import ctypes

import numpy as np
import torch

from _attack import bits, mismatches, poisoned  # noqa: F401  (re-exported)
from _poison import QNAN  # noqa: F401

KS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)       # both sides of every KPAD
GAP_FACTOR = 1000.0


def kpad(k):
    kp = 4
    while kp < k:
        kp *= 2
    return kp


def krum_tile(k):
    """The distance launch's tile (csrc/krum.h: KRUM_TILE_FLOATS / KPAD)."""
    return 8192 // kpad(k)


def ps_for_tile(E):
    return (1, 3, 255, 257, E - 1, E, E + 1, 3 * E + 5)


def fs(k, zero=True):
    """f in {0, 1, (k - 1) // 2}, deduplicated and valid (2 f < k)."""
    out = []
    for f in ((0,) if zero else ()) + (1, (k - 1) // 2):
        if 0 <= 2 * f < k and f not in out:
            out.append(f)
    return out


def inputs(k, P):
    """Entry j is standard_normal(P) * (1 + 0.25 j) with count 1 + j % 5; the bucket SUMS are
    fp32(x * count), so the division back to the mean is exercised."""
    rs = np.random.RandomState((9000 + 131 * k + 7 * P) % (2 ** 31))
    counts = [1 + j % 5 for j in range(k)]
    ents = [np.ascontiguousarray((rs.standard_normal(P) * (1 + 0.25 * j) * counts[j])
                                 .astype(np.float32)) for j in range(k)]
    return ents, counts


def dist_bound(P):
    return 2.0 * (P + 2) * 2.0 ** -53


def masks(nbr):
    """k ascending lists of neighbours -> [k] uint64 (bit j of word i)."""
    return np.array([sum(1 << j for j in row) for row in nbr], np.uint64)


def text(ents, counts, f):
    """nnm_flat over host arrays -> (mixed [k, P] fp32, dist [k, k] fp64, nbr masks [k] uint64)."""
    from flsim.robust import nnm_flat
    mixed, d, nbr = nnm_flat([torch.from_numpy(np.ascontiguousarray(e, np.float32).copy())
                              for e in ents], counts, f)
    return mixed.numpy().copy(), d.numpy().copy(), masks(nbr)


def cut_gap(d, f):
    """The smallest relative gap (d_next - d_cut) / d_next between the (k - f)-th and the
    (k - f + 1)-th smallest (value, index) over the rows of the text's d; exact ties (equal
    values, +inf twice included) are decided by the index on both sides and count as no cut.
    inf without any cut (f = 0, or ties alone)."""
    k = d.shape[0]
    gap = np.inf
    if f == 0:
        return gap
    for i in range(k):
        order = sorted(range(k), key=lambda j: (d[i, j], j))
        a, b = d[i, order[k - f - 1]], d[i, order[k - f]]
        if a == b:
            continue
        gap = min(gap, 1.0 if np.isinf(b) else (b - a) / b)
    return gap


def c_nnm(ents, counts, f, ptrs=None, k=None):
    """flsim_nnm over host arrays (or the raw addresses `ptrs`) -> (struct, keep-alive)."""
    from flsim._lib import FlsimNnm
    a = FlsimNnm()
    a.f = int(f)
    a.k = len(counts) if k is None else k
    keep = []
    for j in range(min(len(counts), 64)):
        a.count[j] = int(counts[j])
        if ptrs is not None:
            a.entries[j] = ptrs[j]
        else:
            assert ents[j].dtype == np.float32 and ents[j].flags.c_contiguous
            keep.append(ents[j])
            a.entries[j] = ents[j].ctypes.data
    return a, keep


def host_twin(ents, counts, f, out=True):
    """flsim_nnm_eval_host -> (mixed [k, P] or None, dist [k, k], nbr [k] uint64); the outputs
    start poisoned and the entries must keep their bits."""
    from flsim._lib import check, lib
    work = [np.ascontiguousarray(e, np.float32).copy() for e in ents]
    a, keep = c_nnm(work, counts, f)
    k, P = len(work), len(work[0])
    d = np.full((k, k), np.nan)
    nbr = np.full(k, 0xFFFFFFFFFFFFFFFF, np.uint64)
    mixed = poisoned(k * P).reshape(k, P) if out else None
    vp = ctypes.c_void_p
    check(lib().flsim_nnm_eval_host(ctypes.byref(a), P, d.ctypes.data_as(vp),
                                    nbr.ctypes.data_as(vp),
                                    None if mixed is None else mixed.ctypes.data_as(vp)))
    for w, e in zip(work, ents):
        assert np.array_equal(bits(w), bits(e)), "the host twin modified an entry"
    return mixed, d, nbr


def compare(got_mixed, got_d, got_nbr, ents, counts, f, what=""):
    """dist, nbr and the mixed entries against the text; returns the text's (mixed, d, nbr)."""
    k, P = len(ents), len(ents[0])
    ref, d, nbr = text(ents, counts, f)
    bound = dist_bound(P)
    gap = cut_gap(d, f)
    print(f"nnm {what}: k={k} P={P} f={f} cut gap {gap:.3e} dist bound {bound:.3e}")
    assert gap > GAP_FACTOR * bound, (what, "the text's cut is too narrow for these inputs", gap)
    if got_d is not None:
        got_d = np.asarray(got_d, np.float64).reshape(k, k)
        assert np.array_equal(got_d, got_d.T) and (np.diag(got_d) == 0).all(), (what, "dist shape")
        fin = np.isfinite(d)
        assert np.array_equal(np.isinf(got_d), ~fin) and not np.isnan(got_d).any(), (what, "inf")
        err = np.abs(got_d[fin] - d[fin])
        assert (err <= bound * d[fin]).all(), (what, "dist",
                                               float((err / np.maximum(d[fin], 1e-300)).max()), bound)
    got_nbr = np.asarray(got_nbr).view(np.uint64)
    assert np.array_equal(got_nbr, nbr), (what, "nbr", [hex(int(x)) for x in got_nbr],
                                          [hex(int(x)) for x in nbr])
    if got_mixed is not None:
        for i in range(k):
            bad = mismatches(got_mixed[i], ref[i])
            assert bad == 0, (what, "mixed entry", i, bad)
    return ref, d, nbr
