"""Helpers of the geometric-median tests (tests/test_cpu_geomed.py, tests/test_gpu_geomed.py): the
case grid, the seeded inputs of tests/_krum.py, the rule text (flsim/robust.py: geomed_flat and its
parts) as the reference, the host twin, and the stepwise comparison.

Why stepwise.  The kernel's distances differ from the text's in their last bits (the summation
order differs), the next weights depend on them, and so does g: a check of the whole chain cannot
have zero tolerance.  Every stage is pinned at the device's own inputs instead:

  d2[r]        against the text's distances evaluated at the device's own w[r].  The text's z is
               then bit-identical to the kernel's (_wsum: fp64, index order, one multiply and one
               add per term), so both sides sum the same P non-negative terms (x_j - z)^2.  Each
               side commits at most P + 2 fp64 roundings per distance (the square or the fma of
               every term and the adds, in whatever order), so
                   |d2 - d2_text| <= 2 (P + 2) 2^-53 d2_text            (D2_BOUND(P), relative)
  w[r + 1],    against the text's scalar code (geomed_scalar: sqrt, max, divide, sequential sums)
  obj[r]       applied to the device's d2[r]: bit for bit;
  g            against _wsum(x, w[iters]).float(): bit for bit, a NaN where the text has a NaN.
"""
import ctypes

import numpy as np
import torch

from _krum import QNAN, bits, g_mismatches, inputs, outside  # noqa: F401

KS = (1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 64)       # both sides of every KPAD
NU = 1e-6


def d2_bound(P):
    return 2.0 * (P + 2) * 2.0 ** -53


def _tensors(entries):
    return [None if e is None else torch.from_numpy(np.ascontiguousarray(e, np.float32))
            for e in entries]


def cols_of(entries, counts):
    """The bucket means [k, P] fp32 as the text forms them (None: zeros)."""
    from flsim.robust import bucket_means
    ent = _tensors(entries)
    ref = next(e for e in ent if e is not None)
    sums = [torch.zeros_like(ref) if e is None else e for e in ent]
    return torch.stack(bucket_means(sums, counts))


def text(entries, counts, iters, nu=NU, weighted=False):
    """The rule text over bucket sums and counts, from scratch -> (g [P] fp32, w [iters + 1, k],
    d2 [iters, k], obj [iters]) as numpy."""
    from flsim.robust import geomed_flat
    g, w, d2, obj = geomed_flat(_tensors(entries), counts, iters, nu, weighted)
    k = len(counts)
    return (g.numpy().copy(), torch.stack(w).numpy().copy(),
            torch.stack(d2).numpy().copy() if iters else np.zeros((0, k)),
            torch.stack(obj).numpy().copy() if iters else np.zeros(0))


def c_geomed(entries, counts, iters, nu=NU, weighted=False, ptrs=None):
    """flsim_geomed over host arrays (or the raw addresses `ptrs`).  Returns (struct, keep-alive)."""
    from flsim._lib import FlsimGeomed
    r = FlsimGeomed()
    r.iters, r.weighted, r.k, r.nu = int(iters), int(weighted), len(counts), float(nu)
    keep = []
    for j, c in enumerate(counts[:64]):
        r.count[j] = int(c)
        if ptrs is not None:
            r.entries[j] = ptrs[j]
        elif entries[j] is not None:
            a = entries[j] if isinstance(entries[j], np.ndarray) and entries[j].dtype == np.float32 \
                and entries[j].flags.c_contiguous else np.ascontiguousarray(entries[j], np.float32)
            keep.append(a)
            r.entries[j] = a.ctypes.data
    return r, keep


def host_twin(entries, counts, iters, nu=NU, weighted=False):
    """flsim_geomed_eval_host on exactly sized host arrays -> (g, w, d2, obj)."""
    from flsim._lib import check, lib
    r, keep = c_geomed(entries, counts, iters, nu, weighted)
    k = len(counts)
    P = next(len(e) for e in entries if e is not None)
    g = np.empty(P, np.float32)
    g.view(np.uint32)[:] = QNAN
    w = np.full((iters + 1, k), -7.0)
    d2 = np.full((iters, k), -7.0)
    obj = np.full(iters, -7.0)
    vp = ctypes.c_void_p
    check(lib().flsim_geomed_eval_host(ctypes.byref(r), P, w.ctypes.data_as(vp),
                                       d2.ctypes.data_as(vp), obj.ctypes.data_as(vp),
                                       g.ctypes.data_as(vp)))
    return g, w, d2, obj


def f64_mismatches(got, ref):
    """Words where fp64 `got` differs from the text's: bit for bit, a NaN where it has a NaN."""
    got, ref = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    nan = np.isnan(ref)
    return int((~np.where(nan, np.isnan(got), got.view(np.uint64) == ref.view(np.uint64))).sum())


def stepwise(entries, counts, iters, nu, weighted, got, what=""):
    """The stepwise comparison of got = (g, w, d2, obj) against the text (the module docstring).
    Returns the text's alive mask."""
    from flsim.robust import _seqsum, _wsum, geomed_alpha, geomed_dist2, geomed_scalar
    g, w, d2, obj = got
    k = len(counts)
    cols = cols_of(entries, counts)
    P = cols.shape[1]
    assert w.shape == (iters + 1, k) and d2.shape == (iters, k) and obj.shape == (iters,), what
    x = cols.double()
    alive = torch.isfinite(x).all(1)
    alpha = geomed_alpha(counts, weighted)
    a = torch.where(alive, alpha, torch.zeros_like(alpha))
    assert f64_mismatches(w[0], (a / _seqsum(a)).numpy()) == 0, (what, "w0")
    for r in range(iters):
        d2_t = geomed_dist2(x, torch.from_numpy(w[r].copy()), alive).numpy()
        assert outside(d2[r], d2_t, d2_bound(P)) == 0, (what, "d2", r, d2[r], d2_t)
        obj_t, w_t = geomed_scalar(torch.from_numpy(d2[r].copy()), a, alive, nu)
        assert f64_mismatches(obj[r:r + 1], obj_t.numpy().reshape(1)) == 0, (what, "obj", r)
        assert f64_mismatches(w[r + 1], w_t.numpy()) == 0, (what, "w", r + 1)
    g_t = _wsum(x, torch.from_numpy(w[iters].copy())).float().numpy()
    bad = g_mismatches(g, g_t)
    assert bad == 0, (what, "g", bad)
    return alive.numpy()


def ulp_distance(a, b):
    """The distance of two fp32 arrays in units in the last place (finite values)."""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
