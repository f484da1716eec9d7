"""Helpers of the centered-clipping tests (tests/test_cpu_cclip.py, tests/test_gpu_cclip.py): the
case grid and the seeded inputs of tests/_geomed.py, a seeded center, a radius at which some
entries clip and some do not, the rule text (flsim/robust.py: cclip_flat and its parts) as the
reference, the host twin, and the stepwise comparison.

Why stepwise: as for the geometric median (tests/_geomed.py), the kernel's distances differ from
the text's in their last bits, and the next weights and g depend on them.  Every stage is pinned at
the device's own inputs instead:

  d2[r]        against the text's distances evaluated at the device's own (u[r], w[r]).  The
               text's z is then bit-identical to the kernel's up to the sign of a zero, which
               (x - z)^2 does not see, so both sides sum the same P non-negative terms with at
               most P + 2 fp64 roundings each:
                   |d2 - d2_text| <= 2 (P + 2) 2^-53 d2_text            (_geomed.d2_bound(P))
  s[r], u[r + 1], w[r + 1]   against the text's scalar code (cclip_scalar) applied to the
               device's d2[r], u[r], w[r]: bit for bit;
  g            against the text's z at (u[iters], w[iters]), .float(): bit for bit, zero signs
               included, a NaN where the text has a NaN.
"""
import ctypes

import numpy as np
import torch

from _geomed import KS, QNAN, _tensors, bits, cols_of, d2_bound, f64_mismatches  # noqa: F401
from _geomed import g_mismatches, inputs, outside  # noqa: F401

SNAN = 0x7FA00001        # a signalling NaN: the poison of a center that must not be read


def center(P, seed=0):
    """A seeded center [P] fp32: half the scale of an entry's mean."""
    g = torch.Generator().manual_seed(77000 + 13 * seed)
    return np.ascontiguousarray((0.5 * torch.randn(P, generator=g)).numpy())


def distances(entries, counts, cen):
    """The fp64 distances of the live entries' means to the center (None: zero), sorted."""
    x = cols_of(entries, counts).double()
    c = torch.zeros(x.shape[1], dtype=torch.float64) if cen is None else \
        torch.from_numpy(np.ascontiguousarray(cen, np.float32)).double()
    alive = torch.isfinite(x).all(1)
    return np.sort(((x[alive] - c) ** 2).sum(1).sqrt().numpy())


def pick_tau(entries, counts, cen):
    """A radius between the two middle distances of the first iteration: the nearer half of the
    entries is not clipped there, the farther half is (one live entry: 0.6 of its distance, so the
    first iteration clips and a later one does not).  The middle distances are a relative 1e-9
    apart at the least (asserted), far more than the rounding of a distance; the stepwise
    comparison itself needs no such margin, since s is pinned at the device's own d2."""
    d = np.unique(distances(entries, counts, cen))     # (a duplicated entry counts once)
    if len(d) == 1:
        return 0.6 * float(d[0])
    lo, hi = float(d[(len(d) - 1) // 2]), float(d[(len(d) - 1) // 2 + 1])
    assert hi - lo > 1e-9 * hi, (lo, hi)
    return 0.5 * (lo + hi)


def _cen(cen):
    return None if cen is None else torch.from_numpy(np.ascontiguousarray(cen, np.float32))


def text(entries, counts, cen, tau, iters, weighted=False):
    """The rule text over bucket sums, counts and the center (None: fresh), from scratch ->
    (g [P] fp32, u [iters + 1], w [iters + 1, k], d2 [iters, k], s [iters, k]) as numpy."""
    from flsim.robust import cclip_flat
    g, u, w, d2, s = cclip_flat(_tensors(entries), counts, _cen(cen), tau, iters, weighted)
    return (g.numpy().copy(), torch.stack(u).numpy().copy(), torch.stack(w).numpy().copy(),
            torch.stack(d2).numpy().copy(), torch.stack(s).numpy().copy())


def c_cclip(entries, counts, cen, tau, iters, weighted=False, fresh=None, ptrs=None,
            center_ptr=None):
    """flsim_cclip over host arrays (or the raw addresses `ptrs` / `center_ptr`); fresh defaults
    to "no center given".  Returns (struct, keep-alive)."""
    from flsim._lib import FlsimCclip
    r = FlsimCclip()
    r.iters, r.weighted, r.k, r.tau = int(iters), int(weighted), len(counts), float(tau)
    r.fresh = int(cen is None and center_ptr is None) if fresh is None else int(fresh)
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
    if center_ptr is not None:
        r.center = center_ptr
    elif cen is not None:
        a = np.ascontiguousarray(cen, np.float32)
        keep.append(a)
        r.center = a.ctypes.data
    return r, keep


def host_twin(entries, counts, cen, tau, iters, weighted=False, fresh=None):
    """flsim_cclip_eval_host on exactly sized host arrays -> (g, u, w, d2, s, center_out)."""
    from flsim._lib import check, lib
    r, keep = c_cclip(entries, counts, cen, tau, iters, weighted, fresh)
    k = len(counts)
    P = next(len(e) for e in entries if e is not None)
    g, cout = np.empty(P, np.float32), np.empty(P, np.float32)
    g.view(np.uint32)[:] = QNAN
    cout.view(np.uint32)[:] = QNAN
    u = np.full(iters + 1, -7.0)
    w = np.full((iters + 1, k), -7.0)
    d2 = np.full((iters, k), -7.0)
    s = np.full((iters, k), -7.0)
    vp = ctypes.c_void_p
    check(lib().flsim_cclip_eval_host(ctypes.byref(r), P, u.ctypes.data_as(vp),
                                      w.ctypes.data_as(vp), d2.ctypes.data_as(vp),
                                      s.ctypes.data_as(vp), g.ctypes.data_as(vp),
                                      cout.ctypes.data_as(vp)))
    return g, u, w, d2, s, cout


def stepwise(entries, counts, cen, tau, iters, weighted, got, what=""):
    """The stepwise comparison of got = (g, u, w, d2, s) against the text (the module docstring).
    Returns (the text's alive mask, the text's g at the device's final weights)."""
    from flsim.robust import _cclip_z, cclip_dist2, cclip_scalar, geomed_alpha
    g, u, w, d2, s = got[:5]
    k = len(counts)
    cols = cols_of(entries, counts)
    P = cols.shape[1]
    assert u.shape == (iters + 1,) and w.shape == (iters + 1, k), what
    assert d2.shape == (iters, k) and s.shape == (iters, k), what
    x = cols.double()
    c = None if cen is None else _cen(cen).double()
    alive = torch.isfinite(x).all(1)
    alpha = geomed_alpha(counts, weighted)
    a = torch.where(alive, alpha, torch.zeros_like(alpha))
    assert f64_mismatches(u[:1], np.ones(1)) == 0 and f64_mismatches(w[0], np.zeros(k)) == 0, what
    for r in range(iters):
        u_r, w_r = torch.tensor(float(u[r]), dtype=torch.float64), torch.from_numpy(w[r].copy())
        d2_t = cclip_dist2(x, c, u_r, w_r, alive).numpy()
        if np.isnan(d2_t).any():            # (a NaN center: NaN distances on both sides)
            assert np.array_equal(np.isnan(d2[r]), np.isnan(d2_t)), (what, "d2 nan", r)
        else:
            assert outside(d2[r], d2_t, d2_bound(P)) == 0, (what, "d2", r, d2[r], d2_t)
        s_t, u_t, w_t = cclip_scalar(torch.from_numpy(d2[r].copy()), a, alive, tau, u_r, w_r)
        assert f64_mismatches(s[r], s_t.numpy()) == 0, (what, "s", r, s[r], s_t)
        assert f64_mismatches(u[r + 1:r + 2], u_t.numpy().reshape(1)) == 0, (what, "u", r + 1)
        assert f64_mismatches(w[r + 1], w_t.numpy()) == 0, (what, "w", r + 1)
    g_t = _cclip_z(x, c, torch.tensor(float(u[iters]), dtype=torch.float64),
                   torch.from_numpy(w[iters].copy())).float().numpy()
    bad = g_mismatches(g, g_t)
    assert bad == 0, (what, "g", bad)
    return alive.numpy(), g_t
