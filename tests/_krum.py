"""Helpers of the Krum tests (tests/test_cpu_krum.py, tests/test_gpu_krum.py): the case grid, the
seeded inputs, the rule text (flsim/robust.py: krum_flat) as the reference, the host twin, and
the comparison.

Tolerance, derived: every summand of a distance is non-negative and each side commits at most
P + 2 fp64 roundings per distance, so

    |d - d_text| <= 2 (P + 2) 2^-53 d_text            (DIST_BOUND(P), relative)
    |s - s_text| <= 2 * that * s_text                 (the second factor: a swap at the row's cut
                                                       between near-equal distances)

Everything else (the selection, g) has no tolerance; the inputs keep the text's m-th and
(m + 1)-th smallest scores at least 1000 bounds apart (asserted per case by the tests, never
skipped), so the selection cannot depend on the rounding.
"""
import ctypes

import numpy as np
import torch

KS = (4, 5, 8, 9, 16, 17, 32, 33, 64)       # both sides of every KPAD
QNAN = 0x7FC12345


def grid(k):
    """(f, m) at k entries: f in {0, 1, (k - 3) // 2} with k >= 2f + 3 and k - f - 2 >= 2;
    m in {1, 2, (k - f + 1) // 2, k - f}."""
    out = []
    for f in sorted({0, 1, (k - 3) // 2}):
        if f < 0 or k < 2 * f + 3 or k - f - 2 < 2:
            continue
        for m in sorted({1, 2, (k - f + 1) // 2, k - f}):
            if 1 <= m <= k - f:
                out.append((f, m))
    return out


GRID = [(k, f, m) for k in KS for (f, m) in grid(k)]


def dist_bound(P):
    return 2.0 * (P + 2) * 2.0 ** -53


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def inputs(k, P, seed=0):
    """k bucket SUMS of P values, randn * count, and their counts in 1 .. 4."""
    g = torch.Generator().manual_seed(9000 + 131 * k + 7 * seed)
    counts = [int(c) for c in torch.randint(1, 5, (k,), generator=g)]
    x = torch.randn(k, P, generator=g) * torch.tensor(counts, dtype=torch.float32)[:, None]
    return [np.ascontiguousarray(r) for r in x.numpy()], counts


def text(entries, counts, f, m):
    """The rule text over bucket sums and counts -> (g, dist, score, sel) as numpy / list."""
    from flsim.robust import krum_flat
    ent = [None if e is None else torch.from_numpy(np.ascontiguousarray(e)) for e in entries]
    g, d, s, sel = krum_flat(ent, counts, f, m)
    return g.numpy().copy(), d.numpy().copy(), s.numpy().copy(), [int(j) for j in sel]


def score_gap(score, m):
    """The relative gap between the m-th and the (m + 1)-th smallest text score (inf: m = k)."""
    s = np.sort(np.asarray(score, np.float64))
    if m >= len(s):
        return float("inf")
    return float((s[m] - s[m - 1]) / s[m - 1]) if s[m - 1] > 0 else float("inf")


def c_krum(entries, counts, f, m, ptrs=None):
    """flsim_krum over host arrays (or the raw addresses `ptrs`).  Returns (struct, keep-alive)."""
    from flsim._lib import FlsimKrum
    r = FlsimKrum()
    r.f, r.m, r.k = int(f), int(m), len(counts)
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


def host_twin(entries, counts, f, m):
    """flsim_krum_eval_host on exactly sized host arrays -> (g, dist, score, sel)."""
    from flsim._lib import check, lib
    r, keep = c_krum(entries, counts, f, m)
    k = len(counts)
    P = next(len(e) for e in entries if e is not None)
    g = np.empty(P, np.float32)
    g.view(np.uint32)[:] = QNAN
    d = np.full((k, k), np.nan)
    s = np.full(k, np.nan)
    sel = np.full(m, -1, np.int32)
    vp = ctypes.c_void_p
    check(lib().flsim_krum_eval_host(ctypes.byref(r), P, d.ctypes.data_as(vp),
                                     s.ctypes.data_as(vp), sel.ctypes.data_as(vp),
                                     g.ctypes.data_as(vp)))
    return g, d, s, [int(j) for j in sel]


def outside(got, ref, rel):
    """Entries of `got` further than rel * ref from the text's `ref` (inf equals inf only)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    fin = np.isfinite(ref)
    ok = np.where(fin, np.abs(got - np.where(fin, ref, 0)) <= rel * np.where(fin, ref, 0),
                  got == ref)
    return int((~ok).sum())


def g_mismatches(got, ref):
    """Words where g differs from the text's: bit for bit, a NaN where it has a NaN."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    nan = np.isnan(ref)
    return int((~np.where(nan, np.isnan(got), bits(got) == bits(ref))).sum())
