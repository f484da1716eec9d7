"""Helpers of the robust-rule tests (tests/test_cpu_robust.py, tests/test_gpu_robust.py): the case
grid the issue fixes, the inputs, the rule text (flsim/robust.py) as the reference, and the
comparison "equal as numbers":

  the same 32 bits wherever the text's value is neither zero nor NaN,
  a zero (of either sign) where the text gives a zero,
  a NaN where the text gives a NaN.
"""
import ctypes

import numpy as np
import torch

KS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64)      # both sides of every KPAD
COUNTS = (1, 3, 128)
QNAN = 0x7FC12345


def rules(k):
    """The (kind, trim) grid at k entries: the median, and the trimmed mean with trim in
    {0, 1, (k - 1) // 2}, whichever are valid (2 * trim < k)."""
    out = [("median", 0)]
    for trim in sorted({0, 1, (k - 1) // 2}):
        if 2 * trim < k:
            out.append(("trimmed_mean", trim))
    return out


GRID = [(k, kind, trim) for k in KS for (kind, trim) in rules(k)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def counts_for(k, seed=0):
    """Mixed counts in {1, 3, 128} (all three present from k = 3 on)."""
    rs = np.random.RandomState(100 + k + seed)
    c = [COUNTS[(j + seed) % 3] for j in range(k)]
    rs.shuffle(c)
    return [int(x) for x in c]


def values(rs, k, P):
    """k bucket SUMS of P nonzero normal random values (no zero, no NaN, no subnormal)."""
    x = rs.standard_normal((k, P)).astype(np.float32)
    x[np.abs(x) < 1e-6] = np.float32(0.5)
    assert np.isfinite(x).all() and (np.abs(x) >= 1e-6).all()
    return [np.ascontiguousarray(r) for r in x]


def text(entries, counts, kind, trim):
    """The rule text (flsim/robust.py, torch on the CPU) over bucket sums and counts."""
    from flsim.robust import robust_flat
    ent = [None if e is None else torch.from_numpy(np.ascontiguousarray(e)) for e in entries]
    return robust_flat(ent, counts, kind, trim).numpy().copy()


def c_robust(entries, counts, kind, trim, ptrs=None):
    """flsim_robust over host arrays (or the raw addresses `ptrs`); kind may be an int (an
    unknown kind).  Returns (struct, keep-alive list)."""
    from flsim._lib import ROBUST_KINDS, FlsimRobust
    r = FlsimRobust()
    r.kind = ROBUST_KINDS[kind] if isinstance(kind, str) else int(kind)
    r.trim = int(trim)
    r.k = len(counts)
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


def host_twin(entries, counts, kind, trim):
    """flsim_robust_eval_host on exactly sized host arrays."""
    from flsim._lib import check, lib
    r, keep = c_robust(entries, counts, kind, trim)
    P = next(len(e) for e in entries if e is not None)
    out = np.full(P, np.float32(np.nan))
    out.view(np.uint32)[:] = QNAN
    check(lib().flsim_robust_eval_host(ctypes.byref(r), P, out.ctypes.data_as(ctypes.c_void_p)))
    return out


def mismatches(got, ref):
    """Elements where `got` does not equal the text's `ref` as a number (see the module text)."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    assert got.shape == ref.shape
    nan, zero = np.isnan(ref), ref == 0
    ok = np.where(nan, np.isnan(got), np.where(zero, got == 0, bits(got) == bits(ref)))
    return int((~ok).sum())


def special_cases(k, P, seed=0):
    """Named input sets at (k, P) beside the plain random one: duplicated values across entries;
    +-inf and NaN in 1, ceil(k / 2) and k entries; one NULL entry; a -0.0 / +0.0 tie."""
    rs = np.random.RandomState(7000 + 10 * k + seed)
    out = {}
    d = values(rs, k, P)
    for j in range(1, k, 2):                   # every other entry repeats its neighbour's means
        d[j] = d[j - 1].copy()
    out["duplicates"] = (d, [3] * k)
    for name, n_bad in (("special1", 1), ("special_half", -(-k // 2)), ("special_all", k)):
        s = values(rs, k, P)
        rows = rs.permutation(k)[:n_bad]
        for i, j in enumerate(rows):
            pat = np.array([np.inf, -np.inf, np.nan, 1.0], np.float32)
            s[j][:] = pat[(np.arange(P) + i) % 4]
        out[name] = (s, counts_for(k, seed))
    n = values(rs, k, P)
    n[rs.randint(k)] = None
    if all(e is None for e in n):              # k = 1: keep one real entry for the shape
        n = values(rs, k, P)
    out["null"] = (n, counts_for(k, seed))
    z = values(rs, k, P)
    for j in range(k):                         # half the entries -0.0, half +0.0, every element
        z[j][:] = np.float32(-0.0) if j % 2 == 0 else np.float32(0.0)
    out["zero_tie"] = (z, counts_for(k, seed))
    return out
