"""Helpers of the Min-Max / Min-Sum attack tests (tests/test_cpu_attack_opt.py,
tests/test_gpu_attack_opt.py): the inputs of tests/_attack.py (and a variant in which every entry
is read), the text (flsim/robust.py: opt_attack_flat) as the reference, an independent numpy
restatement of it, the host twin, and the stage-by-stage yardstick at the device's own outputs:

  dist       within 2 (P + 2) 2^-53 relative of the text's (the pairwise stage's existing bound);
  a_i, q     within the same relative bound (sums of non-negative terms);
  c_i        within 2 (P + 2) 2^-53 * sqrt(a_i q) absolute (Cauchy-Schwarz on the absolute terms);
  gamma      bit for bit opt_gamma of the device's own a, c, q, dist;
  b, entries equal as numbers (tests/_attack.py) to the text evaluated with the device's gamma.

A bound that is zero (a_i = 0, say) asserts equality; a NaN in the text asks for a NaN, an inf for
the same inf.
"""
import ctypes

import numpy as np
import torch

import _attack as A

KINDS = ("minmax", "minsum")
DIRS = ("unit", "std", "sign")
U53 = 2.0 ** -53


def inputs(k, P, seed=0, full=False):
    """tests/_attack.py's inputs; full: the fully Byzantine entries become mixed ones, so that
    every entry is read (kh = k) -- honest-only and mixed entries remain."""
    ents, honest, byz = A.inputs(k, P, seed)
    if full:
        g = torch.Generator().manual_seed(9100 + 17 * k + seed)
        for j in range(k):
            if honest[j] == 0:
                honest[j] = int(torch.randint(1, 5, (1,), generator=g))
                ents[j] = ((torch.randn(P, generator=g) * 0.5 + 0.3) * honest[j]).numpy()
    return ents, honest, byz


def _tensors(ents, honest):
    return [torch.from_numpy(np.ascontiguousarray(e, np.float32).copy()) if h else None
            for e, h in zip(ents, honest)]


def text(ents, honest, byz, kind, dirn, strength, use_gamma=None):
    """opt_attack_flat over host arrays -> dict of numpy values (gamma a Python float: the text's
    own; use_gamma: b and the entries are evaluated with that one)."""
    from flsim.robust import opt_attack_flat
    out, counts, b, gamma, a, c, q, dist = opt_attack_flat(_tensors(ents, honest), honest, byz,
                                                           kind, dirn, strength, use_gamma)
    return dict(entries=[None if o is None else o.numpy().copy() for o in out], counts=counts,
                b=b.numpy().copy(), gamma=gamma, a=a.numpy(), c=c.numpy(), q=float(q),
                dist=dist.numpy())


def text_mix(ents, honest, byz, dirn, strength, gamma):
    """The text's b and entries for a given gamma."""
    from flsim.robust import opt_attack_mix
    out, counts, b = opt_attack_mix(_tensors(ents, honest), honest, byz, dirn, strength,
                                    float(gamma))
    return [None if o is None else o.numpy().copy() for o in out], counts, b.numpy().copy()


def numpy_parts(ents, honest, dirn):
    """y, mu, p in numpy: fp64, plain loops for every ordered sum."""
    with np.errstate(all="ignore"):
        y = [np.asarray(e, np.float32).astype(np.float64) / np.float64(h)
             for e, h in zip(ents, honest) if h >= 1]
        s = y[0].copy()
        for t in y[1:]:
            s = s + t
        mu = s / np.float64(len(y))
        if dirn == "unit":
            p = -mu
        elif dirn == "std":
            v = None
            for t in y:
                d = t - mu
                v = d * d if v is None else v + d * d
            p = -np.sqrt(v / np.float64(len(y)))
        else:
            p = np.where(mu > 0, -1.0, np.where(mu < 0, 1.0, -mu))
    return y, mu, p


def _loopsum(v):
    s = np.float64(v[0])
    for t in v[1:]:
        s = s + t
    return s


def numpy_text(ents, honest, byz, kind, dirn, strength):
    """An independent restatement: numpy for the element-wise part, Python loops for every sum
    over elements and entries, the quadratic solved with math.sqrt."""
    import math
    with np.errstate(all="ignore"):
        y, mu, p = numpy_parts(ents, honest, dirn)
        kh = len(y)
        a = [float(_loopsum((mu - t) * (mu - t))) for t in y]
        c = [float(_loopsum((mu - t) * p)) for t in y]
        q = float(_loopsum(p * p))
        x = [(np.asarray(e, np.float32) / np.float32(h)).astype(np.float64)
             for e, h in zip(ents, honest) if h >= 1]
        dist = np.zeros((kh, kh))
        for i in range(kh):
            for j in range(kh):
                if i != j:
                    d = float(((x[i] - x[j]) ** 2).sum())
                    dist[i, j] = math.inf if d != d else d

        def root(c_, q_, r):
            r = 0.0 if r < 0 else r
            return (math.sqrt(c_ * c_ + q_ * r) - c_) / q_
        if q == 0:
            gamma = 0.0
        elif kind == "minmax":
            D = float(dist.max())
            gs = [root(c[i], q, D - a[i]) for i in range(kh)]
            gamma = math.nan if any(g != g for g in gs) else min(gs)
        else:
            S = max(float(_loopsum(dist[i])) for i in range(kh))
            gamma = root(float(_loopsum(c)), kh * q, S - float(_loopsum(a)))
        b64 = mu + p * (np.float64(gamma) * np.float64(strength))
        b = b64.astype(np.float32)
        out = []
        for e, h, n in zip(ents, honest, byz):
            if n == 0:
                out.append(np.asarray(e, np.float32).copy())
                continue
            t = b * np.float32(n)
            out.append(np.asarray(e, np.float32) + t if h >= 1 else t)
    return dict(entries=out, b=b, b64=b64, y=y, gamma=gamma, a=np.asarray(a), c=np.asarray(c),
                q=q, dist=dist)


def c_attack_opt(ents, honest, byz, kind, dirn, strength, ptrs=None, k=None):
    """flsim_attack_opt over host arrays (or the raw addresses `ptrs`) -> (struct, keep-alive)."""
    from flsim._lib import OPT_ATTACK_DIRS, OPT_ATTACK_KINDS, FlsimAttackOpt
    a = FlsimAttackOpt()
    a.kind = kind if isinstance(kind, int) else OPT_ATTACK_KINDS[kind]
    a.dir = dirn if isinstance(dirn, int) else OPT_ATTACK_DIRS[dirn]
    a.k = len(honest) if k is None else k
    a.strength = float(strength)
    keep = []
    for j in range(min(len(honest), 64)):
        a.honest[j], a.byz[j] = int(honest[j]), int(byz[j])
        if ptrs is not None:
            a.entries[j] = ptrs[j]
        elif ents[j] is not None:
            assert ents[j].dtype == np.float32 and ents[j].flags.c_contiguous
            keep.append(ents[j])
            a.entries[j] = ents[j].ctypes.data
    return a, keep


def host_twin(ents, honest, byz, kind, dirn, strength, b_out=True):
    """flsim_attack_opt_eval_host on copies of the entries -> dict; b, dist, stats and gamma start
    poisoned."""
    from flsim._lib import ATTACK_OPT_STATS, check, lib
    work = [np.ascontiguousarray(e, np.float32).copy() for e in ents]
    a, keep = c_attack_opt(work, honest, byz, kind, dirn, strength)
    P = len(work[0])
    kh = sum(1 for h in honest if h >= 1)
    b = A.poisoned(P) if b_out else None
    dist = np.full(kh * kh, np.nan)
    stats = np.full(ATTACK_OPT_STATS, np.nan)
    gamma = np.full(1, np.nan)
    vp = ctypes.c_void_p
    check(lib().flsim_attack_opt_eval_host(
        ctypes.byref(a), dist.ctypes.data_as(vp), stats.ctypes.data_as(vp),
        gamma.ctypes.data_as(vp), None if b is None else b.ctypes.data_as(vp), P))
    return dict(entries=work, b=b, gamma=float(gamma[0]), a=stats[:kh].copy(),
                c=stats[64:64 + kh].copy(), q=float(stats[128]), dist=dist.reshape(kh, kh))


def within(got, ref, bound):
    """Element-wise: |got - ref| <= bound; a NaN for a NaN; where ref is infinite or the bound is
    zero, equality.  Returns the number of misses."""
    got, ref, bound = np.broadcast_arrays(np.asarray(got, np.float64), np.asarray(ref, np.float64),
                                          np.asarray(bound, np.float64))
    with np.errstate(all="ignore"):
        nan = np.isnan(ref)
        exact = np.isinf(ref) | (bound == 0)
        ok = np.where(nan, np.isnan(got), np.where(exact, got == ref, np.abs(got - ref) <= bound))
    assert not np.isinf(bound[~nan & ~exact]).any(), "a vacuous bound"
    return int((~ok).sum())


def same_f64(x, y):
    return (x != x and y != y) or np.float64(x).view(np.uint64) == np.float64(y).view(np.uint64)


def check_stages(got, ents, honest, byz, kind, dirn, strength, what=""):
    """The yardstick of the module docstring over `got` (a host_twin-style dict); returns the
    text's dict."""
    from flsim.robust import opt_gamma
    P = len(ents[0])
    ref = text(ents, honest, byz, kind, dirn, strength, use_gamma=float(got["gamma"]))
    rel = 2 * (P + 2) * U53
    with np.errstate(all="ignore"):
        assert within(got["dist"], ref["dist"], rel * np.abs(ref["dist"])) == 0, (what, "dist")
        assert within(got["a"], ref["a"], rel * np.abs(ref["a"])) == 0, (what, "a")
        assert within(got["q"], ref["q"], rel * abs(ref["q"])) == 0, (what, "q")
        assert within(got["c"], ref["c"], rel * np.sqrt(ref["a"] * ref["q"])) == 0, (what, "c")
    g = opt_gamma(kind, [float(v) for v in got["a"]], [float(v) for v in got["c"]],
                  float(got["q"]), [[float(v) for v in row] for row in got["dist"]])
    assert same_f64(got["gamma"], g), (what, "gamma", got["gamma"], g)
    out, counts, b = ref["entries"], ref["counts"], ref["b"]
    if got["b"] is not None:
        bad = A.mismatches(got["b"], b)
        assert bad == 0, (what, "b", bad)
    for j, (x, r) in enumerate(zip(got["entries"], out)):
        if byz[j] == 0:
            assert np.array_equal(A.bits(x), A.bits(ents[j])), (what, "untouched entry", j)
        else:
            bad = A.mismatches(x, r)
            assert bad == 0, (what, "entry", j, bad)
    return ref
