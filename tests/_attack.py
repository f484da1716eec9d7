"""Helpers of the attack tests (tests/test_cpu_attack.py, tests/test_gpu_attack.py): seeded bucket
sums with honest-only, mixed and fully Byzantine entries, the text (flsim/robust.py: attack_flat)
as the reference, an independent numpy restatement of it, the host twin, and the comparison "equal
as numbers": the same 32 bits wherever the text's value is neither zero nor NaN, a zero where it
gives a zero, a NaN where it gives a NaN.  There is no tolerance anywhere: the attack is purely
element-wise, and every operation of the text is one correctly rounded IEEE operation.
"""
import ctypes

import numpy as np
import torch

from _poison import QNAN

KINDS = ("ipm", "alie")
STRENGTH = {"ipm": 1.3, "alie": 0.8416212335729143}     # (no powers of two: every product rounds)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def poisoned(P, pat=QNAN):
    a = np.empty(P, np.float32)
    a.view(np.uint32)[:] = pat
    return a


def inputs(k, P, seed=0):
    """k bucket sums of P values with their honest and Byzantine counts.  Entry j is mixed
    (honest 1 .. 4, Byzantine 1 .. 3) for j % 3 == 0, honest-only for j % 3 == 1 and fully
    Byzantine for j % 3 == 2; a fully Byzantine entry is never read and holds the quiet-NaN
    pattern of tests/_poison.py.  Honest sums are randn * honest + a common offset, so mu is not
    small against sigma."""
    g = torch.Generator().manual_seed(7000 + 131 * k + 7 * seed + (P % 97))
    h = [int(c) for c in torch.randint(1, 5, (k,), generator=g)]
    b = [int(c) for c in torch.randint(1, 4, (k,), generator=g)]
    honest = [0 if j % 3 == 2 else h[j] for j in range(k)]
    byz = [0 if j % 3 == 1 else b[j] for j in range(k)]
    base = torch.randn(P, generator=g)
    x = (torch.randn(k, P, generator=g) * 0.5 + base) * \
        torch.tensor(h, dtype=torch.float32)[:, None]
    ents = [np.ascontiguousarray(r) if honest[j] else poisoned(P)
            for j, r in enumerate(x.numpy())]
    return ents, honest, byz


def _tensors(ents, honest):
    return [torch.from_numpy(np.ascontiguousarray(e, np.float32).copy()) if h else None
            for e, h in zip(ents, honest)]


def text(ents, honest, byz, kind, strength):
    """attack_flat over host arrays -> (entries [k] of numpy [P], counts, b numpy [P])."""
    from flsim.robust import attack_flat
    out, counts, b = attack_flat(_tensors(ents, honest), honest, byz, kind, strength)
    return [None if o is None else o.numpy().copy() for o in out], counts, b.numpy().copy()


def numpy_text(ents, honest, byz, kind, strength):
    """An independent restatement in numpy: fp64, plain loops for every ordered sum (numpy's fp64
    division and sqrt are the IEEE ones)."""
    with np.errstate(all="ignore"):
        y = [np.asarray(e, np.float32).astype(np.float64) / np.float64(h)
             for e, h in zip(ents, honest) if h >= 1]
        kh = np.float64(len(y))
        s = y[0].copy()
        for t in y[1:]:
            s = s + t
        mu = s / kh
        if kind == "ipm":
            b = mu * np.float64(-strength)
        else:
            v = None
            for t in y:
                d = t - mu
                v = d * d if v is None else v + d * d
            b = mu - np.sqrt(v / kh) * np.float64(strength)
        b = b.astype(np.float32)
        out = []
        for e, h, c in zip(ents, honest, byz):
            if c == 0:
                out.append(np.asarray(e, np.float32).copy())
                continue
            t = b * np.float32(c)
            out.append(np.asarray(e, np.float32) + t if h >= 1 else t)
    return out, [h + c for h, c in zip(honest, byz)], b


def mismatches(got, ref):
    """Words where fp32 `got` differs from the text's `ref` as numbers."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    nan, zero = np.isnan(ref), ref == 0
    ok = np.where(nan, np.isnan(got), np.where(zero, got == 0, bits(got) == bits(ref)))
    return int((~ok).sum())


def c_attack(ents, honest, byz, kind, strength, ptrs=None, k=None):
    """flsim_attack over host arrays (or the raw addresses `ptrs`).  Returns (struct, keep-alive);
    the arrays of `ents` are used in place when they are contiguous fp32."""
    from flsim._lib import ATTACK_KINDS, FlsimAttack
    a = FlsimAttack()
    a.kind = kind if isinstance(kind, int) else ATTACK_KINDS[kind]
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


def host_twin(ents, honest, byz, kind, strength, b_out=True):
    """flsim_attack_eval_host on copies of the entries -> (entries after, b); b starts poisoned."""
    from flsim._lib import check, lib
    work = [np.ascontiguousarray(e, np.float32).copy() for e in ents]
    a, keep = c_attack(work, honest, byz, kind, strength)
    P = len(work[0])
    b = poisoned(P) if b_out else None
    check(lib().flsim_attack_eval_host(
        ctypes.byref(a), None if b is None else b.ctypes.data_as(ctypes.c_void_p), P))
    return work, b


def compare(got_entries, got_b, ents, honest, byz, kind, strength, what=""):
    """Entries and b against the text as numbers; an entry with byz == 0 keeps its bits."""
    ref, counts, b = text(ents, honest, byz, kind, strength)
    if got_b is not None:
        bad = mismatches(got_b, b)
        assert bad == 0, (what, "b", bad)
    for j, (g, r) in enumerate(zip(got_entries, ref)):
        if byz[j] == 0:
            assert np.array_equal(bits(g), bits(ents[j])), (what, "untouched entry", j)
        else:
            bad = mismatches(g, r)
            assert bad == 0, (what, "entry", j, bad)
    return ref, counts, b
