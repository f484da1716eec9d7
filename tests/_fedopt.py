"""Shared by tests/test_cpu_fedopt.py and tests/test_gpu_fedopt.py: the rule text of the two
server optimizers of Adaptive Federated Optimization (Reddi et al. 2021) the fused step carries,
evaluated with torch CPU ops in the text's order and numpy's sqrt in between (numpy's fp32 sqrt is
correctly rounded like the kernels' sqrt_rn; torch's vectorised one is not).

    Adagrad (torch.optim.Adagrad, _single_tensor_adagrad)
        if wd != 0: g = g.add(p, alpha=wd)
        sum.addcmul_(g, g, value=1)
        p.addcdiv_(g, sum.sqrt().add_(eps), value=-clr)      clr = lr / (1 + (step - 1) * lr_decay)

    Yogi (flsim.optim.Yogi: Zaheer et al. 2018 without bias correction)
        if wd != 0: g = g.add(p, alpha=wd)
        exp_avg.lerp_(g, 1 - beta1)
        g2 = g * g
        exp_avg_sq.addcmul_(torch.sign(exp_avg_sq - g2), g2, value=-(1 - beta2))
        p.addcdiv_(exp_avg, exp_avg_sq.sqrt().add_(eps), value=-lr)
"""
import numpy as np
import torch

# the cap on the share of elements of p that may differ when the sqrt is torch's own instead of a
# correctly rounded one (the project's cap for Adam against torch's sqrt)
MAX_SQRT_SHARE = 0.005


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def n_diff(a, b):
    return int((bits(a) != bits(b)).sum())


def sqrt_rn(t):
    """Correctly rounded fp32 sqrt of a CPU tensor (numpy's)."""
    with np.errstate(all="ignore"):
        return torch.from_numpy(np.sqrt(t.numpy()))


def n_state(o):
    if o["kind"] == "adagrad":
        return 1
    if o["kind"] == "sgd":
        return 1 if o.get("momentum", 0) != 0 else 0
    return 2


def adagrad_expected(g, p, s, step, lr=1e-2, lr_decay=0.0, weight_decay=0.0, eps=1e-10,
                     sqrt=sqrt_rn):
    """(p, sum) after torch.optim.Adagrad's step `step` (the count after increment) on the
    gradient g, op by op.  -> numpy arrays."""
    tg = torch.from_numpy(np.ascontiguousarray(g, np.float32).copy())
    tp = torch.from_numpy(np.ascontiguousarray(p, np.float32).copy())
    ts = torch.from_numpy(np.ascontiguousarray(s, np.float32).copy())
    if weight_decay != 0:
        tg = tg.add(tp, alpha=weight_decay)
    clr = lr / (1 + (step - 1) * lr_decay)
    ts.addcmul_(tg, tg, value=1)
    tp.addcdiv_(tg, sqrt(ts).add_(eps), value=-clr)
    return tp.numpy(), ts.numpy()


def yogi_expected(g, p, m, v, step=1, lr=1e-2, betas=(0.9, 0.99), eps=1e-3, weight_decay=0.0,
                  sqrt=sqrt_rn):
    """(p, exp_avg, exp_avg_sq) after one Yogi step on the gradient g, op by op (step is accepted
    for symmetry: without bias correction the update does not depend on it)."""
    tg = torch.from_numpy(np.ascontiguousarray(g, np.float32).copy())
    tp = torch.from_numpy(np.ascontiguousarray(p, np.float32).copy())
    tm = torch.from_numpy(np.ascontiguousarray(m, np.float32).copy())
    tv = torch.from_numpy(np.ascontiguousarray(v, np.float32).copy())
    if weight_decay != 0:
        tg = tg.add(tp, alpha=weight_decay)
    tm.lerp_(tg, 1 - betas[0])
    g2 = tg * tg
    tv.addcmul_(torch.sign(tv - g2), g2, value=-(1 - betas[1]))
    tp.addcdiv_(tm, sqrt(tv).add_(eps), value=-lr)
    return tp.numpy(), tm.numpy(), tv.numpy()


def expected(o, g, p, m, v, step):
    """(p, m, v) after the update of an Optim-style dict o (kind "adagrad" or "yogi"); the state
    arrays the kind does not own come back None."""
    hp = {k: x for k, x in o.items() if k not in ("kind", "initial_accumulator_value")}
    if o["kind"] == "adagrad":
        pe, se = adagrad_expected(g, p, m, step, **hp)
        return pe, se, None
    assert o["kind"] == "yogi"
    return yogi_expected(g, p, m, v, step, **hp)


def sqrt_bound(p_new, p_old):
    """The largest |dp| a differing element may show when a 1-ulp sqrt replaces the correctly
    rounded one: 2^-21 * |update| + 2^-23 * |p| (twice the derived bound: the denominator is at
    most 1 ulp off, the quotient is rounded twice, p once)."""
    upd = np.abs(p_new.astype(np.float64) - p_old.astype(np.float64))
    return 2.0 ** -21 * upd + 2.0 ** -23 * np.abs(p_new.astype(np.float64))


def check_sqrt_close(p_got, p_ref, p_old, state, label=""):
    """The conditions on p (from torch, whose sqrt of `state` is its own) against a yardstick that
    differs only in that sqrt's rounding: p differs only where torch's root of `state` differs from
    the correctly rounded one, on at most MAX_SQRT_SHARE of the elements, each within sqrt_bound.
    Prints the figures, then asserts all three.  -> (share, worst ratio to the bound, share of
    differing roots)."""
    with np.errstate(all="ignore"):
        root_diff = bits(torch.from_numpy(np.ascontiguousarray(state).copy()).sqrt()) != \
            bits(np.sqrt(state))
    root_share = float(root_diff.mean())
    diff = bits(p_got) != bits(p_ref)
    share = float(diff.mean())
    d = np.abs(p_got.astype(np.float64) - p_ref.astype(np.float64))[diff]
    b = sqrt_bound(p_ref, p_old)[diff]
    worst = float((d / b).max()) if diff.any() else 0.0
    unexplained = int((diff & ~root_diff).sum())
    print(f"{label}: p differs on {share:.5%}, worst {worst:.3f} of the bound; torch's sqrt "
          f"differs on {root_share:.3%}; differing p at an equal root: {unexplained}")
    assert unexplained == 0, unexplained
    assert share <= MAX_SQRT_SHARE, (share, root_share)
    assert worst <= 1.0, worst
    return share, worst, root_share


def inputs(P, ns, seed):
    """tests/test_gpu_optim.py's _inputs: S with the division paths' edge values (+-0, a subnormal,
    a huge gradient whose square is inf), stale entries, p, m, v -- and `acc`, a non-negative
    accumulator for Adagrad's sum."""
    rs = np.random.RandomState(seed)
    S = (rs.standard_normal(P) * 1e-2).astype(np.float32)
    S[::17] = 0.0
    S[1::17] = -0.0
    S[2::17] = np.float32(3e-39) * rs.choice([-1, 1], len(S[2::17]))
    S[3::17] = np.float32(1e30)
    stale = [(rs.standard_normal(P) * 1e-2).astype(np.float32) for _ in range(ns)]
    p = rs.standard_normal(P).astype(np.float32)
    m = (rs.standard_normal(P) * 1e-3).astype(np.float32)
    v = (rs.rand(P) * 1e-5).astype(np.float32)
    return S, stale, p, m, v, np.abs(m)


def mean(entries, sizes):
    """rule(): the oracle's cascade mean per tensor."""
    from oracle import oracle as O
    g = np.empty_like(entries[0])
    off = 0
    for n in sizes:
        g[off:off + n] = O.cascade_mean([e[off:off + n] for e in entries])
        off += n
    return g
