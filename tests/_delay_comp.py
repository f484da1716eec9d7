"""Shared by tests/test_cpu_delay_comp.py and tests/test_gpu_delay_comp.py: the rule text of delay
compensation (DC-ASGD), evaluated by torch on CPU tensors, and the inputs the tests use.

    def compensate(x, theta_now, theta_src, lam):          # per parameter tensor, fp32
        return x + (x * x) * lam * (theta_now - theta_src)

Five fp32 roundings per element: x*x, times f32(lam), theta_now - theta_src, their product, the add.
"""
import numpy as np
import torch

WEIGHTS = [(1.0 + 50) ** -0.5, 1.0 / 3.0, 1e-3]
LAMBDAS = [2.0, 0.04]
# Scale of the compensated arrays' ordinary values.  An entry is a SUM over its epoch's workers, so
# it is larger than one worker's gradient; at this scale the correction lam * x * (theta_now -
# theta_src) is comparable to x, so that fusing the last product into the add (one rounding
# instead of two) changes the rounded result in a good share of the elements -- enough for tensors
# of a thousand elements to tell a contracting compiler from the text.  The tests assert that.
COMP_SCALE = 300.0


def compensate(x, theta_now, theta_src, lam):
    return x + (x * x) * lam * (theta_now - theta_src)


def rule(ups_list):
    return [torch.stack([u[i] for u in ups_list]).mean(0) for i in range(len(ups_list[0]))]


def weighted_rule(ups_list, weights, normalize="weights"):
    W = float(sum(weights)) if normalize == "weights" else float(len(ups_list))
    return [torch.stack([x[i] * w for x, w in zip(ups_list, weights)]).sum(0) / W
            for i in range(len(ups_list[0]))]


def compensated_rule(ups_list, snaps, theta_now, lam, weights=None, normalize="weights"):
    # snaps[j] is None for an entry that is this epoch's S_t (no compensation), else theta_src of j
    ys = [u if s is None else [compensate(u[i], theta_now[i], s[i], lam) for i in range(len(u))]
          for u, s in zip(ups_list, snaps)]
    return rule(ys) if weights is None else weighted_rule(ys, weights, normalize)


def compensate_contracted(x, theta_now, theta_src, lam):
    """What a compiler that contracts the last product into the add would give: x*x, times
    f32(lam) and the difference rounded to fp32 as in the text, then fma(h, d, x) with ONE rounding
    (emulated in float64: the product of two fp32 values is exact there)."""
    x, p, th = (np.asarray(a, np.float32) for a in (x, theta_now, theta_src))
    with np.errstate(all="ignore"):
        h = ((x * x) * np.float32(lam)).astype(np.float32)
        d = (p - th).astype(np.float32)
        return (x.astype(np.float64) + h.astype(np.float64) * d.astype(np.float64)).astype(
            np.float32)


def split(flat, sizes):
    out, off = [], 0
    for n in sizes:
        out.append(torch.from_numpy(flat[off:off + n]))
        off += n
    return out


def values_S(rs, n, scale=1e-2):
    """S_t: gradient-like values with the edge cases +-0, subnormals, +-1e30, 1.2e-38."""
    v = (rs.standard_normal(n) * scale).astype(np.float32)
    v[::17] = 0.0
    v[1::17] = -0.0
    v[2::17] = np.float32(3e-39) * rs.choice([-1, 1], len(v[2::17]))
    v[3::17] = np.float32(1e30) * rs.choice([-1, 1], len(v[3::17]))
    v[4::17] = np.float32(1.2e-38) * rs.choice([-1, 1], len(v[4::17]))
    return v


def values_comp(rs, n, scale=COMP_SCALE):
    """A compensated array: the same edge values with +-1e15 in the +-1e30 lane (x*x finite)."""
    v = values_S(rs, n, scale)
    v[3::17] = np.float32(1e15) * rs.choice([-1, 1], len(v[3::17]))
    return v


def theta_src(rs, now):
    """A snapshot: theta_now + noise of about 1e-3, every fifth element equal to theta_now (the
    d = 0 case)."""
    src = (now + (rs.standard_normal(now.size) * 1e-3).astype(np.float32)).astype(np.float32)
    src[::5] = now[::5]
    return src


def theta_pair(rs, n):
    """(theta_now, a snapshot of it).  theta is small next to g so that plain SGD with lr = 1
    (theta - g) keeps g's low bits."""
    now = (rs.standard_normal(n) * 1e-3).astype(np.float32)
    return now, theta_src(rs, now)


def text_flat(entries, snaps, theta_now, lam, full, sizes, normalize="weights", comp=compensate):
    """The text over flat numpy entries (entries[j], snaps[j] or None per weight_ups entry), per
    tensor -> flat g.  full: the k weights, or None (the plain mean).  comp: the compensation
    (compensate, or compensate_contracted for the input-condition checks)."""
    th = split(theta_now, sizes)
    ups = []
    for e, s in zip(entries, snaps):
        u = split(e, sizes)
        if s is not None:
            ss = split(s, sizes)
            u = [torch.as_tensor(comp(u[i], th[i], ss[i], lam)) for i in range(len(u))]
        ups.append(u)
    g = rule(ups) if full is None else weighted_rule(ups, full, normalize)
    return torch.cat(g).numpy()


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def input_conditions(g, g_plain, g_contracted):
    """(g is finite everywhere; share of elements compensation changes; elements where the
    contracted evaluation differs from the text)."""
    return (bool(np.isfinite(g).all()), float((bits(g) != bits(g_plain)).mean()),
            int((bits(g) != bits(g_contracted)).sum()))
