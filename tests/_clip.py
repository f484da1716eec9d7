"""Shared by tests/test_cpu_clip.py and tests/test_gpu_clip.py: the text of global-norm clipping in
the server step (include/flsim.h), evaluated with torch and numpy on the CPU.

    total_norm = float32(sqrt(sum_e float64(g_e) ** 2))          # the correctly rounded norm
    coef       = clamp(max_norm / (total_norm + 1e-6), max=1.0)  # torch: reciprocal() * max_norm
    g'         = g * coef                                        # clip_grads_with_norm_

Everything after the norm is torch's own torch.nn.utils.clip_grads_with_norm_.  The norm is not
torch's: get_total_norm accumulates the squares in fp32 and lands up to 1e-4 relative below the
exact value on a layout of millions of elements.
"""
import ctypes
import math

import numpy as np
import torch

# the smallest relative distance of the exact norm to an fp32 rounding midpoint the tests accept:
# any fp64 summation order (error of the order of 1e-16 per add, far below this) then rounds to
# the same fp32
MIN_MIDPOINT_DISTANCE = 1e-10
vp = ctypes.c_void_p


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def exact_norm(g):
    """(the exact 2-norm of fp32 g as a double, its fp32 rounding, the relative distance of the
    exact value to the nearer fp32 rounding midpoint)."""
    g64 = np.asarray(g, np.float32).astype(np.float64)
    exact = math.sqrt(math.fsum(g64 * g64))
    f = np.float32(exact)
    up = np.nextafter(f, np.float32(np.inf))
    dn = np.nextafter(f, np.float32(-np.inf))
    mids = [(float(f) + float(up)) / 2.0, (float(f) + float(dn)) / 2.0]
    dist = min(abs(exact - mid) for mid in mids) / exact if exact > 0 else float("inf")
    return exact, f, dist


def torch_coef(total_norm, max_norm):
    """torch's coefficient for an fp32 norm, as clip_grads_with_norm_ computes it; also asserts
    what the kernels rely on: torch's `max_norm / tensor` is reciprocal() * max_norm."""
    t = torch.tensor(np.float32(total_norm))
    coef = torch.clamp(max_norm / (t + 1e-6), max=1.0)
    spelled = torch.clamp((t + 1e-6).reciprocal() * max_norm, max=1.0)
    assert coef.dtype == torch.float32
    assert bits(coef.numpy()) == bits(spelled.numpy()) or (coef != coef and spelled != spelled)
    return np.float32(coef.item())


def torch_clip(g, sizes, max_norm, total_norm):
    """g' = torch.nn.utils.clip_grads_with_norm_ on per-tensor parameters whose .grad are the
    pieces of the flat g, with the given fp32 total_norm.  -> flat fp32 g'."""
    g = np.asarray(g, np.float32)
    params, off = [], 0
    for n in sizes:
        p = torch.nn.Parameter(torch.zeros(n))
        p.grad = torch.from_numpy(g[off:off + n].copy())
        params.append(p)
        off += n
    torch.nn.utils.clip_grads_with_norm_(params, max_norm, torch.tensor(np.float32(total_norm)))
    return torch.cat([p.grad for p in params]).numpy()


def has_negative_zero(a):
    a = np.asarray(a, np.float32)
    return bool(((a == 0) & np.signbit(a)).any())


def values(rs, n, scale=1e-2):
    """Gradient-like values without zeros of either sign (a k = 1 rule would turn -0 into +0): a
    normal body with subnormal and near-subnormal lanes."""
    v = (rs.standard_normal(n) * scale).astype(np.float32)
    v[v == 0] = np.float32(scale)
    v[2::17] = np.float32(3e-39) * rs.choice([-1, 1], len(v[2::17]))
    v[4::17] = np.float32(1.2e-38) * rs.choice([-1, 1], len(v[4::17]))
    return v


def split(flat, sizes):
    out, off = [], 0
    for n in sizes:
        out.append(flat[off:off + n])
        off += n
    return out


def arrs(arrays):
    return (vp * max(1, len(arrays)))(*[(a.ctypes.data if a is not None else None)
                                        for a in arrays])


def existing_twin(words, info, S, arrays, w, divisor, theta_now, snaps, lam, tail):
    """g of the twins that tests/test_cpu_stale_weight.py and test_cpu_delay_comp.py pin to torch."""
    from flsim import _lib
    L = _lib.lib()
    n, na = S.size, len(arrays)
    out = np.empty(n, np.float32)
    a = (words.ctypes.data_as(vp), info.ctypes.data_as(vp), S.ctypes.data_as(vp), arrs(arrays))
    t = tail.astype(np.uint8)
    if w is None and snaps is None:
        rc = L.flsim_cascade_eval_host(*a, na, t.ctypes.data_as(vp), n, out.ctypes.data_as(vp))
        out = (out / np.float32(divisor)).astype(np.float32)
    else:
        cw = (ctypes.c_double * max(1, na))(*w) if w is not None else None
        rc = L.flsim_cascade_eval_host_c(
            *a, cw, na, float(divisor), theta_now.ctypes.data_as(vp),
            arrs(snaps) if snaps is not None else None, float(lam), t.ctypes.data_as(vp), n,
            out.ctypes.data_as(vp))
    assert rc == 0, L.flsim_last_error()
    return out


def tail_mask(sizes, weighted):
    m = []
    for n in sizes:
        body = (n // 4 * 4) if (weighted and n < 8) else n // 32 * 32
        m.append(np.arange(n) >= body)
    return np.concatenate(m)
