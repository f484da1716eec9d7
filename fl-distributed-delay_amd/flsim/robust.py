"""Robust aggregation rules in plain torch: the coordinate-wise median and the beta-trimmed mean
(Yin et al. 2018), usually run over bucket means of the workers ("bucketing", Karimireddy et al.
2022).  They run on any device and are usable as Agg(rule) through the FL.agents facade, where
they stay unfused like any custom rule.  This text is the yardstick of the fused HIP step
(flsim_robust_optim_step, include/flsim.h) and of its host twin: both equal it as numbers -- the
same 32 bits wherever the text's value is neither zero nor NaN, a zero where it gives a zero, a
NaN where it gives a NaN.

    Agg(median_rule)                                  # the lower median of the workers' updates
    Agg(lambda ups: trimmed_mean_rule(ups, trim=1))   # drop the lowest and the highest, average
    Agg(lambda ups: krum_rule(ups, f=1))              # the update closest to its neighbours
    Agg(lambda ups: multi_krum_rule(ups, f=1, m=3))   # the mean of the three closest
"""
from __future__ import annotations

import torch

KINDS = ("median", "trimmed_mean")


def _robust(cols, kind, trim):             # cols: [k, numel] fp32, already bucket means
    k = cols.shape[0]
    s = cols.sort(0).values                # ascending; torch puts NaN last
    if kind == "median":
        return s[(k - 1) // 2].clone()     # lower median (= torch.median when there is no NaN)
    xs = s[trim:k - trim]                  # trimmed mean: drop `trim` lowest and `trim` highest
    acc = xs[0].clone()
    for r in xs[1:]:                       # sequential fp32 adds, ascending order
        acc += r
    return acc / (k - 2 * trim)            # one IEEE fp32 division


def check(kind, trim, k):
    """The cases the library refuses (ValueError), and rule()'s IndexError on an empty list.
    For "krum" / "multi_krum" `trim` is the pair (f, m), and (f, m) is returned."""
    if kind in KRUM_KINDS:
        return check_krum(trim[0], trim[1], k)
    if kind not in KINDS:
        raise ValueError(f"robust rule {kind!r} (supported: {KINDS})")
    if k == 0:
        raise IndexError("empty weight_ups (reference: IndexError in rule, main.py:25)")
    trim = int(trim)
    if trim < 0 or 2 * trim >= k:
        raise ValueError(f"Invalid trim {trim} for k = {k} entries: 0 <= 2 * trim < k")
    if kind == "median" and trim != 0:
        raise ValueError(f"the median takes no trim (trim = {trim})")
    return trim


def _per_tensor(ups_list, kind, trim):
    trim = check(kind, trim, len(ups_list))
    out = []
    for i in range(len(ups_list[0])):
        cols = torch.stack([u[i].reshape(-1) for u in ups_list])
        out.append(_robust(cols, kind, trim).view(ups_list[0][i].shape))
    return out


def median_rule(ups_list):
    """rule() with the coordinate-wise lower median in place of the mean: ups_list is the list of
    per-worker (or per-bucket) updates, each a list of per-parameter tensors."""
    return _per_tensor(ups_list, "median", 0)


def trimmed_mean_rule(ups_list, trim):
    """rule() with the coordinate-wise trimmed mean: per coordinate the `trim` lowest and the `trim`
    highest values are dropped, the rest averaged (2 * trim < len(ups_list))."""
    return _per_tensor(ups_list, "trimmed_mean", trim)


def bucket_means(sums, counts):
    """Bucket sums -> bucket means: fp32 IEEE division by the integer n."""
    return [s / n for s, n in zip(sums, counts)]


def robust_flat(entries, counts, kind, trim=0):
    """The text over flat bucket SUMS (1-d fp32 tensors; None = an all-zero entry) with their
    counts: what flsim_robust_optim_step computes as g."""
    ref = next(e for e in entries if e is not None)
    sums = [torch.zeros_like(ref) if e is None else e for e in entries]
    trim = check(kind, trim, len(sums))
    return _robust(torch.stack(bucket_means(sums, counts)), kind, trim)


# ---- Krum and Multi-Krum (Blanchard et al. 2017): not coordinate-wise, the distances are over the
# whole model.  The yardstick of flsim_krum_optim_step (include/flsim.h) and of its host twin:
# dist within 2 (P + 2) 2^-53 relative, score within twice that, the selection equal, g bit for bit.
KRUM_KINDS = ("krum", "multi_krum")


def krum_select(cols, f, m):                 # cols: [k, numel] fp32, already bucket means
    k = cols.shape[0]
    x = cols.double()
    d = torch.stack([((x[i] - x) ** 2).sum(1) for i in range(k)])      # fp64, exactly symmetric
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    score = []
    for i in range(k):
        row = torch.cat([d[i, :i], d[i, i + 1:]]).sort().values[:k - f - 2]
        acc = row[0].clone()
        for r in row[1:]:                    # ascending, sequential fp64 adds
            acc += r
        score.append(acc)
    order = sorted(range(k), key=lambda i: (score[i].item(), i))       # ties: lowest index
    return d, torch.stack(score), sorted(order[:m])                    # selection in index order


def _krum(cols, f, m):
    _, _, sel = krum_select(cols, f, m)
    acc = cols[sel[0]].clone()
    for j in sel[1:]:                        # sequential fp32 adds, ascending entry index
        acc += cols[j]
    return acc / m                           # one IEEE fp32 division (m = 1: the entry itself)


def check_krum(f, m, k):
    """The cases the library refuses (ValueError), and rule()'s IndexError on an empty list."""
    f, m = int(f), int(m)
    if k == 0:
        raise IndexError("empty weight_ups (reference: IndexError in rule, main.py:25)")
    if f < 0 or k < 2 * f + 3:
        raise ValueError(f"Invalid f = {f} for k = {k} entries: f >= 0 and k >= 2 * f + 3")
    if m < 1 or m > k - f:
        raise ValueError(f"Invalid m = {m} for k = {k} entries and f = {f}: 1 <= m <= k - f")
    return f, m


def multi_krum_rule(ups_list, f, m):
    """rule() with Multi-Krum: the mean of the m updates closest to their k - f - 2 nearest
    neighbours, over all tensors flattened together (the distances are over the whole model)."""
    f, m = check_krum(f, m, len(ups_list))
    cols = torch.stack([torch.cat([u.reshape(-1) for u in ups]) for ups in ups_list])
    g = _krum(cols, f, m)
    out, off = [], 0
    for u in ups_list[0]:
        out.append(g[off:off + u.numel()].view(u.shape))
        off += u.numel()
    return out


def krum_rule(ups_list, f):
    """rule() with Krum: the one update closest to its neighbours (Multi-Krum with m = 1)."""
    return multi_krum_rule(ups_list, f, 1)


def krum_flat(entries, counts, f, m=1):
    """The text over flat bucket SUMS (None = an all-zero entry) with their counts: what
    flsim_krum_optim_step computes.  Returns (g, dist, score, sel)."""
    ref = next(e for e in entries if e is not None)
    sums = [torch.zeros_like(ref) if e is None else e for e in entries]
    f, m = check_krum(f, m, len(sums))
    cols = torch.stack(bucket_means(sums, counts))
    d, score, sel = krum_select(cols, f, m)
    return _krum(cols, f, m), d, score, sel


def parse_rule(spec):
    """FLSimulation's robust_rule argument -> (kind, trim): None, "median", "trimmed_mean" (trim
    0), or ("trimmed_mean", trim); or ("krum", f) -> ("krum", f, 1) and ("multi_krum", f, m) as
    it stands (f has no default: the bare strings are refused)."""
    if spec is None or spec == "none":
        return None
    if isinstance(spec, str):
        spec = (spec,)
    spec = tuple(spec)
    kind = spec[0]
    if kind in KRUM_KINDS:
        if len(spec) != (2 if kind == "krum" else 3):
            raise ValueError(f"robust_rule {spec!r} (supported: ('krum', f), ('multi_krum', f, m))")
        f, m = int(spec[1]), (1 if kind == "krum" else int(spec[2]))
        if f < 0 or m < 1:
            raise ValueError(f"robust_rule {spec!r}: f must be >= 0 and m >= 1")
        return kind, f, m
    if kind not in KINDS or len(spec) > 2:
        raise ValueError(f"robust_rule {spec!r} (supported: None, 'median', ('trimmed_mean', trim), "
                         "('krum', f), ('multi_krum', f, m))")
    trim = int(spec[1]) if len(spec) == 2 else 0
    if trim < 0 or (kind == "median" and trim != 0):
        raise ValueError(f"robust_rule {spec!r}: trim must be >= 0, and 0 for the median")
    return kind, trim
