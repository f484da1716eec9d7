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
    Agg(lambda ups: bulyan_rule(ups, f=1))            # Krum repeated, then a mean around the median
    Agg(CenteredClip(tau=10.0, iters=1))              # centered clipping; the object keeps its center
    Agg(NNM(median_rule, f=1))                        # nearest-neighbour mixing, then any rule
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


# ---- Bulyan (El Mhamdi, Guerraoui and Rouault 2018): Krum's selection repeated until theta =
# k - 2f entries are chosen, then per coordinate the mean of the beta = theta - 2f values closest to
# the median of the chosen ones.  The yardstick of flsim_bulyan_optim_step (include/flsim.h) and of
# its host twin, stage by stage at the device's own outputs: dist within 2 (P + 2) 2^-53 relative;
# order, the winning scores (bit for bit) and sel equal to bulyan_order on that dist; g equal to
# _bulyan_coord over that sel as numbers.
BULYAN_KIND = "bulyan"


def bulyan_order(d, f):
    """d: [k, k] fp64 distance matrix, symmetric, zero diagonal, no NaN (NaN -> +inf), as
    krum_select / pair_matrix form it.  theta = k - 2f rounds; in a round with r entries left, the
    score of a remaining i is the sum of its n = max(r - f - 2, 1) smallest distances to the OTHER
    remaining entries, added in ascending (value, index) order, sequential fp64 adds; the lowest
    (score, index) wins and is removed.  r == 1 (only when f == 0): the one left wins, score 0.0.
    -> (order: theta indices in round order, win: theta fp64 winning scores)."""
    k = d.shape[0]
    left = list(range(k))
    order, win = [], []
    for _ in range(k - 2 * f):
        r = len(left)
        if r == 1:
            order.append(left[0])
            win.append(torch.tensor(0.0, dtype=torch.float64))
            break
        n = max(r - f - 2, 1)
        sc = {}
        for i in left:
            row = sorted((d[i, j].item(), j) for j in left if j != i)[:n]
            acc = torch.tensor(row[0][0], dtype=torch.float64)
            for v, _ in row[1:]:
                acc = acc + v
            sc[i] = acc
        w = min(left, key=lambda i: (sc[i].item(), i))
        order.append(w)
        win.append(sc[w])
        left.remove(w)
    return order, torch.stack(win)


def _bulyan_coord(s_cols, f):
    """s_cols: [theta, numel] fp32, the selected bucket means.  Per coordinate: sort ascending (NaN
    last), med = s[(theta-1)//2]; the window starts as {median} and grows beta - 1 times by the
    closer of its two outer neighbours: right iff a right neighbour exists and (no left neighbour
    or (s[hi+1] - med) < (med - s[lo-1]) in fp32; a false compare, ties and NaN included, goes
    left).  g = the window's values added in ascending order, sequential fp32 adds, / float(beta)."""
    th = s_cols.shape[0]
    beta = th - 2 * f
    s = s_cols.sort(0).values
    mi = (th - 1) // 2
    med = s[mi]
    n = s.shape[1]
    lo = torch.full((n,), mi)
    hi = torch.full((n,), mi)
    for _ in range(beta - 1):
        lok, rok = lo > 0, hi < th - 1
        dl = med - s.gather(0, (lo - 1).clamp(min=0)[None])[0]
        dr = s.gather(0, (hi + 1).clamp(max=th - 1)[None])[0] - med
        right = rok & (~lok | (dr < dl))
        hi = torch.where(right, hi + 1, hi)
        lo = torch.where(right, lo, lo - 1)
    acc = torch.zeros(n)
    started = torch.zeros(n, dtype=torch.bool)
    for p in range(th):
        inw = (p >= lo) & (p <= hi)
        acc = torch.where(inw, torch.where(started, acc + s[p], s[p]), acc)
        started |= inw
    return acc / beta


def check_bulyan(f, k):
    """The cases the library refuses (ValueError), and rule()'s IndexError on an empty list."""
    f = int(f)
    if k == 0:
        raise IndexError("empty weight_ups (reference: IndexError in rule, main.py:25)")
    if f < 0 or k < 4 * f + 3:
        raise ValueError(f"Invalid f = {f} for k = {k} entries: f >= 0 and k >= 4 * f + 3")
    return f


def _bulyan(cols, f):
    """cols [k, numel] fp32 (bucket means) -> (g, dist, order, win, sel)."""
    d, _, _ = krum_select(cols, 0, 1)        # (the distances alone: Krum's f and m play no part)
    order, win = bulyan_order(d, f)
    sel = sorted(order)
    return _bulyan_coord(cols[sel], f), d, order, win, sel


def bulyan_flat(entries, counts, f):
    """The text over flat bucket SUMS (None = an all-zero entry) with their counts: what
    flsim_bulyan_optim_step computes.  Returns (g, dist, order, win, sel), sel = sorted(order)."""
    ref = next(e for e in entries if e is not None)
    sums = [torch.zeros_like(ref) if e is None else e for e in entries]
    f = check_bulyan(f, len(sums))
    return _bulyan(torch.stack(bucket_means(sums, counts)), f)


def bulyan_rule(ups_list, f):
    """rule() with Bulyan: Krum's selection repeated until len(ups_list) - 2f updates are chosen,
    then per coordinate the mean of the len(ups_list) - 4f values closest to the median of the
    chosen ones, over all tensors flattened together (the distances are over the whole model)."""
    f = check_bulyan(f, len(ups_list))
    cols = torch.stack([torch.cat([u.reshape(-1) for u in ups]) for ups in ups_list])
    g = _bulyan(cols, f)[0]
    out, off = [], 0
    for u in ups_list[0]:
        out.append(g[off:off + u.numel()].view(u.shape))
        off += u.numel()
    return out


# ---- Nearest-neighbour mixing (NNM; Allouah et al. 2023, "Fixing by Mixing"): a pre-aggregation
# stage, not a rule.  Every entry is replaced by the mean of its k - f nearest entries, itself
# included, and any rule then runs over the mixed entries (count 1 each).  The distances are
# Krum's, over the whole model.  The yardstick of flsim_nnm_entries (include/flsim.h) and of its
# host twin: dist within 2 (P + 2) 2^-53 relative, nbr equal wherever the text's cut is wider than
# that, and given equal nbr the mixed entries equal _nnm as numbers.
def nnm_neighbours(cols, f):                 # cols: [k, numel] fp32, already bucket means
    k = cols.shape[0]
    x = cols.double()
    d = torch.stack([((x[i] - x) ** 2).sum(1) for i in range(k)])      # fp64, exactly symmetric
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    # an entry is always its own nearest neighbour, even one that holds a NaN (whose distance to
    # itself is NaN -> +inf above): it keeps itself among its neighbours and stays NaN, and the
    # rule behind treats it as it treats any poisoned entry.  Every other row sees it at +inf,
    # hence last.
    d.fill_diagonal_(0.0)
    nbr = []
    for i in range(k):
        order = sorted(range(k), key=lambda j: (d[i, j].item(), j))    # ties: lowest index
        nbr.append(sorted(order[:k - f]))    # the k - f nearest, in index order; i is among them
    return d, nbr


def _nnm(cols, f):
    _, nbr = nnm_neighbours(cols, f)
    out = []
    for i in range(cols.shape[0]):
        acc = cols[nbr[i][0]].clone()
        for j in nbr[i][1:]:                 # sequential fp32 adds, ascending entry index
            acc += cols[j]
        out.append(acc / (cols.shape[0] - f))    # one IEEE fp32 division
    return torch.stack(out)


def check_nnm(f, k):
    """The cases the library refuses (ValueError), and rule()'s IndexError on an empty list."""
    f = int(f)
    if k == 0:
        raise IndexError("empty weight_ups (reference: IndexError in rule, main.py:25)")
    if f < 0 or 2 * f >= k:
        raise ValueError(f"Invalid NNM f = {f} for k = {k} entries: f >= 0 and 2 * f < k")
    return f


def nnm_flat(entries, counts, f):
    """The text over flat bucket SUMS (None = an all-zero entry) with their counts: what
    flsim_nnm_entries computes.  Returns (mixed [k, P] fp32, dist [k, k] fp64, nbr: k lists)."""
    ref = next(e for e in entries if e is not None)
    sums = [torch.zeros_like(ref) if e is None else e for e in entries]
    f = check_nnm(f, len(sums))
    cols = torch.stack(bucket_means(sums, counts))
    d, nbr = nnm_neighbours(cols, f)
    return _nnm(cols, f), d, nbr


class NNM:
    """Nearest-neighbour mixing in front of any rule, as a rule: NNM(median_rule, f=1)(ups_list).
    All tensors are flattened together (the distances are over the whole model), the k updates are
    mixed, un-flattened into k per-parameter lists and handed to `rule`."""

    def __init__(self, rule, f):
        self.rule, self.f = rule, int(f)
        if self.f < 0:
            raise ValueError(f"Invalid NNM f = {self.f}: it must be >= 0")

    def __call__(self, ups_list):
        f = check_nnm(self.f, len(ups_list))
        cols = torch.stack([torch.cat([u.reshape(-1) for u in ups]) for ups in ups_list])
        mixed = _nnm(cols, f)
        out = []
        for row in mixed:
            ups, off = [], 0
            for u in ups_list[0]:
                ups.append(row[off:off + u.numel()].view(u.shape))
                off += u.numel()
            out.append(ups)
        return self.rule(out)


# ---- the geometric median by smoothed Weiszfeld iterations ("RFA", Pillutla, Kakade and Harchaoui
# 2022): breakdown point 1/2, no Byzantine count from the user; the entries are re-weighted
# continuously by 1 / distance to the iterate.  The yardstick of flsim_geomed_optim_step
# (include/flsim.h) and of its host twin, stage by stage at the device's own inputs: d2[r] within
# 2 (P + 2) 2^-53 relative of the distances at w[r]; w[r + 1], obj[r] (geomed_scalar on d2[r]) and
# g (_wsum at w[iters]) bit for bit.
GEOMED_KIND = "geomed"
GEOMED_WEIGHTS = ("uniform", "count")
GEOMED_MAX_ITERS = 32


def _seqsum(v):                              # sequential fp64 adds, index order
    acc = v[0].clone()
    for t in v[1:]:
        acc = acc + t
    return acc


def _wsum(x, w):
    """z = sum_j w[j] * x[j]: fp64, index order, one multiply and one add per term (two roundings,
    never an fma); terms with w[j] == 0 are skipped (not read); the first term kept initialises
    the sum."""
    z = None
    for j in range(x.shape[0]):
        if w[j] == 0:
            continue
        t = x[j] * w[j]
        z = t if z is None else z + t
    return torch.zeros_like(x[0]) if z is None else z


def _sqrt_rn(v):
    """The correctly rounded fp64 square root of a small 1-d tensor, element by element
    (math.sqrt: torch's vectorised CPU sqrt is 1 ulp off for some inputs on some machines)."""
    import math
    return torch.tensor([math.sqrt(t) for t in v.tolist()], dtype=torch.float64, device=v.device)


def geomed_scalar(d2_r, a, alive, nu):
    """One iteration's scalar code from the squared distances (dead: +inf) -> (obj, next w)."""
    d = _sqrt_rn(d2_r)
    live = [j for j in range(len(a)) if alive[j]]
    obj = _seqsum((a * d)[live]) if live else torch.tensor(float("nan"), dtype=torch.float64)
    beta = a / torch.maximum(d, torch.tensor(nu, dtype=torch.float64))  # dead: 0 / inf = 0
    return obj, beta / _seqsum(beta)


def geomed_dist2(x, w_r, alive):
    """The squared distances of the entries x [k, numel] fp64 to z = _wsum(x, w_r); dead: +inf."""
    z = _wsum(x, w_r)
    d2_r = ((x - z) ** 2).sum(1)
    d2_r[~alive] = float("inf")
    return d2_r


def geomed_steps(cols, alpha, iters, nu):    # cols [k, numel] fp32 (bucket means), alpha [k] fp64 > 0
    x = cols.double()
    alive = torch.isfinite(x).all(1)         # an entry with any NaN / inf element is dead
    a = torch.where(alive, alpha, torch.zeros_like(alpha))
    # (not alive.any(): a / 0 below is NaN throughout, and so is g)
    w = [a / _seqsum(a)]                     # w^(0): z_0 is the alpha-weighted mean of the live entries
    d2, obj = [], []
    for r in range(iters):
        d2_r = geomed_dist2(x, w[r], alive)
        o, w_next = geomed_scalar(d2_r, a, alive, nu)
        obj.append(o)                        # sum_j alpha_j ||x_j - z_r||
        w.append(w_next)                     # the smoothed Weiszfeld weights, normalised
        d2.append(d2_r)
    g = _wsum(x, w[iters]).float()           # one fp64 -> fp32 rounding
    return g, w, d2, obj


def check_geomed(iters, nu, weights, k):
    """The cases the library refuses (ValueError), and rule()'s IndexError on an empty list.
    Returns (iters, nu, weights) with weights None -> "uniform"."""
    import math
    if k == 0:
        raise IndexError("empty weight_ups (reference: IndexError in rule, main.py:25)")
    iters, nu = int(iters), float(nu)
    weights = "uniform" if weights is None else weights
    if iters < 0 or iters > GEOMED_MAX_ITERS:
        raise ValueError(f"Invalid iters = {iters}: 0 <= iters <= {GEOMED_MAX_ITERS}")
    if not (math.isfinite(nu) and nu > 0):
        raise ValueError(f"Invalid nu = {nu}: it must be finite and > 0")
    if weights not in GEOMED_WEIGHTS:
        raise ValueError(f"Invalid weights {weights!r} (supported: {GEOMED_WEIGHTS})")
    return iters, nu, weights


def geomed_rule(ups_list, iters=3, nu=1e-6, weights=None):
    """rule() with the geometric median of the updates (`iters` smoothed Weiszfeld iterations from
    their mean), over all tensors flattened together.  weights: None (uniform) or a sequence of
    positive per-update weights (RFA's sample counts)."""
    alpha = None
    if weights is not None and not isinstance(weights, str):
        alpha = torch.as_tensor(list(weights), dtype=torch.float64)
        if alpha.numel() != len(ups_list) or not bool((alpha > 0).all()):
            raise ValueError("weights: one positive weight per update")
        weights = "count"
    iters, nu, _ = check_geomed(iters, nu, weights, len(ups_list))
    if alpha is None:
        alpha = torch.ones(len(ups_list), dtype=torch.float64)
    cols = torch.stack([torch.cat([u.reshape(-1) for u in ups]) for ups in ups_list])
    g = geomed_steps(cols, alpha, iters, nu)[0]
    out, off = [], 0
    for u in ups_list[0]:
        out.append(g[off:off + u.numel()].view(u.shape))
        off += u.numel()
    return out


def geomed_alpha(counts, weighted):
    return torch.tensor([float(c) if weighted else 1.0 for c in counts], dtype=torch.float64)


def geomed_flat(entries, counts, iters=3, nu=1e-6, weighted=False):
    """The text over flat bucket SUMS (None = an all-zero entry) with their counts: what
    flsim_geomed_optim_step computes.  Returns (g, w, d2, obj): w iters + 1 tensors [k], d2 iters
    tensors [k], obj iters scalars."""
    iters, nu, _ = check_geomed(iters, nu, "count" if weighted else "uniform", len(entries))
    ref = next(e for e in entries if e is not None)
    sums = [torch.zeros_like(ref) if e is None else e for e in entries]
    cols = torch.stack(bucket_means(sums, counts))
    return geomed_steps(cols, geomed_alpha(counts, weighted), iters, nu)


# ---- centered clipping with a carried center ("CClip", Karimireddy, He and Jaggi 2021: "Learning
# from History for Byzantine Robust Optimization"): every entry is pulled towards the iterate with
# weight min(1, tau / distance), and the first iterate is the previous epoch's aggregate, so the
# rule has memory across epochs.  The iterate v_l = v_(l-1) + sum_j lam_j s_j (x_j - v_(l-1)) is
# never formed: it is the affine combination u_l * c + sum_j w_l[j] * x_j of the center and the
# entries.  The yardstick of flsim_cclip_optim_step (include/flsim.h) and of its host twin, stage by
# stage at the device's own inputs: d2[r] within 2 (P + 2) 2^-53 relative of the distances at
# (u[r], w[r]); s[r], u[r + 1], w[r + 1] (cclip_scalar on d2[r]) and g bit for bit.  fp64
# throughout, one rounding per operation, never an fma.
CCLIP_KIND = "cclip"
CCLIP_WEIGHTS = GEOMED_WEIGHTS
CCLIP_MAX_ITERS = 32


def _cclip_z(x, c, u_r, w_r):
    """u_r * c + sum_j w_r[j] * x[j] as _wsum forms it: the center's term first, then the entries
    in index order; c is None (fresh): no center term."""
    z = None
    if c is not None and u_r != 0:           # (_wsum's rule for the center's term)
        z = c * u_r
    for j in range(x.shape[0]):
        if w_r[j] == 0:
            continue
        t = x[j] * w_r[j]
        z = t if z is None else z + t
    return torch.zeros_like(x[0]) if z is None else z


def cclip_dist2(x, c, u_r, w_r, alive):
    """The squared distances of the entries x [k, numel] fp64 to the iterate of weights
    (u_r, w_r); dead: +inf."""
    z = _cclip_z(x, c, u_r, w_r)
    d2_r = ((x - z) ** 2).sum(1)
    d2_r[~alive] = float("inf")
    return d2_r


def cclip_scalar(d2_r, a, alive, tau, u_r, w_r):
    """One iteration's scalar code from the squared distances (dead: +inf) -> (s, u_next, w_next)."""
    d = _sqrt_rn(d2_r)
    q = torch.tensor(tau, dtype=torch.float64) / d           # d = 0: +inf
    one = torch.ones_like(q)
    s = torch.where(q < 1, q, torch.where(q >= 1, one, q))   # min(1, q); a NaN q stays
    s[~alive] = 0.0
    # (no entry alive: lam = 0, not 0 / 0: g is the center, "keep the last aggregate")
    lam = a / _seqsum(a) if bool(alive.any()) else torch.zeros_like(a)
    t = lam * s
    om = 1.0 - _seqsum(t)
    return s, u_r * om, w_r * om + t                         # a multiply, then an add


def cclip_steps(cols, center, alpha, iters, tau):
    """cols [k, numel] fp32 (bucket means), center [numel] fp32 or None (fresh: all zero),
    alpha [k] fp64 > 0 -> (g, u, w, d2, s): u iters + 1 scalars, w iters + 1 tensors [k], d2 and
    s iters tensors [k].  The next step's center is g."""
    x = cols.double()
    c = None if center is None else center.double()
    alive = torch.isfinite(x).all(1)         # an entry with any NaN / inf element is dead
    a = torch.where(alive, alpha, torch.zeros_like(alpha))
    u = [torch.tensor(1.0, dtype=torch.float64)]             # v_0 = c
    w = [torch.zeros(x.shape[0], dtype=torch.float64)]
    d2, s = [], []
    for r in range(iters):
        d2_r = cclip_dist2(x, c, u[r], w[r], alive)
        s_r, u_next, w_next = cclip_scalar(d2_r, a, alive, tau, u[r], w[r])
        d2.append(d2_r)
        s.append(s_r)
        u.append(u_next)
        w.append(w_next)
    g = _cclip_z(x, c, u[iters], w[iters]).float()           # one fp64 -> fp32 rounding
    return g, u, w, d2, s


def check_cclip(iters, tau, weights, k):
    """The cases the library refuses (ValueError), and rule()'s IndexError on an empty list.
    Returns (iters, tau, weights) with weights None -> "uniform"."""
    import math
    if k == 0:
        raise IndexError("empty weight_ups (reference: IndexError in rule, main.py:25)")
    iters, tau = int(iters), float(tau)
    weights = "uniform" if weights is None else weights
    if iters < 1 or iters > CCLIP_MAX_ITERS:
        raise ValueError(f"Invalid iters = {iters}: 1 <= iters <= {CCLIP_MAX_ITERS}")
    if not (math.isfinite(tau) and tau > 0):
        raise ValueError(f"Invalid tau = {tau}: it must be finite and > 0")
    if weights not in CCLIP_WEIGHTS:
        raise ValueError(f"Invalid weights {weights!r} (supported: {CCLIP_WEIGHTS})")
    return iters, tau, weights


def cclip_flat(entries, counts, center, tau, iters=1, weighted=False):
    """The text over flat bucket SUMS (None = an all-zero entry) with their counts and the center
    (None: fresh): what flsim_cclip_optim_step computes.  Returns (g, u, w, d2, s)."""
    iters, tau, _ = check_cclip(iters, tau, "count" if weighted else "uniform", len(entries))
    ref = next(e for e in entries if e is not None)
    sums = [torch.zeros_like(ref) if e is None else e for e in entries]
    cols = torch.stack(bucket_means(sums, counts))
    return cclip_steps(cols, center, geomed_alpha(counts, weighted), iters, tau)


def cclip_rule(ups_list, center, tau, iters=1, weights=None):
    """rule() with centered clipping of the updates around `center` (a flat fp32 tensor over all
    tensors flattened together, or None: all zero), `iters` iterations.  weights: None (uniform)
    or a sequence of positive per-update weights.  Returns (out_list, new_center_flat): the rule
    is stateful, the caller passes new_center_flat as the next call's center (CenteredClip)."""
    alpha = None
    if weights is not None and not isinstance(weights, str):
        alpha = torch.as_tensor(list(weights), dtype=torch.float64)
        if alpha.numel() != len(ups_list) or not bool((alpha > 0).all()):
            raise ValueError("weights: one positive weight per update")
        weights = "count"
    iters, tau, _ = check_cclip(iters, tau, weights, len(ups_list))
    if alpha is None:
        alpha = torch.ones(len(ups_list), dtype=torch.float64)
    cols = torch.stack([torch.cat([u.reshape(-1) for u in ups]) for ups in ups_list])
    g = cclip_steps(cols, center, alpha, iters, tau)[0]
    out, off = [], 0
    for u in ups_list[0]:
        out.append(g[off:off + u.numel()].view(u.shape))
        off += u.numel()
    return out, g


class CenteredClip:
    """cclip_rule with its center kept between calls, usable as Agg(CenteredClip(tau, iters)): the
    first call clips around zero, every later one around the previous aggregate.  It stays unfused
    like any custom rule."""

    def __init__(self, tau, iters=1, weights=None):
        check_cclip(iters, tau, weights if isinstance(weights, str) or weights is None else "count", 1)
        self.tau, self.iters, self.weights = float(tau), int(iters), weights
        self.center = None

    def __call__(self, ups_list):
        out, self.center = cclip_rule(ups_list, self.center, self.tau, self.iters, self.weights)
        return out


def parse_rule(spec):
    """FLSimulation's robust_rule argument -> (kind, trim): None, "median", "trimmed_mean" (trim
    0), or ("trimmed_mean", trim); or ("krum", f) -> ("krum", f, 1) and ("multi_krum", f, m) as
    it stands (f has no default: the bare strings are refused); or ("bulyan", f) as it stands
    (the bare string is refused, like Krum's); or "geomed", ("geomed", iters),
    ("geomed", iters, nu), ("geomed", iters, nu, "uniform" | "count") -> ("geomed", iters, nu,
    weights), defaults 3, 1e-6, "uniform"; or ("cclip", tau), ("cclip", tau, iters), ("cclip", tau,
    iters, "uniform" | "count") -> ("cclip", tau, iters, weights), defaults 1, "uniform" (tau has
    no default, its scale is the gradients': the bare string is refused)."""
    if spec is None or spec == "none":
        return None
    if isinstance(spec, str):
        spec = (spec,)
    spec = tuple(spec)
    kind = spec[0]
    if kind == CCLIP_KIND:
        if len(spec) < 2 or len(spec) > 4:
            raise ValueError(f"robust_rule {spec!r} (supported: ('cclip', tau), ('cclip', tau, "
                             "iters), ('cclip', tau, iters, 'uniform' | 'count'))")
        try:
            iters, tau, weights = check_cclip(spec[2] if len(spec) > 2 else 1, spec[1],
                                              spec[3] if len(spec) > 3 else None, 1)
        except (TypeError, ValueError) as e:
            raise ValueError(f"robust_rule {spec!r}: {e}") from None
        return kind, tau, iters, weights
    if kind == GEOMED_KIND:
        if len(spec) > 4:
            raise ValueError(f"robust_rule {spec!r} (supported: 'geomed', ('geomed', iters), "
                             "('geomed', iters, nu), ('geomed', iters, nu, 'uniform' | 'count'))")
        try:
            iters, nu, weights = check_geomed(spec[1] if len(spec) > 1 else 3,
                                              spec[2] if len(spec) > 2 else 1e-6,
                                              spec[3] if len(spec) > 3 else None, 1)
        except (TypeError, ValueError) as e:
            raise ValueError(f"robust_rule {spec!r}: {e}") from None
        return kind, iters, nu, weights
    if kind in KRUM_KINDS:
        if len(spec) != (2 if kind == "krum" else 3):
            raise ValueError(f"robust_rule {spec!r} (supported: ('krum', f), ('multi_krum', f, m))")
        f, m = int(spec[1]), (1 if kind == "krum" else int(spec[2]))
        if f < 0 or m < 1:
            raise ValueError(f"robust_rule {spec!r}: f must be >= 0 and m >= 1")
        return kind, f, m
    if kind == BULYAN_KIND:
        if len(spec) != 2:
            raise ValueError(f"robust_rule {spec!r} (supported: ('bulyan', f))")
        f = int(spec[1])
        if f < 0:
            raise ValueError(f"robust_rule {spec!r}: f must be >= 0")
        return kind, f
    if kind not in KINDS or len(spec) > 2:
        raise ValueError(f"robust_rule {spec!r} (supported: None, 'median', ('trimmed_mean', trim), "
                         "('krum', f), ('multi_krum', f, m))")
    trim = int(spec[1]) if len(spec) == 2 else 0
    if trim < 0 or (kind == "median" and trim != 0):
        raise ValueError(f"robust_rule {spec!r}: trim must be >= 0, and 0 for the median")
    return kind, trim


# ---- simulated Byzantine workers: the omniscient attacks the robust rules are measured against.
# IPM (inner-product manipulation, Xie et al. 2020): every Byzantine worker sends -eps * mu.  ALIE
# ("A Little Is Enough", Baruch et al. 2019): every Byzantine worker sends mu - z * sigma.  The
# yardstick of flsim_attack_entries (include/flsim.h) and of its host twin: both equal attack_flat
# as numbers -- the same 32 bits wherever the text's value is neither zero nor NaN, a zero where it
# gives a zero, a NaN where it gives a NaN.
# One limit: the simulator holds bucket SUMS, not per-worker gradients, so mu and sigma are taken
# over the honest-part means of the buckets, unweighted.  With one worker per bucket that is exactly
# the papers' definition; with larger buckets the attacker sees sigma at bucket granularity.  The
# population standard deviation (not the unbiased one) is chosen so that a single honest entry is
# defined (sigma = 0).
ATTACK_KINDS = ("ipm", "alie")


def attack_vector(sums, honest, kind, strength):
    """sums[j]: fp32 [P] sum of bucket j's honest workers (read only where honest[j] >= 1),
    honest[j] >= 0.  fp64 throughout, one rounding per operation, never an fma."""
    y = [sums[j].double() / honest[j] for j in range(len(sums)) if honest[j] >= 1]   # IEEE fp64 division
    kh = len(y)
    mu = _seqsum(y) / kh                               # index order
    if kind == "ipm":
        b = mu * (-strength)
    else:                                              # alie
        var = _seqsum([(t - mu) * (t - mu) for t in y]) / kh      # population variance
        b = mu - _sqrt_rn(var) * strength              # correctly rounded sqrt, multiply, subtract
    return b.float()                                   # one fp64 -> fp32 rounding


def check_attack(kind, strength, honest, byz):
    """The cases the library refuses (ValueError), in its order.  Returns (kind, strength)."""
    import math
    if kind not in ATTACK_KINDS:
        raise ValueError(f"Invalid attack kind {kind!r} (supported: {ATTACK_KINDS})")
    honest, byz = [int(h) for h in honest], [int(b) for b in byz]
    if len(honest) != len(byz):
        raise ValueError(f"{len(byz)} Byzantine counts for {len(honest)} honest counts")
    if not 1 <= len(honest) <= 64:
        raise ValueError(f"attack over k = {len(honest)} entries (1 .. 64)")
    strength = float(strength)
    if not (math.isfinite(strength) and strength >= 0):
        raise ValueError(f"Invalid attack strength = {strength}: it must be finite and >= 0")
    for j, (h, b) in enumerate(zip(honest, byz)):
        if h < 0:
            raise ValueError(f"Invalid honest count {h} of entry {j}: it must be >= 0")
        if b < 0:
            raise ValueError(f"Invalid Byzantine count {b} of entry {j}: it must be >= 0")
        if h + b == 0:
            raise ValueError(f"entry {j} holds no worker: honest + byz must be >= 1")
    if not any(h >= 1 for h in honest):
        raise ValueError("no entry holds an honest worker: the attacker has nothing to observe")
    if not any(b >= 1 for b in byz):
        raise ValueError("no entry holds a Byzantine worker: nothing to attack")
    return kind, strength


def attack_flat(sums, honest, byz, kind, strength):
    """-> (entries, counts, b): entries[j] = sums[j] + b * float(byz[j])   (fp32: a multiply, then an add)
    where honest[j] >= 1 and byz[j] >= 1; b * float(byz[j]) where honest[j] == 0; sums[j] itself
    (same bits) where byz[j] == 0.  counts[j] = honest[j] + byz[j].  sums[j] is not looked at
    where honest[j] == 0 (it may be None).

    mu and sigma are taken over the honest-part means of the entries, unweighted: the simulator
    holds bucket sums, not per-worker gradients.  With one worker per bucket that is the papers'
    definition; with larger buckets the attacker sees sigma at bucket granularity."""
    kind, strength = check_attack(kind, strength, honest, byz)
    b = attack_vector(sums, honest, kind, strength)
    entries = []
    for j in range(len(sums)):
        if byz[j] == 0:
            entries.append(sums[j])
            continue
        t = b * torch.tensor(float(byz[j]), dtype=torch.float32)
        entries.append(sums[j] + t if honest[j] >= 1 else t)
    return entries, [int(h) + int(c) for h, c in zip(honest, byz)], b


def alie_z(n, f):
    """The ALIE paper's default z for n workers of which f are Byzantine: with s = n // 2 + 1 - f
    honest workers to win over, z = the standard normal quantile of (n - s) / n."""
    import statistics
    n, f = int(n), int(f)
    if not (0 < f and 2 * f < n):
        raise ValueError(f"Invalid f = {f} Byzantine of n = {n} workers: 0 < f and 2 * f < n")
    s = n // 2 + 1 - f
    return statistics.NormalDist().inv_cdf((n - s) / n)


# ---- the optimised attacks Min-Max and Min-Sum (Shejwalkar and Houmansadr, NDSS 2021,
# "Manipulating the Byzantine"): b = mu + gamma * p, gamma the largest coefficient at which b stays
# no farther from any honest entry than the honest entries are from each other (Min-Max: the
# largest squared distance; Min-Sum: the largest sum of squared distances).  The inputs, y_j, mu,
# var and the mix are attack_vector's and attack_flat's.  The yardstick of flsim_attack_opt_entries
# (include/flsim.h) and of its host twin: dist, a_i and q within 2 (P + 2) 2^-53 relative, c_i
# within that times sqrt(a_i q) absolute, gamma bit for bit opt_gamma of the device's own a, c, q,
# dist, b and the entries equal as numbers to the text evaluated with the device's gamma.
OPT_ATTACK_KINDS = ("minmax", "minsum")
OPT_ATTACK_DIRS = ("unit", "std", "sign")


def _elemsum(v):
    """The sum of a 1-d fp64 tensor as sequential adds in element order (a 1-d cumsum on the CPU
    is that loop)."""
    return torch.cumsum(v, 0)[-1]


def opt_attack_parts(sums, honest, dirn):
    """-> (y, mu, p): y_j and mu as attack_vector forms them; the perturbation direction p is
    -mu ("unit": unnormalised, the solved gamma absorbs 1 / |mu|), -sqrt(var) ("std") or
    -sign(mu) ("sign": sign(0) = 0, a NaN stays a NaN)."""
    y = [sums[j].double() / honest[j] for j in range(len(sums)) if honest[j] >= 1]
    kh = len(y)
    mu = _seqsum(y) / kh
    if dirn == "unit":
        p = -mu
    elif dirn == "std":
        var = _seqsum([(t - mu) * (t - mu) for t in y]) / kh
        p = -_sqrt_rn(var)
    else:
        one = torch.ones_like(mu)
        p = torch.where(mu > 0, -one, torch.where(mu < 0, one, -mu))
    return y, mu, p


def opt_dist(sums, honest):
    """The pairwise-distance stage's matrix (krum_select's d: fp64, NaN -> +inf; nnm_neighbours'
    zero diagonal) over the fp32 means of the honest entries alone."""
    hs = [j for j in range(len(sums)) if honest[j] >= 1]
    cols = torch.stack(bucket_means([sums[j] for j in hs], [honest[j] for j in hs]))
    return nnm_neighbours(cols, 0)[0]


def opt_gamma(kind, a, c, q, dist):
    """The largest gamma of the budget, in closed form, as scalar Python floats: a, c lists of kh
    floats, q a float, dist kh lists of kh floats.  Every constraint |e_i + gamma p|^2 <= r is the
    convex quadratic q gamma^2 + 2 c_i gamma + a_i <= r, which holds at gamma = 0."""
    import math
    kh = len(a)
    if q == 0:
        return 0.0

    def root(c_, q_, r):
        if r < 0:
            r = 0.0
        return (math.sqrt(c_ * c_ + q_ * r) - c_) / q_
    if kind == "minmax":
        D = dist[0][0]
        for row in dist:
            for v in row:
                D = v if v > D else D
        gs = [root(c[i], q, D - a[i]) for i in range(kh)]
        if any(g != g for g in gs):
            return float("nan")
        gamma = gs[0]
        for g in gs[1:]:
            if g < gamma:
                gamma = g
        return gamma
    S = A = C = None
    for i in range(kh):
        s = dist[i][0]
        for v in dist[i][1:]:
            s = s + v
        S = s if S is None or s > S else S
        A = a[i] if A is None else A + a[i]
        C = c[i] if C is None else C + c[i]
    return root(C, kh * q, S - A)


def check_opt_attack(kind, dirn, strength, honest, byz):
    """The cases the library refuses (ValueError), in its order.  Returns (kind, dir, strength)."""
    if kind not in OPT_ATTACK_KINDS:
        raise ValueError(f"Invalid attack kind {kind!r} (supported: {OPT_ATTACK_KINDS})")
    if dirn not in OPT_ATTACK_DIRS:
        raise ValueError(f"Invalid attack direction {dirn!r} (supported: {OPT_ATTACK_DIRS})")
    return (kind, dirn, check_attack("ipm", strength, honest, byz)[1])


def opt_attack_flat(sums, honest, byz, kind, dirn="std", strength=1.0, use_gamma=None):
    """-> (entries, counts, b, gamma, a, c, q, dist): the entries and counts as attack_flat mixes
    them, b = (mu + p * (gamma * strength)).float(); gamma a Python float; a, c fp64 [kh], q an
    fp64 scalar, dist fp64 [kh, kh].  use_gamma (a float): b and the entries are evaluated with it
    in place of the solved gamma, which is still what is returned -- the form in which the device's
    b is checked, since its gamma is solved from its own sums."""
    kind, dirn, strength = check_opt_attack(kind, dirn, strength, honest, byz)
    y, mu, p = opt_attack_parts(sums, honest, dirn)
    a = torch.stack([_elemsum((mu - t) * (mu - t)) for t in y])
    c = torch.stack([_elemsum((mu - t) * p) for t in y])
    q = _elemsum(p * p)
    dist = opt_dist(sums, honest)
    gamma = opt_gamma(kind, a.tolist(), c.tolist(), q.item(), dist.tolist())
    entries, counts, b = _opt_mix(sums, honest, byz, mu, p, strength,
                                  gamma if use_gamma is None else use_gamma)
    return entries, counts, b, gamma, a, c, q, dist


def opt_attack_mix(sums, honest, byz, dirn, strength, gamma):
    """The crafted vector and the mix for a given gamma (a Python float) -> (entries, counts, b)."""
    _, mu, p = opt_attack_parts(sums, honest, dirn)
    return _opt_mix(sums, honest, byz, mu, p, strength, gamma)


def _opt_mix(sums, honest, byz, mu, p, strength, gamma):
    """One multiply for the scalar, a multiply and an add per element, one fp64 -> fp32 rounding,
    then attack_flat's mix."""
    coef = torch.tensor(float(gamma), dtype=torch.float64) * \
        torch.tensor(float(strength), dtype=torch.float64)
    b = (mu + p * coef).float()
    entries = []
    for j in range(len(sums)):
        if byz[j] == 0:
            entries.append(sums[j])
            continue
        t = b * torch.tensor(float(byz[j]), dtype=torch.float32)
        entries.append(sums[j] + t if honest[j] >= 1 else t)
    return entries, [int(h) + int(n) for h, n in zip(honest, byz)], b


def _parse_opt_attack(spec):
    import math
    if len(spec) > 3:
        raise ValueError(f"attack {spec!r} (supported: '{spec[0]}', ('{spec[0]}', dir), "
                         f"('{spec[0]}', dir, strength))")
    dirn = "std" if len(spec) < 2 or spec[1] is None else spec[1]
    if dirn not in OPT_ATTACK_DIRS:
        raise ValueError(f"attack {spec!r}: the direction must be one of {OPT_ATTACK_DIRS}")
    if len(spec) < 3 or spec[2] is None:
        return spec[0], dirn, 1.0
    try:
        strength = float(spec[2])
    except (TypeError, ValueError):
        raise ValueError(f"attack {spec!r}: the strength must be a number") from None
    if not (math.isfinite(strength) and strength >= 0):
        raise ValueError(f"attack {spec!r}: the strength must be finite and >= 0")
    return spec[0], dirn, strength


def parse_attack(spec):
    """FLSimulation's attack argument -> None or (kind, strength): None, "ipm" (eps = 1),
    ("ipm", eps), "alie" (strength None: alie_z of every epoch's fast-worker and Byzantine counts)
    or ("alie", z); or (kind, dir, strength) for "minmax" / "minsum", ("minmax", dir) and
    ("minmax", dir, strength): dir one of OPT_ATTACK_DIRS (default "std"), strength default 1."""
    import math
    if spec is None or spec == "none":
        return None
    if isinstance(spec, str):
        spec = (spec,)
    spec = tuple(spec)
    if spec and spec[0] in OPT_ATTACK_KINDS:
        return _parse_opt_attack(spec)
    if not spec or spec[0] not in ATTACK_KINDS or len(spec) > 2:
        raise ValueError(f"attack {spec!r} (supported: None, 'ipm', ('ipm', eps), 'alie', "
                         "('alie', z))")
    kind = spec[0]
    if len(spec) == 1 or spec[1] is None:
        return kind, (1.0 if kind == "ipm" else None)
    try:
        strength = float(spec[1])
    except (TypeError, ValueError):
        raise ValueError(f"attack {spec!r}: the strength must be a number") from None
    if not (math.isfinite(strength) and strength >= 0):
        raise ValueError(f"attack {spec!r}: the strength must be finite and >= 0")
    return kind, strength
