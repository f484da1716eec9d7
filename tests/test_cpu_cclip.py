"""CPU: centered clipping with a carried center (flsim/robust.py: cclip_steps and its parts;
csrc/cclip.h through flsim_cclip_eval_host; the refusals of flsim_cclip_optim_step, parse_rule,
check_cclip and main.py; FLSimulation on a CPU stand-in).

  text vs the paper's form   cclip_steps (the affine weights u, w) against a naive fp64 loop that
                materialises v_l; the tolerance is measured (below);
  host twin vs the text      stepwise (tests/_cclip.py): d2 within 2 (P + 2) 2^-53, s, u, w and g
                bit for bit, over KS x P x iters x weightings x fresh / carried center;
  refusals      status 1 before any launch, with bogus addresses (nothing is dereferenced).
"""
import ctypes

import numpy as np
import pytest
import torch

import _cclip as C

# Measured on the inputs of test_text_equals_the_papers_form (k in (1, 3, 8), P = 257, iters in
# (1, 3), both weightings, fresh and carried center): the largest relative difference between the
# text's fp64 iterate u * c + sum_j w[j] * x_j and the naive loop's v is 2.92e-16 (max norm over the
# elements, relative to max |v|), and between the text's s and the naive loop's 2.40e-16.  Both
# sides are fp64 and differ in the order of their sums only; 4 x the measured figure is allowed
# (summation-order slack of another machine's vectorised sums).
MEASURED_G, MEASURED_S = 2.92e-16, 2.40e-16
G_TOL, S_TOL = 4 * MEASURED_G, 4 * MEASURED_S


def _naive(cols, cen, alpha, iters, tau):
    """The paper's form: v_0 = c; v_(l+1) = v_l + sum_j lam_j min(1, tau / ||x_j - v_l||) (x_j - v_l)."""
    x = cols.double()
    v = torch.zeros(x.shape[1], dtype=torch.float64) if cen is None else cen.double().clone()
    lam = alpha / alpha.sum()
    ss = []
    for _ in range(iters):
        diff = x - v
        d = (diff ** 2).sum(1).sqrt()
        s = torch.minimum(torch.ones_like(d), tau / d)
        v = v + (lam[:, None] * s[:, None] * diff).sum(0)
        ss.append(s)
    return v, torch.stack(ss)


@pytest.mark.parametrize("k", (1, 3, 8))
def test_text_equals_the_papers_form(k):
    from flsim.robust import _cclip_z, cclip_steps, geomed_alpha
    P = 257
    worst_g = worst_s = 0.0
    for iters in (1, 3):
        for weighted in (False, True):
            for fresh in (True, False):
                ent, cnt = C.inputs(k, P)
                cen = None if fresh else C.center(P)
                tau = C.pick_tau(ent, cnt, cen)
                cols, a = C.cols_of(ent, cnt), geomed_alpha(cnt, weighted)
                g, u, w, d2, s = cclip_steps(cols, C._cen(cen), a, iters, tau)
                s = torch.stack(s)
                # some but not all clip: within the first iteration (k = 1: over the iterations)
                pool = s[0] if k > 1 else s
                if k > 1 or iters == 3:
                    assert bool((pool < 1).any()) and bool((pool == 1).any()), (k, iters, s)
                z = _cclip_z(cols.double(), None if fresh else C._cen(cen).double(), u[iters],
                             w[iters])
                assert torch.equal(g, z.float())
                v, sn = _naive(cols, C._cen(cen), a, iters, tau)
                rg = float((z - v).abs().max() / v.abs().max())
                rs = float(((s - sn).abs() / sn).max())
                print(f"k={k} iters={iters} weighted={weighted} fresh={fresh}: g {rg:.3e} s {rs:.3e}")
                worst_g, worst_s = max(worst_g, rg), max(worst_s, rs)
                assert rg <= G_TOL and rs <= S_TOL, (k, iters, weighted, fresh, rg, rs)
                assert len(u) == iters + 1 and len(w) == iters + 1 and len(d2) == iters
    print(f"k={k}: worst g {worst_g:.3e} (allowed {G_TOL:.3e}), worst s {worst_s:.3e} "
          f"(allowed {S_TOL:.3e})")


@pytest.mark.parametrize("k", (1, 3, 8))
def test_sanity_identities(k):
    """tau = 1e30, iters = 1, fresh: nothing clips, u[1] == 0 exactly (uniform weights: 1 / k sums
    to 1 for these k) and g is the alpha-weighted mean as _wsum forms it.  All entries equal to the
    center: g == center bit for bit."""
    from flsim.robust import _seqsum, _wsum, cclip_flat, geomed_alpha
    P = 257
    ent, cnt = C.inputs(k, P)
    for weighted in (False, True):
        g, u, w, d2, s = cclip_flat(C._tensors(ent), cnt, None, 1e30, 1, weighted)
        a = geomed_alpha(cnt, weighted)
        lam = a / _seqsum(a)
        assert bool((s[0] == 1).all())
        assert float(u[1]) == float(1.0 - _seqsum(lam))
        if not weighted:
            assert float(u[1]) == 0.0
        assert torch.equal(w[1], lam)
        assert torch.equal(g, _wsum(C.cols_of(ent, cnt).double(), lam).float())
    cen = C.center(P)
    for iters in (1, 3):
        for weighted in (False, True):
            g, u, w, d2, s = cclip_flat([torch.from_numpy(cen)] * k, [1] * k, torch.from_numpy(cen),
                                        0.25, iters, weighted)
            # (a later iterate is c / k + ... + c / k: c up to fp64 rounding, and c after .float())
            assert bool((d2[0] == 0).all()) and bool((torch.stack(d2) < 1e-24).all())
            assert bool((torch.stack(s) == 1).all())
            assert np.array_equal(C.bits(g.numpy()), C.bits(cen))


def _cases(k, P, seed=0):
    for iters in (1, 3):
        for weighted in (False, True):
            for fresh in (True, False):
                ent, cnt = C.inputs(k, P, seed)
                cen = None if fresh else C.center(P, seed)
                yield ent, cnt, cen, C.pick_tau(ent, cnt, cen), iters, weighted


@pytest.mark.parametrize("k", C.KS)
def test_host_twin_equals_the_text_stepwise(k):
    """KS x P in (1, 255, 257) x iters in (1, 3) x both weightings x fresh / carried center; the
    next center has the bits of g, the sign of zeros included."""
    for P in (1, 255, 257):
        for ent, cnt, cen, tau, iters, weighted in _cases(k, P):
            what = (k, P, iters, weighted, cen is None)
            got = C.host_twin(ent, cnt, cen, tau, iters, weighted)
            alive, g_t = C.stepwise(ent, cnt, cen, tau, iters, weighted, got, what)
            assert alive.all()
            assert np.array_equal(C.bits(got[5]), C.bits(got[0])), what
            # and the whole chain from scratch: the host twin sums in element order, the text
            # in torch's; they agree to the distance bound at the first iteration
            t = C.text(ent, cnt, cen, tau, iters, weighted)
            assert C.outside(got[3][0], t[3][0], C.d2_bound(P)) == 0, what


def test_special_inputs():
    """A NULL entry; a duplicate pointer; one dead entry (NaN, +inf, -inf): no redo, s = 0, w = 0
    and g finite; every entry dead: g == center (fresh: zero) and u stays 1; a NaN center: g and the
    next center all NaN; d = 0: s = 1; the sign of a zero g is carried into the center."""
    P, k = 257, 5
    for ent, cnt, cen, tau, iters, weighted in _cases(k, P, 3):
        ent[1] = None
        got = C.host_twin(ent, cnt, cen, tau, iters, weighted)
        C.stepwise(ent, cnt, cen, tau, iters, weighted, got, "null")
    for ent, cnt, cen, tau, iters, weighted in _cases(k, P, 2):
        ent[1], cnt[1] = ent[0], cnt[0]
        got = C.host_twin(ent, cnt, cen, tau, iters, weighted)
        C.stepwise(ent, cnt, cen, tau, iters, weighted, got, "duplicate")
        assert (got[3][:, 0] == got[3][:, 1]).all() and (got[2][:, 0] == got[2][:, 1]).all()
    for bad in (np.nan, np.inf, -np.inf):
        for ent, cnt, cen, tau, iters, weighted in _cases(k, P, 1):
            j = k // 2
            ent[j] = ent[j].copy()
            ent[j][3::7] = bad
            tau = C.pick_tau(ent, cnt, cen)
            got = C.host_twin(ent, cnt, cen, tau, iters, weighted)
            alive, _ = C.stepwise(ent, cnt, cen, tau, iters, weighted, got, (bad, iters))
            g, u, w, d2, s, cout = got
            assert not alive[j] and alive.sum() == k - 1
            assert (s[:, j] == 0).all() and (w[:, j] == 0).all() and np.isinf(d2[:, j]).all()
            assert np.isfinite(g).all() and np.isfinite(np.delete(w, j, 1)).all()
            assert np.isfinite(u).all() and np.array_equal(C.bits(cout), C.bits(g))
    nan = [np.full(P, np.nan, np.float32) for _ in range(k)]
    for cen in (None, C.center(P)):
        for iters in (1, 3):
            got = C.host_twin(nan, [1] * k, cen, 1.0, iters)
            alive, _ = C.stepwise(nan, [1] * k, cen, 1.0, iters, False, got, "all dead")
            g, u, w, d2, s, cout = got
            assert not alive.any() and (u == 1).all() and (w == 0).all() and (s == 0).all()
            assert np.array_equal(C.bits(g), C.bits(np.zeros(P, np.float32) if cen is None else cen))
            assert np.array_equal(C.bits(cout), C.bits(g))
    ent, cnt = C.inputs(k, P)
    cen = C.center(P)
    cen[5] = np.nan
    for iters in (1, 3):
        got = C.host_twin(ent, cnt, cen, 1.0, iters)
        C.stepwise(ent, cnt, cen, 1.0, iters, False, got, "nan center")
        assert np.isnan(got[0]).all() and np.isnan(got[5]).all()
    # d = 0: the entry sits on the center, s = 1 (tau / 0 = +inf)
    cen = C.center(P)
    ent[2], cnt[2] = cen.copy(), 1
    got = C.host_twin(ent, cnt, cen, 1e-3, 1)
    C.stepwise(ent, cnt, cen, 1e-3, 1, False, got, "d = 0")
    assert got[3][0, 2] == 0 and got[4][0, 2] == 1 and (np.delete(got[4][0], 2) < 1).all()
    # a zero g keeps its sign in the center: x = -0 everywhere, fresh, nothing clips
    neg = [np.full(P, -0.0, np.float32)]
    got = C.host_twin(neg, [1], None, 1.0, 1)
    _, g_t = C.stepwise(neg, [1], None, 1.0, 1, False, got, "-0")
    assert (C.bits(g_t) == 0x80000000).all() and np.array_equal(C.bits(got[5]), C.bits(g_t))


def test_parse_rule_and_check():
    from flsim.robust import check_cclip, parse_rule
    assert parse_rule(("cclip", 2.5)) == ("cclip", 2.5, 1, "uniform")
    assert parse_rule(["cclip", 2, 3]) == ("cclip", 2.0, 3, "uniform")
    assert parse_rule(("cclip", 0.5, 32, "count")) == ("cclip", 0.5, 32, "count")
    # existing return values stay
    assert parse_rule("geomed") == ("geomed", 3, 1e-6, "uniform")
    assert parse_rule(("geomed", 5)) == ("geomed", 5, 1e-6, "uniform")
    assert parse_rule("median") == ("median", 0) and parse_rule(None) is None
    assert parse_rule(("trimmed_mean", 2)) == ("trimmed_mean", 2)
    assert parse_rule(("krum", 2)) == ("krum", 2, 1)
    assert parse_rule(("multi_krum", 2, 3)) == ("multi_krum", 2, 3)
    for bad in ("cclip", ("cclip",), ("cclip", 0.0), ("cclip", -1.0), ("cclip", float("nan")),
                ("cclip", float("inf")), ("cclip", 1.0, 0), ("cclip", 1.0, 33),
                ("cclip", 1.0, 1, "mean"), ("cclip", 1.0, 1, "count", 1), ("cclip", "x")):
        with pytest.raises(ValueError, match="robust_rule"):
            parse_rule(bad)
    assert check_cclip(1, 1.0, None, 3) == (1, 1.0, "uniform")
    assert check_cclip(32, 1e-3, "count", 1) == (32, 1e-3, "count")
    with pytest.raises(IndexError):
        check_cclip(1, 1.0, None, 0)
    for args, what in (((0, 1.0, None), "Invalid iters"), ((33, 1.0, None), "Invalid iters"),
                       ((1, 0.0, None), "Invalid tau"), ((1, float("nan"), None), "Invalid tau"),
                       ((1, float("inf"), None), "Invalid tau"), ((1, 1.0, "mean"), "Invalid weights")):
        with pytest.raises(ValueError, match=what):
            check_cclip(*args, 3)


def test_rules_over_the_flattened_model():
    """cclip_rule over lists of per-parameter tensors returns (out_list, new_center_flat); the
    CenteredClip closure keeps the center between calls."""
    from flsim.robust import CenteredClip, cclip_flat, cclip_rule, cclip_steps
    g = torch.Generator().manual_seed(5)
    ups = [[torch.randn(3, 4, generator=g), torch.randn(5, generator=g)] for _ in range(4)]
    flat = [torch.cat([u.reshape(-1) for u in up]) for up in ups]
    out, cen = cclip_rule(ups, None, 2.0, 2)
    ref = cclip_flat(flat, [1] * 4, None, 2.0, 2)[0]
    assert torch.equal(cen, ref) and torch.equal(torch.cat([o.reshape(-1) for o in out]), ref)
    assert [o.shape for o in out] == [u.shape for u in ups[0]]
    out2, cen2 = cclip_rule(ups, cen, 2.0, 2, weights=[1, 2, 3, 4])
    alpha = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64)
    assert torch.equal(cen2, cclip_steps(torch.stack(flat), cen, alpha, 2, 2.0)[0])
    assert not torch.equal(cen2, cclip_rule(ups, cen, 2.0, 2)[1])
    rule = CenteredClip(2.0, 2)
    a = rule(ups)
    assert torch.equal(rule.center, cen) and torch.equal(a[0], out[0])
    b = rule(ups)
    assert torch.equal(rule.center, cclip_rule(ups, cen, 2.0, 2)[1]) and b[0].shape == (3, 4)
    with pytest.raises(IndexError):
        cclip_rule([], None, 1.0)
    with pytest.raises(ValueError, match="Invalid tau"):
        CenteredClip(0.0)
    with pytest.raises(ValueError, match="weights"):
        cclip_rule(ups, None, 1.0, weights=[1, 2])


# ---- refusals of the entry point (status 1, before any launch) -------------------------------------
F = {name: 0x1000000 * (i + 1) for i, name in enumerate(
    ["p", "m", "v", "g", "G", "D", "O", "e0", "e1", "e2", "sp", "su", "sw", "sd", "ss", "st", "c"])}
P = 64


def _optim(**kw):
    from flsim.engine import Optim
    return Optim(**kw).c_struct()


def _clip(max_norm=1.0, G=None, partials=None, n=1 << 20, out=None):
    from flsim._lib import FlsimClip
    c = FlsimClip()
    c.max_norm = max_norm
    c.G = F["G"] if G is None else G
    c.partials = F["D"] if partials is None else partials
    c.n_partials = n
    c.out = F["O"] if out is None else out
    return c


def _scratch(n=1 << 20, **kw):
    from flsim._lib import FlsimCclipScratch
    s = FlsimCclipScratch()
    s.n_partials = n
    for field, name in (("partials", "sp"), ("u", "su"), ("w", "sw"), ("d2", "sd"), ("s", "ss"),
                        ("state", "st")):
        setattr(s, field, kw.get(field, F[name]))
    return s


def _call(iters=3, tau=1.0, weighted=0, fresh=0, counts=(1, 3, 4), ents=None, scratch="default",
          clip=None, g_out=0, p=None, mm=0, v=0, n=P, step=1, optim="sgd", center=None):
    from flsim._lib import lib
    ents = [F["e0"], F["e1"], F["e2"]][:len(counts)] if ents is None else ents
    ents = list(ents) + [0] * (min(len(counts), 64) - len(ents))
    r, _ = C.c_cclip(None, list(counts), None, tau, iters, 0, fresh, ptrs=ents,
                     center_ptr=F["c"] if center is None else center)
    r.k = len(counts)
    r.weighted = weighted
    s = _scratch() if scratch == "default" else scratch
    o = None if optim is None else (optim if not isinstance(optim, str) else
                                     _optim(kind=optim, lr=0.1))
    vp = ctypes.c_void_p
    rc = lib().flsim_cclip_optim_step(
        ctypes.byref(r), None if s is None else ctypes.byref(s),
        None if clip is None else ctypes.byref(clip), vp(g_out), vp(F["p"] if p is None else p),
        vp(mm), vp(v), n, step, None if o is None else ctypes.byref(o), None)
    return rc, lib().flsim_last_error().decode()


N_HYPER = 17        # the leading REFUSALS that are about flsim_cclip's numbers alone
REFUSALS = [
    (dict(counts=()), "k = 0 entries"),
    (dict(counts=(1,) * 65), "k = 65 entries"),
    (dict(iters=0), "Invalid iters = 0"),
    (dict(iters=-1), "Invalid iters = -1"),
    (dict(iters=33), "Invalid iters = 33"),
    (dict(tau=0.0), "Invalid tau"),
    (dict(tau=-1e-6), "Invalid tau"),
    (dict(tau=float("nan")), "Invalid tau"),
    (dict(tau=float("inf")), "Invalid tau"),
    (dict(tau=float("-inf")), "Invalid tau"),
    (dict(weighted=2), "Invalid weighted = 2"),
    (dict(weighted=-1), "Invalid weighted = -1"),
    (dict(fresh=2), "Invalid fresh = 2"),
    (dict(fresh=-1), "Invalid fresh = -1"),
    (dict(counts=(1, 0, 3)), "Invalid count 0 of entry 1"),
    (dict(counts=(1, 3, -5)), "Invalid count -5 of entry 2"),
    (dict(counts=(0,)), "Invalid count 0 of entry 0"),
    # what check_optim / check_clip refuse, still before any pointer (p = NULL everywhere)
    (dict(optim=_optim(kind="sgd", lr=-1.0), p=0, scratch=None), "Invalid learning rate"),
    (dict(optim=_optim(kind="sgd", lr=0.1, momentum=-0.5), p=0), "Invalid momentum"),
    (dict(optim=_optim(kind="adam", weight_decay=-1.0), p=0), "Invalid weight_decay"),
    (dict(optim=_optim(kind="yogi", betas=(1.0, 0.9)), p=0), "Invalid beta parameter at index 0"),
    (dict(optim=_optim(kind="adagrad", lr_decay=-1.0), p=0), "Invalid lr_decay"),
    (dict(clip=_clip(max_norm=0.0), p=0), "max_norm"),
    (dict(clip=_clip(max_norm=float("nan")), p=0, scratch=None), "max_norm"),
    (dict(optim=None), "null optimizer"),
    (dict(optim=None, g_out=F["g"], clip=_clip()), "null optimizer"),
    # the pointers
    (dict(p=0), "null pointer"),
    (dict(optim="adam", mm=F["m"]), "null pointer"),
    (dict(optim=_optim(kind="sgd", lr=0.1, momentum=0.9)), "null pointer"),
    (dict(p=F["p"] + 4), "16-byte aligned"),
    (dict(g_out=F["g"] + 8), "16-byte aligned"),
    (dict(n=0), "out of range"),
    (dict(n=1 << 31), "out of range"),
    (dict(step=0), "step must be >= 1"),
    (dict(g_out=F["p"]), "overlap each other"),
    # the center
    (dict(center=0, p=F["p"]), "null centered-clipping center"),
    (dict(center=0, fresh=1), "null centered-clipping center"),
    (dict(center=F["c"] + 4), "center must be 16-byte aligned"),
    (dict(center=F["c"] + 8, fresh=1), "center must be 16-byte aligned"),
    (dict(center=F["p"]), "center overlaps p/m/v/g_out"),
    (dict(center=F["p"] + 4 * (P - 4)), "center overlaps p/m/v/g_out"),
    (dict(optim="adam", mm=F["m"], v=F["v"], center=F["m"] + 16), "center overlaps p/m/v/g_out"),
    (dict(optim="adam", mm=F["m"], v=F["v"], center=F["v"]), "center overlaps p/m/v/g_out"),
    (dict(g_out=F["g"], center=F["g"] + 32), "center overlaps p/m/v/g_out"),
    # the scratch
    (dict(scratch=None), "null centered-clipping scratch"),
    (dict(scratch=_scratch(partials=0)), "null centered-clipping scratch"),
    (dict(scratch=_scratch(u=0)), "null centered-clipping scratch"),
    (dict(scratch=_scratch(w=0)), "null centered-clipping scratch"),
    (dict(scratch=_scratch(d2=0)), "null centered-clipping scratch"),
    (dict(scratch=_scratch(s=0)), "null centered-clipping scratch"),
    (dict(scratch=_scratch(state=0)), "null centered-clipping scratch"),
    (dict(scratch=_scratch(partials=F["sp"] + 8)), "scratch must be 16-byte aligned"),
    (dict(scratch=_scratch(u=F["su"] + 8)), "scratch must be 16-byte aligned"),
    (dict(scratch=_scratch(w=F["sw"] + 8)), "scratch must be 16-byte aligned"),
    (dict(scratch=_scratch(d2=F["sd"] + 8)), "scratch must be 16-byte aligned"),
    (dict(scratch=_scratch(s=F["ss"] + 8)), "scratch must be 16-byte aligned"),
    (dict(scratch=_scratch(state=F["st"] + 4)), "scratch must be 16-byte aligned"),
    (dict(scratch=_scratch(n=3)), "n_partials = 3, this step writes 4"),
    (dict(scratch=_scratch(w=F["sp"] + 16)), "scratch buffers overlap"),
    (dict(scratch=_scratch(u=F["sw"] + 80)), "scratch buffers overlap"),
    (dict(scratch=_scratch(s=F["sd"] + 64)), "scratch buffers overlap"),
    (dict(scratch=_scratch(state=F["su"] + 16)), "scratch buffers overlap"),
    (dict(scratch=_scratch(state=F["p"] + 16)), "scratch overlaps p/m/v/g_out"),
    (dict(scratch=_scratch(s=F["G"] + 16), clip=_clip()), "scratch overlaps clip G"),
    (dict(scratch=_scratch(u=F["c"] + 16)), "center overlaps the centered-clipping scratch"),
    (dict(scratch=_scratch(partials=F["c"] - 16)), "center overlaps the centered-clipping scratch"),
    (dict(center=F["st"]), "center overlaps the centered-clipping scratch"),
    (dict(clip=_clip(G=F["c"] + 16)), "center overlaps clip G"),
    # the entries
    (dict(ents=[F["e0"], F["e1"] + 2, F["e2"]]), "entry 1 must be 4-byte aligned"),
    (dict(ents=[F["e0"], F["p"], F["e2"]]), "entry 1 overlaps"),
    (dict(ents=[F["p"] + 4 * (P - 1), F["e1"], F["e2"]]), "entry 0 overlaps"),
    (dict(optim="adam", mm=F["m"], v=F["v"], ents=[F["m"] + 16, F["e1"], F["e2"]]),
     "entry 0 overlaps"),
    (dict(g_out=F["g"], ents=[F["e0"], F["e1"], F["g"] + 32]), "entry 2 overlaps"),
    (dict(clip=_clip(), ents=[F["G"] + 4, F["e1"], F["e2"]]), "entry 0 overlaps clip G"),
    (dict(ents=[F["sp"] + 8, F["e1"], F["e2"]]), "entry 0 overlaps the centered-clipping scratch"),
    (dict(ents=[F["e0"], F["su"] - 4 * (P - 1), F["e2"]]),
     "entry 1 overlaps the centered-clipping scratch"),
    (dict(ents=[F["e0"], F["e1"], F["ss"] + 16]), "entry 2 overlaps the centered-clipping scratch"),
    (dict(ents=[F["st"], F["e1"], F["e2"]]), "entry 0 overlaps the centered-clipping scratch"),
    (dict(ents=[F["c"], F["e1"], F["e2"]]), "entry 0 overlaps the centered-clipping center"),
    (dict(ents=[F["e0"], F["c"] + 4 * (P - 1), F["e2"]]),
     "entry 1 overlaps the centered-clipping center"),
    (dict(ents=[F["e0"], F["e1"], F["c"] - 4 * (P - 1)], fresh=1),
     "entry 2 overlaps the centered-clipping center"),
    (dict(clip=_clip(G=0)), "null clip buffer"),
    (dict(clip=_clip(G=F["G"] + 4)), "16-byte aligned"),
    (dict(clip=_clip(G=F["p"] + 16)), "clip G overlaps"),
    (dict(clip=_clip(n=0)), "n_partials"),
]


@pytest.mark.parametrize("kw,message", REFUSALS, ids=[f"{i}-{m[:24]}" for i, (_, m) in
                                                       enumerate(REFUSALS)])
def test_entry_point_refusals(kw, message):
    rc, err = _call(**kw)
    assert rc == 1, (rc, err)
    assert message in err, err


def test_refusal_order_partials_and_host_twin_refusals():
    """Hyper-parameters come before pointers (everything NULL still names iters); adjacent buffers
    do not overlap, so the next check is reached; flsim_cclip_partials is what the step asks for and
    equals the geometric median's (the geometry is shared); the host twin refuses the same numbers."""
    from flsim._lib import lib
    L = lib()
    rc, err = _call(iters=40, p=0, ents=[0, 0, 0], scratch=None, center=0)
    assert rc == 1 and "Invalid iters = 40" in err
    rc, err = _call(ents=[F["p"] - 4 * P, F["p"] + 4 * P, F["e2"]], center=F["c"],
                    scratch=_scratch(u=F["c"] + 4 * P, w=F["c"] - 96), clip=_clip(n=0))
    assert rc == 1 and "clip n_partials" in err, err
    for k in C.KS:
        E = L.flsim_cclip_tile_elems(k)
        assert E >= 256 and E % 256 == 0 and E == L.flsim_geomed_tile_elems(k)
        for n in (1, E - 1, E, E + 1, 3 * E + 5, 5596090, (1 << 31) - 1):
            need = L.flsim_cclip_partials(n, k)
            assert need >= k + 1 and need % (k + 1) == 0 and need == L.flsim_geomed_partials(n, k)
            # (the center far from p: at these n the bogus addresses are closer than 4 n bytes)
            rc, err = _call(counts=(1,) * k, n=n, scratch=_scratch(n=need - 1), center=1 << 44)
            assert rc == 1 and f"this step writes {need}" in err, err
        assert L.flsim_cclip_partials(E, k) < L.flsim_cclip_partials(E + 1, k)
    assert L.flsim_cclip_partials(0, 8) == 0 and L.flsim_cclip_partials(8, 65) == 0
    assert L.flsim_cclip_partials(1 << 31, 8) == 0 and L.flsim_cclip_partials(8, 0) == 0
    assert L.flsim_cclip_tile_elems(0) == 0 and L.flsim_cclip_tile_elems(65) == 0
    vp = ctypes.c_void_p
    u, w, d2, s = np.zeros(33), np.zeros(33 * 64), np.zeros(32 * 64), np.zeros(32 * 64)
    a = (u.ctypes.data_as(vp), w.ctypes.data_as(vp), d2.ctypes.data_as(vp), s.ctypes.data_as(vp),
         None, None)
    for kw, message in REFUSALS[:N_HYPER]:
        counts = list(kw.get("counts", (1, 3, 4)))
        ent = [np.ones(4, np.float32) for _ in counts[:64]]
        r, keep = C.c_cclip(ent, counts, np.zeros(4, np.float32), kw.get("tau", 1.0),
                            kw.get("iters", 3), 0, kw.get("fresh", 0))
        r.k = len(counts)
        r.weighted = kw.get("weighted", 0)
        assert L.flsim_cclip_eval_host(ctypes.byref(r), 4, *a) == 1
        assert message in L.flsim_last_error().decode()
    ent = [np.ones(4, np.float32)] * 3
    r, keep = C.c_cclip(ent, [1] * 3, np.zeros(4, np.float32), 1.0, 3)
    assert L.flsim_cclip_eval_host(ctypes.byref(r), 0, *a) == 1
    assert L.flsim_cclip_eval_host(ctypes.byref(r), 4, None, *a[1:]) == 1
    assert L.flsim_cclip_eval_host(ctypes.byref(r), 4, a[0], None, *a[2:]) == 1
    assert L.flsim_cclip_eval_host(ctypes.byref(r), 4, a[0], a[1], None, *a[3:]) == 1
    assert L.flsim_cclip_eval_host(ctypes.byref(r), 4, a[0], a[1], a[2], None, None, None) == 1
    assert L.flsim_cclip_eval_host(None, 4, *a) == 1
    assert L.flsim_cclip_eval_host(ctypes.byref(r), 4, *a) == 0
    r2, keep2 = C.c_cclip(ent, [1] * 3, None, 1.0, 3, fresh=0)      # not fresh, no center
    assert L.flsim_cclip_eval_host(ctypes.byref(r2), 4, *a) == 1
    assert "null centered-clipping center" in L.flsim_last_error().decode()
    r3, keep3 = C.c_cclip(ent, [1] * 3, None, 1.0, 3)               # fresh: the center is not read
    assert L.flsim_cclip_eval_host(ctypes.byref(r3), 4, *a) == 0


def test_abi_exports():
    from flsim import _lib
    L = _lib.lib()
    new = {"flsim_cclip_partials", "flsim_cclip_tile_elems", "flsim_cclip_optim_step",
           "flsim_cclip_eval_host"}
    assert new <= set(_lib.EXPORTS)
    for n in new:
        assert hasattr(L, n), n
    assert ctypes.sizeof(_lib.FlsimCclip) == 16 + 8 + 8 * 64 + 4 * 64 + 8
    assert _lib.FlsimCclip.center.offset == 792 and _lib.FlsimCclip.tau.offset == 16
    assert ctypes.sizeof(_lib.FlsimCclipScratch) == 7 * 8
    names = [L.flsim_probe_kernel_name(i).decode() for i in range(L.flsim_probe_kernel_count())]
    assert {"cclip_dist", "cclip_finish", "cclip_apply"} <= set(names)


def test_cclip_object():
    from flsim.engine import CClip
    e = [torch.zeros(8) for _ in range(3)]
    cen = torch.zeros(8)
    r = CClip(2.5, 3, True, e, [1, 3, 4], cen, fresh=True)
    c = r.c_struct()
    assert (c.iters, c.weighted, c.k, c.fresh, c.tau) == (3, 1, 3, 1, 2.5)
    assert list(c.count[:3]) == [1, 3, 4] and c.entries[0] == e[0].data_ptr() and r.k == 3
    assert c.center == cen.data_ptr()
    c = CClip(1.0, 1, False, [None] * 3, [4] * 3, None).c_struct()
    assert c.entries[0] is None and c.center is None and c.fresh == 0
    with pytest.raises(ValueError, match="counts"):
        CClip(1.0, 1, False, e, [1, 2], cen)
    with pytest.raises(ValueError, match="65 entries"):
        CClip(1.0, 1, False, [None] * 65, [1] * 65, cen)


# ---- FLSimulation on a CPU stand-in ----------------------------------------------------------------
def _standin():
    from test_cpu_geomed import StandInEngine

    class CClipStandIn(StandInEngine):
        def cclip_step(self, cc, theta, m, v, step, optim=None, clip=None, **kw):
            from flsim.robust import cclip_flat
            g, u, w, d2, s = cclip_flat(cc.entries, cc.counts, None if cc.fresh else cc.center,
                                        cc.tau, cc.iters, cc.weighted)
            cc.u, cc.w, cc.d2, cc.s = torch.stack(u), torch.stack(w), torch.stack(d2), torch.stack(s)
            cc.center.copy_(g)
            theta -= optim.lr * g
    return CClipStandIn()


def _sim(**kw):
    from flsim.sim import FLSimulation
    eng = _standin()
    kw.setdefault("delay", 2)
    return FLSimulation(kw.pop("n", 6), device="cpu", engine=eng, device_pool=object(),
                        theta0=torch.zeros(eng.P), optimizer="sgd", lr=0.125, **kw)


@pytest.mark.parametrize("weights", ("uniform", "count"))
def test_epoch_center_log_and_refusals(weights):
    """n = 6, worker 5 slow with delay 2, four buckets: the first epoch runs fresh, every later one
    around the previous epoch's g; theta and cclip_log() follow the text over last_entries."""
    from flsim.robust import cclip_flat
    ind = dict(semantics="independent")
    tau = 10.0                  # (some of the stand-in's entries clip at this radius, some do not)
    sim = _sim(robust_rule=("cclip", tau, 2, weights), buckets=4, keep_entries=True, **ind)
    assert sim.robust == ("cclip", tau, 2, weights)
    assert sim.last_cclip is None and sim.center is None and sim.cclip_log() == []
    pops, prev, clipped = 0, None, set()
    for t in range(5):
        before = sim.theta.clone()
        sim.epoch()
        ents, counts = sim.last_entries
        pops += bool(sim.trace[-1].stale)
        assert (sim.last_center is None) == (t == 0) and sim.last_cclip.fresh == (t == 0)
        if t:
            assert torch.equal(sim.last_center, prev)
        g, u, w, d2, s = cclip_flat(ents, counts, sim.last_center, tau, 2, weights == "count")
        assert torch.equal(sim.theta, before - 0.125 * g) and torch.equal(sim.center, g)
        prev = g.clone()
        ul, wl, nl = sim.cclip_log()[-1]
        assert ul == float(u[-1]) and wl == [float(x) for x in w[-1]]
        assert nl == int((s[-1] < 1).sum()) and type(ul) is float and type(nl) is int
        clipped |= {bool(x < 1) for x in torch.stack(s).reshape(-1)}
    assert pops >= 1 and len(sim.cclip_log()) == 5 and clipped == {True, False}
    for bad in ("cclip", ("cclip", 0.0), ("cclip", 1.0, 33), ("cclip", 1.0, 1, "mean")):
        with pytest.raises(ValueError, match="robust_rule"):
            _sim(robust_rule=bad, **ind)
    rule = ("cclip", 1.0)
    for sem in ("reference", "torch1"):
        with pytest.raises(NotImplementedError, match="independent"):
            _sim(robust_rule=rule, semantics=sem)
    with pytest.raises(NotImplementedError, match="distributed"):
        _sim(robust_rule=rule, distributed=True, **ind)
    with pytest.raises(NotImplementedError, match="staleness discount"):
        _sim(robust_rule=rule, stale_weight=("poly", 0.5), **ind)
    with pytest.raises(NotImplementedError, match="delay compensation"):
        _sim(robust_rule=rule, delay_comp=0.5, **ind)
    with pytest.raises(ValueError, match="buckets"):
        _sim(robust_rule=rule, buckets=0, **ind)
    big = _sim(n=70, robust_rule=rule, buckets=65, **ind)
    with pytest.raises(ValueError, match="65 entries"):
        big.epoch()
    one = _sim(robust_rule=rule, buckets=1, **ind)
    one.epoch()
    assert one.last_cclip is None and one.last_center is None and len(one.cclip_log()) == 1
    assert _sim(robust_rule=("cclip", 2, 3), **ind)._stale_config()["robust_rule"] == \
        ["cclip", 2.0, 3, "uniform"]


def test_main_arguments():
    import main
    a = main.parse(["--robust_rule", "cclip", "--cclip_tau", "2.5"])
    assert main.robust_spec(a) == ("cclip", 2.5, 1, "uniform")
    a = main.parse(["--robust_rule", "cclip", "--cclip_tau", "0.5", "--cclip_iters", "4",
                    "--cclip_weights", "count"])
    assert main.robust_spec(a) == ("cclip", 0.5, 4, "count")
    with pytest.raises(SystemExit, match="cclip_tau"):
        main.robust_spec(main.parse(["--robust_rule", "cclip"]))
    with pytest.raises(SystemExit):
        main.parse(["--robust_rule", "cclip", "--cclip_weights", "mean"])
    # the other rules' arguments are as they were
    assert main.robust_spec(main.parse(["--robust_rule", "geomed"])) == \
        ("geomed", 3, 1e-6, "uniform")
    assert main.robust_spec(main.parse([])) is None
