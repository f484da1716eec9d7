"""CPU: the geometric median over bucket means by smoothed Weiszfeld iterations (RFA).

The rule text (flsim/robust.py: geomed_steps) against an independent numpy restatement; the host twin
flsim_geomed_eval_host (distances summed in element order, then the scalar code the finish kernel
runs: csrc/geomed.h, one host + device function) against the text stepwise (tests/_geomed.py: d2
within the derived bound at the twin's own weights; w, obj and g bit for bit).  Then the special
inputs, every refusal of flsim_geomed_optim_step (they come before any launch, so made-up device
addresses are never read), check_geomed / parse_rule, FLSimulation on a CPU stand-in, and the
robustness property on the text and on the twin.
"""
import ctypes

import numpy as np
import pytest
import torch

import _geomed as G

PS = (1, 2, 257)
ITERS = (0, 1, 3, 8)


def _numpy_geomed(cols, alpha, iters, nu):
    """An independent fp64 restatement in numpy (plain loops for every ordered sum)."""
    x = cols.astype(np.float64)
    k = x.shape[0]
    alive = np.isfinite(x).all(1)
    a = np.where(alive, alpha, 0.0)

    def seq(v):
        s = v[0]
        for t in v[1:]:
            s = s + t
        return s

    def wsum(w):
        z = None
        for j in range(k):
            if w[j] == 0:
                continue
            t = x[j] * w[j]
            z = t if z is None else z + t
        return z

    with np.errstate(all="ignore"):
        w = [a / seq(a)]
        d2s, objs = [], []
        for r in range(iters):
            z = wsum(w[r])
            d2 = np.array([((x[j] - z) ** 2).sum() if alive[j] else np.inf for j in range(k)])
            d = np.sqrt(d2)
            objs.append(seq(np.array([a[j] * d[j] for j in range(k) if alive[j]])))
            beta = np.array([a[j] / max(d[j], nu) for j in range(k)])
            w.append(beta / seq(beta))
            d2s.append(d2)
        return wsum(w[iters]).astype(np.float32), np.array(w), np.array(d2s), np.array(objs)


@pytest.mark.parametrize("k", (1, 2, 5, 16, 33))
def test_text_equals_a_numpy_restatement(k):
    """w^(0) bit for bit and the first distances (numpy's pairwise sum against torch's) within the
    bound; the later stages inherit the distances' rounding and are close.  The weights sum to 1
    and the objective does not grow."""
    for P in (1, 257):
        for weighted in (False, True):
            ent, cnt = G.inputs(k, P)
            g, w, d2, obj = G.text(ent, cnt, 3, G.NU, weighted)
            alpha = np.array([float(c) if weighted else 1.0 for c in cnt])
            g2, w2, d22, obj2 = _numpy_geomed(G.cols_of(ent, cnt).numpy(), alpha, 3, G.NU)
            assert G.f64_mismatches(w2[0], w[0]) == 0
            assert G.outside(d22[0], d2[0], G.d2_bound(P)) == 0
            # from the first distances on the two differ by rounding: the later stages are close
            np.testing.assert_allclose(w2, w, rtol=1e-9)
            np.testing.assert_allclose(obj2, obj, rtol=1e-9)
            np.testing.assert_allclose(g2, g, rtol=1e-5, atol=1e-7)
            assert abs(w.sum(1) - 1).max() < 1e-12 and (w > 0).all()
            # Weiszfeld descends: the objective does not grow
            assert (np.diff(obj) <= 1e-12 * obj[:-1]).all(), obj


@pytest.mark.parametrize("k", G.KS)
def test_host_twin_equals_the_text_stepwise(k):
    for P in PS:
        ent, cnt = G.inputs(k, P)
        for iters in ITERS:
            for weighted in (False, True):
                got = G.host_twin(ent, cnt, iters, G.NU, weighted)
                alive = G.stepwise(ent, cnt, iters, G.NU, weighted, got, (k, P, iters, weighted))
                assert alive.all()
                assert np.isfinite(got[0]).all()


def test_iters_zero_is_the_weighted_mean():
    ent, cnt = G.inputs(5, 257)
    cols = G.cols_of(ent, cnt).double()
    for weighted in (False, True):
        g, w, d2, obj = G.host_twin(ent, cnt, 0, G.NU, weighted)
        a = np.array([float(c) if weighted else 1.0 for c in cnt])
        assert np.allclose(w[0], a / a.sum(), rtol=1e-15)
        ref = (cols * torch.from_numpy(a / a.sum())[:, None]).sum(0).numpy()
        np.testing.assert_allclose(g, ref, rtol=1e-6, atol=1e-7)
        assert d2.shape == (0, 5) and obj.shape == (0,)


def test_special_inputs():
    # a NULL entry is all zero
    ent, cnt = G.inputs(5, 257, 3)
    ent[2] = None
    got = G.host_twin(ent, cnt, 3)
    G.stepwise(ent, cnt, 3, G.NU, False, got, "null")
    # duplicates: distance 0, where the nu floor acts
    ent = [np.array([v], np.float32) for v in (1, 1, 1, 5)]
    for nu in (1e-6, 2.0):
        g, w, d2, obj = got = G.host_twin(ent, [1] * 4, 3, nu)
        G.stepwise(ent, [1] * 4, 3, nu, False, got, ("dup", nu))
        assert np.array_equal(d2[0], [1.0, 1.0, 1.0, 9.0]) and obj[0] == 6.0      # z_0 = 2
        beta = np.array([1 / max(1.0, nu)] * 3 + [1 / 3.0])
        assert np.array_equal(w[1], beta / ((beta[0] + beta[1] + beta[2]) + beta[3]))
        assert 1.0 < g[0] < 2.0 and (np.diff(obj) < 0).all()
    same = [np.array([3.0], np.float32) for _ in range(4)]
    g, w, d2, obj = got = G.host_twin(same, [1] * 4, 3)
    G.stepwise(same, [1] * 4, 3, G.NU, False, got, "all equal")
    assert (d2 == 0).all() and (obj == 0).all() and (w == 0.25).all() and g[0] == 3.0
    # one dead entry: weight exactly 0 in every w, d2 +inf, g finite
    for k in (2, 5, 9, 33):
        for bad in (np.nan, np.inf, -np.inf):
            for iters in (0, 3):
                ent, cnt = G.inputs(k, 255, 1)
                j = k // 2
                ent[j] = ent[j].copy()
                ent[j][3::7] = bad
                g, w, d2, obj = got = G.host_twin(ent, cnt, iters)
                alive = G.stepwise(ent, cnt, iters, G.NU, False, got, (k, bad, iters))
                assert not alive[j] and alive.sum() == k - 1
                assert (w[:, j] == 0).all() and np.isinf(d2[:, j]).all()
                assert np.isfinite(np.delete(w, j, 1)).all() and np.isfinite(g).all()
                assert np.isfinite(obj).all()
    # every entry dead: g is all NaN
    ent = [np.full(255, np.nan, np.float32) for _ in range(4)]
    g, w, d2, obj = got = G.host_twin(ent, [1] * 4, 2)
    G.stepwise(ent, [1] * 4, 2, G.NU, False, got, "all dead")
    assert np.isnan(g).all() and np.isinf(d2).all()
    assert np.isnan(G.text(ent, [1] * 4, 2)[0]).all()


@pytest.mark.parametrize("k,f", ((9, 2), (16, 5), (64, 20)))
def test_robustness(k, f):
    """Honest rows around a common offset and f rows replaced by far outliers: the geometric
    median stays within half the closest honest row's distance of the honest mean, where the
    plain mean is more than 50 such distances away.  On the text first (an input condition,
    never skipped), then on the host twin."""
    P, iters = 4101, 8
    ent, cnt = G.inputs(k, P)
    rows = [(e / np.float32(c) + np.float32(0.5)).astype(np.float32) for e, c in zip(ent, cnt)]
    rs = np.random.RandomState(77 + k)
    for j in range(f):
        rows[j] = (1e3 * rs.standard_normal(P)).astype(np.float32)
    honest = np.stack(rows[f:]).astype(np.float64)
    hm = honest.mean(0)
    near = np.sqrt(((honest - hm) ** 2).sum(1)).min()
    plain = np.stack(rows).astype(np.float64).mean(0)
    ones = [1] * k
    g_t = G.text(rows, ones, iters)[0]
    assert np.linalg.norm(g_t - hm) <= 0.5 * near, np.linalg.norm(g_t - hm) / near
    assert np.linalg.norm(plain - hm) > 50 * near, np.linalg.norm(plain - hm) / near
    g = G.host_twin(rows, ones, iters)[0]
    assert np.linalg.norm(g - hm) <= 0.5 * near, np.linalg.norm(g - hm) / near


def test_rules_over_the_flattened_model():
    """flsim/robust.py itself: the list form is what Agg(rule) calls; the distances are over all
    tensors together, the input shapes are kept."""
    from FL.agents import Agg
    from flsim.robust import check_geomed, geomed_flat, geomed_rule, geomed_steps
    gen = torch.Generator().manual_seed(5)
    ups = [[torch.randn(4, 3, generator=gen), torch.randn(5, generator=gen)] for _ in range(7)]
    ups[3] = [u + 50 for u in ups[3]]
    out = Agg(lambda u: geomed_rule(u, iters=8)).rule(ups)
    flat = [torch.cat([t.reshape(-1) for t in u]) for u in ups]
    g, w, d2, obj = geomed_flat(flat, [1] * 7, 8, 1e-6, False)
    assert torch.equal(torch.cat([t.reshape(-1) for t in out]), g)
    assert [t.shape for t in out] == [t.shape for t in ups[0]]
    assert int(torch.argmin(w[-1])) == 3 and len(w) == 9 and len(d2) == 8 and len(obj) == 8
    mean = torch.stack(flat).mean(0)
    honest = torch.stack(flat[:3] + flat[4:]).mean(0)
    assert (g - honest).norm() < 0.25 * (mean - honest).norm()
    dflt = geomed_rule(ups)
    assert torch.equal(torch.cat([t.reshape(-1) for t in dflt]), geomed_flat(flat, [1] * 7)[0])
    cw = geomed_rule(ups, 2, 1e-6, [1, 2, 3, 4, 1, 2, 3])
    alpha = torch.tensor([1, 2, 3, 4, 1, 2, 3], dtype=torch.float64)
    assert torch.equal(torch.cat([t.reshape(-1) for t in cw]),
                       geomed_steps(torch.stack(flat), alpha, 2, 1e-6)[0])
    assert not torch.equal(cw[0], geomed_rule(ups, 2)[0])
    assert check_geomed(3, 1e-6, None, 7) == (3, 1e-6, "uniform")
    assert check_geomed(0, 2.0, "count", 1) == (0, 2.0, "count")
    with pytest.raises(IndexError):
        geomed_rule([])
    with pytest.raises(IndexError):
        check_geomed(3, 1e-6, None, 0)
    for iters, nu, wt, what in ((-1, 1e-6, None, "Invalid iters"), (33, 1e-6, None, "Invalid iters"),
                                (3, 0.0, None, "Invalid nu"), (3, -1.0, None, "Invalid nu"),
                                (3, float("nan"), None, "Invalid nu"),
                                (3, float("inf"), None, "Invalid nu"),
                                (3, 1e-6, "median", "Invalid weights")):
        with pytest.raises(ValueError, match=what):
            check_geomed(iters, nu, wt, 5)
    with pytest.raises(ValueError, match="Invalid iters"):
        geomed_rule(ups, iters=40)
    with pytest.raises(ValueError, match="weights"):
        geomed_rule(ups, weights=[1, 2])


def test_parse_rule():
    from flsim.robust import parse_rule
    assert parse_rule("geomed") == ("geomed", 3, 1e-6, "uniform")
    assert parse_rule(("geomed", 5)) == ("geomed", 5, 1e-6, "uniform")
    assert parse_rule(["geomed", 0, 1e-3]) == ("geomed", 0, 1e-3, "uniform")
    assert parse_rule(("geomed", 32, 0.5, "count")) == ("geomed", 32, 0.5, "count")
    assert parse_rule("median") == ("median", 0) and parse_rule(None) is None
    assert parse_rule(("krum", 2)) == ("krum", 2, 1)
    for bad in (("geomed", -1), ("geomed", 33), ("geomed", 3, 0.0), ("geomed", 3, float("nan")),
                ("geomed", 3, float("inf")), ("geomed", 3, 1e-6, "mean"),
                ("geomed", 3, 1e-6, "count", 1), ("geomed", "x"), "geo", "krum"):
        with pytest.raises(ValueError, match="robust_rule"):
            parse_rule(bad)


# ---- refusals of the entry point (status 1, before any launch) -------------------------------------
F = {name: 0x1000000 * (i + 1) for i, name in enumerate(
    ["p", "m", "v", "g", "G", "D", "O", "e0", "e1", "e2", "sp", "sw", "sd", "so", "st"])}
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


def _scratch(partials=None, n=1 << 20, w=None, d2=None, obj=None, state=None):
    from flsim._lib import FlsimGeomedScratch
    s = FlsimGeomedScratch()
    s.partials = F["sp"] if partials is None else partials
    s.n_partials = n
    s.w = F["sw"] if w is None else w
    s.d2 = F["sd"] if d2 is None else d2
    s.obj = F["so"] if obj is None else obj
    s.state = F["st"] if state is None else state
    return s


def _call(iters=3, nu=1e-6, weighted=0, counts=(1, 3, 4), ents=None, scratch="default", clip=None,
          g_out=0, p=None, mm=0, v=0, n=P, step=1, optim="sgd"):
    from flsim._lib import lib
    ents = [F["e0"], F["e1"], F["e2"]][:len(counts)] if ents is None else ents
    ents = list(ents) + [0] * (min(len(counts), 64) - len(ents))
    r, _ = G.c_geomed(None, list(counts), iters, nu, 0, ptrs=ents)
    r.k = len(counts)
    r.weighted = weighted
    s = _scratch() if scratch == "default" else scratch
    o = None if optim is None else (optim if not isinstance(optim, str) else
                                     _optim(kind=optim, lr=0.1))
    vp = ctypes.c_void_p
    rc = lib().flsim_geomed_optim_step(
        ctypes.byref(r), None if s is None else ctypes.byref(s),
        None if clip is None else ctypes.byref(clip), vp(g_out), vp(F["p"] if p is None else p),
        vp(mm), vp(v), n, step, None if o is None else ctypes.byref(o), None)
    return rc, lib().flsim_last_error().decode()


N_HYPER = 14        # the leading REFUSALS that are about flsim_geomed alone
REFUSALS = [
    (dict(counts=()), "k = 0 entries"),
    (dict(counts=(1,) * 65), "k = 65 entries"),
    (dict(iters=-1), "Invalid iters = -1"),
    (dict(iters=33), "Invalid iters = 33"),
    (dict(nu=0.0), "Invalid nu"),
    (dict(nu=-1e-6), "Invalid nu"),
    (dict(nu=float("nan")), "Invalid nu"),
    (dict(nu=float("inf")), "Invalid nu"),
    (dict(nu=float("-inf")), "Invalid nu"),
    (dict(weighted=2), "Invalid weighted = 2"),
    (dict(weighted=-1), "Invalid weighted = -1"),
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
    (dict(scratch=None), "null geometric-median scratch"),
    (dict(scratch=_scratch(partials=0)), "null geometric-median scratch"),
    (dict(scratch=_scratch(w=0)), "null geometric-median scratch"),
    (dict(scratch=_scratch(d2=0)), "null geometric-median scratch"),
    (dict(scratch=_scratch(obj=0)), "null geometric-median scratch"),
    (dict(scratch=_scratch(state=0)), "null geometric-median scratch"),
    (dict(scratch=_scratch(partials=F["sp"] + 8)), "scratch must be 16-byte aligned"),
    (dict(scratch=_scratch(w=F["sw"] + 8)), "scratch must be 16-byte aligned"),
    (dict(scratch=_scratch(d2=F["sd"] + 8)), "scratch must be 16-byte aligned"),
    (dict(scratch=_scratch(obj=F["so"] + 8)), "scratch must be 16-byte aligned"),
    (dict(scratch=_scratch(state=F["st"] + 4)), "scratch must be 16-byte aligned"),
    (dict(scratch=_scratch(n=3)), "n_partials = 3, this step writes 4"),
    (dict(scratch=_scratch(w=F["sp"] + 16)), "scratch buffers overlap"),
    (dict(scratch=_scratch(state=F["sw"] + 80)), "scratch buffers overlap"),
    (dict(scratch=_scratch(state=F["p"] + 16)), "scratch overlaps p/m/v/g_out"),
    (dict(scratch=_scratch(obj=F["G"] + 16), clip=_clip()), "scratch overlaps clip G"),
    (dict(ents=[F["e0"], F["e1"] + 2, F["e2"]]), "entry 1 must be 4-byte aligned"),
    (dict(ents=[F["e0"], F["p"], F["e2"]]), "entry 1 overlaps"),
    (dict(ents=[F["p"] + 4 * (P - 1), F["e1"], F["e2"]]), "entry 0 overlaps"),
    (dict(ents=[F["e0"], F["e1"], F["p"] - 4 * (P - 1)]), "entry 2 overlaps"),
    (dict(optim="adam", mm=F["m"], v=F["v"], ents=[F["m"] + 16, F["e1"], F["e2"]]),
     "entry 0 overlaps"),
    (dict(optim="adam", mm=F["m"], v=F["v"], ents=[F["e0"], F["v"], F["e2"]]), "entry 1 overlaps"),
    (dict(g_out=F["g"], ents=[F["e0"], F["e1"], F["g"] + 32]), "entry 2 overlaps"),
    (dict(clip=_clip(), ents=[F["G"] + 4, F["e1"], F["e2"]]), "entry 0 overlaps clip G"),
    (dict(ents=[F["sp"] + 8, F["e1"], F["e2"]]), "entry 0 overlaps the geometric-median scratch"),
    (dict(ents=[F["e0"], F["sw"] - 4 * (P - 1), F["e2"]]),
     "entry 1 overlaps the geometric-median scratch"),
    (dict(ents=[F["e0"], F["e1"], F["sd"] + 16]), "entry 2 overlaps the geometric-median scratch"),
    (dict(ents=[F["e0"], F["e1"], F["so"]]), "entry 2 overlaps the geometric-median scratch"),
    (dict(ents=[F["st"], F["e1"], F["e2"]]), "entry 0 overlaps the geometric-median scratch"),
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
    do not overlap, so the next check is reached; flsim_geomed_partials is what the step asks for;
    with iters = 0 the empty d2 and obj overlap nothing."""
    from flsim._lib import lib
    L = lib()
    rc, err = _call(iters=40, p=0, ents=[0, 0, 0], scratch=None)
    assert rc == 1 and "Invalid iters = 40" in err
    rc, err = _call(ents=[F["p"] - 4 * P, F["p"] + 4 * P, F["e2"]], clip=_clip(n=0))
    assert rc == 1 and "n_partials" in err
    rc, err = _call(iters=0, scratch=_scratch(d2=F["sw"] + 16, obj=F["p"] + 16), clip=_clip(n=0))
    assert rc == 1 and "clip n_partials" in err, err
    for k in G.KS:
        E = L.flsim_geomed_tile_elems(k)
        assert E >= 256 and E % 256 == 0
        for n in (1, E - 1, E, E + 1, 3 * E + 5, 5596090, (1 << 31) - 1):
            need = L.flsim_geomed_partials(n, k)
            assert need >= k + 1 and need % (k + 1) == 0
            rc, err = _call(counts=(1,) * k, n=n, scratch=_scratch(n=need - 1))
            assert rc == 1 and f"this step writes {need}" in err, err
        assert L.flsim_geomed_partials(E, k) < L.flsim_geomed_partials(E + 1, k)
    assert L.flsim_geomed_partials(0, 8) == 0 and L.flsim_geomed_partials(8, 65) == 0
    assert L.flsim_geomed_tile_elems(0) == 0 and L.flsim_geomed_tile_elems(65) == 0
    vp = ctypes.c_void_p
    w, d2, obj = np.zeros(33 * 64), np.zeros(32 * 64), np.zeros(32)
    a = (w.ctypes.data_as(vp), d2.ctypes.data_as(vp), obj.ctypes.data_as(vp), None)
    for kw, message in REFUSALS[:N_HYPER]:
        counts = list(kw.get("counts", (1, 3, 4)))
        ent = [np.ones(4, np.float32) for _ in counts[:64]]
        r, keep = G.c_geomed(ent, counts, kw.get("iters", 3), kw.get("nu", 1e-6))
        r.k = len(counts)
        r.weighted = kw.get("weighted", 0)
        assert L.flsim_geomed_eval_host(ctypes.byref(r), 4, *a) == 1
        assert message in L.flsim_last_error().decode()
    r, keep = G.c_geomed([np.ones(4, np.float32)] * 3, [1] * 3, 3)
    assert L.flsim_geomed_eval_host(ctypes.byref(r), 0, *a) == 1
    assert L.flsim_geomed_eval_host(ctypes.byref(r), 4, None, a[1], a[2], None) == 1
    assert L.flsim_geomed_eval_host(ctypes.byref(r), 4, a[0], None, a[2], None) == 1
    assert L.flsim_geomed_eval_host(None, 4, *a) == 1
    assert L.flsim_geomed_eval_host(ctypes.byref(r), 4, *a) == 0


def test_geomed_object():
    from flsim.engine import GeoMed
    e = [torch.zeros(8) for _ in range(3)]
    r = GeoMed(3, 1e-6, True, e, [1, 3, 4])
    c = r.c_struct()
    assert (c.iters, c.weighted, c.k, c.nu) == (3, 1, 3, 1e-6) and list(c.count[:3]) == [1, 3, 4]
    assert c.entries[0] == e[0].data_ptr() and r.k == 3
    assert GeoMed(0, 1.0, False, [None] * 3, [4] * 3).c_struct().entries[0] is None
    with pytest.raises(ValueError, match="counts"):
        GeoMed(3, 1e-6, False, e, [1, 2])
    with pytest.raises(ValueError, match="65 entries"):
        GeoMed(3, 1e-6, False, [None] * 65, [1] * 65)


# ---- FLSimulation on a CPU stand-in (mirrors the one of tests/test_cpu_krum.py) -------------------
class StandInEngine:
    SIZES = [40, 24]
    STATS_PER_WORKER = 0

    def __init__(self):
        self.P = sum(self.SIZES)
        self.chunk_workers = 3
        self.acc = torch.zeros(self.P, dtype=torch.float64)

    def begin_epoch(self, theta):
        self.acc.zero_()

    def run_chunk(self, theta, pool, workers_dev, n_chunk, n_total, seed, dropout, loss_out,
                  backward=True):
        for j, (t, i, k, _) in enumerate(workers_dev.tolist()):
            self.acc += torch.arange(self.P, dtype=torch.float64).mul_(0.1 * (i + 1)).sin_() + k
            loss_out[j] = float(t + 0.001 * i)

    def end_epoch(self, S):
        S.copy_(self.acc.float())

    def aggregate_rule(self, S, rule, theta, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                       S_out=None, optim=None, **kw):
        if S_out is not None:
            S_out[:self.P].copy_(S)
        theta -= 0.125 * S / rule.k

    def geomed_step(self, gm, theta, m, v, step, optim=None, clip=None, **kw):
        from flsim.robust import geomed_flat
        g, w, d2, obj = geomed_flat(gm.entries, gm.counts, gm.iters, gm.nu, gm.weighted)
        gm.w, gm.obj = torch.stack(w), torch.stack(obj) if obj else torch.zeros(0)
        gm.d2 = torch.stack(d2) if d2 else torch.zeros(0, gm.k)
        theta -= optim.lr * g


class BNStandIn(StandInEngine):
    STATS_PER_WORKER = 8


def _sim(engine=None, **kw):
    from flsim.sim import FLSimulation
    eng = engine or StandInEngine()
    kw.setdefault("delay", 2)
    return FLSimulation(kw.pop("n", 6), device="cpu", engine=eng, device_pool=object(),
                        theta0=torch.zeros(eng.P), optimizer="sgd", lr=0.125, **kw)


def test_constructor_accepts_and_refuses():
    ind = dict(semantics="independent")
    assert _sim(robust_rule="geomed", **ind).robust == ("geomed", 3, 1e-6, "uniform")
    assert _sim(robust_rule=("geomed", 5, 1e-3, "count"), **ind).robust == \
        ("geomed", 5, 1e-3, "count")
    for bad in (("geomed", 33), ("geomed", 3, 0.0), ("geomed", 3, 1e-6, "mean")):
        with pytest.raises(ValueError, match="robust_rule"):
            _sim(robust_rule=bad, **ind)
    rule = "geomed"
    for sem in ("reference", "torch1"):
        with pytest.raises(NotImplementedError, match="independent"):
            _sim(robust_rule=rule, semantics=sem)
    with pytest.raises(NotImplementedError, match="distributed"):
        _sim(robust_rule=rule, distributed=True, **ind)
    with pytest.raises(NotImplementedError, match="staleness discount"):
        _sim(robust_rule=rule, stale_weight=("poly", 0.5), **ind)
    with pytest.raises(NotImplementedError, match="delay compensation"):
        _sim(robust_rule=rule, delay_comp=0.5, **ind)
    with pytest.raises(NotImplementedError, match="batch_size"):
        _sim(robust_rule=rule, batch_size=64, **ind)
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        _sim(BNStandIn(), robust_rule=rule, **ind)
    with pytest.raises(ValueError, match="buckets"):
        _sim(robust_rule=rule, buckets=0, **ind)


@pytest.mark.parametrize("weights", ("uniform", "count"))
def test_epoch_entries_log_and_refusals(weights):
    """n = 6, worker 5 slow with delay 2, four buckets: the entries are the buckets of the five fast
    workers, then a popped class slot; theta and geomed_log() follow the text over last_entries."""
    from flsim.robust import geomed_flat
    sim = _sim(robust_rule=("geomed", 2, 1e-6, weights), buckets=4, keep_entries=True,
               semantics="independent")
    assert sim.last_geomed is None and sim.geomed_log() == []
    pops = 0
    for t in range(5):
        before = sim.theta.clone()
        sim.epoch()
        ents, counts = sim.last_entries
        plan = sim.trace[-1]
        assert counts[:4] == [1, 1, 1, 2] and len(ents) == 4 + bool(plan.stale)
        pops += bool(plan.stale)
        g, w, d2, obj = geomed_flat(ents, counts, 2, 1e-6, weights == "count")
        assert torch.equal(sim.theta, before - 0.125 * g)
        assert sim.last_geomed.k == len(ents) and sim.last_geomed.weighted == (weights == "count")
        o, wf = sim.geomed_log()[-1]
        assert o == [float(x) for x in obj] and wf == [float(x) for x in w[-1]]
        assert all(type(x) is float for x in o + wf)
    assert pops >= 1 and len(sim.geomed_log()) == 5
    ind = dict(semantics="independent")
    big = _sim(n=70, robust_rule="geomed", buckets=65, **ind)
    with pytest.raises(ValueError, match="65 entries"):
        big.epoch()
    # k = 1 and k = 2 are fine (Krum needs three entries)
    one = _sim(robust_rule="geomed", buckets=1, **ind)
    one.epoch()
    # without keep_entries nothing is kept
    assert one.last_geomed is None and one.last_entries is None and len(one.geomed_log()) == 1


def test_checkpoint_config_round_trip():
    """The config a checkpoint records holds the rule as [kind, iters, nu, weights]; a run whose
    rule differs refuses the checkpoint.  (A robust run needs the independent-entry semantics,
    whose state no checkpoint holds yet: the recorded config is moved into a reference-semantics
    checkpoint.)"""
    kw = dict(buckets=4, semantics="independent")
    a = _sim(robust_rule=("geomed", 5), **kw)
    assert a._stale_config()["robust_rule"] == ["geomed", 5, 1e-6, "uniform"]
    cfg = _sim(robust_rule=("geomed", 2, 1e-3, "count"), **kw)._stale_config()
    assert cfg["robust_rule"] == ["geomed", 2, 1e-3, "count"] and cfg["buckets"] == 4
    with pytest.raises(NotImplementedError, match="independent"):
        a.checkpoint()
    plain = _sim(buckets=4)
    plain.epoch()
    ck = plain.checkpoint()
    assert ck["config"]["robust_rule"] is None
    _sim(buckets=4).restore(ck)
    for rule in (["geomed", 3, 1e-6, "uniform"], ["geomed", 2, 1e-3, "count"]):
        with pytest.raises(ValueError, match="robust_rule"):
            _sim(buckets=4).restore(dict(ck, config=dict(ck["config"], robust_rule=rule)))
    # torch.save / weights_only load keeps the recorded list as it is
    import io
    buf = io.BytesIO()
    torch.save(dict(ck, config=dict(ck["config"], robust_rule=cfg["robust_rule"])), buf)
    buf.seek(0)
    back = torch.load(buf, map_location="cpu", weights_only=True)
    assert back["config"]["robust_rule"] == ["geomed", 2, 1e-3, "count"]


def test_main_arguments():
    import main
    a = main.parse(["--robust_rule", "geomed"])
    assert main.robust_spec(a) == ("geomed", 3, 1e-6, "uniform")
    a = main.parse(["--robust_rule", "geomed", "--geomed_iters", "5", "--geomed_nu", "1e-3",
                    "--geomed_weights", "count"])
    assert main.robust_spec(a) == ("geomed", 5, 1e-3, "count")
