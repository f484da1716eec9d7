"""GPU: the clipped server step (csrc/server.hip: the OK_GOUT streams, k_clip_finish, k_clip_apply
through flsim_aggregate_optim_clip_push), bit for bit against the text of tests/_clip.py:

    total_norm = float32(sqrt(sum_e float64(g_e) ** 2))          # correctly rounded
    coef       = clamp(max_norm / (total_norm + 1e-6), max=1.0)  # torch's own ops
    g'         = g * coef                                        # clip_grads_with_norm_

g is taken from the EXISTING kernels, not from the code under test: uncompensated rules through
plain SGD with lr = 1 from p = 0 (p = -g exactly), compensated ones through the host twin
flsim_cascade_eval_host_c.  The yardstick of the update is the unclipped step of the existing API on
g' (aggregate_adam_sum(g', 1, ...)), with g' from clip_grads_with_norm_ on the CPU.  Every case
asserts its input conditions first (tests/_clip.py): the exact norm is at least 1e-10 (relative)
away from an fp32 rounding midpoint, and g' holds no -0 (the yardstick's k = 1 rule would turn it
into +0).  Every comparison asks for zero differing words.
"""
import math

import numpy as np
import pytest
import torch

import _clip as K
import _delay_comp as D
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

DEV = "cuda:0"
SGD1 = dict(kind="sgd", lr=1.0)
LAM = 0.04
# tensor tails, a tensor below 8 elements, edge pieces only; and with streaming blocks and several
# hundred partials (the finisher's tree has depth)
LAYOUTS = {"edges": [33, 7, 1000, 4101], "stream": [33, 7, 1000, 4101, 300000]}
# (k, events [(position, array)], arrays, null arrays)
RULES = {
    "k5": (5, [(4, 0)], 1, ()),
    "k513": (513, [(512, 0)], 1, ()),
    "general": (40, [(0, 1), (7, 0), (8, 0), (21, 2), (33, 1), (39, 2)], 3, ()),
    "null": (5, [(4, 0)], 1, (0,)),
}
FORMS = ["plain", "weighted", "compensated"]
KINDS = {
    "adam": dict(kind="adam", lr=1e-3),
    "adamw": dict(kind="adamw", lr=1e-3, weight_decay=0.1),
    "sgdm": dict(kind="sgd", lr=0.01, momentum=0.9, weight_decay=1e-3),
    "sgd": dict(kind="sgd", lr=0.01),
}
QNAN = 0x7FC12345


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if a is not None else None


def _sgd(g, p, lr):
    """torch.optim.SGD's step on the CPU (the yardstick tests/test_gpu_optim.py pins the SGD
    kernels to)."""
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.SGD([tp], lr=lr)
    tp.grad = torch.from_numpy(np.ascontiguousarray(g).copy())
    opt.step()
    return tp.detach().numpy().copy()


class Case:
    """One (layout, rule, form): host inputs, the device rule, and g from the existing kernels."""

    def __init__(self, layout, rule, form):
        from flsim.engine import ProgramStager, Rule, aggregate_rule, cascade_program
        self.sizes = LAYOUTS[layout]
        self.P = P = sum(self.sizes)
        k, events, na, nulls = RULES[rule]
        rs = np.random.RandomState(1000 * list(RULES).index(rule) + 10 * FORMS.index(form) +
                                   len(self.sizes))
        self.S = K.values(rs, P)
        arrays = [K.values(rs, P, 3.0) for _ in range(na)]
        for q in nulls:
            arrays[q] = None
        self.theta, first = D.theta_pair(rs, P)
        snaps = [first] + [D.theta_src(rs, self.theta) for _ in range(na - 1)]
        w = None if form == "plain" else [D.WEIGHTS[q % 3] for q in range(na)]
        sn = snaps if form == "compensated" else None
        full = [1.0] * k
        for pos, a in events:
            full[pos] = 1.0 if w is None else w[a]
        self.dS = _dev(self.S)
        dA, dT = [_dev(a) for a in arrays], [_dev(s) for s in snaps]
        kw = {}
        if w is not None:
            kw.update(weights=w, divisor=float(sum(full)))
        if sn is not None:
            kw.update(snapshots=dT, delay_comp=LAM)
        if rule == "general":
            self.make = lambda: Rule(k, dA, events=events, stager=ProgramStager(DEV), **kw)
        else:
            self.make = lambda: Rule(k, dA, c=k - na, **kw)
        self.compensated = sn is not None
        if not self.compensated:
            # the existing stream: plain SGD, lr = 1, from p = 0 gives p = -g exactly
            dp = torch.zeros(P, device=DEV)
            aggregate_rule(self.dS, self.make(), dp, None, None, 1, self.sizes, optim=SGD1)
            self.g = -dp.cpu().numpy()
        else:
            words, info = cascade_program(k, events)
            tail = K.tail_mask(self.sizes, True)
            div = float(sum(full)) if w is not None else float(k)
            self.g_at = lambda theta: K.existing_twin(words, info, self.S, arrays, w, div,
                                                      np.ascontiguousarray(theta), sn, LAM, tail)
            self.g = self.g_at(self.theta)
        self.exact, self.norm = self.conditions(self.g)

    @staticmethod
    def conditions(g):
        """The input conditions on a case's g; -> (exact norm, its fp32 rounding)."""
        assert np.isfinite(g).all() and (g != 0).all()
        exact, norm, dist = K.exact_norm(g)
        assert dist >= K.MIN_MIDPOINT_DISTANCE, dist
        return exact, norm

    def state(self, seed=5):
        rs = np.random.RandomState(seed)
        m = (rs.standard_normal(self.P) * 1e-3).astype(np.float32)
        v = (rs.rand(self.P) * 1e-5).astype(np.float32)
        return self.theta.copy(), m, v

    def clipped(self, clip, p, m, v, step, optim, **kw):
        from flsim.engine import aggregate_rule
        aggregate_rule(self.dS, self.make(), p, m, v, step, self.sizes, optim=optim, clip=clip,
                       **kw)


CASES = [(lay, r, f) for lay in LAYOUTS for r in RULES for f in FORMS]


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(layout, rule, form):
        key = (layout, rule, form)
        if key not in cache:
            cache[key] = Case(*key)
        return cache[key]
    return get


@pytest.mark.parametrize("layout,rule,form", CASES)
def test_norm_and_coefficient(cases, layout, rule, form):
    """clip.total_norm = float32(sqrt(fsum)) and clip.coef = torch's clamp(max_norm / (t + 1e-6),
    max=1.0) with t the engine's own norm, at max_norm = 0.5x, 1x, 2x the norm and inf."""
    from flsim.engine import Clip
    C = cases(layout, rule, form)
    for mn in (float(C.norm) * 0.5, float(C.norm), float(C.norm) * 2.0, float("inf")):
        clip = Clip(mn)
        p = _dev(C.theta)
        C.clipped(clip, p, None, None, 1, SGD1)
        t, coef = clip.total_norm.cpu().numpy(), clip.coef.cpu().numpy()
        assert K.bits(t) == K.bits(C.norm), (mn, t, C.norm, C.exact)
        ref = K.torch_coef(t, mn)
        assert K.bits(coef) == K.bits(ref), (mn, coef, ref)
        assert coef == 1.0 if mn >= float(C.norm) * 2.0 else coef <= 1.0
        assert mn >= float(C.norm) or coef < 0.75
        # theta - g': torch SGD with lr = 1 on the CPU
        pe = _sgd(K.torch_clip(C.g, C.sizes, mn, t), C.theta, 1.0)
        assert int((_bits(p) != pe.view(np.uint32)).sum()) == 0, mn


@pytest.mark.parametrize("layout,rule,form", CASES)
def test_update_equals_unclipped_step_on_clipped_gradient(cases, layout, rule, form):
    """theta, m, v after the clipped step = the unclipped step of the existing API on g' (from
    clip_grads_with_norm_ on the CPU), all four kinds, steps 1 and 2; S_out and theta_out come out
    as the parent writes them; unowned m / v are passed poisoned and stay untouched.  A
    compensated rule's g depends on theta, so its step 2 takes g from the twin at the theta step 1
    left."""
    from flsim.engine import Clip, aggregate_adam_sum
    C = cases(layout, rule, form)
    mn = float(C.norm) * 0.5

    def clipped_gradient(g, norm):
        gp = K.torch_clip(g, C.sizes, mn, norm)
        assert not K.has_negative_zero(gp)                              # input condition
        assert not np.array_equal(K.bits(gp), K.bits(g))                # clipping acts
        return _dev(gp)
    dgp1 = clipped_gradient(C.g, C.norm)
    for name, o in KINDS.items():
        nstate = 2 if o["kind"] != "sgd" else (1 if o.get("momentum") else 0)
        p0, m0, v0 = C.state()
        if nstate < 1:
            m0 = np.full(C.P, QNAN, np.uint32).view(np.float32)
        if nstate < 2:
            v0 = np.full(C.P, QNAN, np.uint32).view(np.float32)
        a = [_dev(x) for x in (p0, m0, v0)]
        b = [_dev(x) for x in (p0, m0, v0)]
        arg = lambda s: [s[0], s[1] if nstate >= 1 else None,          # noqa: E731
                         s[2] if nstate >= 2 else None]
        clip = Clip(mn)
        for step in (1, 2):
            before = a[0].clone()
            dgp = dgp1
            if C.compensated and step == 2:
                g2 = C.g_at(before.cpu().numpy())
                dgp = clipped_gradient(g2, C.conditions(g2)[1])
            s_out = torch.full((C.P,), float("nan"), device=DEV)
            t_out = torch.full((C.P,), float("nan"), device=DEV) if C.compensated else None
            # (the clipped step is handed the poisoned arrays it does not own)
            C.clipped(clip, a[0], a[1], a[2], step, o, S_out=s_out, theta_out=t_out)
            aggregate_adam_sum(dgp, 1, *arg(b), step, C.sizes, optim=o)
            if C.compensated:
                assert np.array_equal(_bits(t_out), _bits(before)), (name, step)
            assert np.array_equal(_bits(s_out), K.bits(C.S)), (name, step)
            for x, y, what in zip(a, b, "pmv"):
                bad = int((_bits(x) != _bits(y)).sum())
                assert bad == 0, (name, step, what, bad)
        assert not torch.equal(a[0], _dev(p0))
        if nstate < 2:
            assert int((_bits(a[2]) != QNAN).sum()) == 0, name
        if nstate < 1:
            assert int((_bits(a[1]) != QNAN).sum()) == 0, name


@pytest.mark.parametrize("layout,rule,form", CASES)
def test_coefficient_one_equals_the_unclipped_step(cases, layout, rule, form):
    """max_norm = inf: coef = 1.0, and theta, m, v equal the unclipped step of the same rule bit
    for bit (g * 1.0 is exact, -0 included), for all four kinds at steps 1 and 2."""
    from flsim.engine import Clip, aggregate_rule
    C = cases(layout, rule, form)
    clip = Clip(float("inf"))
    for name, o in KINDS.items():
        nstate = 2 if o["kind"] != "sgd" else (1 if o.get("momentum") else 0)
        p0, m0, v0 = C.state(9)
        a = [_dev(x) for x in (p0, m0, v0)]
        b = [_dev(x) for x in (p0, m0, v0)]
        arg = lambda s: [s[0], s[1] if nstate >= 1 else None,          # noqa: E731
                         s[2] if nstate >= 2 else None]
        for step in (1, 2):
            C.clipped(clip, *arg(a), step, o)
            aggregate_rule(C.dS, C.make(), *arg(b), step, C.sizes, optim=o)
            assert float(clip.coef) == 1.0
            for x, y, what in zip(a, b, "pmv"):
                bad = int((_bits(x) != _bits(y)).sum())
                assert bad == 0, (name, step, what, bad)


def test_minus_zero_gradient_survives_the_apply():
    """A -0 gradient (the rule's division rounds -1e-45 / 5 to -0) stays -0 through g * 1.0 and
    the update: plain SGD at p = -0 gives fma(-0, -lr, -0) = +0 + -0 = +0 for g = -0 but -0 for
    g = +0, so the sign of the zero is visible in theta."""
    from flsim.engine import Clip, Rule, aggregate_rule
    sizes = [64, 40]
    P = sum(sizes)
    S = np.linspace(-1, 1, P).astype(np.float32)
    S[3::7] = np.float32(-1e-45)
    S[4::7] = np.float32(1e-45)
    p0 = np.full(P, -0.0, np.float32)
    res = []
    for clip in (None, Clip(float("inf"))):
        p = _dev(p0)
        aggregate_rule(_dev(S), Rule(5, [None] * 4, c=1), p, None, None, 1, sizes,
                       optim=dict(kind="sgd", lr=0.5), clip=clip)
        res.append(_bits(p))
    assert np.array_equal(res[0], res[1])
    assert (res[0][3::7] == 0).all() and (res[0][4::7] == 0x80000000).all()


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_results_ignore_scratch_contents(cases, layout):
    """G, partials and out pre-poisoned with NaN, then with another pattern: the same bits as on
    fresh scratch (nothing relies on the buffers' earlier contents), run after run."""
    from flsim.engine import Clip
    C = cases(layout, "general", "weighted")
    o = KINDS["adam"]
    res = []
    for pattern in (None, QNAN, QNAN, 0x40490FDB):
        clip = Clip(float(C.norm) * 0.5)
        clip.c_struct(torch.device(DEV), C.P)
        if pattern is not None:
            signed = pattern - (1 << 32) if pattern >= 1 << 31 else pattern
            for buf in clip._scratch[(DEV, C.P)]:
                buf.view(torch.int32).fill_(signed)
        d = [_dev(x) for x in C.state()]
        for step in (1, 2):                     # twice: the second run reads what the first left
            C.clipped(clip, *d, step, o)
        res.append([_bits(x) for x in d] + [_bits(clip.total_norm.reshape(1)),
                                            _bits(clip.coef.reshape(1))])
    for r in res[1:]:
        for x, y in zip(res[0], r):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_against_torch_clip_grad_norm(cases, layout):
    """torch's own clip_grad_norm_ end to end: its norm accumulates in fp32, ours is the correctly
    rounded one, so |ours - torch's| <= |torch's - exact| + 1 ulp (the triangle inequality)."""
    from flsim.engine import Clip
    C = cases(layout, "k513", "plain")
    params, off = [], 0
    for n in C.sizes:
        q = torch.nn.Parameter(torch.zeros(n))
        q.grad = torch.from_numpy(C.g[off:off + n].copy())
        params.append(q)
        off += n
    mn = float(C.norm) * 0.5
    t_torch = float(torch.nn.utils.clip_grad_norm_(params, mn))
    clip = Clip(mn)
    C.clipped(clip, _dev(C.theta), None, None, 1, SGD1)
    ours = float(clip.total_norm)
    ulp = float(np.spacing(np.float32(C.exact)))
    d_ours, d_torch = abs(ours - t_torch), abs(t_torch - C.exact)
    print(f"MEASURED layout={layout} P={C.P} |ours-torch|={d_ours:.3e} |torch-exact|={d_torch:.3e} "
          f"ulp={ulp:.3e}")
    assert d_ours <= d_torch + ulp
    # ... and the clipped gradients agree to torch's own error in the coefficient
    gt = torch.cat([q.grad for q in params]).numpy()
    gp = K.torch_clip(C.g, C.sizes, mn, ours)
    assert np.allclose(gt, gp, rtol=4 * (d_torch / C.exact + 2.0 ** -23), atol=3e-45)


def test_refused_on_the_device_like_on_the_host(cases):
    """G aliasing p or S, and too few partials: status 1 (ValueError), nothing launched."""
    from flsim.engine import Clip
    C = cases("edges", "k5", "plain")
    clip = Clip(1.0)
    c = clip.c_struct(torch.device(DEV), C.P)
    G, partials, out = clip._scratch[(DEV, C.P)]
    p = _dev(C.theta)
    before = p.clone()
    clip._scratch[(DEV, C.P)] = (p, partials, out)
    with pytest.raises(ValueError, match="overlaps"):
        C.clipped(clip, p, None, None, 1, SGD1)
    clip._scratch[(DEV, C.P)] = (G, partials[:2], out)
    with pytest.raises(ValueError, match="n_partials"):
        C.clipped(clip, p, None, None, 1, SGD1)
    torch.cuda.synchronize()
    assert torch.equal(p, before) and c.max_norm == 1.0


# ---- FLSimulation on PN1 ------------------------------------------------------------------------
N, DELAY, EPOCHS, LR = 4, 2, 6, 0.01
SIMS = {
    "adam": dict(optimizer="adam", lr=1e-3),
    "sgd_comp_weights": dict(optimizer="sgd", lr=LR, delay_comp=1.0e4, stale_weight=("poly", 0.5)),
}


@pytest.fixture(scope="module")
def pool():
    from oracle import oracle as O
    return O.make_pool(0)


def _sim(pool, cfg, clip):
    from flsim.sim import FLSimulation
    return FLSimulation(N, delay=DELAY, throttle=True, device=DEV, chunk_workers=2, pool=pool,
                        keep_S=True, clip_grad_norm=clip, **SIMS[cfg])


def _run(sim):
    rec = []
    for _ in range(EPOCHS):
        sim.epoch()
        rec.append((sim.comm[:sim.P].cpu().numpy().copy(), sim.theta.clone()))
    return rec


@pytest.mark.parametrize("cfg", list(SIMS))
def test_simulation_bit_exact_and_inf_equals_none(pool, cfg):
    """n = 4, d = 2, 6 epochs across two ticks.  Each epoch, g' is rebuilt on the CPU with torch
    from the run's own S_t, popped slots and snapshots, and an independent theta / m / v copy is
    stepped through the unclipped API: the simulation's theta equals it bit for bit.  The run with
    clip_grad_norm = inf is bit-identical to the run with None, epoch by epoch."""
    from flsim.engine import aggregate_adam_sum, staleness_weight
    none = _run(_sim(pool, cfg, None))
    s_inf = _sim(pool, cfg, float("inf"))
    inf = _run(s_inf)
    for (_, a), (_, b) in zip(none, inf):
        assert np.array_equal(_bits(a), _bits(b))
    norms = s_inf.grad_norms()
    assert len(norms) == EPOCHS and all(math.isfinite(x) and x > 0 for x in norms)
    mn = 0.5 * min(norms)                       # clips every epoch
    sim = _sim(pool, cfg, mn)
    theta0 = sim.theta.cpu().numpy().copy()
    rec = _run(sim)
    norms = sim.grad_norms()
    assert len(norms) == EPOCHS and all(math.isfinite(x) and x > mn for x in norms)
    sizes = list(sim.engine.SIZES)
    o = sim.optim
    lam = SIMS[cfg].get("delay_comp")
    sfn = staleness_weight(SIMS[cfg].get("stale_weight"))
    th = _dev(theta0)
    m = torch.zeros_like(th) if o.n_state >= 1 else None
    v = torch.zeros_like(th) if o.n_state >= 2 else None
    before = [theta0] + [t.cpu().numpy() for (_, t) in rec[:-1]]          # theta_t, per epoch
    ticks = 0
    for t, (plan, (S, theta)) in enumerate(zip(sim.trace, rec)):
        ents = [S] * plan.c_t + [rec[src][0] for (_, src) in plan.stale]
        snaps = [None] * plan.c_t + [before[src] if lam is not None else None
                                     for (_, src) in plan.stale]
        ws = [float(sfn(t - src)) for (_, src) in plan.stale]
        full = None if all(w == 1.0 for w in ws) else [1.0] * plan.c_t + ws
        ticks += bool(plan.stale)
        g = D.text_flat(ents, snaps, before[t], lam or 0.0, full, sizes)
        assert np.isfinite(g).all()
        # the norm: float64 pairwise sum (its error, about 1e-15, is far inside the distance asked)
        g64 = g.astype(np.float64)
        exact = math.sqrt(float(np.sum(g64 * g64)))
        f = np.float32(exact)
        mids = [(float(f) + float(np.nextafter(f, np.float32(s)))) / 2 for s in (np.inf, -np.inf)]
        assert min(abs(exact - x) for x in mids) / exact >= K.MIN_MIDPOINT_DISTANCE
        assert K.bits(np.float32(norms[t])) == K.bits(f), (t, norms[t], exact)
        gp = K.torch_clip(g, sizes, mn, np.float32(norms[t]))
        assert not K.has_negative_zero(gp)                              # input condition
        aggregate_adam_sum(_dev(gp), 1, th, m, v, t + 1, sizes, optim=o)
        bad = int((_bits(th) != _bits(theta)).sum())
        print(cfg, t, plan.c_t, plan.stale, "norm", norms[t], "differing words:", bad)
        assert bad == 0, (t, bad)
    assert ticks == 2
    assert not np.array_equal(_bits(rec[-1][1]), _bits(none[-1][1]))    # clipping acts


def test_facade_clips_between_grad_and_step(pool):
    """Central(model, optim, clip_grad_norm=): one epoch of two workers through FL.agents; theta
    equals torch SGD on clip_grads_with_norm_ of the gradient read back; central.total_norm is the
    engine's norm."""
    import torch.nn as nn
    from FL.agents import Agg, Central, Worker, rule
    from FL.models import PerformantNet1
    from flsim.engine import PN1_SIZES
    from oracle import oracle as O
    torch.manual_seed(0)
    model = PerformantNet1().to(DEV)
    central = Central(model, torch.optim.SGD(model.parameters(), lr=LR), clip_grad_norm=0.05)
    ws = [Worker(nn.CrossEntropyLoss()) for _ in range(2)]
    model.train()
    ups = None
    for i, w in enumerate(ws):
        w.model = model
        rs = np.random.RandomState(10 + i)
        idx = rs.randint(0, pool[0].shape[0], 128)
        ups, _ = w.fwd_bkwd(torch.from_numpy(O.normalize_lut()[pool[0][idx]]).to(DEV),
                            torch.from_numpy(pool[1][idx]).to(DEV))
    ctx = central.ctx
    S = torch.cat([t.reshape(-1) for t in ups]).cpu().numpy().copy()
    before = ctx.theta[:ctx.P].cpu().numpy().copy()
    central.update_model(Agg(rule).rule([ups, ups]))
    after = ctx.theta[:ctx.P].cpu().numpy().copy()
    g = D.text_flat([S, S], [None, None], before, 0.0, None, PN1_SIZES)
    g64 = g.astype(np.float64)
    f = np.float32(math.sqrt(float(np.sum(g64 * g64))))
    t = np.float32(float(central.total_norm))
    assert abs(float(t) - float(f)) <= float(np.spacing(f)) and float(t) > 0.05
    pe = _sgd(K.torch_clip(g, PN1_SIZES, 0.05, t), before, LR)
    assert int((pe.view(np.uint32) != after.view(np.uint32)).sum()) == 0
