"""GPU: the delay-compensated server step (csrc/server.hip's C kernels through
flsim_aggregate_optim_crule_push and flsim_<net>_server_step_crule), bit for bit against the text of
tests/_delay_comp.py evaluated by torch on the CPU:

    def compensate(x, theta_now, theta_src, lam):          # per parameter tensor, fp32
        return x + (x * x) * lam * (theta_now - theta_src)

g is read through plain SGD with lr = 1 on a non-zero theta (theta enters g now; it is small next
to g, so theta - g keeps g's low bits); Adam and SGD with momentum use the oracle's adam_step /
torch SGD as tests/test_gpu_optim.py does.  Every comparison asks for zero differing words.  Each
test asserts its input conditions on the CPU first: g finite, compensation changing more than 10 %
of the elements, and a contracted evaluation (the last product and the add in one rounding)
differing from the text in at least 10 elements -- a compiler that contracts cannot pass.
"""
import types

import numpy as np
import pytest
import torch

import _delay_comp as D
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

DEV = "cuda:0"
SGD1 = dict(kind="sgd", lr=1.0)
# (sizes, c, n_stale): > 8 row_sum tails -> split launches, the LDS-staged stream (3 entry arrays);
# the register streams with one (NY = 1) and two (NY = 2) stale arrays
LAYOUTS = {
    "tails_lds": ([5, 37, 64, 1, 96, 100, 33, 2, 3, 70, 9, 11], 6, 3),
    "reg_ny1": ([1000, 4096, 33, 7], 3, 1),
    "reg_ny2": ([1000, 4096, 33, 7], 3, 2),
}
GENERAL = dict(sizes=[1000, 4096, 33, 7], k=40,
               events=[(0, 1), (7, 0), (8, 0), (21, 2), (33, 3), (39, 1)],   # array 2 = zeros
               aw=[D.WEIGHTS[0], D.WEIGHTS[1], D.WEIGHTS[2], 1.0])
ALL_LAYOUTS = ["tails_lds", "reg_ny1", "reg_ny2", "general"]


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _sgd_expected(g, p, lr=1.0, momentum=0.0, buf=None):
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.SGD([tp], lr=lr, momentum=momentum)
    tp.grad = torch.from_numpy(g.copy())
    if buf is not None:
        opt.state[tp]["momentum_buffer"] = torch.from_numpy(buf.copy())
    opt.step()
    nb = opt.state[tp]["momentum_buffer"].numpy().copy() if momentum else None
    return tp.detach().numpy().copy(), nb


def _case(layout):
    """(sizes, k, events, arrays' weights, make_rule(dev arrays, **kw))"""
    from flsim.engine import ProgramStager, Rule
    if layout == "general":
        G = GENERAL
        return (G["sizes"], G["k"], G["events"], G["aw"],
                lambda d, **kw: Rule(G["k"], d, events=G["events"], stager=ProgramStager(DEV),
                                     **kw))
    sizes, c, ns = LAYOUTS[layout]
    aw = (D.WEIGHTS[:ns - 1] + [1.0]) if ns == 3 else D.WEIGHTS[:ns]
    return (sizes, c + ns, [(c + q, q) for q in range(ns)], aw,
            lambda d, **kw: Rule(c + ns, d, c=c, **kw))


class _Inputs:
    """One layout's host inputs: S_t (+-1e30 lane), the stale arrays (+-1e15 lane; array 2 of the
    general order is a torch-1.x zero entry), theta_now and one snapshot per array (theta_now +
    noise of about 1e-3, every fifth element equal)."""

    def __init__(self, layout, seed):
        self.sizes, self.k, self.events, self.aw, self.make = _case(layout)
        self.P = P = sum(self.sizes)
        rs = np.random.RandomState(seed)
        self.S = D.values_S(rs, P)
        self.arrays = [D.values_comp(rs, P) for _ in self.aw]
        if layout == "general":
            self.arrays[2] = None
        self.theta, first = D.theta_pair(rs, P)
        self.snaps = [first] + [D.theta_src(rs, self.theta) for _ in self.aw[1:]]

    def text(self, lam, weighted, asnap=None, comp=D.compensate):
        """g of the text; asnap: the arrays' snapshots (default: all of them)."""
        asnap = self.snaps if asnap is None else asnap
        ents, snaps, full = [self.S] * self.k, [None] * self.k, [1.0] * self.k
        for pos, a in self.events:
            ents[pos] = self.arrays[a] if self.arrays[a] is not None else np.zeros_like(self.S)
            snaps[pos] = asnap[a] if self.arrays[a] is not None else None
            if weighted:
                full[pos] = self.aw[a]
        return D.text_flat(ents, snaps, self.theta, lam, full if weighted else None, self.sizes,
                           comp=comp)

    def dev(self):
        to = lambda a: torch.from_numpy(a).to(DEV) if a is not None else None   # noqa: E731
        return to(self.S), [to(a) for a in self.arrays], [to(s) for s in self.snaps]


@pytest.mark.parametrize("lam", D.LAMBDAS)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("layout", ALL_LAYOUTS)
def test_stream_reads_g_exactly(layout, weighted, lam):
    """theta' = theta - g: plain SGD, lr = 1, on the theta that enters g."""
    from flsim.engine import aggregate_rule
    I = _Inputs(layout, 7)
    g = I.text(lam, weighted)
    assert np.isfinite(g).all()
    pe, _ = _sgd_expected(g, I.theta)
    if lam == 2.0:      # the inputs tell compensation from none, and the text from a contraction
        plain, _ = _sgd_expected(I.text(lam, weighted, asnap=[None] * len(I.aw)), I.theta)
        contr, _ = _sgd_expected(I.text(lam, weighted, comp=D.compensate_contracted), I.theta)
        _, changed, contracted = D.input_conditions(pe, plain, contr)
        print(layout, weighted, "changed %.3f" % changed, "contracted", contracted)
        assert changed > 0.10 and contracted >= 10, (changed, contracted)
    dS, dA, dT = I.dev()
    kw = dict(weights=I.aw) if weighted else {}
    dp = torch.from_numpy(I.theta.copy()).to(DEV)
    aggregate_rule(dS, I.make(dA, snapshots=dT, delay_comp=lam, **kw), dp, None, None, 1, I.sizes,
                   optim=SGD1)
    torch.cuda.synchronize()
    bad = int((_bits(dp) != pe.view(np.uint32)).sum())
    print(layout, weighted, lam, "differing words:", bad)
    assert bad == 0
    # compensation acts: the uncompensated step gives another theta
    dq = torch.from_numpy(I.theta.copy()).to(DEV)
    aggregate_rule(dS, I.make(dA, **kw), dq, None, None, 1, I.sizes, optim=SGD1)
    assert not torch.equal(dp, dq)


@pytest.mark.parametrize("layout", ["reg_ny1", "general"])
def test_stream_adam_and_sgd_momentum(layout):
    from flsim.engine import aggregate_rule
    from oracle import oracle as O
    I = _Inputs(layout, 11)
    P = I.P
    rs = np.random.RandomState(5)
    p = I.theta
    m = (rs.standard_normal(P) * 1e-3).astype(np.float32)
    v = (rs.rand(P) * 1e-5).astype(np.float32)
    g = I.text(2.0, True)
    assert np.isfinite(g).all()
    dS, dA, dT = I.dev()
    rule = I.make(dA, weights=I.aw, snapshots=dT, delay_comp=2.0)
    # Adam, step 3 (the oracle's adam_step: correctly rounded sqrt, like the kernel's)
    pe, me, ve = p.copy(), m.copy(), v.copy()
    O.adam_step(pe, me, ve, g, 3, lr=1e-3)
    d = [torch.from_numpy(x.copy()).to(DEV) for x in (p, m, v)]
    aggregate_rule(dS, rule, *d, 3, I.sizes, lr=1e-3)
    torch.cuda.synchronize()
    bad = [int((_bits(x) != y.view(np.uint32)).sum()) for x, y in zip(d, (pe, me, ve))]
    print(layout, "adam differing words:", bad)
    assert bad == [0, 0, 0]
    # SGD momentum 0.9, step 3
    pe, be = _sgd_expected(g, p, lr=0.01, momentum=0.9, buf=m)
    d = [torch.from_numpy(x.copy()).to(DEV) for x in (p, m)]
    aggregate_rule(dS, rule, d[0], d[1], None, 3, I.sizes,
                   optim=dict(kind="sgd", lr=0.01, momentum=0.9))
    torch.cuda.synchronize()
    bad = [int((_bits(x) != y.view(np.uint32)).sum()) for x, y in zip(d, (pe, be))]
    print(layout, "sgd momentum differing words:", bad)
    assert bad == [0, 0]


@pytest.mark.parametrize("layout", ALL_LAYOUTS)
def test_stream_snapshot_write(layout):
    """With S_out and theta_out given, theta_out receives the pre-update theta and S_out S_t, and
    the update is what it is without the two writes; theta_out alone (a push without a pop: no
    snapshots) writes it too."""
    from flsim.engine import aggregate_rule
    I = _Inputs(layout, 17)
    P = I.P
    dS, dA, dT = I.dev()
    rule = lambda: I.make(dA, weights=I.aw, snapshots=dT, delay_comp=2.0)       # noqa: E731
    ref = torch.from_numpy(I.theta.copy()).to(DEV)
    aggregate_rule(dS, rule(), ref, None, None, 1, I.sizes, optim=SGD1)
    dp = torch.from_numpy(I.theta.copy()).to(DEV)
    s_out = torch.full((P,), float("nan"), device=DEV)
    t_out = torch.full((P,), float("nan"), device=DEV)
    aggregate_rule(dS, rule(), dp, None, None, 1, I.sizes, optim=SGD1, S_out=s_out,
                   theta_out=t_out)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(t_out), I.theta.view(np.uint32))
    assert np.array_equal(_bits(s_out), I.S.view(np.uint32))
    assert np.array_equal(_bits(dp), _bits(ref)) and not torch.equal(dp, t_out)
    # theta_out without any snapshot: the uncompensated rule's theta, and the snapshot
    plain = torch.from_numpy(I.theta.copy()).to(DEV)
    aggregate_rule(dS, I.make(dA, weights=I.aw), plain, None, None, 1, I.sizes, optim=SGD1)
    dq = torch.from_numpy(I.theta.copy()).to(DEV)
    t_out.fill_(float("nan"))
    aggregate_rule(dS, I.make(dA, weights=I.aw), dq, None, None, 1, I.sizes, optim=SGD1,
                   theta_out=t_out)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(t_out), I.theta.view(np.uint32))
    assert np.array_equal(_bits(dq), _bits(plain))


@pytest.mark.parametrize("layout", ALL_LAYOUTS)
def test_null_snapshots_equal_the_weighted_entry_point(layout):
    """Every snapshot NULL: the C kernels compensate nothing and must give the words of the
    weighted entry point (flsim_aggregate_optim_wrule_push)."""
    from flsim.engine import aggregate_rule
    I = _Inputs(layout, 13)
    P = I.P
    dS, dA, _ = I.dev()
    rs = np.random.RandomState(3)
    m = (rs.standard_normal(P) * 1e-3).astype(np.float32)
    v = (rs.rand(P) * 1e-5).astype(np.float32)
    wrule = I.make(dA, weights=I.aw)
    crule = I.make(dA, weights=I.aw, snapshots=[None] * len(I.aw), delay_comp=2.0)
    assert wrule.c_comp is None and crule.c_comp is not None
    for hp in (dict(lr=1e-3), dict(optim=SGD1)):
        res = []
        for rule in (wrule, crule):
            d = [torch.from_numpy(x.copy()).to(DEV) for x in (I.theta, m, v)]
            aggregate_rule(dS, rule, *d, 2, I.sizes, **hp)
            res.append(d)
        torch.cuda.synchronize()
        for x, y in zip(*res):
            assert int((x.view(torch.int32) != y.view(torch.int32)).sum()) == 0
        assert not torch.equal(res[0][0], torch.from_numpy(I.theta).to(DEV))


@pytest.fixture(scope="module")
def pool():
    from oracle import oracle as O
    return O.make_pool(0)


def test_fused_step_equals_reduce_then_stream(pool):
    """The 2-worker PN1 chunk of tests/test_gpu_stale_weight.py: the fused compensated slab step
    against end_epoch + the compensated stream: theta, the owned state arrays, S_out and the
    written snapshot bit-identical, for a tick rule and the general-order rule, with and without
    weights, SGD momentum and Adam; and it differs from the uncompensated step."""
    from flsim.data import DevicePool
    from flsim.engine import PN1Engine, ProgramStager, Rule, worker_table
    from flsim.sim import default_theta
    items = [(0, 0, 1), (0, 3, 7)]
    eng = PN1Engine(DEV, chunk_workers=len(items))
    theta = default_theta(0, eng.MODEL).to(DEV)
    eng.begin_epoch(theta)
    loss = torch.zeros(len(items), device=DEV)
    eng.run_chunk(theta, DevicePool(DEV, 0, pool), worker_table(items, DEV), len(items), 8, 0,
                  True, loss)
    P = eng.P
    S = torch.zeros(P + 64, device=DEV)
    eng.end_epoch(S)
    g = torch.Generator(device="cpu").manual_seed(11)
    arrs = [(torch.randn(P + 64, generator=g) * 1e-1).to(DEV) for _ in range(3)]
    snaps = [(theta + (torch.randn(P, generator=g) * 1e-3).to(DEV)) for _ in range(3)]
    m0 = (torch.randn(P, generator=g) * 1e-4).to(DEV)
    v0 = (torch.rand(P, generator=g) * 1e-6).to(DEV)
    ev = GENERAL["events"]
    lam = 50.0

    def tick(comp, **kw):
        ckw = dict(snapshots=[snaps[0]], delay_comp=lam) if comp else {}
        return Rule(6, [arrs[0]], c=5, **ckw, **kw)

    def general(comp, **kw):
        ckw = dict(snapshots=[snaps[0], snaps[1], None, None], delay_comp=lam) if comp else {}
        return Rule(40, [arrs[0], arrs[1], None, arrs[2]], events=ev, stager=ProgramStager(DEV),
                    **ckw, **kw)
    cases = [(tick, None, dict(kind="sgd", lr=0.01, momentum=0.9)),
             (tick, [D.WEIGHTS[1]], dict(kind="adam", lr=1e-3)),
             (general, GENERAL["aw"], dict(kind="sgd", lr=0.01, momentum=0.9)),
             (general, None, dict(kind="adam", lr=1e-3)),
             (tick, None, dict(kind="sgd", lr=0.01))]
    for make, aw, o in cases:
        kw = dict(weights=aw) if aw is not None else {}
        nstate = 2 if o["kind"] == "adam" else (1 if o.get("momentum") else 0)
        a = [theta.clone(), m0.clone(), v0.clone()]
        b = [theta.clone(), m0.clone(), v0.clone()]
        c = [theta.clone(), m0.clone(), v0.clone()]
        arg = lambda s: [s[0], s[1] if nstate >= 1 else None,       # noqa: E731
                         s[2] if nstate >= 2 else None]
        ta = torch.full((P,), float("nan"), device=DEV)
        tb = torch.full((P,), float("nan"), device=DEV)
        eng.aggregate_rule(S, make(True, **kw), *arg(a), 3, optim=o, theta_out=ta)
        out = torch.full_like(S, float("nan"))
        eng.server_step(out, make(True, **kw), *arg(b), 3, optim=o, theta_out=tb)
        eng.server_step(None, make(False, **kw), *arg(c), 3, optim=o)     # the uncompensated step
        torch.cuda.synchronize()
        assert torch.equal(out[:P], S[:P])
        assert np.array_equal(_bits(ta), _bits(theta)) and np.array_equal(_bits(tb), _bits(theta))
        for x, y, what in zip(a, b, "pmv"):
            bad = int((x.view(torch.int32) != y.view(torch.int32)).sum())
            assert bad == 0, (o, what, bad)
        assert not torch.equal(b[0], c[0]) and not torch.equal(b[0], theta)
        if nstate < 2:
            assert torch.equal(b[2], v0)
        if nstate < 1:
            assert torch.equal(b[1], m0)


# ---- FLSimulation on PN1 ------------------------------------------------------------------------
N, DELAY, EPOCHS, LR = 4, 2, 5, 0.01
# an entry is the sum of four workers' gradients, about 1e-2 per element, and theta moves by about
# 1e-4 per epoch at this lr: lam * x * (theta_t - theta_src) is about 1e-2 of x at lam = 1e4
LAM_SIM = 1.0e4


def _sim(pool, **kw):
    from flsim.sim import FLSimulation
    return FLSimulation(N, delay=DELAY, throttle=True, device=DEV, chunk_workers=2, pool=pool,
                        lr=LR, optimizer="sgd", **{**dict(delay_comp=LAM_SIM), **kw})


@pytest.fixture(scope="module")
def straight(pool):
    """The keep_S run: per epoch (S_t, theta after the step), its trace and theta_0."""
    sim = _sim(pool, keep_S=True)
    theta0 = sim.theta.cpu().numpy().copy()
    rec = []
    for _ in range(EPOCHS):
        sim.epoch()
        rec.append((sim.comm[:sim.P].cpu().numpy().copy(), sim.theta.cpu().numpy().copy()))
    return dict(theta0=theta0, rec=rec, trace=list(sim.trace), sizes=list(sim.engine.SIZES))


def test_simulation_teacher_forced_bit_exact(straight):
    """Each epoch's theta = the text + torch SGD on the CPU, applied to the device's own S_t,
    theta and snapshots (theta before the step of the epoch an entry was pushed in)."""
    tp = torch.nn.Parameter(torch.from_numpy(straight["theta0"].copy()))
    opt = torch.optim.SGD([tp], lr=LR)
    sizes = straight["sizes"]
    rec = straight["rec"]
    before = [straight["theta0"]] + [th for (_, th) in rec[:-1]]       # theta_t, per epoch
    popped, acted = [], 0
    for t, (plan, (S, theta)) in enumerate(zip(straight["trace"], rec)):
        ents = [S] * plan.c_t + [rec[src][0] for (_, src) in plan.stale]
        snaps = [None] * plan.c_t + [before[src] for (_, src) in plan.stale]
        if plan.stale:
            popped.append((t, [src for (_, src) in plan.stale]))
        g = D.text_flat(ents, snaps, before[t], LAM_SIM, None, sizes)
        assert np.isfinite(g).all()
        acted += int((D.bits(g) != D.bits(D.text_flat(ents, [None] * len(ents), before[t], LAM_SIM,
                                                      None, sizes))).sum())
        tp.grad = torch.from_numpy(g)
        opt.step()
        bad = int((tp.detach().numpy().view(np.uint32) != theta.view(np.uint32)).sum())
        print(t, plan.c_t, plan.stale, "differing words:", bad)
        assert bad == 0, (t, bad)
    assert popped == [(2, [0]), (4, [2])]               # two ticks
    assert acted > 0.10 * 2 * sum(sizes)                # compensation changed g at both


def test_simulation_paths_end_bit_identical(pool, straight):
    """Without keep_S the epoch ends in the fused compensated step, which also writes the
    snapshot; fused=False in the stream."""
    for kw in (dict(), dict(fused=False)):
        sim = _sim(pool, **kw)
        for _ in range(EPOCHS):
            sim.epoch()
        assert np.array_equal(sim.theta.cpu().numpy().view(np.uint32),
                              straight["rec"][-1][1].view(np.uint32)), kw
        # the live slot (pushed at t = 4) carries theta_4
        assert sorted(sim.stale_theta) == [4]
        assert np.array_equal(_bits(sim.stale_theta[4][:sim.P]),
                              straight["rec"][3][1].view(np.uint32)), kw
    plain = _sim(pool, delay_comp=None)             # compensation acts
    for _ in range(EPOCHS):
        plain.epoch()
    assert not np.array_equal(plain.theta.cpu().numpy(), straight["rec"][-1][1])


def _batch(pool, seed):
    from oracle import oracle as O
    rs = np.random.RandomState(seed)
    idx = rs.randint(0, pool[0].shape[0], 128)
    return (torch.from_numpy(O.normalize_lut()[pool[0][idx]]).to(DEV),
            torch.from_numpy(pool[1][idx]).to(DEV))


def test_facade_compensated_rule_tick_epoch(pool):
    """Two epochs through FL.agents: epoch 0 fills the FIFO entry and takes its snapshot with
    snapshot_parameters, epoch 1 is a tick whose weight_ups = [S_1, S_1, S_0] goes through
    compensated_rule.  The result equals the text + torch SGD on the gradients read back, and
    FLSimulation's step for that epoch run on the facade's buffers."""
    import torch.nn as nn
    from FL.agents import Agg, Central, Worker, compensated_rule, rule, snapshot_parameters
    from FL.models import PerformantNet1
    from flsim.engine import PN1_SIZES
    from flsim.sim import FLSimulation
    torch.manual_seed(0)
    model = PerformantNet1().to(DEV)
    central = Central(model, torch.optim.SGD(model.parameters(), lr=LR))
    ws = [Worker(nn.CrossEntropyLoss()) for _ in range(2)]
    model.train()
    ups0 = ups1 = None
    snap0 = snapshot_parameters(model)
    for i, w in enumerate(ws):
        w.model = model
        ups0, _ = w.fwd_bkwd(*_batch(pool, 10 + i))
    central.update_model(Agg(rule).rule([ups0, ups0]))
    for i, w in enumerate(ws):
        ups1, _ = w.fwd_bkwd(*_batch(pool, 20 + i))
    S1, S0 = (torch.cat([t.reshape(-1) for t in u]).cpu().numpy().copy() for u in (ups1, ups0))
    ctx = central.ctx
    before = ctx.theta[:ctx.P].cpu().numpy().copy()
    th0 = snap0.cpu().numpy().copy()
    assert not np.array_equal(before, th0)
    agg = Agg(lambda ups: compensated_rule(ups, [None, None, snap0], LAM_SIM))
    central.update_model(agg.rule([ups1, ups1, ups0]))
    after = ctx.theta[:ctx.P].cpu().numpy().copy()
    g = D.text_flat([S1, S1, S0], [None, None, th0], before, LAM_SIM, None, PN1_SIZES)
    pe, _ = _sgd_expected(g, before, lr=LR)
    bad = int((pe.view(np.uint32) != after.view(np.uint32)).sum())
    print("facade tick differing words:", bad)
    assert bad == 0
    plain = D.text_flat([S1, S1, S0], [None] * 3, before, LAM_SIM, None, PN1_SIZES)
    assert not np.array_equal(_sgd_expected(plain, before, lr=LR)[0], after)
    # FLSimulation's step on the same buffers
    sim = FLSimulation(3, delay=1, device=DEV, engine=ctx.engine, device_pool=object(),
                       theta0=torch.from_numpy(before), lr=LR, optimizer="sgd",
                       delay_comp=LAM_SIM)
    plan = types.SimpleNamespace(t=1, c_t=2, s_t=1, stale=[(2, 0)],
                                 fast=np.array([1, 1, 0], np.uint8))
    dS1, dS0 = (torch.from_numpy(x).to(DEV) for x in (S1, S0))
    sim.stale_theta[0] = torch.from_numpy(th0).to(DEV)
    r = sim._rule(plan, [dS0])
    assert r.delay_comp == LAM_SIM and r.snapshots[0] is sim.stale_theta[0] and r.weights is None
    ctx.engine.aggregate_rule(dS1, r, sim.theta, None, None, 2, optim=sim._optim_arg)
    torch.cuda.synchronize()
    assert np.array_equal(sim.theta.cpu().numpy().view(np.uint32), after.view(np.uint32))
    with pytest.raises(ValueError):                 # one snapshot per entry
        compensated_rule([[None]], [None, None], 2.0)
