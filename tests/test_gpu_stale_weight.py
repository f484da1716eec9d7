"""GPU: the staleness-weighted server step (csrc/server.hip's W kernels through
flsim_aggregate_optim_wrule_push and flsim_<net>_server_step_wrule), bit for bit against

    def weighted_rule(ups_list, weights, normalize="weights"):
        W = float(sum(weights)) if normalize == "weights" else float(len(ups_list))
        return [torch.stack([x[i] * w for x, w in zip(ups_list, weights)]).sum(0) / W
                for i in range(len(ups_list[0]))]

evaluated by torch on the CPU, per parameter tensor.  g is read exactly through plain SGD with
p = 0 and lr = 1 (theta = -g); one Adam and one SGD-momentum case use the oracle's adam_step /
torch SGD as tests/test_gpu_optim.py does.  Every comparison asks for zero differing words.
"""
import types

import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

DEV = "cuda:0"
WEIGHTS = [(1.0 + 50) ** -0.5, 1.0 / 3.0, 1e-3]
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
               aw=[WEIGHTS[0], WEIGHTS[1], WEIGHTS[2], 1.0])


def weighted_rule(ups_list, weights, normalize="weights"):
    W = float(sum(weights)) if normalize == "weights" else float(len(ups_list))
    return [torch.stack([x[i] * w for x, w in zip(ups_list, weights)]).sum(0) / W
            for i in range(len(ups_list[0]))]


def _split(flat, sizes):
    out, off = [], 0
    for n in sizes:
        out.append(torch.from_numpy(flat[off:off + n]))
        off += n
    return out


def _rule_text(entries, full, sizes, normalize):
    """The text over flat numpy entries, per tensor -> flat g."""
    g = weighted_rule([_split(e, sizes) for e in entries], full, normalize)
    return torch.cat(g).numpy()


def _values(rs, n, scale=1e-2):
    """Gradient-like values with the edge cases: +-0, subnormals, +-1e30."""
    v = (rs.standard_normal(n) * scale).astype(np.float32)
    v[::17] = 0.0
    v[1::17] = -0.0
    v[2::17] = np.float32(3e-39) * rs.choice([-1, 1], len(v[2::17]))
    v[3::17] = np.float32(1e30) * rs.choice([-1, 1], len(v[3::17]))
    v[4::17] = np.float32(1.2e-38) * rs.choice([-1, 1], len(v[4::17]))
    return v


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
    aw = (WEIGHTS[:ns - 1] + [1.0]) if ns == 3 else WEIGHTS[:ns]     # 1.0 on one stale array
    return (sizes, c + ns, [(c + q, q) for q in range(ns)], aw,
            lambda d, **kw: Rule(c + ns, d, c=c, **kw))


def _host_inputs(layout, seed):
    sizes, k, events, aw, make = _case(layout)
    P = sum(sizes)
    rs = np.random.RandomState(seed)
    S = _values(rs, P)
    arrays = [_values(rs, P) for _ in aw]
    if layout == "general":
        arrays[2] = None                        # a torch-1.x zero entry
    ents, full = [S] * k, [1.0] * k
    for pos, a in events:
        ents[pos] = arrays[a] if arrays[a] is not None else np.zeros_like(S)
        full[pos] = aw[a]
    return sizes, k, aw, make, S, arrays, ents, full


@pytest.mark.parametrize("normalize", ["weights", "count"])
@pytest.mark.parametrize("layout", ["tails_lds", "reg_ny1", "reg_ny2", "general"])
def test_stream_reads_g_exactly(layout, normalize):
    """theta = -g: plain SGD, p = 0, lr = 1."""
    from flsim.engine import aggregate_rule
    sizes, k, aw, make, S, arrays, ents, full = _host_inputs(layout, 7)
    P = sum(sizes)
    g = _rule_text(ents, full, sizes, normalize)
    pe, _ = _sgd_expected(g, np.zeros(P, np.float32))
    W = float(sum(full)) if normalize == "weights" else float(k)
    dS = torch.from_numpy(S).to(DEV)
    dA = [torch.from_numpy(a).to(DEV) if a is not None else None for a in arrays]
    dp = torch.zeros(P, device=DEV)
    rule = make(dA, weights=aw, divisor=W)
    if normalize == "weights":                  # Rule's own divisor is the text's
        assert make(dA, weights=aw).divisor == W
    aggregate_rule(dS, rule, dp, None, None, 1, sizes, optim=SGD1)
    torch.cuda.synchronize()
    bad = int((_bits(dp) != pe.view(np.uint32)).sum())
    print(layout, normalize, "differing words:", bad)
    assert bad == 0
    # the discount acts: the plain mean gives another theta
    dq = torch.zeros(P, device=DEV)
    aggregate_rule(dS, make(dA), dq, None, None, 1, sizes, optim=SGD1)
    assert not torch.equal(dp, dq)


@pytest.mark.parametrize("layout", ["reg_ny1", "general"])
def test_stream_adam_and_sgd_momentum(layout):
    from flsim.engine import aggregate_rule
    from oracle import oracle as O
    sizes, k, aw, make, S, arrays, ents, full = _host_inputs(layout, 11)
    P = sum(sizes)
    rs = np.random.RandomState(5)
    p = rs.standard_normal(P).astype(np.float32)
    m = (rs.standard_normal(P) * 1e-3).astype(np.float32)
    v = (rs.rand(P) * 1e-5).astype(np.float32)
    g = _rule_text(ents, full, sizes, "weights")
    dS = torch.from_numpy(S).to(DEV)
    dA = [torch.from_numpy(a).to(DEV) if a is not None else None for a in arrays]
    rule = make(dA, weights=aw)
    # Adam, step 3 (the oracle's adam_step: correctly rounded sqrt, like the kernel's)
    pe, me, ve = p.copy(), m.copy(), v.copy()
    O.adam_step(pe, me, ve, g, 3, lr=1e-3)
    d = [torch.from_numpy(x.copy()).to(DEV) for x in (p, m, v)]
    aggregate_rule(dS, rule, *d, 3, sizes, lr=1e-3)
    torch.cuda.synchronize()
    bad = [int((_bits(x) != y.view(np.uint32)).sum()) for x, y in zip(d, (pe, me, ve))]
    print(layout, "adam differing words:", bad)
    assert bad == [0, 0, 0]
    # SGD momentum 0.9, step 3
    pe, be = _sgd_expected(g, p, lr=0.01, momentum=0.9, buf=m)
    d = [torch.from_numpy(x.copy()).to(DEV) for x in (p, m)]
    aggregate_rule(dS, rule, d[0], d[1], None, 3, sizes,
                   optim=dict(kind="sgd", lr=0.01, momentum=0.9))
    torch.cuda.synchronize()
    bad = [int((_bits(x) != y.view(np.uint32)).sum()) for x, y in zip(d, (pe, be))]
    print(layout, "sgd momentum differing words:", bad)
    assert bad == [0, 0]


@pytest.mark.parametrize("layout", ["tails_lds", "reg_ny1", "reg_ny2", "general"])
def test_unit_weights_equal_the_unweighted_entry_point(layout):
    """weights=None is the unweighted entry point; all weights 1.0 with the divisor k runs the
    W kernels (one multiply by 1.0, the IEEE division by k) and must give the same words.

    Tensors of 4 .. 7 elements are left out of the second comparison: there torch sums the first
    four columns with multi_row_sum (ATen's scalar path), which the weighted kernels follow
    (test_stream_reads_g_exactly holds them to torch on these very layouts) and the unweighted
    ones, pinned to the oracle's 32-column rule, do not.  No model has such a tensor."""
    from flsim.engine import aggregate_rule
    sizes, k, aw, make, S, arrays, _, _ = _host_inputs(layout, 13)
    P = sum(sizes)
    dS = torch.from_numpy(S).to(DEV)
    dA = [torch.from_numpy(a).to(DEV) if a is not None else None for a in arrays]
    rs = np.random.RandomState(3)
    p = rs.standard_normal(P).astype(np.float32)
    m = (rs.standard_normal(P) * 1e-3).astype(np.float32)
    v = (rs.rand(P) * 1e-5).astype(np.float32)
    plain = make(dA)
    none = make(dA, weights=None)
    unit = make(dA, weights=[1.0] * len(aw), divisor=k)
    assert plain.c_weights is None and none.c_weights is None and unit.c_weights is not None
    for hp in (dict(lr=1e-3), dict(optim=SGD1)):
        res = []
        for rule in (plain, none, unit):
            d = [torch.from_numpy(x.copy()).to(DEV) for x in (p, m, v)]
            aggregate_rule(dS, rule, *d, 2, sizes, **hp)
            res.append(d)
        torch.cuda.synchronize()
        keep = torch.ones(P, dtype=torch.bool, device=DEV)
        off = 0
        for n in sizes:
            if 4 <= n < 8:
                keep[off:off + n] = False
            off += n
        assert int(keep.sum()) >= P - 7
        for x, y in zip(res[0], res[1]):            # weights=None: every word
            assert int((x.view(torch.int32) != y.view(torch.int32)).sum()) == 0
        for x, y in zip(res[0], res[2]):
            assert int(((x.view(torch.int32) != y.view(torch.int32)) & keep).sum()) == 0
        assert not torch.equal(res[0][0], torch.from_numpy(p).to(DEV))


@pytest.fixture(scope="module")
def pool():
    from oracle import oracle as O
    return O.make_pool(0)


def test_fused_step_equals_reduce_then_weighted_stream(pool):
    """The 2-worker PN1 chunk of tests/test_gpu_optim.py: the fused weighted slab step against
    end_epoch + the weighted stream: theta, the owned state arrays and S_out bit-identical, for a
    weighted tick rule and the weighted general-order rule, SGD momentum and Adam; and it differs
    from the unweighted step."""
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
    arrs = [(torch.randn(P + 64, generator=g) * 1e-3).to(DEV) for _ in range(3)]
    m0 = (torch.randn(P, generator=g) * 1e-4).to(DEV)
    v0 = (torch.rand(P, generator=g) * 1e-6).to(DEV)
    ev = GENERAL["events"]

    def tick(**kw):
        return Rule(6, [arrs[0]], c=5, **kw)

    def general(**kw):
        return Rule(40, [arrs[0], arrs[1], None, arrs[2]], events=ev, stager=ProgramStager(DEV),
                    **kw)
    cases = [(tick, [WEIGHTS[0]], dict(kind="sgd", lr=0.01, momentum=0.9), "weights"),
             (tick, [WEIGHTS[1]], dict(kind="adam", lr=1e-3), "count"),
             (general, GENERAL["aw"], dict(kind="sgd", lr=0.01, momentum=0.9), "weights"),
             (general, GENERAL["aw"], dict(kind="adam", lr=1e-3), "weights")]
    for make, aw, o, normalize in cases:
        kw = dict(weights=aw) if normalize == "weights" else \
            dict(weights=aw, divisor=make().k)
        nstate = 1 if o["kind"] == "sgd" else 2
        a = [theta.clone(), m0.clone(), v0.clone()]
        b = [theta.clone(), m0.clone(), v0.clone()]
        c = [theta.clone(), m0.clone(), v0.clone()]
        arg = lambda s: [s[0], s[1], s[2] if nstate >= 2 else None]  # noqa: E731
        eng.aggregate_rule(S, make(**kw), *arg(a), 3, optim=o)
        out = torch.full_like(S, float("nan"))
        eng.server_step(out, make(**kw), *arg(b), 3, optim=o)
        eng.server_step(None, make(), *arg(c), 3, optim=o)           # the unweighted step
        torch.cuda.synchronize()
        assert torch.equal(out[:P], S[:P])
        for x, y, what in zip(a, b, "pmv"):
            bad = int((x.view(torch.int32) != y.view(torch.int32)).sum())
            assert bad == 0, (o["kind"], what, bad)
        assert not torch.equal(b[0], c[0]) and not torch.equal(b[0], theta)
        if nstate < 2:
            assert torch.equal(b[2], v0)


# ---- FLSimulation on PN1 ------------------------------------------------------------------------
N, DELAY, EPOCHS, LR = 4, 2, 5, 0.01
SPEC = ("poly", 0.5)


def _sim(pool, **kw):
    from flsim.sim import FLSimulation
    return FLSimulation(N, delay=DELAY, throttle=True, device=DEV, chunk_workers=2, pool=pool,
                        lr=LR, optimizer="sgd", **{**dict(stale_weight=SPEC), **kw})


@pytest.fixture(scope="module")
def straight(pool):
    """The keep_S run: per epoch (S_t, theta), its trace and theta_0."""
    sim = _sim(pool, keep_S=True)
    theta0 = sim.theta.cpu().numpy().copy()
    rec = []
    for _ in range(EPOCHS):
        sim.epoch()
        rec.append((sim.comm[:sim.P].cpu().numpy().copy(), sim.theta.cpu().numpy().copy()))
    return dict(theta0=theta0, rec=rec, trace=list(sim.trace), sizes=list(sim.engine.SIZES))


def test_simulation_teacher_forced_bit_exact(straight):
    """Each epoch's theta = the rule text + torch SGD on the CPU, applied to the device's own
    S_t and stale slots."""
    tp = torch.nn.Parameter(torch.from_numpy(straight["theta0"].copy()))
    opt = torch.optim.SGD([tp], lr=LR)
    sizes = straight["sizes"]
    discounted = []
    for t, (plan, (S, theta)) in enumerate(zip(straight["trace"], straight["rec"])):
        ents = [S] * plan.c_t + [straight["rec"][src][0] for (_, src) in plan.stale]
        full = [1.0] * plan.c_t + [(1.0 + (t - src)) ** (-0.5) for (_, src) in plan.stale]
        if plan.stale:
            discounted.append((t, [t - src for (_, src) in plan.stale]))
        tp.grad = torch.from_numpy(_rule_text(ents, full, sizes, "weights"))
        opt.step()
        bad = int((tp.detach().numpy().view(np.uint32) != theta.view(np.uint32)).sum())
        print(t, plan.c_t, plan.stale, "differing words:", bad)
        assert bad == 0, (t, bad)
    assert discounted == [(2, [2]), (4, [2])]


def test_simulation_paths_end_bit_identical(pool, straight):
    """Without keep_S the epoch ends in the fused weighted step; fused=False in the stream."""
    for kw in (dict(), dict(fused=False)):
        sim = _sim(pool, **kw)
        for _ in range(EPOCHS):
            sim.epoch()
        assert np.array_equal(sim.theta.cpu().numpy().view(np.uint32),
                              straight["rec"][-1][1].view(np.uint32)), kw
    plain = _sim(pool, stale_weight=None)           # the discount acts
    for _ in range(EPOCHS):
        plain.epoch()
    assert not np.array_equal(plain.theta.cpu().numpy(), straight["rec"][-1][1])


def _batch(pool, seed):
    from oracle import oracle as O
    rs = np.random.RandomState(seed)
    idx = rs.randint(0, pool[0].shape[0], 128)
    return (torch.from_numpy(O.normalize_lut()[pool[0][idx]]).to(DEV),
            torch.from_numpy(pool[1][idx]).to(DEV))


def _facade_tick(pool, read_grads):
    """Two epochs through FL.agents: epoch 0 fills the FIFO entry, epoch 1 is a tick whose
    weight_ups = [S_1, S_1, S_0] goes through weighted_rule with the age-1 discount.  ->
    (theta before the tick, theta after it, the Central, (S_1, S_0) when read_grads)."""
    import torch.nn as nn
    from FL.agents import Agg, Central, Worker, rule, weighted_rule as facade_rule
    from FL.models import PerformantNet1
    torch.manual_seed(0)
    model = PerformantNet1().to(DEV)
    central = Central(model, torch.optim.SGD(model.parameters(), lr=LR))
    ws = [Worker(nn.CrossEntropyLoss()) for _ in range(2)]
    model.train()
    ups0 = ups1 = None
    for i, w in enumerate(ws):
        w.model = model
        ups0, _ = w.fwd_bkwd(*_batch(pool, 10 + i))
    central.update_model(Agg(rule).rule([ups0, ups0]))
    for i, w in enumerate(ws):
        ups1, _ = w.fwd_bkwd(*_batch(pool, 20 + i))
    reads = None
    if read_grads:
        reads = tuple(torch.cat([t.reshape(-1) for t in u]).cpu().numpy().copy()
                      for u in (ups1, ups0))
    ctx = central.ctx
    before = ctx.theta[:ctx.P].cpu().numpy().copy()
    w_stale = (1.0 + 1) ** (-0.5)
    agg = Agg(lambda ups: facade_rule(ups, [1.0, 1.0, w_stale]))
    central.update_model(agg.rule([ups1, ups1, ups0]))
    return before, ctx.theta[:ctx.P].cpu().numpy().copy(), central, reads


def test_facade_weighted_rule_tick_epoch(pool):
    """A tick epoch through FL.agents with weighted_rule: the buffered path (a .grad was read) and
    the fused one end bit-identical; both equal the rule text + torch SGD on the gradients the
    buffered run read; and both equal FLSimulation's step for that epoch -- the Rule its _rule
    builds for (t = 1, two fast workers, one entry popped from epoch 0) run on the same buffers."""
    from FL.agents import weighted_rule as facade_rule
    from flsim.engine import PN1_SIZES
    from flsim.sim import FLSimulation
    before, after, central, (S1, S0) = _facade_tick(pool, True)
    _, after_fused, _, _ = _facade_tick(pool, False)
    assert np.array_equal(after.view(np.uint32), after_fused.view(np.uint32))
    full = [1.0, 1.0, 2.0 ** -0.5]
    g = _rule_text([S1, S1, S0], full, PN1_SIZES, "weights")
    pe, _ = _sgd_expected(g, before, lr=LR)
    bad = int((pe.view(np.uint32) != after.view(np.uint32)).sum())
    print("facade tick differing words:", bad)
    assert bad == 0
    assert not np.array_equal(_sgd_expected(_rule_text([S1, S1, S0], [1.0] * 3, PN1_SIZES,
                                                       "weights"), before, lr=LR)[0], after)
    # FLSimulation's step on the same buffers
    ctx = central.ctx
    sim = FLSimulation(3, delay=1, device=DEV, engine=ctx.engine, device_pool=object(),
                       theta0=torch.from_numpy(before), lr=LR, optimizer="sgd",
                       stale_weight=SPEC)
    plan = types.SimpleNamespace(t=1, c_t=2, s_t=1, stale=[(2, 0)],
                                 fast=np.array([1, 1, 0], np.uint8))
    dS1, dS0 = (torch.from_numpy(x).to(DEV) for x in (S1, S0))
    rule = sim._rule(plan, [dS0])
    assert rule.weights == [2.0 ** -0.5] and rule.divisor == float(sum(full))
    ctx.engine.aggregate_rule(dS1, rule, sim.theta, None, None, 2, optim=sim._optim_arg)
    torch.cuda.synchronize()
    assert np.array_equal(sim.theta.cpu().numpy().view(np.uint32), after.view(np.uint32))
    with pytest.raises(ValueError):                 # one weight per entry
        facade_rule([[None]], [1.0, 2.0])
