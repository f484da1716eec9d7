"""GPU: FedAdagrad and FedYogi in the server step (csrc/server.hip: OK_ADAGRAD and OK_YOGI in every
rule-carrying kernel and in k_clip_apply), through the existing entry points.

Expected values come from tests/_fedopt.py: torch CPU ops in the rule text's order with numpy's
correctly rounded sqrt in between (tests/test_cpu_fedopt.py pins that text to
torch.optim.Adagrad.step() and to flsim.optim.Yogi).  g is the oracle's cascade mean per tensor, or
the weighted / compensated rule text evaluated by torch (tests/_delay_comp.py), or the clipped
gradient of tests/_clip.py.  Every comparison asks for zero differing words in p and in every state
array the kind owns; Adagrad's v is passed poisoned and must come back untouched, or is None.
"""
import numpy as np
import pytest
import torch

import _clip as K
import _delay_comp as D
import _fedopt as F
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

DEV = "cuda:0"
POISON = np.uint32(0x7FC12345)          # a NaN payload no arithmetic produces

KINDS = {
    "adagrad": dict(kind="adagrad", lr=1e-2, eps=1e-10),
    "adagrad_decay_wd": dict(kind="adagrad", lr=1e-2, eps=1e-10, lr_decay=0.05, weight_decay=5e-4),
    "yogi": dict(kind="yogi", lr=1e-2, betas=(0.9, 0.99), eps=1e-3),
    "yogi_wd": dict(kind="yogi", lr=1e-2, betas=(0.9, 0.99), eps=1e-3, weight_decay=5e-4),
}
BOTH = ["adagrad_decay_wd", "yogi_wd"]
# tests/test_gpu_optim.py's layouts (sizes, c, n_stale): > 8 row_sum tails -> split launches, the
# LDS-staged stream (3 entry arrays); the register streams with one float4 group per thread (a
# stale array) and with two (none)
LAYOUTS = {
    "tails_lds": ([5, 37, 64, 1, 96, 100, 33, 2, 3, 70, 9, 11], 6, 3),
    "reg_g1": ([1000, 4096, 33, 7], 3, 1),
    "reg_g2": ([1000, 4096, 33, 7], 9, 0),
}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV) if a is not None else None


def _poison(P):
    return np.full(P, POISON, np.uint32).view(np.float32)


def _step_and_compare(o, g, run, p, m, v, step, with_none=False, label=""):
    """run(dp, dm, dv) performs one device step; p / m / v (host) are its inputs, g the gradient
    the text is evaluated on.  Zero differing words in p and the owned state; the rest poisoned
    and untouched."""
    P = p.size
    nstate = F.n_state(o)
    pe, me, ve = F.expected(o, g, p, m, v, step)
    dp = _dev(p)
    dm = _dev(m if nstate >= 1 else _poison(P))
    dv = _dev(v if nstate >= 2 else _poison(P))
    run(dp, dm if (nstate >= 1 or not with_none) else None,
        dv if (nstate >= 2 or not with_none) else None)
    torch.cuda.synchronize()
    bad = {"p": F.n_diff(dp, pe), "m": F.n_diff(dm, me if nstate >= 1 else _poison(P)),
           "v": F.n_diff(dv, ve if nstate >= 2 else _poison(P))}
    print(label, o, step, bad)
    assert bad == {"p": 0, "m": 0, "v": 0}, bad
    assert F.n_diff(dp, p) > P // 2                          # the step acts
    return dp, dm, dv


def _stream_case(o, rule_of, entries_of, sizes, ns, step, seed, with_none=False):
    from flsim.engine import aggregate_rule
    P = sum(sizes)
    S, stale, p, m, v, acc = F.inputs(P, ns, seed)
    if o["kind"] == "adagrad":
        m = acc
    g = F.mean(entries_of(S, stale), sizes)
    dS, dst = _dev(S), [_dev(s) for s in stale]
    _step_and_compare(o, g, lambda dp, dm, dv: aggregate_rule(dS, rule_of(dst), dp, dm, dv, step,
                                                              sizes, optim=o),
                      p, m, v, step, with_none, label=str(sizes[:2]))


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_stream_step_bit_exact_vs_text(kind, step, layout):
    """The inputs hold +-0, a subnormal and 1e30 (Yogi's g^2 = inf, Adagrad's sum = inf)."""
    from flsim.engine import Rule
    sizes, c, ns = LAYOUTS[layout]
    _stream_case(KINDS[kind], lambda dst: Rule(c + ns, dst, c=c),
                 lambda S, stale: [S] * c + stale, sizes, ns, step,
                 seed=1000 * step + 10 * c + ns)


def test_yogi_sign_cases():
    """c = 1: g = S.  v is g * g on a third of the elements (sign 0), half of it on another third
    (sign -1) and twice it on the rest (sign +1).  A few more elements hold g = 1e30 on v = inf:
    v - g^2 is NaN, its sign 0, and -0 * inf must come out as a NaN, not as v (no select around
    the fma).  A NaN a device generates and one x86 generates differ in the sign bit, so those
    elements are compared with the sign bit masked (exponent and payload equal), every other one
    bit for bit."""
    from flsim.engine import Rule, aggregate_rule
    sizes = [1000, 4096, 33, 7]
    P = sum(sizes)
    rs = np.random.RandomState(42)
    S = K.values(rs, P)
    hot = np.zeros(P, bool)
    hot[3::170] = True
    S[hot] = np.float32(1e30)
    g = F.mean([S], sizes)
    assert F.n_diff(g, S) == 0
    with np.errstate(over="ignore"):
        g2 = (g * g).astype(np.float32)
    v = g2.copy()
    v[1::3] = (g2 * np.float32(0.5))[1::3]
    v[2::3] = (g2 * np.float32(2.0))[2::3]
    v[hot] = np.float32(np.inf)
    with np.errstate(invalid="ignore"):
        d = v - g2
    shares = {"zero": float((d == 0).mean()), "minus": float((d < 0).mean()),
              "plus": float((d > 0).mean()), "nan": float(np.isnan(d).mean())}
    print(shares)
    assert min(shares["zero"], shares["minus"], shares["plus"]) >= 0.10, shares
    assert np.isnan(d[hot]).all() and hot.sum() >= 20
    p = rs.standard_normal(P).astype(np.float32)
    m = (rs.standard_normal(P) * 1e-3).astype(np.float32)
    o = KINDS["yogi"]
    pe, me, ve = F.yogi_expected(g, p, m, v, 2, **{k: x for k, x in o.items() if k != "kind"})
    assert np.isnan(ve[hot]).all() and np.isnan(pe[hot]).all() and np.isfinite(ve[~hot]).all()
    dp, dm, dv = _dev(p), _dev(m), _dev(v)
    aggregate_rule(_dev(S), Rule(1, [], c=1), dp, dm, dv, 2, sizes, optim=o)
    torch.cuda.synchronize()
    gp, gm, gv = (t.cpu().numpy() for t in (dp, dm, dv))
    assert F.n_diff(gm, me) == 0
    assert F.n_diff(gp[~hot], pe[~hot]) == 0 and F.n_diff(gv[~hot], ve[~hot]) == 0
    assert np.isnan(gv[hot]).all() and np.isnan(gp[hot]).all()
    mask = np.uint32(0x7FFFFFFF)
    assert np.array_equal(F.bits(gv[hot]) & mask, F.bits(ve[hot]) & mask)
    assert np.array_equal(F.bits(gp[hot]) & mask, F.bits(pe[hot]) & mask)


@pytest.mark.parametrize("layout", ["tails_lds", "reg_g1"])
def test_adagrad_v_may_be_none(layout):
    """Adagrad owns no v: None is accepted for it (the poisoned-v form runs in
    test_stream_step_bit_exact_vs_text)."""
    from flsim.engine import Rule
    sizes, c, ns = LAYOUTS[layout]
    _stream_case(KINDS["adagrad_decay_wd"], lambda dst: Rule(c + ns, dst, c=c),
                 lambda S, stale: [S] * c + stale, sizes, ns, 3, seed=77, with_none=True)


@pytest.mark.parametrize("kind", BOTH)
def test_general_order(kind):
    """A general-order rule (the staged program, k_agg_stream<false>)."""
    from flsim.engine import ProgramStager, Rule
    sizes = [1000, 4096, 33, 7]
    k, events = 40, [(0, 1), (7, 0), (8, 0), (21, 2), (33, 3), (39, 1)]   # array 3 = zeros

    def rule_of(dst):
        return Rule(k, dst + [None], events=events, stager=ProgramStager(DEV))

    def entries_of(S, stale):
        ents = [S] * k
        for pos, a in events:
            ents[pos] = stale[a] if a < 3 else np.zeros_like(S)
        return ents
    _stream_case(KINDS[kind], rule_of, entries_of, sizes, 3, 3, seed=5)


@pytest.mark.parametrize("form", ["weighted", "compensated"])
@pytest.mark.parametrize("kind", BOTH)
def test_weighted_and_compensated_stream(kind, form):
    """The W and W,C streams: g is the rule text evaluated by torch (tests/_delay_comp.py) --
    weighted: one discounted stale array on the register stream; compensated: three arrays with
    snapshots, weights and lambda on the LDS-staged stream; theta_out receives the pre-update p."""
    from flsim.engine import Rule, aggregate_rule
    o = KINDS[kind]
    sizes, c, ns = LAYOUTS["reg_g1" if form == "weighted" else "tails_lds"]
    P = sum(sizes)
    rs = np.random.RandomState(31 + len(kind) + ns)
    S = D.values_S(rs, P)
    stale = [D.values_comp(rs, P) for _ in range(ns)]
    p, first = D.theta_pair(rs, P)
    snaps = [first] + [D.theta_src(rs, p) for _ in range(ns - 1)]
    w = [D.WEIGHTS[q % 3] for q in range(ns)]
    lam = D.LAMBDAS[1]
    comp = form == "compensated"
    m = np.abs(rs.standard_normal(P) * 1e-3).astype(np.float32)
    v = (rs.rand(P) * 1e-5).astype(np.float32)
    full = [1.0] * c + w
    g = D.text_flat([S] * c + stale, [None] * c + (snaps if comp else [None] * ns), p, lam, full,
                    sizes)
    g_plain = D.text_flat([S] * c + stale, [None] * (c + ns), p, lam, None, sizes)
    assert F.n_diff(g, g_plain) > P // 2                     # the weights (and snapshots) act
    dS, dst, dsn = _dev(S), [_dev(s) for s in stale], [_dev(s) for s in snaps]
    t_out = torch.full((P,), float("nan"), device=DEV) if comp else None
    kw = dict(snapshots=dsn, delay_comp=lam) if comp else {}

    def run(dp, dm, dv):
        aggregate_rule(dS, Rule(c + ns, dst, c=c, weights=w, **kw), dp, dm, dv, 2, sizes, optim=o,
                       theta_out=t_out)
    _step_and_compare(o, g, run, p, m, v, 2, label=form)
    if comp:
        assert F.n_diff(t_out, p) == 0


@pytest.mark.parametrize("kind", BOTH)
def test_clipped_step(kind):
    """g from the existing kernels (plain SGD with lr = 1 from p = 0 leaves p = -g), the norm and
    g' = g * coef from tests/_clip.py, then the text's update on g'."""
    from flsim.engine import Clip, Rule, aggregate_rule
    o = KINDS[kind]
    sizes = [33, 7, 1000, 4101]
    P = sum(sizes)
    rs = np.random.RandomState(8 + len(kind))
    S, arr = K.values(rs, P), K.values(rs, P, 3.0)
    dS, dA = _dev(S), _dev(arr)
    rule = lambda: Rule(5, [dA], c=4)                        # noqa: E731
    dg = torch.zeros(P, device=DEV)
    aggregate_rule(dS, rule(), dg, None, None, 1, sizes, optim=dict(kind="sgd", lr=1.0))
    g = -dg.cpu().numpy()
    assert np.isfinite(g).all() and (g != 0).all()
    exact, norm, dist = K.exact_norm(g)
    assert dist >= K.MIN_MIDPOINT_DISTANCE, dist
    mn = 0.5 * float(norm)
    gp = K.torch_clip(g, sizes, mn, norm)
    assert F.n_diff(gp, g) > P // 2                          # clipping acts
    p = rs.standard_normal(P).astype(np.float32)
    m = np.abs(rs.standard_normal(P) * 1e-3).astype(np.float32)
    v = (rs.rand(P) * 1e-5).astype(np.float32)
    clip = Clip(mn)
    for step in (1, 3):
        _step_and_compare(o, gp, lambda dp, dm, dv: aggregate_rule(dS, rule(), dp, dm, dv, step,
                                                                   sizes, optim=o, clip=clip),
                          p, m, v, step, label="clip")
        assert K.bits(clip.total_norm.cpu().numpy()) == K.bits(norm)
        assert K.bits(clip.coef.cpu().numpy()) == K.bits(K.torch_coef(norm, mn))


# ---- the fused step ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    from oracle import oracle as O
    return O.make_pool(0)


def _filled_engine(cls, pool, items, n_total=8):
    from flsim.data import DevicePool
    from flsim.engine import worker_table
    from flsim.sim import default_theta
    eng = cls(DEV, chunk_workers=len(items))
    theta = default_theta(0, eng.MODEL).to(DEV)
    eng.begin_epoch(theta)
    loss = torch.zeros(len(items), device=DEV)
    kw = {"stats_out": torch.zeros(len(items), eng.STATS_PER_WORKER, device=DEV)} \
        if eng.STATS_PER_WORKER else {}
    eng.run_chunk(theta, DevicePool(DEV, 0, pool), worker_table(items, DEV), len(items), n_total,
                  0, True, loss, **kw)
    return eng, theta


@pytest.mark.parametrize("model", ["PerformantNet1", "vgg11", "vgg11_bn"])
def test_fused_step_equals_reduce_then_stream(pool, model):
    """One tiny chunk (2 workers), twice from the same state: the fused slab step against
    end_epoch + the streaming step, per kind, on the reference-order and the general-order
    kernels.  theta, the owned state and S_out bit-identical; Adagrad's v untouched."""
    from flsim.engine import ProgramStager, Rule, engine_class
    eng, theta = _filled_engine(engine_class(model), pool, [(0, 0, 1), (0, 3, 7)])
    P = eng.P
    S = torch.zeros(P + 64, device=DEV)
    eng.end_epoch(S)
    g = torch.Generator(device="cpu").manual_seed(11)
    arrs = [(torch.randn(P + 64, generator=g) * 1e-3).to(DEV) for _ in range(3)]
    m0 = (torch.randn(P, generator=g) * 1e-4).abs().to(DEV)
    v0 = (torch.rand(P, generator=g) * 1e-6).to(DEV)
    tick = Rule(6, [arrs[0]], c=5)
    general = Rule(40, [arrs[0], arrs[1], None, arrs[2]],
                   events=[(0, 1), (7, 0), (8, 0), (21, 2), (33, 3), (39, 1)],
                   stager=ProgramStager(DEV))
    for kind in BOTH:
        o = KINDS[kind]
        nstate = F.n_state(o)
        for name, rule in (("tick", tick), ("general", general)):
            a = [theta.clone(), m0.clone(), v0.clone()]
            b = [theta.clone(), m0.clone(), v0.clone()]
            arg = lambda s: [s[0], s[1], s[2] if nstate >= 2 else None]      # noqa: E731
            eng.aggregate_rule(S, rule, *arg(a), 3, optim=o)
            out = torch.full_like(S, float("nan"))
            eng.server_step(out, rule, *arg(b), 3, optim=o)
            torch.cuda.synchronize()
            assert torch.equal(out[:P], S[:P]), (kind, name)
            assert not torch.equal(a[0], theta), (kind, name)
            for x, y, what in zip(a, b, "pmv"):
                bad = int((x.view(torch.int32) != y.view(torch.int32)).sum())
                assert bad == 0, (model, kind, name, what, bad)
            if nstate < 2:
                assert torch.equal(a[2], v0) and torch.equal(b[2], v0)


@pytest.mark.parametrize("kind", BOTH)
def test_fused_step_weighted_and_compensated_vs_text(pool, kind):
    """The fused step's W,C form on PerformantNet1 against the text: S_t from end_epoch, one
    discounted and compensated stale array; theta_out receives the pre-update theta."""
    from flsim.engine import PN1Engine, Rule
    o = KINDS[kind]
    eng, theta = _filled_engine(PN1Engine, pool, [(0, 0, 1), (0, 3, 7)])
    P = eng.P
    sizes = list(eng.SIZES)
    dS = torch.zeros(P + 64, device=DEV)
    eng.end_epoch(dS)
    S = dS[:P].cpu().numpy()
    rs = np.random.RandomState(17)
    arr = (rs.standard_normal(P) * 1e-2).astype(np.float32)
    p = theta.cpu().numpy()
    snap = D.theta_src(rs, p)
    m = np.abs(rs.standard_normal(P) * 1e-3).astype(np.float32)
    v = (rs.rand(P) * 1e-5).astype(np.float32)
    w, lam, c = D.WEIGHTS[0], 50.0, 5
    g = D.text_flat([S] * c + [arr], [None] * c + [snap], p, lam, [1.0] * c + [w], sizes)
    g_plain = D.text_flat([S] * c + [arr], [None] * (c + 1), p, lam, [1.0] * c + [w], sizes)
    assert np.isfinite(g).all() and F.n_diff(g, g_plain) > P // 4      # compensation acts
    pad = lambda a: np.concatenate([a, np.zeros(64, np.float32)])       # noqa: E731
    dA, dT = _dev(pad(arr)), _dev(pad(snap))
    out = torch.full_like(dS, float("nan"))
    t_out = torch.full_like(dS, float("nan"))

    def run(dp, dm, dv):
        eng.server_step(out, Rule(c + 1, [dA], c=c, weights=[w], snapshots=[dT], delay_comp=lam),
                        dp, dm, dv, 2, optim=o, theta_out=t_out)
    _step_and_compare(o, g, run, p, m, v, 2, label="fused W,C")
    assert torch.equal(out[:P], dS[:P])
    assert F.n_diff(t_out[:P], p) == 0


# ---- FLSimulation ------------------------------------------------------------------------------
N, DELAY, EPOCHS = 4, 2, 6
SIMS = {
    "adagrad": dict(optimizer="adagrad", lr=1e-2, lr_decay=0.05, weight_decay=5e-4,
                    initial_accumulator_value=0.1),
    "yogi": dict(optimizer="yogi", lr=1e-2, weight_decay=5e-4),
}


def _sim(pool, kind, **kw):
    from flsim.sim import FLSimulation
    return FLSimulation(N, delay=DELAY, throttle=True, device=DEV, chunk_workers=2, pool=pool,
                        **{**SIMS[kind], **kw})


def _state(sim):
    return [None if t is None else t.clone() for t in (sim.theta, sim.m, sim.v)]


def _same(a, b):
    return all((x is None and y is None) or
               bool((x.view(torch.int32) == y.view(torch.int32)).all()) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", sorted(SIMS))
def test_simulation_paths_checkpoint_and_accumulator(pool, kind, tmp_path):
    """n = 4, delay 2, 6 epochs across a tick: the fused run, the keep_S run and the distributed
    path at world 1 end bit-identical; a checkpoint at epoch 3 resumes bit for bit; after step 1
    the state is the text's step from the initial accumulator value (default: Yogi's 1e-6)."""
    import torch.distributed as dist
    a = _sim(pool, kind, keep_S=True)
    o = a.optim
    assert o.initial_accumulator_value == (0.1 if kind == "adagrad" else 1e-6)
    assert o.eps == (1e-10 if kind == "adagrad" else 1e-3)
    assert tuple(o.betas) == ((0.9, 0.999) if kind == "adagrad" else (0.9, 0.99))
    assert (a.v is None) == (kind == "adagrad")
    theta0 = a.theta.cpu().numpy().copy()
    acc = a.m if kind == "adagrad" else a.v
    assert bool((acc == np.float32(o.initial_accumulator_value)).all())
    a.epoch()
    S = a.comm[:a.P].cpu().numpy().copy()
    plan = a.trace[0]
    assert not plan.stale
    g = F.mean([S] * plan.c_t, list(a.engine.SIZES))
    hp = dict(kind=kind, lr=o.lr, eps=o.eps, weight_decay=o.weight_decay)
    hp.update(dict(lr_decay=o.lr_decay) if kind == "adagrad" else dict(betas=tuple(o.betas)))
    iav = np.full(a.P, o.initial_accumulator_value, np.float32)
    zero = np.zeros(a.P, np.float32)
    pe, me, ve = F.expected(hp, g, theta0, iav if kind == "adagrad" else zero, iav, 1)
    assert F.n_diff(a.theta, pe) == 0 and F.n_diff(a.m, me) == 0
    if kind == "adagrad":
        assert float(a.m.min()) >= 0.1
    else:
        assert F.n_diff(a.v, ve) == 0
        assert float(a.v.min()) >= 0.98e-6       # v_0 - (1 - beta2) g^2 >= 0.99 v_0 where g^2 < v_0
    for _ in range(1, EPOCHS):
        a.epoch()
    assert [t for t, pl in enumerate(a.trace) if pl.stale] == [2, 4]
    end = _state(a)
    assert not torch.equal(end[0], torch.from_numpy(theta0).to(DEV))
    b = _sim(pool, kind)                                     # the fused step
    for t in range(EPOCHS):
        b.epoch()
        if t == 2:
            path = tmp_path / "ck.pt"
            b.save_checkpoint(path)
    assert _same(_state(b), end)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["config"]["optimizer"] == kind
    assert ck["config"]["initial_accumulator_value"] == o.initial_accumulator_value
    assert ck["config"]["lr_decay"] == o.lr_decay and ("v" in ck) == (kind == "yogi")
    c = _sim(pool, kind)
    c.restore(path)
    for _ in range(3, EPOCHS):
        c.epoch()
    assert _same(_state(c), end)
    with pytest.raises(ValueError, match="initial_accumulator_value"):
        _sim(pool, kind, initial_accumulator_value=0.5).restore(path)
    # the distributed path (sharding, the all-reduce, the streaming step) over a one-rank group
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'pg'}", rank=0, world_size=1)
    try:
        d = _sim(pool, kind, distributed=True)
        assert d.distributed and d.world == 1
        for _ in range(EPOCHS):
            d.epoch()
        assert _same(_state(d), end)
    finally:
        dist.destroy_process_group()


# ---- the facade --------------------------------------------------------------------------------
def _one_update(pool, make):
    import torch.nn as nn
    from FL.agents import Agg, Central, Worker, rule
    from FL.models import PerformantNet1
    from oracle import oracle as O
    idx = O.batch_indices(0, 0, 0, 0, 2, O.class_lists(pool[1]))
    x = torch.from_numpy(O.normalize_lut()[pool[0][idx]]).to(DEV)
    y = torch.from_numpy(pool[1][idx]).to(DEV)
    torch.manual_seed(0)
    model = PerformantNet1().to(DEV)
    before = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).clone()
    optimizer = make(model.parameters())
    central = Central(model, optimizer)
    w = Worker(nn.CrossEntropyLoss())
    w.model = central.model
    ups, _ = w.fwd_bkwd(x, y)
    central.update_model(Agg(rule).rule([ups]))
    after = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    assert not torch.equal(before, after)
    return model, optimizer, central


def test_facade_takes_adagrad(pool):
    from FL.models import PerformantNet1
    model, optimizer, central = _one_update(
        pool, lambda ps: torch.optim.Adagrad(ps, lr=1e-2, initial_accumulator_value=0.1))
    ctx = central.ctx
    acc = ctx.m[:ctx.P]
    assert float(acc.min()) >= 0.1 and float(acc.max()) > 0.1
    off = 0
    for p in model.parameters():
        st = optimizer.state[p]
        assert set(st) == {"step", "sum"} and float(st["step"]) == 1.0
        assert st["sum"].shape == p.shape
        assert torch.equal(st["sum"].reshape(-1), acc[off:off + p.numel()])
        off += p.numel()
    fresh_model = PerformantNet1()
    fresh = torch.optim.Adagrad(fresh_model.parameters(), lr=1e-2, initial_accumulator_value=0.1)
    fresh.load_state_dict(optimizer.state_dict())
    p0 = next(fresh_model.parameters())
    assert torch.equal(fresh.state[p0]["sum"].reshape(-1), acc[:p0.numel()].cpu())
    assert float(fresh.state[p0]["step"]) == 1.0


def test_facade_takes_yogi(pool):
    from FL.models import PerformantNet1
    from flsim.optim import Yogi
    model, optimizer, central = _one_update(pool, lambda ps: Yogi(ps, lr=1e-2))
    ctx = central.ctx
    v = ctx.v[:ctx.P]
    assert float(v.min()) >= 0.98e-6 and float(v.max()) > 1e-6
    off = 0
    for p in model.parameters():
        st = optimizer.state[p]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 1.0
        assert torch.equal(st["exp_avg"].reshape(-1), ctx.m[off:off + p.numel()])
        assert torch.equal(st["exp_avg_sq"].reshape(-1), v[off:off + p.numel()])
        off += p.numel()
    fresh_model = PerformantNet1()
    fresh = Yogi(fresh_model.parameters(), lr=1e-2)
    fresh.load_state_dict(optimizer.state_dict())
    p0 = next(fresh_model.parameters())
    assert torch.equal(fresh.state[p0]["exp_avg_sq"].reshape(-1), v[:p0.numel()].cpu())
    assert torch.equal(fresh.state[p0]["exp_avg"].reshape(-1), ctx.m[:p0.numel()].cpu())
