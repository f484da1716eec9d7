"""GPU: the server step with a chosen optimizer (csrc/server.hip, flsim_aggregate_optim_rule_push
and flsim_<net>_server_step_optim): torch.optim.SGD (momentum, dampening, weight decay, nesterov),
torch.optim.Adam with weight_decay and torch.optim.AdamW.

Expected values: g = the oracle's cascade mean per tensor; SGD = torch.optim.SGD itself on CPU
tensors (.grad = g, the momentum buffer preset for steps > 1); the Adam family = torch CPU's
weight-decay prologue (g.add(p, alpha=wd), or p.mul_(1 - lr * wd) for AdamW) followed by the
oracle's Adam step, whose sqrt is correctly rounded like the kernel's.  Every comparison is bit
for bit: zero differing words in p and in every state array the kind owns; the arrays a kind does
not own (v for SGD, m and v for SGD without momentum) are passed poisoned and must come back
untouched, or are passed as None.
"""
import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

DEV = "cuda:0"
POISON = np.uint32(0x7FC12345)          # a NaN payload no arithmetic produces

KINDS = {
    "sgd": dict(kind="sgd", lr=0.01),
    "sgd_m": dict(kind="sgd", lr=0.01, momentum=0.9),
    "sgd_m_damp_wd": dict(kind="sgd", lr=0.01, momentum=0.9, dampening=0.1, weight_decay=5e-4),
    "sgd_nesterov_wd": dict(kind="sgd", lr=0.01, momentum=0.9, weight_decay=5e-4, nesterov=True),
    "adam_wd": dict(kind="adam", lr=1e-3, weight_decay=5e-4),
    "adamw": dict(kind="adamw", lr=1e-3, weight_decay=1e-2),
}
# (sizes, c, n_stale): > 8 row_sum tails -> split launches, the LDS-staged stream (3 entry arrays);
# the register streams with one float4 group per thread (a stale array) and with two (none)
LAYOUTS = {
    "tails_lds": ([5, 37, 64, 1, 96, 100, 33, 2, 3, 70, 9, 11], 6, 3),
    "reg_g1": ([1000, 4096, 33, 7], 3, 1),
    "reg_g2": ([1000, 4096, 33, 7], 9, 0),
}


def _n_state(o):
    return 2 if o["kind"] != "sgd" else (1 if o.get("momentum", 0) != 0 else 0)


def _inputs(P, ns, seed):
    """S with the division paths' edge values (+-0, a subnormal, a huge gradient), stale entries,
    p, m, v."""
    rs = np.random.RandomState(seed)
    S = (rs.standard_normal(P) * 1e-2).astype(np.float32)
    S[::17] = 0.0
    S[1::17] = -0.0
    S[2::17] = np.float32(3e-39) * rs.choice([-1, 1], len(S[2::17]))
    S[3::17] = np.float32(1e30)
    stale = [(rs.standard_normal(P) * 1e-2).astype(np.float32) for _ in range(ns)]
    p = rs.standard_normal(P).astype(np.float32)
    m = (rs.standard_normal(P) * 1e-3).astype(np.float32)
    v = (rs.rand(P) * 1e-5).astype(np.float32)
    return S, stale, p, m, v


def _mean(entries, sizes):
    from oracle import oracle as O
    g = np.empty_like(entries[0])
    off = 0
    for n in sizes:
        g[off:off + n] = O.cascade_mean([e[off:off + n] for e in entries])
        off += n
    return g


def _expected(o, g, p, m, v, step):
    """(p, m, v) after the update, m / v None where the kind owns no such array."""
    from oracle import oracle as O
    if o["kind"] == "sgd":
        hp = {k: o[k] for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov")
              if k in o}
        tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
        opt = torch.optim.SGD([tp], **hp)
        tp.grad = torch.from_numpy(g.copy())
        if _n_state(o) and step > 1:
            opt.state[tp]["momentum_buffer"] = torch.from_numpy(m.copy())
        opt.step()
        buf = opt.state[tp]["momentum_buffer"].numpy().copy() if _n_state(o) else None
        return tp.detach().numpy().copy(), buf, None
    tp, tg = torch.from_numpy(p.copy()), torch.from_numpy(g.copy())
    if o["kind"] == "adamw":
        tp.mul_(1 - o["lr"] * o["weight_decay"])
    else:
        tg = tg.add(tp, alpha=o["weight_decay"])
    pe, me, ve = tp.numpy().copy(), m.copy(), v.copy()
    O.adam_step(pe, me, ve, np.ascontiguousarray(tg.numpy()), step, lr=o["lr"])
    return pe, me, ve


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _run_and_compare(o, rule_of, entries_of, sizes, ns, step, seed, with_none=False):
    """One streaming step on the device against _expected."""
    from flsim.engine import aggregate_rule
    P = sum(sizes)
    S, stale, p, m, v = _inputs(P, ns, seed)
    nstate = _n_state(o)
    g = _mean(entries_of(S, stale), sizes)
    pe, me, ve = _expected(o, g, p, m, v, step)
    dS = torch.from_numpy(S).to(DEV)
    dst = [torch.from_numpy(s).to(DEV) for s in stale]
    dp = torch.from_numpy(p.copy()).to(DEV)
    poison = np.full(P, POISON, np.uint32).view(np.float32)
    dm = torch.from_numpy((m if nstate >= 1 else poison).copy()).to(DEV)
    dv = torch.from_numpy((v if nstate >= 2 else poison).copy()).to(DEV)
    am = dm if (nstate >= 1 or not with_none) else None
    av = dv if (nstate >= 2 or not with_none) else None
    aggregate_rule(dS, rule_of(dst), dp, am, av, step, sizes, optim=o)
    torch.cuda.synchronize()
    bad = {"p": int((_bits(dp) != pe.view(np.uint32)).sum())}
    bad["m"] = int((_bits(dm) != (me if nstate >= 1 else poison).view(np.uint32)).sum())
    bad["v"] = int((_bits(dv) != (ve if nstate >= 2 else poison).view(np.uint32)).sum())
    print(o, sizes[:2], ns, step, bad)
    assert bad == {"p": 0, "m": 0, "v": 0}, bad


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("step", [1, 3])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_stream_step_bit_exact_vs_torch(kind, step, layout):
    from flsim.engine import Rule
    sizes, c, ns = LAYOUTS[layout]
    _run_and_compare(KINDS[kind], lambda dst: Rule(c + ns, dst, c=c),
                     lambda S, stale: [S] * c + stale, sizes, ns, step,
                     seed=1000 * step + 10 * c + ns)


@pytest.mark.parametrize("kind", ["sgd", "sgd_m"])
def test_sgd_state_arrays_may_be_none(kind):
    """SGD owns no v (and without momentum no m): None is accepted for them."""
    from flsim.engine import Rule
    sizes, c, ns = LAYOUTS["tails_lds"]
    _run_and_compare(KINDS[kind], lambda dst: Rule(c + ns, dst, c=c),
                     lambda S, stale: [S] * c + stale, sizes, ns, 3, seed=77, with_none=True)
    sizes, c, ns = LAYOUTS["reg_g1"]
    _run_and_compare(KINDS[kind], lambda dst: Rule(c + ns, dst, c=c),
                     lambda S, stale: [S] * c + stale, sizes, ns, 3, seed=78, with_none=True)


def test_general_order_sgd_momentum():
    """A general-order rule (the staged program, k_agg_stream<false>) with SGD momentum 0.9."""
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
    _run_and_compare(KINDS["sgd_m"], rule_of, entries_of, sizes, 3, 3, seed=5)


def test_convenience_forms_take_optim():
    """aggregate_adam / aggregate_adam_sum with optim= equal aggregate_rule with the same rule."""
    from flsim.engine import Rule, aggregate_adam, aggregate_adam_sum, aggregate_rule
    sizes, c, ns = LAYOUTS["reg_g1"]
    P = sum(sizes)
    S, stale, p, m, _ = _inputs(P, ns, 9)
    o = KINDS["sgd_m"]
    dS = torch.from_numpy(S).to(DEV)
    dst = [torch.from_numpy(s).to(DEV) for s in stale]
    for call, rule in ((lambda a, b: aggregate_adam(dS, c, dst, a, b, None, 2, sizes, optim=o),
                        Rule(c + ns, dst, c=c)),
                       (lambda a, b: aggregate_adam_sum(dS, 7, a, b, None, 2, sizes, optim=o),
                        Rule(7, [], c=1))):
        a = [torch.from_numpy(x.copy()).to(DEV) for x in (p, m)]
        b = [torch.from_numpy(x.copy()).to(DEV) for x in (p, m)]
        call(*a)
        aggregate_rule(dS, rule, b[0], b[1], None, 2, sizes, optim=o)
        torch.cuda.synchronize()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert not torch.equal(a[0], torch.from_numpy(p).to(DEV))


@pytest.fixture(scope="module")
def pool():
    from oracle import oracle as O
    return O.make_pool(0)


def test_fused_step_equals_reduce_then_stream(pool):
    """One tiny PN1 chunk (2 workers), twice from the same state: the fused slab step with
    optim= against end_epoch + the streaming step with optim=.  theta, the state arrays the kind
    owns and S_out bit-identical; SGD momentum 0.9 nesterov on the reference-order and the
    general-order kernels, plus the other kernel kinds (plain SGD, AdamW) on the reference order."""
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
    tick = Rule(6, [arrs[0]], c=5)
    general = Rule(40, [arrs[0], arrs[1], None, arrs[2]],
                   events=[(0, 1), (7, 0), (8, 0), (21, 2), (33, 3), (39, 1)],
                   stager=ProgramStager(DEV))
    cases = [("sgd_nesterov_wd", tick), ("sgd_nesterov_wd", general), ("sgd", tick),
             ("adamw", tick)]
    for kind, rule in cases:
        o = KINDS[kind]
        nstate = _n_state(o)
        a = [theta.clone(), m0.clone(), v0.clone()]
        b = [theta.clone(), m0.clone(), v0.clone()]
        arg = lambda s: [s[0], s[1] if nstate >= 1 else None, s[2] if nstate >= 2 else None]  # noqa: E731
        eng.aggregate_rule(S, rule, *arg(a), 3, optim=o)
        out = torch.full_like(S, float("nan"))
        eng.server_step(out, rule, *arg(b), 3, optim=o)
        torch.cuda.synchronize()
        assert torch.equal(out[:P], S[:P]), kind
        assert not torch.equal(a[0], theta), kind
        for x, y, what in zip(a, b, "pmv"):
            bad = int((x.view(torch.int32) != y.view(torch.int32)).sum())
            assert bad == 0, (kind, what, bad)
        for j in range(nstate + 1, 3):       # not owned: untouched
            assert torch.equal(a[j], (m0, v0)[j - 1]) and torch.equal(b[j], (m0, v0)[j - 1])
