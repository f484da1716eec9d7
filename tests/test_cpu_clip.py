"""CPU checks of global-norm gradient clipping in the server step (tests/_clip.py holds
the text): the refusals of the C-ABI (max_norm before any pointer, then the clip buffers) and of the
Python layers; the host twin flsim_cascade_eval_host_clip against the text evaluated with torch
(reciprocal, *, clamp, clip_grads_with_norm_ on per-tensor views) on the g of the existing twins;
FLSimulation(clip_grad_norm=) over a CPU stand-in engine whose server step is that text, against a
plain torch loop, in one process and on two gloo ranks; checkpoint round trip and an older
checkpoint; main.parse and the facade keyword; clip_grad_norm=None leaves the trajectory alone.
"""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _clip as K
import _delay_comp as D

vp = ctypes.c_void_p
SIZES = [33, 7, 1000, 4101]


# ---- refusals -------------------------------------------------------------------------------------
def _abi_call(max_norm, G=None, partials=None, n_partials=0, out=None, S=None, S_out=None, p=None,
              arrays=(), snaps=(), theta_out=None, P=64):
    """flsim_aggregate_optim_clip_push with made-up addresses: the host never reads them, and every
    call here is refused before a launch."""
    from flsim import _lib
    L = _lib.lib()
    clip = _lib.FlsimClip()
    clip.max_norm = max_norm
    clip.G, clip.partials, clip.n_partials, clip.out = G, partials, n_partials, out
    o = _lib.FlsimOptim()
    o.kind, o.lr = 2, 0.1                      # SGD
    rule = _lib.FlsimRule()
    rule.k, rule.c, rule.n_arrays = 4 + len(arrays), 4, len(arrays)
    for q, a in enumerate(arrays):
        rule.arrays[q] = a
    comp = None
    if snaps:
        comp = _lib.FlsimRuleComp()
        comp.n, comp.lam = len(arrays), 0.5
        for q, t in enumerate(snaps):
            comp.theta_src[q] = t
    sizes = (ctypes.c_long * 1)(P)
    rc = L.flsim_aggregate_optim_clip_push(
        S, S_out, theta_out, ctypes.byref(rule), None,
        ctypes.byref(comp) if comp is not None else None, ctypes.byref(clip), p, None, None, P,
        sizes, 1, 1, ctypes.byref(o), None)
    return rc, L.flsim_last_error().decode()


def test_abi_refuses_bad_max_norm_before_any_pointer():
    from flsim import _lib
    for mn in (0.0, -1.0, float("nan"), -float("inf")):
        rc, msg = _abi_call(mn)                       # every data pointer NULL
        assert rc == 1 and "max_norm" in msg, (mn, rc, msg)
    # a good max_norm (inf included): the next refusal is the null pointers'
    for mn in (1.0, float("inf")):
        rc, msg = _abi_call(mn)
        assert rc == 1 and "null pointer" in msg, msg
    with pytest.raises(ValueError):
        _lib.check(_abi_call(0.0)[0])


def test_abi_refuses_bad_clip_buffers():
    S, p, y, th, G, part, out = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000
    ok = dict(S=S, p=p, G=G, partials=part, n_partials=1 << 20, out=out)
    for miss in ("G", "partials", "out"):
        rc, msg = _abi_call(1.0, **dict(ok, **{miss: None}))
        assert rc == 1 and "null clip buffer" in msg, (miss, msg)
    for k in ("G", "partials", "out"):
        rc, msg = _abi_call(1.0, **dict(ok, **{k: ok[k] + 4}))
        assert rc == 1 and "16-byte aligned" in msg, (k, msg)
    rc, msg = _abi_call(1.0, **dict(ok, n_partials=0))
    assert rc == 1 and "n_partials" in msg, msg
    # G over S, S_out, p, theta_out (whole or in part: P = 64 floats = 256 bytes)
    for kw in (dict(G=S), dict(G=p), dict(G=S + 128), dict(G=S - 240), dict(S_out=G),
               dict(theta_out=G + 16)):
        rc, msg = _abi_call(1.0, **dict(ok, **kw))
        assert rc == 1 and "overlaps" in msg, (kw, msg)
    # ... a stale array, a snapshot
    rc, msg = _abi_call(1.0, arrays=[G], **ok)
    assert rc == 1 and "overlaps entry array 0" in msg, msg
    rc, msg = _abi_call(1.0, arrays=[y], snaps=[G + 64], **ok)
    assert rc == 1 and "overlaps entry array 0" in msg, msg
    # adjacent buffers do not overlap: the next refusal (too few partials) is reached
    rc, msg = _abi_call(1.0, arrays=[y], snaps=[th], **dict(ok, G=S - 256, n_partials=0))
    assert rc == 1 and "n_partials" in msg, msg


def test_partials_bound_covers_the_layouts_in_use():
    """flsim_clip_partials(P) is at least the blocks any launch sequence writes: one per 1024
    elements plus the edge pieces; it grows with P and is small."""
    from flsim import _lib
    from flsim.engine import PN1_SIZES
    L = _lib.lib()
    for sizes in (SIZES, SIZES + [300000], PN1_SIZES):
        P = sum(sizes)
        n = L.flsim_clip_partials(P)
        assert P // 1024 + 8 * len(sizes) <= n <= 16 * (P // 1024) + 16384, (P, n)
    assert L.flsim_clip_partials(0) > 0 and L.flsim_clip_partials(-5) == 0


def test_python_refusals_and_keywords():
    import main
    from FL import agents, models
    from flsim.engine import Clip
    from flsim.sim import FLSimulation
    for mn in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError):
            Clip(mn)
        with pytest.raises(ValueError):
            _sim(clip_grad_norm=mn)
    assert Clip(float("inf")).max_norm == float("inf") and Clip(2).max_norm == 2.0
    assert _sim().clip is None and _sim().grad_norms() == []
    assert _sim(clip_grad_norm=3).clip.max_norm == 3.0
    assert isinstance(_sim(), FLSimulation)
    assert main.parse([]).clip_grad_norm is None
    assert main.parse(["--clip_grad_norm", "2.5"]).clip_grad_norm == 2.5
    assert main.parse(["--clip_grad_norm", "inf"]).clip_grad_norm == float("inf")
    # the facade keyword: refused like Clip before anything else; a good value reaches the
    # device check of a CPU model
    model = models.PerformantNet1()
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    with pytest.raises(ValueError):
        agents.Central(model, opt, clip_grad_norm=-1.0)
    with pytest.raises(RuntimeError, match="GPU"):
        agents.Central(model, opt, clip_grad_norm=1.0)


# ---- the host twin against the text ---------------------------------------------------------------
_arrs = K.arrs
_existing_twin = K.existing_twin


def _clip_twin(words, info, S, arrays, w, divisor, theta_now, snaps, lam, tail, max_norm):
    from flsim import _lib
    L = _lib.lib()
    n, na = S.size, len(arrays)
    out, nc = np.empty(n, np.float32), np.empty(2, np.float32)
    cw = (ctypes.c_double * max(1, na))(*w) if w is not None else None
    t = tail.astype(np.uint8)
    rc = L.flsim_cascade_eval_host_clip(
        words.ctypes.data_as(vp), info.ctypes.data_as(vp), S.ctypes.data_as(vp), _arrs(arrays), cw,
        na, float(divisor), theta_now.ctypes.data_as(vp),
        _arrs(snaps) if snaps is not None else None, float(lam), t.ctypes.data_as(vp), n,
        float(max_norm), out.ctypes.data_as(vp), nc.ctypes.data_as(vp))
    assert rc == 0, L.flsim_last_error()
    return out, nc[0], nc[1]


_tail_mask = K.tail_mask
FORMS = ["plain", "weighted", "compensated"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k,events,na", [(5, [(4, 0)], 1), (513, [(512, 0)], 1),
                                         (9, [(0, 1), (2, 0), (3, 0), (5, 2), (6, 1), (8, 2)], 3)])
def test_twin_equals_text(k, events, na, form):
    from flsim.engine import cascade_program
    P = sum(SIZES)
    rs = np.random.RandomState(1000 * k + FORMS.index(form))
    S = K.values(rs, P)
    arrays = [K.values(rs, P, 3.0) for _ in range(na)]
    theta_now, first = D.theta_pair(rs, P)
    snaps = [first] + [D.theta_src(rs, theta_now) for _ in range(na - 1)]
    w = None if form == "plain" else [D.WEIGHTS[q % 3] for q in range(na)]
    sn = snaps if form == "compensated" else None
    full = [1.0] * k
    for pos, a in events:
        full[pos] = 1.0 if w is None else w[a]
    divisor = float(k) if w is None else float(sum(full))
    words, info = cascade_program(k, events)
    tail = _tail_mask(SIZES, form != "plain")
    g = _existing_twin(words, info, S, arrays, w, divisor, theta_now, sn, 0.04, tail)
    assert np.isfinite(g).all()
    exact, norm, dist = K.exact_norm(g)
    assert dist >= K.MIN_MIDPOINT_DISTANCE, dist          # input condition
    for mn in (float(norm) * 0.5, float(norm), float(norm) * 2.0, float("inf")):
        got, t, coef = _clip_twin(words, info, S, arrays, w, divisor, theta_now, sn, 0.04, tail,
                                  mn)
        assert K.bits(t) == K.bits(norm), (t, norm)
        ref_coef = K.torch_coef(norm, mn)
        assert K.bits(coef) == K.bits(ref_coef), (mn, coef, ref_coef)
        ref = K.torch_clip(g, SIZES, mn, norm)
        assert np.array_equal(K.bits(got), K.bits(ref)), mn
        if mn >= float(norm) * 2.0:
            assert coef == 1.0 and np.array_equal(K.bits(got), K.bits(g))
        elif mn < float(norm):
            assert coef < 1.0 and not np.array_equal(K.bits(got), K.bits(g))


def test_twin_nan_norm_gives_nan_coefficient_and_minus_zero_survives():
    from flsim.engine import cascade_program
    words, info = cascade_program(1, [])
    n = 40
    S = np.linspace(-1, 1, n).astype(np.float32)
    S[3] = np.float32(-1e-45)           # the rule's division by 5 rounds it to -0
    tail = np.arange(n) >= 32
    th = np.zeros(n, np.float32)
    g = (S / np.float32(5.0)).astype(np.float32)
    assert K.has_negative_zero(g)
    got, t, coef = _clip_twin(words, info, S, [], None, 5.0, th, None, 0.0, tail, float("inf"))
    assert coef == 1.0 and np.array_equal(K.bits(got), K.bits(g))      # -0 stays -0
    S[5] = np.nan
    got, t, coef = _clip_twin(words, info, S, [], None, 5.0, th, None, 0.0, tail, 1.0)
    assert np.isnan(t) and np.isnan(coef) and np.isnan(got).all()
    assert np.isnan(K.torch_coef(np.float32("nan"), 1.0))              # as torch.clamp keeps it


# ---- FLSimulation over a stand-in engine --------------------------------------------------------
class StandInEngine:
    """CPU stand-in with the engine's interface (as in tests/test_cpu_delay_comp.py): a
    worker-step contributes an integer-valued vector, so S_t is exact in fp32 in any order; the
    server step is the rule text on torch, then the clipping text of tests/_clip.py when a Clip is
    given, then plain SGD, theta -= lr * g."""
    P = 4096 + 33
    SIZES = [4096, 33]

    def __init__(self):
        self.chunk_workers = 3
        self.acc = torch.zeros(self.P)
        self.log = []

    @staticmethod
    def grad(t, i, k, P):
        return ((torch.arange(P) * (i + 1) + 7 * t + 3 * k) % 17 - 8).float()

    def begin_epoch(self, theta):
        self.acc.zero_()

    def run_chunk(self, theta, pool, workers_dev, n_chunk, n_total, seed, dropout, loss_out,
                  backward=True):
        for j, (t, i, k, _) in enumerate(workers_dev.tolist()):
            self.acc += self.grad(t, i, k, self.P)
            loss_out[j] = float(t + 0.001 * i)

    def end_epoch(self, S):
        S.copy_(self.acc)

    def _update(self, g, theta, optim, clip):
        if clip is not None:
            g, norm = clip_text(g, self.SIZES, clip.max_norm)
            clip.total_norm = torch.tensor(norm)
            clip.coef = torch.tensor(K.torch_coef(norm, clip.max_norm))
        self.log.append(clip is not None)
        theta -= optim.lr * g

    def aggregate_rule(self, S, rule, theta, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                       S_out=None, optim=None, theta_out=None, clip=None):
        P = self.P
        if S_out is not None:
            S_out[:P].copy_(S)
        if theta_out is not None:
            theta_out[:P].copy_(theta)
        na = len(rule.arrays)
        asn = rule.snapshots if rule.snapshots is not None else [None] * na
        aw = rule.weights if rule.weights is not None else [1.0] * na
        ev = [(rule.c + q, q) for q in range(na)] if rule.events is None else rule.events
        ents, snaps, full = [[S]] * rule.k, [None] * rule.k, [1.0] * rule.k
        for pos, j in ev:
            ents[pos] = [rule.arrays[j][:P] if rule.arrays[j] is not None else torch.zeros(P)]
            snaps[pos] = None if asn[j] is None else [asn[j][:P]]
            full[pos] = aw[j]
        lam = rule.delay_comp if rule.delay_comp is not None else 0.0
        ys = [u if s is None else [D.compensate(u[0], theta, s[0], lam)]
              for u, s in zip(ents, snaps)]
        if rule.weights is None:
            g = D.rule(ys)[0]
        else:
            g = torch.stack([y[0] * w for y, w in zip(ys, full)]).sum(0) / rule.divisor
        self._update(g, theta, optim, clip)

    def aggregate_adam_sum(self, S, k, theta, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                           optim=None, clip=None):
        self._update(S / float(k), theta, optim, clip)


def clip_text(g, sizes, max_norm):
    """The clipping text on a flat torch g -> (g', fp32 norm)."""
    _, norm, _ = K.exact_norm(g.numpy())
    return torch.from_numpy(K.torch_clip(g.numpy(), sizes, max_norm, norm)), norm


def _torch_loop(n, delays, throttle, epochs, seed, lr, lam, spec, max_norm, semantics):
    """main.py:126-188 restated with the stand-in's gradients (as tests/test_cpu_delay_comp.py
    does), with torch's clipping between the aggregate and the step.  -> per epoch (norm, theta)."""
    from flsim.engine import staleness_weight
    s = staleness_weight(spec)
    rs = np.random.RandomState(seed)
    P = StandInEngine.P
    theta = torch.zeros(P)
    fifo = {i: [] for i in range(n) if delays[i] != 0}
    window, gone, out = 0, False, []
    for t in range(epochs):
        ks = rs.randint(0, n, size=n)
        S = torch.zeros(P)                     # the epoch's aliased .grad (agents.py:35)
        ups, snaps, wts = [], [], []
        for i in range(n):
            if delays[i] != 0:
                gone = False
                popped = None
                if t == 0 or t % delays[i] == 0:
                    S += StandInEngine.grad(t, i, int(ks[i]), P)
                    fifo[i].append((t, S, theta.clone()))
                    if t != 0:
                        popped = fifo[i].pop(0)
                if popped is not None:
                    ups.append([popped[1] if semantics == "reference" else torch.zeros(P)])
                    snaps.append([popped[2]] if lam is not None and semantics == "reference"
                                 else None)
                    wts.append(float(s(t - popped[0])))
                    gone = True
            elif window <= 0:
                S += StandInEngine.grad(t, i, int(ks[i]), P)
                ups.append([S])
                snaps.append(None)
                wts.append(1.0)
                if throttle:
                    window = 1
                    if not gone:
                        window = min(window * 2, 32)
            if window > 0:
                window -= 1
        lam_ = lam if lam is not None else 0.0
        if all(w == 1.0 for w in wts):
            g = D.compensated_rule(ups, snaps, [theta], lam_)[0]
        else:
            g = D.compensated_rule(ups, snaps, [theta], lam_, wts)[0]
        norm = None
        if max_norm is not None:
            g, norm = clip_text(g, StandInEngine.SIZES, max_norm)
        theta = theta - lr * g
        out.append((norm, theta.clone()))
    return out


def _sim(**kw):
    from flsim.sim import FLSimulation
    eng = StandInEngine()
    kw.setdefault("delay", 2)
    return FLSimulation(kw.pop("n", 4), throttle=kw.pop("throttle", True), device="cpu",
                        engine=eng, device_pool=object(), theta0=torch.zeros(eng.P),
                        optimizer="sgd", lr=kw.pop("lr", 0.125), **kw)


def _run(rank, world, out, port, kw):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "fl-distributed-delay_amd"))
    if world > 1:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    sim = _sim(n=kw["n"], delay=None, delays=kw["delays"], throttle=kw["throttle"], lr=kw["lr"],
               seed=kw["seed"], stale_weight=kw["spec"], delay_comp=kw["lam"],
               clip_grad_norm=kw["max_norm"], semantics=kw["semantics"])
    thetas = []
    for _ in range(kw["epochs"]):
        sim.epoch()
        thetas.append(sim.theta.numpy().copy())
    res = dict(thetas=thetas, norms=sim.grad_norms(), log=list(sim.engine.log))
    if world > 1:
        dist.destroy_process_group()
    out[rank] = res


# n = 4, d = 2 for 7 epochs: the ticks t = 2, 4, 6 pop a stale entry.  The stand-in's S_t has a norm
# of several hundred, so max_norm = 100 clips every epoch
KW = dict(n=4, delays=[0, 0, 0, 2], throttle=True, epochs=7, seed=3, lr=0.125, lam=2.0 ** -9,
          spec=("poly", 0.5), max_norm=100.0, semantics="reference")


def _ref(kw):
    return _torch_loop(kw["n"], kw["delays"], kw["throttle"], kw["epochs"], kw["seed"], kw["lr"],
                       kw["lam"], kw["spec"], kw["max_norm"], kw["semantics"])


def _compare(res, ref, clipped=True):
    for e, (norm, theta) in enumerate(ref):
        assert np.array_equal(res["thetas"][e].view(np.uint32), theta.numpy().view(np.uint32)), e
        if clipped:
            assert K.bits(np.float32(res["norms"][e])) == K.bits(norm), (e, res["norms"][e], norm)
    assert len(res["norms"]) == (len(ref) if clipped else 0)
    assert all(x == clipped for x in res["log"])


@pytest.mark.parametrize("kw", [
    KW,
    dict(KW, lam=None, spec=None, throttle=False),
    dict(KW, n=5, delays=[0, 2, 0, 3, 2], throttle=False, epochs=8),       # a general order
    dict(KW, semantics="torch1", lam=None),
    dict(KW, max_norm=float("inf")),
], ids=["comp+weights+throttle", "plain", "heterogeneous", "torch1", "inf"])
def test_simulation_matches_torch_loop(kw):
    ref = _ref(kw)
    assert all(np.isfinite(n_) and n_ > 0 for (n_, _) in ref)
    out = {}
    _run(0, 1, out, 0, kw)
    _compare(out[0], ref)
    # None takes today's path: the same trajectory as the loop without clipping, no norms
    off = {}
    _run(0, 1, off, 0, dict(kw, max_norm=None))
    _compare(off[0], _ref(dict(kw, max_norm=None)), clipped=False)
    same = np.array_equal(off[0]["thetas"][-1], out[0]["thetas"][-1])
    assert same == (kw["max_norm"] == float("inf"))       # clipping acts; inf does not


def test_simulation_independent_semantics_clips_the_mean():
    """Independent entries: S = the sum of the k distinct entries, the mean S / k is clipped."""
    kw = dict(KW, semantics="independent", lam=None, spec=None)
    out, off = {}, {}
    _run(0, 1, out, 0, kw)
    _run(0, 1, off, 0, dict(kw, max_norm=None))
    assert all(out[0]["log"]) and len(out[0]["norms"]) == kw["epochs"]
    assert not any(off[0]["log"]) and off[0]["norms"] == []
    assert not np.array_equal(out[0]["thetas"][-1], off[0]["thetas"][-1])
    # epoch 0: theta_1 = -lr * (g * coef) with g = -theta_1 / lr of the unclipped run (lr = 1/8)
    g0 = -off[0]["thetas"][0] / np.float32(0.125)
    gc, norm = clip_text(torch.from_numpy(g0), StandInEngine.SIZES, 100.0)
    assert K.bits(np.float32(out[0]["norms"][0])) == K.bits(norm)
    assert np.array_equal(out[0]["thetas"][0], (-(np.float32(0.125) * gc.numpy())))


def test_simulation_two_gloo_ranks_match_torch_loop():
    ref = _ref(KW)
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    port = 29500 + (os.getpid() % 1000) + 91
    procs = [ctx.Process(target=_run, args=(r, 2, out, port, KW)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    for r in range(2):
        _compare(out[r], ref)


def test_checkpoint_round_trip_and_older_checkpoint():
    a = _sim(clip_grad_norm=100.0)
    for _ in range(3):
        a.epoch()
    ck = a.checkpoint()
    assert ck["config"]["clip_grad_norm"] == 100.0 and len(ck["grad_norms"]) == 3
    for kw in (dict(), dict(clip_grad_norm=50.0), dict(clip_grad_norm=float("inf"))):
        with pytest.raises(ValueError):
            _sim(**kw).restore(ck)
    b = _sim(clip_grad_norm=100.0)
    b.restore(ck)
    for _ in range(3):
        a.epoch()
        b.epoch()
        assert np.array_equal(a.theta.numpy().view(np.uint32), b.theta.numpy().view(np.uint32))
    assert a.grad_norms() == b.grad_norms() and len(b.grad_norms()) == 6
    # a checkpoint from before clipping existed restores with clipping off
    old = _sim().checkpoint()
    del old["config"]["clip_grad_norm"], old["grad_norms"]
    _sim().restore(old)
    with pytest.raises(ValueError):
        _sim(clip_grad_norm=100.0).restore(old)
    # inf round-trips too
    c = _sim(clip_grad_norm=float("inf"))
    c.epoch()
    _sim(clip_grad_norm=float("inf")).restore(c.checkpoint())
