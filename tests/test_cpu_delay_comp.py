"""CPU checks of delay compensation (DC-ASGD, Zheng et al. 2017): a popped FIFO entry x, pushed when
the model was theta_src and popped when it is theta_now, enters the average as

    def compensate(x, theta_now, theta_src, lam):          # per parameter tensor, fp32
        return x + (x * x) * lam * (theta_now - theta_src)

(tests/_delay_comp.py holds the whole text).  The host twin of the compensated kernels
(flsim_cascade_eval_host_c) must equal that text on torch CPU bit for bit; the refusals of the
C-ABI (before any pointer) and of the Python layers; FLSimulation(delay_comp=) over a CPU stand-in
engine against a plain torch loop that keeps (entry, theta snapshot) in its FIFOs, in one process
and on two gloo ranks; checkpoint and resume across a live snapshot.
"""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _delay_comp as D

vp = ctypes.c_void_p
# (with weights, with one NULL snapshot)
VARIANTS = [(False, False), (True, False), (False, True), (True, True)]


def _twin(words, info, S, arrays, w, divisor, theta_now, snaps, lam, tail):
    from flsim import _lib
    n = S.size
    out = np.empty(n, np.float32)
    na = len(arrays)
    ys = (vp * max(1, na))(*[(a.ctypes.data if a is not None else None) for a in arrays])
    ts = (vp * max(1, na))(*[(a.ctypes.data if a is not None else None) for a in snaps])
    cw = (ctypes.c_double * max(1, na))(*w) if w is not None else None
    t = tail.astype(np.uint8)
    rc = _lib.lib().flsim_cascade_eval_host_c(
        words.ctypes.data_as(vp), info.ctypes.data_as(vp), S.ctypes.data_as(vp), ys, cw, na,
        float(divisor), theta_now.ctypes.data_as(vp), ts, float(lam), t.ctypes.data_as(vp), n,
        out.ctypes.data_as(vp))
    assert rc == 0, _lib.lib().flsim_last_error()
    return out


def _body(n):
    """Main-program columns of a tensor of n elements (rule_body of the weighted kernels)."""
    return n // 4 * 4 if n < 8 else n // 32 * 32


def _check(k, events, arrays, asnap, S, theta_now, lam, aw):
    """events [(position, array)], asnap / aw the arrays' snapshots / weights (aw None: the plain
    mean): the twin against the text.  -> (g, g without compensation, g contracted)."""
    from flsim.engine import cascade_program
    n = S.size
    words, info = cascade_program(k, events)
    ents, snaps, full = [S] * k, [None] * k, [1.0] * k
    for pos, a in events:
        ents[pos] = arrays[a] if arrays[a] is not None else np.zeros_like(S)
        snaps[pos] = asnap[a] if arrays[a] is not None else None
        if aw is not None:
            full[pos] = aw[a]
    W = float(sum(full)) if aw is not None else float(k)
    full = full if aw is not None else None
    ref = D.text_flat(ents, snaps, theta_now, lam, full, [n])
    assert np.isfinite(ref).all()                       # input condition: g is finite
    got = _twin(words, info, S, arrays, aw, W, theta_now, asnap, lam, np.arange(n) >= _body(n))
    bad = np.nonzero(D.bits(got) != D.bits(ref))[0]
    assert bad.size == 0, (k, events, lam, bad[:8], got[bad[:4]], ref[bad[:4]])
    plain = D.text_flat(ents, [None] * k, theta_now, lam, full, [n])
    contr = D.text_flat(ents, snaps, theta_now, lam, full, [n], comp=D.compensate_contracted)
    return got, plain, contr


def _inputs(seed, n, na):
    rs = np.random.RandomState(seed)
    S = D.values_S(rs, n)
    arrays = [D.values_comp(rs, n) for _ in range(na)]
    theta_now, first = D.theta_pair(rs, n)
    # every array its own push epoch, hence its own snapshot
    snaps = [first] + [D.theta_src(rs, theta_now) for _ in range(na - 1)]
    return S, arrays, theta_now, snaps


@pytest.mark.parametrize("lam", D.LAMBDAS)
@pytest.mark.parametrize("ns", [1, 2, 3])
@pytest.mark.parametrize("k", [5, 17, 40, 513])
def test_twin_equals_text_reference_order(k, ns, lam):
    """[S_t] * c + 1..3 stale entries; 1024 multi_row_sum columns + 7 row_sum tail columns; with
    and without weights, and with one array left uncompensated (NULL snapshot)."""
    n = 1024 + 7
    S, arrays, theta_now, snaps = _inputs(100 * k + ns, n, ns)
    events = [(k - ns + q, q) for q in range(ns)]
    for weighted, null_snap in VARIANTS:
        asnap = list(snaps)
        if null_snap:
            asnap[ns - 1] = None
        aw = D.WEIGHTS[:ns] if weighted else None
        got, plain, contr = _check(k, events, arrays, asnap, S, theta_now, lam, aw)
        ok, changed, contracted = D.input_conditions(got, plain, contr)
        print(k, ns, lam, weighted, null_snap, "changed %.3f" % changed, "contracted", contracted)
        if null_snap and ns == 1:
            assert changed == 0.0               # nothing left to compensate
        elif lam == 2.0 and not null_snap:
            # the inputs tell compensation from none, and the text from a contracted evaluation
            assert changed > 0.10 and contracted >= 10, (changed, contracted)


@pytest.mark.parametrize("lam", D.LAMBDAS)
@pytest.mark.parametrize("k", [5, 17, 40, 513])
def test_twin_equals_text_general_order(k, lam):
    """Stale entries among the S_t copies, two entries sharing an array (and its snapshot), one
    null array (torch-1.x zeros: stays 0 whatever its snapshot says)."""
    n = 1024 + 7
    S, arrays, theta_now, snaps = _inputs(k, n, 4)
    arrays[2] = None
    pos = [0, 3, 4, k // 2, k - 1] if k > 5 else [0, 1, 2, 4]
    events = list(zip(pos, [1, 0, 0, 2, 3] if k > 5 else [1, 0, 2, 3]))
    for weighted, null_snap in VARIANTS:
        asnap = list(snaps)
        if null_snap:
            asnap[3] = None
        aw = [D.WEIGHTS[0], D.WEIGHTS[1], D.WEIGHTS[2], 1.0] if weighted else None
        got, plain, contr = _check(k, events, arrays, asnap, S, theta_now, lam, aw)
        ok, changed, contracted = D.input_conditions(got, plain, contr)
        print(k, lam, weighted, null_snap, "changed %.3f" % changed, "contracted", contracted)
        if lam == 2.0:
            assert changed > 0.10 and contracted >= 10, (changed, contracted)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 31, 33])
def test_twin_equals_text_small_tensors(n):
    """Tensors below one 32-column block (the weighted kernels' column rule, as
    tests/test_cpu_stale_weight.py states it)."""
    for k, ns in ((5, 2), (9, 3), (40, 1)):
        if n == 1 and k > 9:
            continue        # a [k, 1] stack is one contiguous row to torch: another sum altogether
        S, arrays, theta_now, snaps = _inputs(1000 * n + k, n, ns)
        events = [(k - ns + q, q) for q in range(ns)]
        for weighted, null_snap in VARIANTS:
            asnap = list(snaps)
            if null_snap:
                asnap[0] = None
            _check(k, events, arrays, asnap, S, theta_now, 2.0,
                   D.WEIGHTS[:ns] if weighted else None)


# ---- refusals -------------------------------------------------------------------------------------
def _abi_call(lam, n=None, arrays=(), snaps=(), S=None, S_out=None, theta_out=None, p=None,
              fused=False, gradstate=None):
    """flsim_aggregate_optim_crule_push (or the fused pn1 step); the pointers are never read on the
    host, so made-up addresses do (the checks under test come before any launch)."""
    from flsim import _lib
    L = _lib.lib()
    comp = _lib.FlsimRuleComp()
    comp.n = len(arrays) if n is None else n
    comp.lam = lam
    for q, t in enumerate(snaps):
        comp.theta_src[q] = t
    o = _lib.FlsimOptim()
    o.kind, o.lr = 2, 0.1                      # SGD
    rule = _lib.FlsimRule()
    rule.k, rule.c, rule.n_arrays = 4 + len(arrays), 4, len(arrays)
    for q, a in enumerate(arrays):
        rule.arrays[q] = a
    sizes = (ctypes.c_long * 1)(64)
    if fused:
        rc = L.flsim_pn1_server_step_crule(gradstate, S_out, theta_out, ctypes.byref(rule), None,
                                           ctypes.byref(comp), p, None, None, 1, ctypes.byref(o),
                                           None)
    else:
        rc = L.flsim_aggregate_optim_crule_push(
            S, S_out, theta_out, ctypes.byref(rule), None, ctypes.byref(comp), p, None, None, 64,
            sizes, 1, 1, ctypes.byref(o), None)
    return rc, L.flsim_last_error().decode()


def test_abi_refuses_bad_lambda_and_count_before_any_pointer():
    from flsim import _lib
    for fused in (False, True):
        for lam in (-0.5, float("nan"), float("inf"), -float("inf")):
            rc, msg = _abi_call(lam, fused=fused)       # every data pointer NULL
            assert rc == 1 and "lambda" in msg, (lam, rc, msg)
        rc, msg = _abi_call(2.0, n=2, arrays=[0x30000], fused=fused)
        assert rc == 1 and "snapshots for 2 arrays" in msg, msg
        # a good lambda and count: the next refusal is the null pointers'
        rc, msg = _abi_call(2.0, fused=fused)
        assert rc == 1 and "null pointer" in msg, msg
    with pytest.raises(ValueError):
        _lib.check(_abi_call(-0.5)[0])


def test_abi_refuses_aliases():
    S, p, y, th, out, so = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    rc, msg = _abi_call(2.0, arrays=[S], snaps=[th], S=S, p=p)
    assert rc == 1 and "S_t itself" in msg, msg
    rc, msg = _abi_call(2.0, arrays=[so], snaps=[th], S=S, S_out=so, p=p)
    assert rc == 1 and "S_t itself" in msg, msg
    rc, msg = _abi_call(2.0, arrays=[y], snaps=[th], S=S, p=p, theta_out=p)
    assert rc == 1 and "theta_out aliases p" in msg, msg
    rc, msg = _abi_call(2.0, arrays=[y], snaps=[th], S=S, p=p, theta_out=th)
    assert rc == 1 and "theta_out aliases the snapshot" in msg, msg
    rc, msg = _abi_call(2.0, arrays=[y], snaps=[th + 4], S=S, p=p, theta_out=out)
    assert rc == 1 and "16-byte aligned" in msg, msg


def test_python_refusals():
    from flsim.engine import Rule
    from flsim.sim import FLSimulation
    with pytest.raises(ValueError):
        Rule(5, [None], c=4, snapshots=[None, None], delay_comp=2.0)
    with pytest.raises(ValueError):
        Rule(5, [None], c=4, snapshots=[None], delay_comp=-1.0)
    with pytest.raises(ValueError):
        Rule(5, [None], c=4, snapshots=[None], delay_comp=float("nan"))
    r = Rule(5, [None], c=4, snapshots=[None], delay_comp=2.0)
    assert r.delay_comp == 2.0 and r.c_comp.n == 1 and r.c_comp.lam == 2.0 and r.c_weights is None
    r = Rule(5, [None], c=4)
    assert r.snapshots is None and r.c_comp is None

    def sim(**kw):
        eng = StandInEngine()
        return FLSimulation(4, delay=2, device="cpu", engine=eng, device_pool=object(),
                            theta0=torch.zeros(eng.P), optimizer="sgd", lr=0.125, **kw)
    with pytest.raises(NotImplementedError):
        sim(semantics="independent", delay_comp=2.0)
    for lam in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            sim(delay_comp=lam)
    assert sim().delay_comp is None and sim(delay_comp=0.5).delay_comp == 0.5


# ---- FLSimulation over a stand-in engine --------------------------------------------------------
class StandInEngine:
    """CPU stand-in with the engine's interface.  A worker-step contributes an integer-valued
    vector that depends on (t, i, k), so S_t is exact in fp32 in any summation order (one process
    or two ranks); the server step is the rule text on torch with the rule's snapshots, lambda,
    weights and divisor, and plain SGD, theta -= lr * g."""
    P = 4096 + 33

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

    def aggregate_rule(self, S, rule, theta, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                       S_out=None, optim=None, theta_out=None):
        P = self.P
        if S_out is not None:
            S_out[:P].copy_(S)
        if theta_out is not None:
            theta_out[:P].copy_(theta)           # the pre-update theta
        na = len(rule.arrays)
        asn = rule.snapshots if rule.snapshots is not None else [None] * na
        aw = rule.weights if rule.weights is not None else [1.0] * na
        if rule.events is None:
            ev = [(rule.c + q, q) for q in range(na)]
        else:
            ev = rule.events
        ents, snaps, full = [[S]] * rule.k, [None] * rule.k, [1.0] * rule.k
        for pos, j in ev:
            ents[pos] = [rule.arrays[j][:P]]
            snaps[pos] = None if asn[j] is None else [asn[j][:P]]
            full[pos] = aw[j]
        lam = rule.delay_comp if rule.delay_comp is not None else 0.0
        if rule.weights is None:
            g = D.compensated_rule(ents, snaps, [theta], lam)[0]
        else:
            g = _weighted_text(ents, snaps, theta, lam, full, rule.divisor)
        self.log.append((sum(s is not None for s in snaps), rule.delay_comp,
                         None if rule.weights is None else list(rule.weights)))
        theta -= optim.lr * g


def _weighted_text(ents, snaps, theta, lam, full, divisor):
    """compensated_rule with weights, the divisor given (sum of the weights or the count)."""
    ys = [u if s is None else [D.compensate(u[0], theta, s[0], lam)] for u, s in zip(ents, snaps)]
    return torch.stack([y[0] * w for y, w in zip(ys, full)]).sum(0) / divisor


def _torch_loop(n, delays, throttle, epochs, seed, lr, lam, spec):
    """main.py:126-188 restated with the stand-in's gradients and a FIFO per slow worker holding
    (push epoch, the aliased S_t, the theta it was pushed at); each popped entry is compensated
    with its own snapshot, then discounted by its age; theta -= lr * g.  -> per epoch (number of
    compensated entries, theta)."""
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
                    ups.append([popped[1]])
                    snaps.append([popped[2]])
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
        if all(w == 1.0 for w in wts):
            g = D.compensated_rule(ups, snaps, [theta], lam)[0]
        else:
            g = D.compensated_rule(ups, snaps, [theta], lam, wts)[0]
        ncomp = sum(x is not None for x in snaps)
        theta = theta - lr * g
        out.append((ncomp, theta.clone()))
    return out


def _run(rank, world, out, port, kw):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "fl-distributed-delay_amd"))
    if world > 1:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from flsim.sim import FLSimulation
    eng = StandInEngine()
    sim = FLSimulation(kw["n"], delays=kw["delays"], throttle=kw["throttle"], device="cpu",
                       engine=eng, device_pool=object(), theta0=torch.zeros(eng.P),
                       optimizer="sgd", lr=kw["lr"], seed=kw["seed"], stale_weight=kw["spec"],
                       delay_comp=kw["lam"])
    thetas, live = [], []
    for _ in range(kw["epochs"]):
        sim.epoch()
        thetas.append(sim.theta.numpy().copy())
        assert sorted(sim.stale_theta) == (sorted(sim.stale_store) if kw["lam"] is not None
                                           else [])
        live.append(len(sim.stale_theta) + len(sim.free_snaps))
    res = dict(thetas=thetas, log=list(eng.log), live=live)
    if world > 1:
        dist.destroy_process_group()
    out[rank] = res


def _compare(res, ref):
    seen = 0
    for e, (ncomp, theta) in enumerate(ref):
        assert res["log"][e][0] == ncomp, (e, res["log"][e], ncomp)
        assert np.array_equal(res["thetas"][e].view(np.uint32),
                              theta.numpy().view(np.uint32)), e
        seen += ncomp > 0
    return seen


# n = 4, d = 2 for 7 epochs: the ticks t = 2, 4, 6 pop a compensated entry
KW = dict(n=4, delays=[0, 0, 0, 2], throttle=True, epochs=7, seed=3, lr=0.125, lam=2.0 ** -9,
          spec=None)


def _ref(kw):
    return _torch_loop(kw["n"], kw["delays"], kw["throttle"], kw["epochs"], kw["seed"], kw["lr"],
                       kw["lam"] if kw["lam"] is not None else 0.0, kw["spec"])


@pytest.mark.parametrize("spec", [None, ("poly", 0.5)])
def test_simulation_matches_torch_loop(spec):
    kw = dict(KW, spec=spec)
    ref = _ref(kw)
    assert [nc for (nc, _) in ref] == [0, 0, 1, 0, 1, 0, 1]
    out = {}
    _run(0, 1, out, 0, kw)
    assert _compare(out[0], ref) == 3                   # three ticks
    # snapshots are recycled with their slots: never more than two buffers in all
    assert max(out[0]["live"]) <= 2
    # compensation acts: the run without it ends elsewhere
    plain = {}
    _run(0, 1, plain, 0, dict(kw, lam=None))
    assert all(c is None for (_, c, _) in plain[0]["log"])
    assert not np.array_equal(plain[0]["thetas"][-1], out[0]["thetas"][-1])


def test_simulation_heterogeneous_delays_match_torch_loop():
    """Three slow workers among the fast ones, two delays: a general order; the two d = 2 workers
    pop entries of one source epoch (one array, one snapshot), and t = 6 also pops S_3 for d = 3
    (another array, another snapshot, another age)."""
    kw = dict(KW, n=5, delays=[0, 2, 0, 3, 2], throttle=False, epochs=8,
              spec=("poly", 0.5))
    ref = _ref(kw)
    assert [nc for (nc, _) in ref] == [0, 0, 2, 1, 2, 0, 3, 0]
    out = {}
    _run(0, 1, out, 0, kw)
    assert _compare(out[0], ref) == 4


def test_simulation_two_gloo_ranks_match_torch_loop():
    kw = dict(KW, spec=("poly", 0.5))
    ref = _ref(kw)
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    port = 29500 + (os.getpid() % 1000) + 57
    procs = [ctx.Process(target=_run, args=(r, 2, out, port, kw)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    for r in range(2):
        assert _compare(out[r], ref) == 3


def test_checkpoint_resumes_across_a_live_snapshot():
    from flsim.sim import FLSimulation

    def sim(**kw):
        eng = StandInEngine()
        return FLSimulation(4, delay=2, throttle=True, device="cpu", engine=eng,
                            device_pool=object(), theta0=torch.zeros(eng.P), optimizer="sgd",
                            lr=0.125, **kw)
    a = sim(delay_comp=2.0 ** -9)
    for _ in range(3):
        a.epoch()
    ck = a.checkpoint()
    assert ck["config"]["delay_comp"] == 2.0 ** -9
    assert sorted(ck["stale_theta"]) == sorted(ck["stale"]) == [2]       # the live slot's snapshot
    assert not torch.equal(ck["stale_theta"][2], ck["theta"])           # theta_2, not theta_3
    for kw in (dict(), dict(delay_comp=0.5)):
        with pytest.raises(ValueError):
            sim(**kw).restore(ck)
    b = sim(delay_comp=2.0 ** -9)
    b.restore(ck)
    for _ in range(3):                                  # t = 4 pops the restored entry
        a.epoch()
        b.epoch()
        assert np.array_equal(a.theta.numpy().view(np.uint32), b.theta.numpy().view(np.uint32))
    assert a.engine.log[-2][0] == 1 and b.engine.log[-2][0] == 1
    # a checkpoint from before delay compensation existed restores with compensation off
    old = sim().checkpoint()
    del old["config"]["delay_comp"], old["stale_theta"]
    sim().restore(old)
    with pytest.raises(ValueError):
        sim(delay_comp=0.5).restore(old)
