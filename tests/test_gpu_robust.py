"""GPU: the fused robust step (csrc/server.hip: k_robust through flsim_robust_optim_step), pinned
to the rule text of flsim/robust.py run by torch on the CPU.

  g        optim = NULL with g_out: equal to the text as numbers (tests/_robust.py), bit for bit on
           the zero-free, NaN-free inputs, over the k / trim grid and P in {1, 257, 4101, 300000};
  update   p / m / v after the fused step against the EXISTING step run on the text's g with k = 1
           (aggregate_adam_sum, the yardstick tests/test_gpu_clip.py uses), every optimizer kind,
           two consecutive steps: zero differing words;
  clipped  norm, coefficient and p against flsim_aggregate_optim_clip_push fed the text's g;
  sim      FLSimulation(robust_rule=...) on PerformantNet1 against the plain independent run, an
           engine pass per bucket and torch.optim.SGD on the text's g.

No comparison has a tolerance; the input conditions (no zero, no NaN where a yardstick would turn
-0 into +0; the norm away from a rounding midpoint) are asserted.
"""
import numpy as np
import pytest
import torch

import _clip as K
import _poison
import _robust as R
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

DEV = "cuda:0"
PS = (1, 257, 4101, 300000)      # the last: several blocks and a finisher tree with depth
PMAX = max(PS)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _poisoned(n):
    return torch.full((n,), R.QNAN, dtype=torch.int32, device=DEV).view(torch.float32)


def _g_only(dents, counts, kind, trim, P):
    from flsim.engine import Robust, robust_step
    g = _poisoned(P + 3)
    robust_step(Robust(kind, trim, dents, counts), None, None, None, 1, P=P, optim=False,
                g_out=g[:P])
    assert int((_bits(g[P:]) != R.QNAN).sum()) == 0          # nothing past P is written
    return g[:P].cpu().numpy()


@pytest.fixture(scope="module")
def inputs():
    """Per k: the bucket sums at the largest P (host and device, one allocation per entry) and
    their counts, made once; smaller P take prefixes."""
    cache = {}

    def get(k):
        if k not in cache:
            rs = np.random.RandomState(500 + k)
            ent = R.values(rs, k, PMAX)
            cache[k] = (ent, [_dev(e) for e in ent], R.counts_for(k))
        return cache[k]
    return get


@pytest.mark.parametrize("k", R.KS)
def test_g_bit_for_bit(inputs, k):
    """optim = NULL, g_out poisoned beforehand: every word of g equals the text's (whose values
    hold no zero and no NaN: asserted)."""
    ent, dent, cnt = inputs(k)
    for kind, trim in R.rules(k):
        for P in PS:
            ref = R.text([e[:P] for e in ent], cnt, kind, trim)
            assert np.isfinite(ref).all() and (ref != 0).all()          # input condition
            got = _g_only([d[:P] for d in dent], cnt, kind, trim, P)
            bad = int((R.bits(got) != R.bits(ref)).sum())
            assert bad == 0, (kind, trim, P, bad)


@pytest.mark.parametrize("k", R.KS)
def test_g_special_values_and_unaligned_entries(inputs, k):
    """Duplicates, +-inf and NaN in 1, ceil(k / 2) and k entries, a NULL entry and the -0 / +0 tie:
    equal as numbers.  Then entries that are rows of one [k, P] array with P = 257 and 4101: their
    addresses are no multiple of 16 bytes (an entry needs only its 4-byte alignment)."""
    P = 257
    for kind, trim in R.rules(k):
        for name, (ent, cnt) in R.special_cases(k, P).items():
            ref = R.text(ent, cnt, kind, trim)
            got = _g_only([_dev(e) for e in ent], cnt, kind, trim, P)
            assert R.mismatches(got, ref) == 0, (kind, trim, name)
    ent, _, cnt = inputs(k)
    for P in (257, 4101):
        rows = _dev(np.stack([e[:P] for e in ent]))
        assert k == 1 or any(r.data_ptr() % 16 for r in rows)
        for kind, trim in R.rules(k):
            ref = R.text([e[:P] for e in ent], cnt, kind, trim)
            got = _g_only(list(rows), cnt, kind, trim, P)
            assert int((R.bits(got) != R.bits(ref)).sum()) == 0, (kind, trim, P)


KINDS = {
    "adam": dict(kind="adam", lr=1e-3),
    "adamw": dict(kind="adamw", lr=1e-3, weight_decay=0.1),
    "sgd": dict(kind="sgd", lr=0.01),
    "sgdm": dict(kind="sgd", lr=0.01, momentum=0.9, weight_decay=1e-3),
    "adagrad": dict(kind="adagrad", lr=0.01, lr_decay=1e-3, eps=1e-10),
    "yogi": dict(kind="yogi", lr=0.01, betas=(0.9, 0.99), eps=1e-3),
}


def _n_state(o):
    from flsim.engine import Optim
    return Optim(**o).n_state


def _state(P, seed):
    rs = np.random.RandomState(seed)
    p = (rs.standard_normal(P) * 0.05).astype(np.float32)
    m = np.abs(rs.standard_normal(P) * 1e-3).astype(np.float32)      # >= 0: Adagrad's sum
    v = (rs.rand(P) * 1e-5 + 1e-8).astype(np.float32)
    return p, m, v


@pytest.mark.parametrize("k", (3, 16, 64))
@pytest.mark.parametrize("name", list(KINDS))
def test_update_equals_existing_step_on_the_texts_g(inputs, name, k):
    """Two consecutive fused steps (the state carries over; the second step's entries differ)
    against the existing k = 1 step on the text's g; arrays a kind does not own are passed
    poisoned to the fused step and stay untouched."""
    from flsim.engine import Robust, aggregate_adam_sum, robust_step
    o = KINDS[name]
    nstate = _n_state(o)
    P = 4101
    ent, dent, cnt = inputs(k)
    for kind, trim in (("median", 0), ("trimmed_mean", 1)):
        p0, m0, v0 = _state(P, 7 * k + trim)
        a = [_dev(p0), _dev(m0) if nstate >= 1 else _poisoned(P),
             _dev(v0) if nstate >= 2 else _poisoned(P)]
        b = [_dev(p0), _dev(m0) if nstate >= 1 else None, _dev(v0) if nstate >= 2 else None]
        for step in (1, 2):
            lo = (step - 1) * P
            g = R.text([e[lo:lo + P] for e in ent], cnt, kind, trim)
            assert np.isfinite(g).all() and (g != 0).all()              # input condition
            robust_step(Robust(kind, trim, [d[lo:lo + P] for d in dent], cnt), a[0], a[1], a[2],
                        step, optim=o)
            aggregate_adam_sum(_dev(g), 1, b[0], b[1], b[2], step, [P], optim=o)
            for x, y, what in zip(a, b, "pmv"):
                if y is None:
                    assert int((_bits(x) != R.QNAN).sum()) == 0, (name, what)
                    continue
                bad = int((_bits(x) != _bits(y)).sum())
                assert bad == 0, (name, kind, step, what, bad)
        assert not np.array_equal(_bits(a[0]), R.bits(p0))


@pytest.mark.parametrize("name", ["adam", "sgdm"])
def test_clipped_step_equals_existing_clipped_step(inputs, name):
    """k = 16, P = 300000, max_norm below and above the norm: total_norm, coef and p / m / v
    against flsim_aggregate_optim_clip_push fed the text's g as a k = 1 rule; g_out also receives
    g; the scratch is poisoned first."""
    from flsim.engine import Clip, Robust, Rule, aggregate_rule, robust_step
    k, P = 16, 300000
    o = KINDS[name]
    nstate = _n_state(o)
    ent, dent, cnt = inputs(k)
    g = R.text(ent, cnt, "trimmed_mean", 1)
    assert np.isfinite(g).all() and (g != 0).all()                      # input condition
    exact, norm, dist = K.exact_norm(g)
    assert dist >= K.MIN_MIDPOINT_DISTANCE
    for mn in (0.5 * float(norm), 2.0 * float(norm)):
        p0, m0, v0 = _state(P, 11)
        a = [_dev(p0), _dev(m0), _dev(v0) if nstate >= 2 else None]
        b = [_dev(p0), _dev(m0), _dev(v0) if nstate >= 2 else None]
        ca, cb = Clip(mn), Clip(mn)
        ca.c_struct(torch.device(DEV), P)
        for buf in ca._scratch[(DEV, P)]:
            buf.view(torch.int32).fill_(R.QNAN)
        gout = _poisoned(P)
        robust_step(Robust("trimmed_mean", 1, dent, cnt), a[0], a[1], a[2], 1, optim=o, clip=ca,
                    g_out=gout)
        aggregate_rule(_dev(g), Rule(1, [], c=1), b[0], b[1], b[2], 1, [P], optim=o, clip=cb)
        assert int((_bits(gout) != R.bits(g)).sum()) == 0
        assert K.bits(ca.total_norm.cpu().numpy()) == K.bits(norm)
        assert K.bits(ca.total_norm.cpu().numpy()) == K.bits(cb.total_norm.cpu().numpy())
        assert K.bits(ca.coef.cpu().numpy()) == K.bits(cb.coef.cpu().numpy())
        assert (float(ca.coef) == 1.0) == (mn > float(norm))
        for x, y, what in zip(a, b, "pmv"):
            if x is not None:
                bad = int((_bits(x) != _bits(y)).sum())
                assert bad == 0, (mn, what, bad)


def test_refusals_on_device_pointers():
    """An entry aliasing p, m, g_out or the clip's G, and a misaligned p / g_out: ValueError, and
    nothing is launched (p keeps its bits)."""
    from flsim.engine import Clip, Robust, robust_step
    P = 1000
    rs = np.random.RandomState(1)
    ent = [_dev(e) for e in R.values(rs, 3, P)]
    buf = _dev(rs.standard_normal(P + 8).astype(np.float32))
    p, m = buf[:P], _dev(np.zeros(P, np.float32))
    before = buf.clone()
    o = KINDS["sgdm"]
    cnt = [1, 3, 128]
    for bad in ([ent[0], p, ent[2]], [buf[4:P + 4], ent[1], ent[2]], [ent[0], ent[1], m]):
        with pytest.raises(ValueError, match="overlaps"):
            robust_step(Robust("median", 0, bad, cnt), p, m, None, 1, optim=o)
    gout = torch.zeros(P, device=DEV)
    with pytest.raises(ValueError, match="overlaps"):
        robust_step(Robust("median", 0, [ent[0], gout, ent[2]], cnt), p, m, None, 1, optim=o,
                    g_out=gout)
    clip = Clip(1.0)
    clip.c_struct(torch.device(DEV), P)
    G = clip._scratch[(DEV, P)][0]
    with pytest.raises(ValueError, match="clip G"):
        robust_step(Robust("median", 0, [ent[0], ent[1], G[:P]], cnt), p, m, None, 1, optim=o,
                    clip=clip)
    with pytest.raises(ValueError, match="16-byte aligned"):
        robust_step(Robust("median", 0, ent, cnt), buf[1:P + 1], m, None, 1, P=P, optim=o)
    with pytest.raises(ValueError, match="16-byte aligned"):
        robust_step(Robust("median", 0, ent, cnt), p, m, None, 1, optim=o, g_out=gout[1:])
    with pytest.raises(ValueError, match="null pointer"):
        robust_step(Robust("median", 0, ent, cnt), None, m, None, 1, P=P, optim=o)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32))


# ---- FLSimulation on PerformantNet1 ----------------------------------------------------------------
N, EPOCHS, LR, CW = 12, 4, 0.01, 4


@pytest.fixture(scope="module")
def pool():
    from oracle import oracle as O
    return O.make_pool(0)


def _sim(pool, **kw):
    from flsim.sim import FLSimulation
    return FLSimulation(N, device=DEV, chunk_workers=CW, pool=pool, dropout=False,
                        semantics="independent", **kw)


def test_simulation_one_bucket_median_is_the_plain_mean(pool):
    """(a) buckets = 1 and a delay so large that nothing pops: the one entry's median is S / n, so
    theta is bit-identical to the plain independent run after every epoch."""
    plain = _sim(pool, delay=100)
    rob = _sim(pool, delay=100, robust_rule="median", buckets=1, keep_entries=True)
    theta0 = rob.theta.clone()
    for t in range(EPOCHS):
        la, lb = plain.epoch(), rob.epoch()
        assert la == lb
        assert not rob.trace[-1].stale and rob.last_entries[1] == [N - 1]
        bad = int((_bits(plain.theta) != _bits(rob.theta)).sum())
        assert bad == 0, (t, bad)
    assert not torch.equal(rob.theta, theta0)                           # the run moved


def _sgd(g, p, lr):
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.SGD([tp], lr=lr)
    tp.grad = torch.from_numpy(np.ascontiguousarray(g).copy())
    opt.step()
    return tp.detach().numpy().copy()


def test_simulation_buckets_trimmed_mean(pool):
    """(b) buckets = 3, one slow worker with delay 2, ("trimmed_mean", 1): every bucket entry is
    bit-identical to an engine pass over exactly those workers' records; theta after each epoch,
    the pop epochs included, equals torch.optim.SGD on the CPU applied to the text's g of
    last_entries.  (c) The same run with keep_entries = False, its engine buffers and free slots
    poisoned before every epoch, gives identical theta."""
    from flsim.engine import PN1Engine, worker_table
    kw = dict(delay=2, robust_rule=("trimmed_mean", 1), buckets=3, optimizer="sgd", lr=LR)
    sim = _sim(pool, keep_entries=True, **kw)
    other = _sim(pool, **kw)
    eng = PN1Engine(DEV, chunk_workers=CW)
    rs = np.random.RandomState(sim.seed)
    pops = 0
    for t in range(EPOCHS):
        before = sim.theta.clone()
        ks = rs.randint(0, N, size=N)
        sim.epoch()
        plan = sim.trace[-1]
        ents, counts = sim.last_entries
        fast = [i for i in range(N) if plan.computes[i] and sim.delays[i] == 0]
        assert len(fast) == N - 1
        bounds = [(j * len(fast)) // 3 for j in range(4)]
        assert counts[:3] == [b1 - b0 for b0, b1 in zip(bounds[:-1], bounds[1:])]
        assert len(ents) == 3 + bool(plan.stale) and all(c <= CW for c in counts[:3])
        for j in range(3):
            ws = fast[bounds[j]:bounds[j + 1]]
            eng.begin_epoch(before)
            eng.run_chunk(before, sim.pool, worker_table([(t, i, int(ks[i])) for i in ws], DEV),
                          len(ws), N, sim.seed, False, torch.zeros(len(ws), device=DEV))
            S = torch.empty(eng.P, device=DEV)
            eng.end_epoch(S)
            assert int((_bits(S) != _bits(ents[j])).sum()) == 0, (t, j)
        if plan.stale:
            pops += 1
            assert counts[3] == 1
        g = R.text([e.cpu().numpy() for e in ents], counts, "trimmed_mean", 1)
        assert np.isfinite(g).all()
        pe = _sgd(g, before.cpu().numpy(), LR)
        bad = int((pe.view(np.uint32) != _bits(sim.theta)).sum())
        assert bad == 0, (t, bad)
        # (c)
        _poison.fill(other.engine, _poison.QNAN)
        for slot in other.free_slots:
            slot[:other.P].view(torch.int32).fill_(_poison.QNAN)
        other.epoch()
        assert other.last_entries is None
        assert int((_bits(other.theta) != _bits(sim.theta)).sum()) == 0, t
    assert pops >= 1
