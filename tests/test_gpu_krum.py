"""GPU: the fused Krum / Multi-Krum step (csrc/server.hip: k_krum_dist, k_krum_finish, k_krum_apply
through flsim_krum_optim_step), pinned to the rule text of flsim/robust.py run by torch on the CPU.

  dist, score  within the derived bound of tests/_krum.py: 2 (P + 2) 2^-53 relative, and twice that;
  sel, g       equal / bit for bit (the text's scores at the cut are >= 1000 bounds apart: asserted
               for every case), over the (f, m) grid and P on both sides of the kernel's tile E;
  determinism  two runs over differently poisoned scratch give identical dist bits;
  update       p / m / v after the fused step against the EXISTING k = 1 step on the text's g, every
               optimizer kind, two consecutive steps: zero differing words;
  clipped      norm, coefficient and p against flsim_aggregate_optim_clip_push fed the text's g;
  sim          FLSimulation(robust_rule=("multi_krum", 1, 3)) on PerformantNet1 against an engine
               pass per bucket and torch.optim.SGD on the text's g.

The scratch, g_out and every unowned array are poisoned before each run.
"""
import numpy as np
import pytest
import torch

import _clip as C
import _krum as K
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

DEV = "cuda:0"
POISONS = (K.QNAN, 0x7F800001)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _poisoned(n, pat=K.QNAN):
    return torch.full((n,), pat, dtype=torch.int32, device=DEV).view(torch.float32)


def _tile(k):
    from flsim._lib import lib
    return int(lib().flsim_krum_tile_elems(k))


def _ps(k):
    E = _tile(k)
    return (1, 255, 256, 257, E - 1, E, E + 1, 3 * E + 5)


def _run(dents, counts, f, m, P, pat=K.QNAN):
    """One g-only step over poisoned scratch and g_out -> (g, dist, score, sel) on the host;
    nothing past P (g), k * k (dist), k (score), m (sel) is written."""
    from flsim.engine import Krum, krum_step
    k = len(counts)
    kr = Krum(f, m, dents, counts)
    kr.c_scratch(torch.device(DEV), P)
    bufs = Krum._scratch[(DEV, P, k)]
    for b in bufs:
        b.view(torch.int32).fill_(pat)
    g = _poisoned(P + 3, pat)
    krum_step(kr, None, None, None, 1, P=P, optim=False, g_out=g[:P])
    torch.cuda.synchronize()
    assert int((_bits(g[P:]) != pat).sum()) == 0
    _, dist, score, sel = bufs
    assert int((dist[k * k:].view(torch.int32) != pat).sum()) == 0
    assert int((score[k:].view(torch.int32) != pat).sum()) == 0
    assert int((sel[m:] != pat).sum()) == 0
    return (g[:P].cpu().numpy(), kr.dist.cpu().numpy().copy(), kr.score.cpu().numpy().copy(),
            [int(j) for j in kr.sel.tolist()])


_TEXT = {}


def _text(k, P, f, m, seed=0):
    """The text at the seeded inputs of (k, P), computed once per case and shared."""
    key = (k, P, f, m, seed)
    if key not in _TEXT:
        ent, cnt = K.inputs(k, P, seed)
        _TEXT[key] = K.text(ent, cnt, f, m)
    return _TEXT[key]


def _check(got, ref, P, m, what):
    g, d, s, sel = got
    g_t, d_t, s_t, sel_t = ref
    assert K.score_gap(s_t, m) >= 1000 * K.dist_bound(P), what              # input condition
    assert K.outside(d, d_t, K.dist_bound(P)) == 0, what
    assert K.outside(s, s_t, 2 * K.dist_bound(P)) == 0, what
    assert np.array_equal(d.view(np.uint64), d.T.copy().view(np.uint64)), what
    assert (np.diag(d) == 0).all(), what
    assert sel == sel_t, (what, sel, sel_t)
    bad = K.g_mismatches(g, g_t)
    assert bad == 0, (what, bad)


@pytest.mark.parametrize("k", K.KS)
def test_dist_score_sel_g(k):
    """The whole (f, m) grid at P in {1, 255, 256, 257, E - 1, E, E + 1, 3E + 5}."""
    for P in _ps(k):
        ent, cnt = K.inputs(k, P)
        dent = [_dev(e) for e in ent]
        for f, m in K.grid(k):
            _check(_run(dent, cnt, f, m, P), _text(k, P, f, m), P, m, (P, f, m))


@pytest.mark.parametrize("k", (4, 64))
def test_a_block_runs_several_tiles(k):
    """A P with more tiles than the grid has blocks (some block grid-strides over two), the last
    tile partial; k = 4 and k = 64 differ in the grid's cap and in the block size."""
    from flsim._lib import lib
    E = _tile(k)
    one_each = 1
    while lib().flsim_krum_partials((one_each + 1) * E, k) > lib().flsim_krum_partials(one_each * E, k):
        one_each *= 2                       # (doubling: the grid's cap is found in a few calls)
    P = one_each * E + 3 * E + 5
    assert lib().flsim_krum_partials(P, k) == lib().flsim_krum_partials(one_each * E, k)
    ent, cnt = K.inputs(k, P)
    dent = [_dev(e) for e in ent]
    for f, m in ((0, 1), (0, 3)):
        _check(_run(dent, cnt, f, m, P), K.text(ent, cnt, f, m), P, m, (k, P, f, m))


@pytest.mark.parametrize("k", (5, 16, 33, 64))
def test_unaligned_entries_and_special_inputs(k):
    """Entries that are rows of one [k, P] array with odd P (4-byte aligned only); a NULL entry; a
    duplicate pointer (distance exactly 0); one NaN entry (never selected, f >= 1); all NaN."""
    f = 1
    for P in (257, 3 * _tile(k) + 5):
        ent, cnt = K.inputs(k, P)
        rows = _dev(np.stack(ent))
        assert any(r.data_ptr() % 16 for r in rows)
        for m in (1, k - f):
            _check(_run(list(rows), cnt, f, m, P), _text(k, P, f, m), P, m, ("rows", P, m))
    P = 257
    ent, cnt = K.inputs(k, P, 3)
    ent[2] = None
    got = _run([_dev(e) for e in ent], cnt, f, 2, P)
    _check(got, K.text(ent, cnt, f, 2), P, 2, "null")
    ent, cnt = K.inputs(k, P, 2)
    dent = [_dev(e) for e in ent]
    dent[1], cnt[1] = dent[0], cnt[0]
    g, d, s, sel = _run(dent, cnt, f, 1, P)
    ref = K.text([ent[0], ent[0]] + ent[2:], cnt, f, 1)
    assert d[0, 1] == 0.0 and d[1, 0] == 0.0 and (d[0, 2:] > 0).all()
    assert K.outside(d, ref[1], K.dist_bound(P)) == 0 and sel == ref[3]
    assert K.g_mismatches(g, ref[0]) == 0
    off = ~np.eye(k, dtype=bool)
    ent, cnt = K.inputs(k, P, 1)
    j = k // 2
    ent[j] = ent[j].copy()
    ent[j][3::7] = np.nan
    for m in (1, k - f):
        g, d, s, sel = _run([_dev(e) for e in ent], cnt, f, m, P)
        g_t, d_t, s_t, sel_t = K.text(ent, cnt, f, m)
        assert j not in sel and sel == sel_t
        assert np.isinf(d[j][off[j]]).all() and np.isinf(s[j]) and d[j, j] == 0
        assert K.outside(d[off], d_t[off], K.dist_bound(P)) == 0
        assert K.outside(s, s_t, 2 * K.dist_bound(P)) == 0
        assert np.isfinite(g).all() and K.g_mismatches(g, g_t) == 0
    nan = [_dev(np.full(P, np.nan, np.float32)) for _ in range(k)]
    g, d, s, sel = _run(nan, [1] * k, f, 3, P)
    assert sel == [0, 1, 2] and np.isnan(g).all() and np.isinf(d[off]).all() and np.isinf(s).all()


@pytest.mark.parametrize("k", (4, 9, 64))
def test_dist_bits_do_not_depend_on_the_scratch(k):
    """Two runs over scratch poisoned with different patterns: identical dist, score and g bits."""
    P = 3 * _tile(k) + 5
    ent, cnt = K.inputs(k, P)
    dent = [_dev(e) for e in ent]
    f, m = K.grid(k)[-1]
    a = _run(dent, cnt, f, m, P, POISONS[0])
    b = _run(dent, cnt, f, m, P, POISONS[1])
    assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))
    assert a[3] == b[3] and np.array_equal(K.bits(a[0]), K.bits(b[0]))


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


@pytest.mark.parametrize("k", (5, 17, 64))
@pytest.mark.parametrize("name", list(KINDS))
def test_update_equals_existing_step_on_the_texts_g(name, k):
    """Two consecutive fused steps (the state carries over; the second step's entries differ)
    against the existing k = 1 step on the text's g; arrays a kind does not own are passed
    poisoned to the fused step and stay untouched."""
    from flsim.engine import Krum, aggregate_adam_sum, krum_step
    o = KINDS[name]
    nstate = _n_state(o)
    P = 3 * _tile(k) + 5
    f = 1
    for m in (1, k - f):
        p0, m0, v0 = _state(P, 7 * k + m)
        a = [_dev(p0), _dev(m0) if nstate >= 1 else _poisoned(P),
             _dev(v0) if nstate >= 2 else _poisoned(P)]
        b = [_dev(p0), _dev(m0) if nstate >= 1 else None, _dev(v0) if nstate >= 2 else None]
        for step in (1, 2):
            ent, cnt = K.inputs(k, P, step)
            g, _, s_t, sel_t = _text(k, P, f, m, step)
            assert K.score_gap(s_t, m) >= 1000 * K.dist_bound(P)         # input condition
            assert np.isfinite(g).all() and (g != 0).all()
            kr = Krum(f, m, [_dev(e) for e in ent], cnt)
            krum_step(kr, a[0], a[1], a[2], step, optim=o)
            assert [int(j) for j in kr.sel.tolist()] == sel_t
            aggregate_adam_sum(_dev(g), 1, b[0], b[1], b[2], step, [P], optim=o)
            for x, y, what in zip(a, b, "pmv"):
                if y is None:
                    assert int((_bits(x) != K.QNAN).sum()) == 0, (name, what)
                    continue
                bad = int((_bits(x) != _bits(y)).sum())
                assert bad == 0, (name, m, step, what, bad)
        assert not np.array_equal(_bits(a[0]), K.bits(p0))


@pytest.mark.parametrize("name", ["adam", "sgdm"])
def test_clipped_step_equals_existing_clipped_step(name):
    """k = 16, Multi-Krum, max_norm below and above the norm: total_norm, coef and p / m / v
    against flsim_aggregate_optim_clip_push fed the text's g as a k = 1 rule; g_out also receives
    g; the scratch is poisoned first."""
    from flsim.engine import Clip, Krum, Rule, aggregate_rule, krum_step
    k, f, m = 16, 2, 5
    P = 3 * _tile(k) + 5
    o = KINDS[name]
    nstate = _n_state(o)
    ent, cnt = K.inputs(k, P)
    dent = [_dev(e) for e in ent]
    g, _, s_t, sel_t = _text(k, P, f, m)
    assert K.score_gap(s_t, m) >= 1000 * K.dist_bound(P)                 # input condition
    assert np.isfinite(g).all() and (g != 0).all()
    exact, norm, dist = C.exact_norm(g)
    assert dist >= C.MIN_MIDPOINT_DISTANCE
    for mn in (0.5 * float(norm), 2.0 * float(norm)):
        p0, m0, v0 = _state(P, 11)
        a = [_dev(p0), _dev(m0), _dev(v0) if nstate >= 2 else None]
        b = [_dev(p0), _dev(m0), _dev(v0) if nstate >= 2 else None]
        ca, cb = Clip(mn), Clip(mn)
        ca.c_struct(torch.device(DEV), P)
        for buf in ca._scratch[(DEV, P)]:
            buf.view(torch.int32).fill_(K.QNAN)
        gout = _poisoned(P)
        kr = Krum(f, m, dent, cnt)
        krum_step(kr, a[0], a[1], a[2], 1, optim=o, clip=ca, g_out=gout)
        aggregate_rule(_dev(g), Rule(1, [], c=1), b[0], b[1], b[2], 1, [P], optim=o, clip=cb)
        assert [int(j) for j in kr.sel.tolist()] == sel_t
        assert int((_bits(gout) != K.bits(g)).sum()) == 0
        assert C.bits(ca.total_norm.cpu().numpy()) == C.bits(norm)
        assert C.bits(ca.total_norm.cpu().numpy()) == C.bits(cb.total_norm.cpu().numpy())
        assert C.bits(ca.coef.cpu().numpy()) == C.bits(cb.coef.cpu().numpy())
        assert (float(ca.coef) == 1.0) == (mn > float(norm))
        for x, y, what in zip(a, b, "pmv"):
            if x is not None:
                bad = int((_bits(x) != _bits(y)).sum())
                assert bad == 0, (mn, what, bad)


def test_refusals_on_device_pointers():
    """An entry aliasing p, m, g_out or the scratch, f / m out of range, a misaligned p:
    ValueError, and nothing is launched (p keeps its bits)."""
    from flsim.engine import Krum, krum_step
    P = 1000
    rs = np.random.RandomState(1)
    ent = [_dev(e) for e in K.inputs(5, P)[0]]
    cnt = [1, 2, 3, 4, 1]
    buf = _dev(rs.standard_normal(P + 8).astype(np.float32))
    p, m = buf[:P], _dev(np.zeros(P, np.float32))
    before = buf.clone()
    o = KINDS["sgdm"]
    for bad in ([ent[0], p] + ent[2:], [buf[4:P + 4]] + ent[1:], ent[:4] + [m]):
        with pytest.raises(ValueError, match="overlaps"):
            krum_step(Krum(1, 1, bad, cnt), p, m, None, 1, optim=o)
    gout = torch.zeros(P, device=DEV)
    with pytest.raises(ValueError, match="overlaps"):
        krum_step(Krum(1, 1, ent[:4] + [gout], cnt), p, m, None, 1, optim=o, g_out=gout)
    kr = Krum(1, 1, ent, cnt)
    kr.c_scratch(torch.device(DEV), P)
    with pytest.raises(ValueError, match="Krum scratch"):
        krum_step(Krum(1, 1, ent[:4] + [kr.partials.view(torch.float32)[:P]], cnt), p, m, None, 1,
                  optim=o)
    for f, mm, what in ((2, 1, "Invalid f"), (-1, 1, "Invalid f"), (1, 5, "Invalid m"),
                        (1, 0, "Invalid m")):
        with pytest.raises(ValueError, match=what):
            krum_step(Krum(f, mm, ent, cnt), p, m, None, 1, optim=o)
    with pytest.raises(ValueError, match="16-byte aligned"):
        krum_step(Krum(1, 1, ent, cnt), buf[1:P + 1], m, None, 1, P=P, optim=o)
    with pytest.raises(ValueError, match="null pointer"):
        krum_step(Krum(1, 1, ent, cnt), None, m, None, 1, P=P, optim=o)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32))


# ---- FLSimulation on PerformantNet1 ----------------------------------------------------------------
N, EPOCHS, LR, CW = 12, 3, 0.01, 4       # (the slow worker's first entry pops in the third epoch)


@pytest.fixture(scope="module")
def pool():
    from oracle import oracle as O
    return O.make_pool(0)


def _sgd(g, p, lr):
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.SGD([tp], lr=lr)
    tp.grad = torch.from_numpy(np.ascontiguousarray(g).copy())
    opt.step()
    return tp.detach().numpy().copy()


def test_simulation_multi_krum(pool):
    """buckets = 6, one slow worker with delay 2, ("multi_krum", 1, 3): every bucket entry is
    bit-identical to an engine pass over exactly those workers' records; last_selected is the
    text's selection over last_entries and theta after each epoch, the pop epochs included, equals
    torch.optim.SGD on the CPU applied to the text's g."""
    from flsim.engine import PN1Engine, worker_table
    from flsim.sim import FLSimulation
    sim = FLSimulation(N, device=DEV, chunk_workers=CW, pool=pool, dropout=False,
                       semantics="independent", delay=2, robust_rule=("multi_krum", 1, 3),
                       buckets=6, optimizer="sgd", lr=LR, keep_entries=True)
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
        bounds = [(j * len(fast)) // 6 for j in range(7)]
        assert counts[:6] == [b1 - b0 for b0, b1 in zip(bounds[:-1], bounds[1:])]
        assert len(ents) == 6 + bool(plan.stale)
        for j in range(6):
            ws = fast[bounds[j]:bounds[j + 1]]
            eng.begin_epoch(before)
            eng.run_chunk(before, sim.pool, worker_table([(t, i, int(ks[i])) for i in ws], DEV),
                          len(ws), N, sim.seed, False, torch.zeros(len(ws), device=DEV))
            S = torch.empty(eng.P, device=DEV)
            eng.end_epoch(S)
            assert int((_bits(S) != _bits(ents[j])).sum()) == 0, (t, j)
        pops += bool(plan.stale)
        g, d, s, sel = K.text([e.cpu().numpy() for e in ents], counts, 1, 3)
        assert K.score_gap(s, 3) >= 1000 * K.dist_bound(eng.P), t          # input condition
        assert np.isfinite(g).all()
        assert sim.last_selected == sel, (t, sim.last_selected, sel)
        pe = _sgd(g, before.cpu().numpy(), LR)
        bad = int((pe.view(np.uint32) != _bits(sim.theta)).sum())
        assert bad == 0, (t, bad)
    assert pops >= 1
