"""GPU: the fused geometric-median step (csrc/server.hip: k_geomed_dist, k_geomed_finish,
k_geomed_apply through flsim_geomed_optim_step), pinned stage by stage to the rule text of
flsim/robust.py run by torch on the CPU (tests/_geomed.py: the stepwise comparison).

  d2[r]         within 2 (P + 2) 2^-53 relative of the text's distances at the device's own w[r];
  w[r + 1], obj[r], g    bit for bit the text's scalar code on the device's d2[r], and _wsum at
                the device's w[iters]; over KS, P on both sides of the kernel's tile E, iters in
                {0, 1, 3}, both weightings;
  determinism   two runs over differently poisoned scratch give identical bits, and nothing past
                the documented extents is written;
  update        p / m / v after the fused step against the EXISTING k = 1 step on the text's g,
                every optimizer kind, two consecutive steps: zero differing words;
  clipped       norm, coefficient and p against flsim_aggregate_optim_clip_push fed the same g;
  sim           FLSimulation(robust_rule=("geomed", 3)) on PerformantNet1 against an engine pass
                per bucket and torch.optim.SGD on g.

The scratch, g_out and every unowned array are poisoned before each run.
"""
import numpy as np
import pytest
import torch

import _clip as C
import _geomed as G
from conftest import has_gpu
from test_gpu_krum import KINDS, _n_state, _state

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

DEV = "cuda:0"
POISONS = (G.QNAN, 0x7F800001)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _poisoned(n, pat=G.QNAN):
    return torch.full((n,), pat, dtype=torch.int32, device=DEV).view(torch.float32)


def _tile(k):
    from flsim._lib import lib
    return int(lib().flsim_geomed_tile_elems(k))


def _ps(k):
    E = _tile(k)
    return (1, 255, 256, 257, E - 1, E, E + 1, 3 * E + 5)


def _poison_scratch(gm, P, pat):
    from flsim.engine import GeoMed
    gm.c_scratch(torch.device(DEV), P)
    bufs = GeoMed._scratch[(DEV, P, gm.k, gm.iters)]
    for b in bufs:
        b.view(torch.int32).fill_(pat)
    return bufs


def _outputs(gm):
    """(w, d2, obj) of the last step as numpy, and the dead flags."""
    return (gm.w.cpu().numpy().copy(), gm.d2.cpu().numpy().copy(), gm.obj.cpu().numpy().copy(),
            gm.dead.cpu().numpy().copy())


def _run(dents, counts, iters, weighted, P, pat=G.QNAN, nu=G.NU):
    """One g-only step over poisoned scratch and g_out -> ((g, w, d2, obj), dead) on the host;
    nothing past P (g), (iters + 1) k (w), iters k (d2), iters (obj), k + 4 (state) is written."""
    from flsim.engine import GeoMed, geomed_step
    k = len(counts)
    gm = GeoMed(iters, nu, weighted, dents, counts)
    _, wb, d2b, ob, sb = _poison_scratch(gm, P, pat)
    g = _poisoned(P + 3, pat)
    geomed_step(gm, None, None, None, 1, P=P, optim=False, g_out=g[:P])
    torch.cuda.synchronize()
    assert int((_bits(g[P:]) != pat).sum()) == 0
    assert int((wb[(iters + 1) * k:].view(torch.int32) != pat).sum()) == 0
    assert int((d2b[iters * k:].view(torch.int32) != pat).sum()) == 0
    assert int((ob[iters:].view(torch.int32) != pat).sum()) == 0
    assert int((sb[k + 4:] != pat).sum()) == 0
    w, d2, obj, dead = _outputs(gm)
    return (g[:P].cpu().numpy(), w, d2, obj), dead


@pytest.mark.parametrize("k", G.KS)
def test_stepwise_against_the_text(k):
    """KS x P in {1, 255, 256, 257, E - 1, E, E + 1, 3E + 5} x iters in {0, 1, 3} x both
    weightings."""
    for P in _ps(k):
        ent, cnt = G.inputs(k, P)
        dent = [_dev(e) for e in ent]
        for iters in (0, 1, 3):
            for weighted in (False, True):
                got, dead = _run(dent, cnt, iters, weighted, P)
                alive = G.stepwise(ent, cnt, iters, G.NU, weighted, got, (k, P, iters, weighted))
                assert alive.all() and not dead.any()


@pytest.mark.parametrize("k", (4, 64))
def test_a_block_runs_several_tiles(k):
    """A P with more tiles than the grid has blocks (some block grid-strides over two), the last
    tile partial; k = 4 and k = 64 differ in the grid's cap and in the tile."""
    from flsim._lib import lib
    E = _tile(k)
    one_each = 1
    while lib().flsim_geomed_partials((one_each + 1) * E, k) > \
            lib().flsim_geomed_partials(one_each * E, k):
        one_each *= 2                       # (doubling: the grid's cap is found in a few calls)
    P = one_each * E + 3 * E + 5
    assert lib().flsim_geomed_partials(P, k) == lib().flsim_geomed_partials(one_each * E, k)
    ent, cnt = G.inputs(k, P)
    dent = [_dev(e) for e in ent]
    got, dead = _run(dent, cnt, 2, True, P)
    G.stepwise(ent, cnt, 2, G.NU, True, got, (k, P))


@pytest.mark.parametrize("k", (2, 5, 16, 33, 64))
def test_unaligned_entries_and_special_inputs(k):
    """Entries that are rows of one [k, P] array with odd P (4-byte aligned only); a NULL entry; a
    duplicate pointer; one dead entry (NaN, +inf, -inf) with iters in {0, 3}: the redo path and the
    no-op pair; every entry dead."""
    for P in (257, 3 * _tile(k) + 5):
        ent, cnt = G.inputs(k, P)
        rows = _dev(np.stack(ent))
        assert any(r.data_ptr() % 16 for r in rows)
        got, _ = _run(list(rows), cnt, 3, False, P)
        G.stepwise(ent, cnt, 3, G.NU, False, got, ("rows", P))
    P = 257
    ent, cnt = G.inputs(k, P, 3)
    ent[1] = None
    got, _ = _run([_dev(e) for e in ent], cnt, 3, True, P)
    G.stepwise(ent, cnt, 3, G.NU, True, got, "null")
    ent, cnt = G.inputs(k, P, 2)
    dent = [_dev(e) for e in ent]
    dent[1], cnt[1] = dent[0], cnt[0]
    got, _ = _run(dent, cnt, 3, False, P)
    G.stepwise([ent[0], ent[0]] + ent[2:], cnt, 3, G.NU, False, got, "duplicate")
    assert (got[2][:, 0] == got[2][:, 1]).all()
    for bad in (np.nan, np.inf, -np.inf):
        for iters in (0, 3):
            ent, cnt = G.inputs(k, P, 1)
            j = k // 2
            ent[j] = ent[j].copy()
            ent[j][3::7] = bad
            got, dead = _run([_dev(e) for e in ent], cnt, iters, False, P)
            alive = G.stepwise(ent, cnt, iters, G.NU, False, got, (bad, iters))
            g, w, d2, obj = got
            assert list(dead) == [int(i == j) for i in range(k)] and not alive[j]
            assert (w[:, j] == 0).all() and np.isinf(d2[:, j]).all()
            assert np.isfinite(np.delete(w, j, 1)).all() and np.isfinite(g).all()
            assert np.isfinite(obj).all()
    nan = [_dev(np.full(P, np.nan, np.float32)) for _ in range(k)]
    got, dead = _run(nan, [1] * k, 2, False, P)
    assert dead.all() and np.isnan(got[0]).all() and np.isinf(got[2]).all()


def test_duplicates_where_the_floor_acts():
    """P = 1, values [1, 1, 1, 5] and four equal values: distance 0, the nu floor acts."""
    ent = [np.array([v], np.float32) for v in (1, 1, 1, 5)]
    for nu in (1e-6, 2.0):
        got, _ = _run([_dev(e) for e in ent], [1] * 4, 3, False, 1, nu=nu)
        G.stepwise(ent, [1] * 4, 3, nu, False, got, ("dup", nu))
        assert np.array_equal(got[2][0], [1.0, 1.0, 1.0, 9.0]) and got[3][0] == 6.0
    same = [np.array([3.0], np.float32) for _ in range(4)]
    got, _ = _run([_dev(e) for e in same], [1] * 4, 3, False, 1)
    G.stepwise(same, [1] * 4, 3, G.NU, False, got, "all equal")
    assert (got[2] == 0).all() and (got[1] == 0.25).all() and got[0][0] == 3.0


@pytest.mark.parametrize("k", (4, 9, 64))
def test_bits_do_not_depend_on_the_scratch(k):
    """Two runs over scratch poisoned with different patterns: identical w, d2, obj and g bits."""
    P = 3 * _tile(k) + 5
    ent, cnt = G.inputs(k, P)
    dent = [_dev(e) for e in ent]
    a, _ = _run(dent, cnt, 3, True, P, POISONS[0])
    b, _ = _run(dent, cnt, 3, True, P, POISONS[1])
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    assert np.array_equal(G.bits(a[0]), G.bits(b[0]))


def _text_g(ent, cnt, w_final):
    """_wsum(x, w_dev[iters]).float(): the text's g at the device's own final weights."""
    from flsim.robust import _wsum
    x = G.cols_of(ent, cnt).double()
    return _wsum(x, torch.from_numpy(np.ascontiguousarray(w_final))).float().numpy()


@pytest.mark.parametrize("k", (5, 17, 64))
@pytest.mark.parametrize("name", list(KINDS))
def test_update_equals_existing_step_on_the_texts_g(name, k):
    """Two consecutive fused steps (the state carries over; the second step's entries differ)
    against the existing k = 1 step on _wsum(x, w_dev[iters]).float(); arrays a kind does not own
    are passed poisoned to the fused step and stay untouched."""
    from flsim.engine import GeoMed, aggregate_adam_sum, geomed_step
    o = KINDS[name]
    nstate = _n_state(o)
    P = 3 * _tile(k) + 5
    p0, m0, v0 = _state(P, 7 * k)
    a = [_dev(p0), _dev(m0) if nstate >= 1 else _poisoned(P),
         _dev(v0) if nstate >= 2 else _poisoned(P)]
    b = [_dev(p0), _dev(m0) if nstate >= 1 else None, _dev(v0) if nstate >= 2 else None]
    for step in (1, 2):
        ent, cnt = G.inputs(k, P, step)
        gm = GeoMed(3, G.NU, step == 2, [_dev(e) for e in ent], cnt)
        _poison_scratch(gm, P, G.QNAN)
        geomed_step(gm, a[0], a[1], a[2], step, optim=o)
        w, d2, obj, dead = _outputs(gm)
        g = _text_g(ent, cnt, w[-1])
        assert np.isfinite(g).all() and (g != 0).all() and not dead.any()
        aggregate_adam_sum(_dev(g), 1, b[0], b[1], b[2], step, [P], optim=o)
        for x, y, what in zip(a, b, "pmv"):
            if y is None:
                assert int((_bits(x) != G.QNAN).sum()) == 0, (name, what)
                continue
            bad = int((_bits(x) != _bits(y)).sum())
            assert bad == 0, (name, step, what, bad)
    assert not np.array_equal(_bits(a[0]), G.bits(p0))


@pytest.mark.parametrize("name", ["adam", "sgdm"])
def test_clipped_step_equals_existing_clipped_step(name):
    """k = 16, max_norm below and above the norm: total_norm, coef and p / m / v against
    flsim_aggregate_optim_clip_push fed the same g as a k = 1 rule; g_out also receives g; the
    scratch is poisoned first."""
    from flsim.engine import Clip, GeoMed, Rule, aggregate_rule, geomed_step
    k = 16
    P = 3 * _tile(k) + 5
    o = KINDS[name]
    nstate = _n_state(o)
    ent, cnt = G.inputs(k, P)
    dent = [_dev(e) for e in ent]
    got, _ = _run(dent, cnt, 3, False, P)
    g = _text_g(ent, cnt, got[1][-1])
    assert G.g_mismatches(got[0], g) == 0
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
            buf.view(torch.int32).fill_(G.QNAN)
        gout = _poisoned(P)
        gm = GeoMed(3, G.NU, False, dent, cnt)
        _poison_scratch(gm, P, G.QNAN)
        geomed_step(gm, a[0], a[1], a[2], 1, optim=o, clip=ca, g_out=gout)
        aggregate_rule(_dev(g), Rule(1, [], c=1), b[0], b[1], b[2], 1, [P], optim=o, clip=cb)
        assert int((_bits(gout) != G.bits(g)).sum()) == 0
        assert C.bits(ca.total_norm.cpu().numpy()) == C.bits(norm)
        assert C.bits(ca.total_norm.cpu().numpy()) == C.bits(cb.total_norm.cpu().numpy())
        assert C.bits(ca.coef.cpu().numpy()) == C.bits(cb.coef.cpu().numpy())
        assert (float(ca.coef) == 1.0) == (mn > float(norm))
        for x, y, what in zip(a, b, "pmv"):
            if x is not None:
                bad = int((_bits(x) != _bits(y)).sum())
                assert bad == 0, (mn, what, bad)


def test_refusals_on_device_pointers():
    """An entry aliasing p, m, g_out or the scratch, a misaligned p, a null p: ValueError, and
    nothing is launched (p keeps its bits)."""
    from flsim.engine import GeoMed, geomed_step
    P = 1000
    rs = np.random.RandomState(1)
    ent = [_dev(e) for e in G.inputs(5, P)[0]]
    cnt = [1, 2, 3, 4, 1]
    buf = _dev(rs.standard_normal(P + 8).astype(np.float32))
    p, m = buf[:P], _dev(np.zeros(P, np.float32))
    before = buf.clone()
    o = KINDS["sgdm"]

    def gm(entries, iters=3):
        return GeoMed(iters, G.NU, False, entries, cnt)

    for bad in ([ent[0], p] + ent[2:], [buf[4:P + 4]] + ent[1:], ent[:4] + [m]):
        with pytest.raises(ValueError, match="overlaps"):
            geomed_step(gm(bad), p, m, None, 1, optim=o)
    gout = torch.zeros(P, device=DEV)
    with pytest.raises(ValueError, match="overlaps"):
        geomed_step(gm(ent[:4] + [gout]), p, m, None, 1, optim=o, g_out=gout)
    own = gm(ent)
    own.c_scratch(torch.device(DEV), P)
    with pytest.raises(ValueError, match="geometric-median scratch"):
        geomed_step(gm(ent[:4] + [own.partials.view(torch.float32)[:P]]), p, m, None, 1, optim=o)
    for iters, what in ((33, "Invalid iters"), (-1, "Invalid iters")):
        with pytest.raises(ValueError, match=what):
            geomed_step(gm(ent, iters), p, m, None, 1, optim=o)
    with pytest.raises(ValueError, match="16-byte aligned"):
        geomed_step(gm(ent), buf[1:P + 1], m, None, 1, P=P, optim=o)
    with pytest.raises(ValueError, match="null pointer"):
        geomed_step(gm(ent), None, m, None, 1, P=P, optim=o)
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


def test_simulation_geomed(pool):
    """buckets = 6, one slow worker with delay 2, ("geomed", 3): every bucket entry is
    bit-identical to an engine pass over exactly those workers' records; last_geomed's log passes
    the stepwise check on last_entries, and theta after each epoch, the pop epochs included, equals
    torch.optim.SGD on the CPU applied to g = _wsum(x, w_dev[iters]).float()."""
    from flsim.engine import PN1Engine, worker_table
    from flsim.sim import FLSimulation
    sim = FLSimulation(N, device=DEV, chunk_workers=CW, pool=pool, dropout=False,
                       semantics="independent", delay=2, robust_rule=("geomed", 3),
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
        gm = sim.last_geomed
        w, d2, obj, dead = _outputs(gm)
        host = [e.cpu().numpy() for e in ents]
        g = _text_g(host, counts, w[-1])
        assert np.isfinite(g).all() and not dead.any()
        G.stepwise(host, counts, 3, 1e-6, False, (g, w, d2, obj), t)
        o_log, w_log = sim.geomed_log()[-1]
        assert o_log == [float(x) for x in obj] and w_log == [float(x) for x in w[-1]]
        pe = _sgd(g, before.cpu().numpy(), LR)
        bad = int((pe.view(np.uint32) != _bits(sim.theta)).sum())
        assert bad == 0, (t, bad)
    assert pops >= 1
