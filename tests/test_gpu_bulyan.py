"""GPU: the fused Bulyan step (csrc/server.hip: k_krum_dist, k_bulyan_finish, k_bulyan_apply through
flsim_bulyan_optim_step), pinned to the rule text of flsim/robust.py run by torch on the CPU.

  stages       at the device's own outputs, no margin needed: dist within 2 (P + 2) 2^-53 relative of
               the text's, symmetric bit for bit, zero diagonal; order, sel and the winning scores
               (bit for bit) equal bulyan_order(device dist); g bit-equal to _bulyan_coord on the
               device's sel;
  end to end   sel, order and g equal bulyan_flat computed from scratch; the input condition (every
               round's winner bit-equal to a rival or >= 1000 score bounds below it) is asserted
               for every case, never skipped;
  dist         bit-equal to Krum(...).dist on the same inputs;
  update       p / m / v after the fused step against the EXISTING k = 1 step on the text's g, every
               optimizer kind; the clipped step against the existing clipped step;
  sim          FLSimulation(robust_rule=("bulyan", 1)) on PerformantNet1, with and without NNM and
               ALIE, every epoch replayed through bulyan_flat.

The scratch, g_out and every unowned array are poisoned before each run.
"""
import numpy as np
import pytest
import torch

import _bulyan as B
import _clip as C
import _krum as K
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

DEV = "cuda:0"


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
    return (1, 257, _tile(k) + 1, 4099)


def _run(dents, counts, f, P, pat=K.QNAN):
    """One g-only step over poisoned scratch and g_out -> (g, dist, order, win, sel) on the host;
    nothing past P (g), k * k (dist), theta (score, order, sel) is written."""
    from flsim.engine import Bulyan, bulyan_step
    k = len(counts)
    th = k - 2 * f
    bu = Bulyan(f, dents, counts)
    bu.c_scratch(torch.device(DEV), P)
    bufs = Bulyan._scratch[(DEV, P, k)]
    for b in bufs:
        b.view(torch.int32).fill_(pat)
    g = _poisoned(P + 3, pat)
    bulyan_step(bu, None, None, None, 1, P=P, optim=False, g_out=g[:P])
    torch.cuda.synchronize()
    assert int((_bits(g[P:]) != pat).sum()) == 0
    _, dist, score, order, sel = bufs
    assert int((dist[k * k:].view(torch.int32) != pat).sum()) == 0
    assert int((score[th:].view(torch.int32) != pat).sum()) == 0
    assert int((order[th:] != pat).sum()) == 0
    assert int((sel[th:] != pat).sum()) == 0
    return (g[:P].cpu().numpy(), bu.dist.cpu().numpy().copy(),
            [int(j) for j in bu.order.tolist()], bu.score.cpu().numpy().copy(),
            [int(j) for j in bu.sel.tolist()])


_TEXT = {}


def _text(k, P, f, seed=0):
    """The text at the seeded inputs of (k, P), computed once per case and shared."""
    key = (k, P, f, seed)
    if key not in _TEXT:
        ent, cnt = K.inputs(k, P, seed)
        _TEXT[key] = B.text(ent, cnt, f)
    return _TEXT[key]


def _check(got, ref, ent, cnt, f, P, what):
    g, d, order, win, sel = got
    g_t, d_t, o_t, w_t, s_t = ref
    assert K.outside(d, d_t, K.dist_bound(P)) == 0, what
    B.stage_check(got, ent, cnt, f, P, what)                    # the device's own outputs
    assert B.min_round_gap(d_t, f) >= B.gap_bar(P), what        # input condition
    assert order == o_t and sel == s_t, (what, order, o_t)      # end to end
    bad = K.g_mismatches(g, g_t)
    assert bad == 0, (what, bad)


@pytest.mark.parametrize("k", B.KS)
def test_stages_and_end_to_end(k):
    """Every f of the grid at P in {1, 257, E + 1, 4099}, the seed-0 inputs (they meet the input
    condition at every case: the smallest gap of the grid is 6.9e-7 at P = 1, 1.98e-6 at P = 4099,
    against bars of 1.3e-12 and 1.8e-9)."""
    for P in _ps(k):
        ent, cnt = K.inputs(k, P)
        dent = [_dev(e) for e in ent]
        for f in B.fs(k):
            _check(_run(dent, cnt, f, P), _text(k, P, f), ent, cnt, f, P, (P, f))


@pytest.mark.parametrize("k", (3, 9, 33, 64))
def test_dist_is_krums_bit_for_bit(k):
    """P = E + 1 (two tiles, the second of one element) and P = 4099 (several tiles and a tail)."""
    from flsim.engine import Krum, krum_step
    for P in (_tile(k) + 1, 4099):
        ent, cnt = K.inputs(k, P)
        dent = [_dev(e) for e in ent]
        f = B.fs(k)[-1]
        d = _run(dent, cnt, f, P)[1]
        kr = Krum(0, 1, dent, cnt)
        krum_step(kr, None, None, None, 1, P=P, optim=False, g_out=_poisoned(P))
        dk = kr.dist.cpu().numpy()
        assert np.array_equal(d.view(np.uint64), dk.view(np.uint64)), P


@pytest.mark.parametrize("k", (7, 16, 33))
def test_unaligned_entries_and_special_inputs(k):
    """f = 1, P = 257.  Rows of one odd-P array (4-byte aligned only); a NULL entry; a duplicated
    pointer; one entry with NaNs (never selected, g finite and bit-equal); +-inf and +-0 scattered
    in two entries (g equals the text as numbers); all entries NaN."""
    f, P = 1, 257
    ent, cnt = K.inputs(k, P)
    rows = _dev(np.stack(ent))
    assert any(r.data_ptr() % 16 for r in rows)
    _check(_run(list(rows), cnt, f, P), _text(k, P, f), ent, cnt, f, P, "rows")
    ent, cnt = K.inputs(k, P, 3)
    ent[2] = None
    got = _run([_dev(e) for e in ent], cnt, f, P)
    _check(got, B.text(ent, cnt, f), ent, cnt, f, P, "null")
    ent, cnt = K.inputs(k, P, 2)
    dent = [_dev(e) for e in ent]
    dent[1], cnt[1] = dent[0], cnt[0]
    ent[1] = ent[0]
    got = _run(dent, cnt, f, P)
    assert got[1][0, 1] == 0.0 and got[1][1, 0] == 0.0 and (got[1][0, 2:] > 0).all()
    _check(got, B.text(ent, cnt, f), ent, cnt, f, P, "dup")
    off = ~np.eye(k, dtype=bool)
    ent, cnt = K.inputs(k, P, 1)
    j = k // 2
    ent[j] = ent[j].copy()
    ent[j][3::7] = np.nan
    got = _run([_dev(e) for e in ent], cnt, f, P)
    ref = B.text(ent, cnt, f)
    assert j not in got[4] and got[4] == ref[4] and got[2] == ref[2]
    assert np.isinf(got[1][j][off[j]]).all() and got[1][j, j] == 0
    assert K.outside(got[1][off], ref[1][off], K.dist_bound(P)) == 0
    assert np.isfinite(got[0]).all() and K.g_mismatches(got[0], ref[0]) == 0
    B.stage_check(got, ent, cnt, f, P, "nan")
    ent, cnt = K.inputs(k, P, 2)
    rs = np.random.RandomState(k)
    for j in (0, k - 1):
        ent[j] = ent[j].copy()
        idx = rs.permutation(P)[:40]
        ent[j][idx] = rs.choice([np.inf, -np.inf, 0.0, -0.0], 40).astype(np.float32)
    got = _run([_dev(e) for e in ent], cnt, f, P)
    assert got[2] == B.order_of(got[1], f)[0] and got[4] == B.text(ent, cnt, f)[4]
    assert B.g_differs(got[0], B.coord(ent, cnt, got[4], f)) == 0
    # specials in most entries, so that some are selected: the window code on NaN, +-inf, +-0
    ent, cnt = K.inputs(k, P, 4)
    for j in range(k):
        ent[j] = ent[j].copy()
        idx = rs.permutation(P)[:P // 6]
        ent[j][idx] = rs.choice([np.nan, np.inf, -np.inf, 0.0, -0.0], len(idx)).astype(np.float32)
    got = _run([_dev(e) for e in ent], cnt, f, P)
    assert got[2] == B.order_of(got[1], f)[0]
    assert B.g_differs(got[0], B.coord(ent, cnt, got[4], f)) == 0
    nan = [_dev(np.full(P, np.nan, np.float32)) for _ in range(k)]
    g, d, order, win, sel = _run(nan, [1] * k, f, P)
    assert order == list(range(k - 2)) == sel and np.isnan(g).all()
    assert np.isinf(d[off]).all() and np.isinf(win).all()


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


@pytest.mark.parametrize("k", (7, 33))
@pytest.mark.parametrize("name", list(KINDS))
def test_update_equals_existing_step_on_the_texts_g(name, k):
    """Two consecutive fused steps (the state carries over; the second step's entries differ)
    against the existing k = 1 step on the text's g; arrays a kind does not own are passed
    poisoned to the fused step and stay untouched."""
    from flsim.engine import Bulyan, aggregate_adam_sum, bulyan_step
    o = KINDS[name]
    nstate = _n_state(o)
    P = _tile(k) + 1
    f = 1
    p0, m0, v0 = _state(P, 7 * k)
    a = [_dev(p0), _dev(m0) if nstate >= 1 else _poisoned(P),
         _dev(v0) if nstate >= 2 else _poisoned(P)]
    b = [_dev(p0), _dev(m0) if nstate >= 1 else None, _dev(v0) if nstate >= 2 else None]
    for step in (1, 2):
        ent, cnt = K.inputs(k, P, step)
        g, d_t, o_t, w_t, s_t = _text(k, P, f, step)
        assert B.min_round_gap(d_t, f) >= B.gap_bar(P)                   # input condition
        assert np.isfinite(g).all() and (g != 0).all()
        bu = Bulyan(f, [_dev(e) for e in ent], cnt)
        bulyan_step(bu, a[0], a[1], a[2], step, optim=o)
        assert [int(j) for j in bu.sel.tolist()] == s_t
        aggregate_adam_sum(_dev(g), 1, b[0], b[1], b[2], step, [P], optim=o)
        for x, y, what in zip(a, b, "pmv"):
            if y is None:
                assert int((_bits(x) != K.QNAN).sum()) == 0, (name, what)
                continue
            bad = int((_bits(x) != _bits(y)).sum())
            assert bad == 0, (name, step, what, bad)
    assert not np.array_equal(_bits(a[0]), K.bits(p0))


@pytest.mark.parametrize("name", ["adam", "sgdm"])
def test_clipped_step_equals_existing_clipped_step(name):
    """k = 16, f = 2, max_norm below and above the norm: total_norm, coef and p / m / v against
    flsim_aggregate_optim_clip_push fed the text's g as a k = 1 rule; g_out also receives g; the
    clip scratch is poisoned first."""
    from flsim.engine import Bulyan, Clip, Rule, aggregate_rule, bulyan_step
    k, f = 16, 2
    P = _tile(k) + 1
    o = KINDS[name]
    nstate = _n_state(o)
    ent, cnt = K.inputs(k, P)
    dent = [_dev(e) for e in ent]
    g, d_t, o_t, w_t, s_t = _text(k, P, f)
    assert B.min_round_gap(d_t, f) >= B.gap_bar(P)                       # input condition
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
        bu = Bulyan(f, dent, cnt)
        bulyan_step(bu, a[0], a[1], a[2], 1, optim=o, clip=ca, g_out=gout)
        aggregate_rule(_dev(g), Rule(1, [], c=1), b[0], b[1], b[2], 1, [P], optim=o, clip=cb)
        assert [int(j) for j in bu.sel.tolist()] == s_t
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
    """An entry aliasing p, m, g_out or the scratch, f out of range, a misaligned p: ValueError,
    and nothing is launched (p keeps its bits)."""
    from flsim.engine import Bulyan, bulyan_step
    P = 1000
    rs = np.random.RandomState(1)
    ent = [_dev(e) for e in K.inputs(7, P)[0]]
    cnt = [1, 2, 3, 4, 1, 2, 3]
    buf = _dev(rs.standard_normal(P + 8).astype(np.float32))
    p, m = buf[:P], _dev(np.zeros(P, np.float32))
    before = buf.clone()
    o = KINDS["sgdm"]
    for bad in ([ent[0], p] + ent[2:], [buf[4:P + 4]] + ent[1:], ent[:6] + [m]):
        with pytest.raises(ValueError, match="overlaps"):
            bulyan_step(Bulyan(1, bad, cnt), p, m, None, 1, optim=o)
    gout = torch.zeros(P, device=DEV)
    with pytest.raises(ValueError, match="overlaps"):
        bulyan_step(Bulyan(1, ent[:6] + [gout], cnt), p, m, None, 1, optim=o, g_out=gout)
    bu = Bulyan(1, ent, cnt)
    bu.c_scratch(torch.device(DEV), P)
    with pytest.raises(ValueError, match="Bulyan scratch"):
        bulyan_step(Bulyan(1, ent[:6] + [bu.partials.view(torch.float32)[:P]], cnt), p, m, None, 1,
                    optim=o)
    for f in (2, -1):
        with pytest.raises(ValueError, match="Invalid f"):
            bulyan_step(Bulyan(f, ent, cnt), p, m, None, 1, optim=o)
    with pytest.raises(ValueError, match="16-byte aligned"):
        bulyan_step(Bulyan(1, ent, cnt), buf[1:P + 1], m, None, 1, P=P, optim=o)
    with pytest.raises(ValueError, match="null pointer"):
        bulyan_step(Bulyan(1, ent, cnt), None, m, None, 1, P=P, optim=o)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32))


# ---- FLSimulation on PerformantNet1 ----------------------------------------------------------------
N, EPOCHS, LR, CW = 16, 3, 0.01, 4


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


@pytest.mark.parametrize("defended", (False, True))
def test_simulation_bulyan(pool, defended):
    """16 workers, 7 buckets, ("bulyan", 1), a few epochs; `defended`: two ALIE workers and NNM with
    f = 1 in front.  keep_entries replays every epoch through bulyan_flat (over the mixed entries
    with count 1 under NNM): the selection matches and theta equals torch.optim.SGD on the CPU
    applied to the text's g, bit for bit."""
    from flsim.sim import FLSimulation
    kw = dict(attack="alie", n_byz=2, nnm=1) if defended else {}
    sim = FLSimulation(N, device=DEV, chunk_workers=CW, pool=pool, dropout=False,
                       semantics="independent", delay=2, robust_rule=("bulyan", 1), buckets=7,
                       optimizer="sgd", lr=LR, keep_entries=True, **kw)
    for t in range(EPOCHS):
        before = sim.theta.clone()
        sim.epoch()
        ents, counts = sim.last_entries
        if defended:
            ents, counts = sim.last_mixed, [1] * len(ents)
        ents = [e.cpu().numpy() for e in ents]
        assert len(ents) in (7, 8)
        g, d, order, win, sel = B.text(ents, counts, 1)
        assert B.min_round_gap(d, 1) >= B.gap_bar(sim.P), t                # input condition
        assert np.isfinite(g).all()
        assert sim.last_selected == sel, (t, sim.last_selected, sel)
        assert sim.selections()[-1] == sel
        pe = _sgd(g, before.cpu().numpy(), LR)
        bad = int((pe.view(np.uint32) != _bits(sim.theta)).sum())
        assert bad == 0, (t, bad)
