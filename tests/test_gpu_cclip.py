"""GPU: the fused centered-clipping step (csrc/server.hip: k_cclip_dist, k_cclip_finish,
k_cclip_apply through flsim_cclip_optim_step), pinned stage by stage to the rule text of
flsim/robust.py run by torch on the CPU (tests/_cclip.py: the stepwise comparison).

  d2[r]         within 2 (P + 2) 2^-53 relative of the text's distances at the device's own u[r],
                w[r]; s[r], u[r + 1], w[r + 1] and g bit for bit the text's scalar code on the
                device's d2[r]; the center after the step has the bits of g; over KS, P on both
                sides of the kernel's tile E, iters in {1, 3}, both weightings, fresh (the center
                passed poisoned with a signalling NaN: it is not read) and carried;
  determinism   two runs over differently poisoned scratch give identical bits, and nothing past
                the documented extents is written;
  update        p / m / v after two consecutive fused steps (the second around the first's
                aggregate) against the EXISTING k = 1 step on the text's g, every optimizer kind;
  clipped       norm, coefficient and p against flsim_aggregate_optim_clip_push fed the same g;
                the stored center is the unclipped g;
  sim           FLSimulation(robust_rule=("cclip", tau, 2)) on PerformantNet1 against the text on
                last_entries / last_center and torch.optim.SGD on g; composed with an IPM attack.

The scratch, g_out and every unowned array are poisoned before each run.
"""
import numpy as np
import pytest
import torch

import _cclip as C
import _clip as CL
from conftest import has_gpu
from test_gpu_krum import KINDS, _n_state, _state

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

DEV = "cuda:0"
POISONS = (C.QNAN, 0x7F800001)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _poisoned(n, pat=C.QNAN):
    return torch.full((n,), pat, dtype=torch.int32, device=DEV).view(torch.float32)


def _tile(k):
    from flsim._lib import lib
    return int(lib().flsim_cclip_tile_elems(k))


def _ps(k):
    E = _tile(k)
    return (1, 255, 256, 257, E - 1, E, E + 1, 3 * E + 5)


def _poison_scratch(cc, P, pat):
    from flsim.engine import CClip
    cc.c_scratch(torch.device(DEV), P)
    bufs = CClip._scratch[(DEV, P, cc.k, cc.iters)]
    for b in bufs:
        b.view(torch.int32).fill_(pat)
    return bufs


def _outputs(cc):
    """(u, w, d2, s) of the last step as numpy, and the dead flags."""
    return (cc.u.cpu().numpy().copy(), cc.w.cpu().numpy().copy(), cc.d2.cpu().numpy().copy(),
            cc.s.cpu().numpy().copy(), cc.dead.cpu().numpy().copy())


def _center(cen, P):
    """The device center [P] inside a poisoned [P + 3] buffer: a copy of `cen`, or (None: a fresh
    step) the signalling-NaN pattern, which the step must not read."""
    buf = _poisoned(P + 3, C.SNAN)
    if cen is not None:
        buf[:P].copy_(_dev(cen))
    return buf


def _run(dents, counts, cen, tau, iters, weighted, P, pat=C.QNAN):
    """One g-only step over poisoned scratch and g_out -> ((g, u, w, d2, s), dead, the center's
    bits after the step) on the host; nothing past P (g, center), iters + 1 (u), (iters + 1) k (w),
    iters k (d2, s), k + 4 (state) is written."""
    from flsim.engine import CClip, cclip_step
    k = len(counts)
    cbuf = _center(cen, P)
    cc = CClip(tau, iters, weighted, dents, counts, cbuf[:P], fresh=cen is None)
    _, ub, wb, d2b, sb, stb = _poison_scratch(cc, P, pat)
    g = _poisoned(P + 3, pat)
    cclip_step(cc, None, None, None, 1, P=P, optim=False, g_out=g[:P])
    torch.cuda.synchronize()
    assert int((_bits(g[P:]) != pat).sum()) == 0
    assert int((_bits(cbuf[P:]) != C.SNAN).sum()) == 0
    assert int((ub[iters + 1:].view(torch.int32) != pat).sum()) == 0
    assert int((wb[(iters + 1) * k:].view(torch.int32) != pat).sum()) == 0
    assert int((d2b[iters * k:].view(torch.int32) != pat).sum()) == 0
    assert int((sb[iters * k:].view(torch.int32) != pat).sum()) == 0
    assert int((stb[k + 4:] != pat).sum()) == 0
    u, w, d2, s, dead = _outputs(cc)
    return (g[:P].cpu().numpy(), u, w, d2, s), dead, _bits(cbuf[:P]).copy()


def _check(ent, cnt, cen, tau, iters, weighted, dent, P, what, pat=C.QNAN):
    got, dead, cbits = _run(dent, cnt, cen, tau, iters, weighted, P, pat)
    alive, g_t = C.stepwise(ent, cnt, cen, tau, iters, weighted, got, what)
    assert np.array_equal(cbits, C.bits(got[0])), (what, "center")
    assert list(dead) == [int(not a) for a in alive], (what, "dead")
    return got, dead, g_t


@pytest.mark.parametrize("k", C.KS)
def test_stepwise_against_the_text(k):
    """KS x P in {1, 255, 256, 257, E - 1, E, E + 1, 3E + 5} x iters in {1, 3} x both weightings x
    fresh (poisoned center) / carried center."""
    clipped = set()
    for P in _ps(k):
        ent, cnt = C.inputs(k, P)
        dent = [_dev(e) for e in ent]
        for fresh in (True, False):
            cen = None if fresh else C.center(P)
            tau = C.pick_tau(ent, cnt, cen)
            for iters in (1, 3):
                for weighted in (False, True):
                    got, dead, _ = _check(ent, cnt, cen, tau, iters, weighted, dent, P,
                                          (k, P, iters, weighted, fresh))
                    assert not dead.any()
                    clipped |= set((got[4] < 1).reshape(-1).tolist())
    assert clipped == {True, False}


@pytest.mark.parametrize("k", (4, 64))
def test_a_block_runs_several_tiles(k):
    """A P with more tiles than the grid has blocks (some block grid-strides over two), the last
    tile partial; k = 4 and k = 64 differ in the grid's cap and in the tile."""
    from flsim._lib import lib
    E = _tile(k)
    one_each = 1
    while lib().flsim_cclip_partials((one_each + 1) * E, k) > \
            lib().flsim_cclip_partials(one_each * E, k):
        one_each *= 2                       # (doubling: the grid's cap is found in a few calls)
    P = one_each * E + 3 * E + 5
    assert lib().flsim_cclip_partials(P, k) == lib().flsim_cclip_partials(one_each * E, k)
    ent, cnt = C.inputs(k, P)
    dent = [_dev(e) for e in ent]
    for cen in (None, C.center(P)):
        tau = C.pick_tau(ent, cnt, cen)
        _check(ent, cnt, cen, tau, 2, True, dent, P, (k, P, cen is None))


@pytest.mark.parametrize("k", (2, 5, 16, 33, 64))
def test_unaligned_entries_and_special_inputs(k):
    """Entries that are rows of one [k, P] array with odd P (4-byte aligned only); a NULL entry; a
    duplicate pointer; one dead entry (NaN, +inf, -inf): no redo, the flags set, s = 0, w = 0 and g
    finite; every entry dead: g is the center (fresh: zero) and u stays 1."""
    for P in (257, 3 * _tile(k) + 5):
        ent, cnt = C.inputs(k, P)
        rows = _dev(np.stack(ent))
        assert any(r.data_ptr() % 16 for r in rows)
        cen = C.center(P)
        _check(ent, cnt, cen, C.pick_tau(ent, cnt, cen), 3, False, list(rows), P, ("rows", P))
    P = 257
    cen = C.center(P, 1)
    ent, cnt = C.inputs(k, P, 3)
    ent[1] = None
    _check(ent, cnt, cen, C.pick_tau(ent, cnt, cen), 3, True, [_dev(e) for e in ent], P, "null")
    ent, cnt = C.inputs(k, P, 2)
    dent = [_dev(e) for e in ent]
    dent[1], cnt[1] = dent[0], cnt[0]
    dup = [ent[0], ent[0]] + ent[2:]
    got, _, _ = _check(dup, cnt, None, C.pick_tau(dup, cnt, None), 3, False, dent, P, "duplicate")
    assert (got[3][:, 0] == got[3][:, 1]).all()
    for bad in (np.nan, np.inf, -np.inf):
        for c in (None, cen):
            ent, cnt = C.inputs(k, P, 1)
            j = k // 2
            ent[j] = ent[j].copy()
            ent[j][3::7] = bad
            tau = C.pick_tau(ent, cnt, c)
            got, dead, _ = _check(ent, cnt, c, tau, 3, False, [_dev(e) for e in ent], P,
                                  (bad, c is None))
            g, u, w, d2, s = got
            assert list(dead) == [int(i == j) for i in range(k)]
            assert (w[:, j] == 0).all() and (s[:, j] == 0).all() and np.isinf(d2[:, j]).all()
            assert np.isfinite(np.delete(w, j, 1)).all() and np.isfinite(g).all()
            assert np.isfinite(u).all()
    nan = [np.full(P, np.nan, np.float32) for _ in range(k)]
    dnan = [_dev(e) for e in nan]
    for c in (None, cen):
        got, dead, _ = _check(nan, [1] * k, c, 1.0, 2, False, dnan, P, ("all dead", c is None))
        g, u, w, d2, s = got
        assert dead.all() and (u == 1).all() and (w == 0).all() and (s == 0).all()
        assert np.array_equal(C.bits(g), C.bits(np.zeros(P, np.float32) if c is None else c))


def test_nan_center_and_zero_distance():
    """A NaN in the carried center: g and the next center are all NaN.  An entry sitting on the
    center: d = 0, s = 1."""
    P, k = 257, 5
    ent, cnt = C.inputs(k, P)
    dent = [_dev(e) for e in ent]
    cen = C.center(P)
    cen[5] = np.nan
    got, _, cbits = _check(ent, cnt, cen, 1.0, 3, False, dent, P, "nan center")
    assert np.isnan(got[0]).all() and np.isnan(cbits.view(np.float32)).all()
    cen = C.center(P)
    ent[2], cnt[2] = cen.copy(), 1
    got, _, _ = _check(ent, cnt, cen, 1e-3, 1, False, [_dev(e) for e in ent], P, "d = 0")
    assert got[3][0, 2] == 0 and got[4][0, 2] == 1 and (np.delete(got[4][0], 2) < 1).all()


@pytest.mark.parametrize("k", (4, 9, 64))
def test_bits_do_not_depend_on_the_scratch(k):
    """Two runs over scratch poisoned with different patterns: identical u, w, d2, s, g and center
    bits (the extents are checked by every run)."""
    P = 3 * _tile(k) + 5
    ent, cnt = C.inputs(k, P)
    dent = [_dev(e) for e in ent]
    for cen in (None, C.center(P)):
        tau = C.pick_tau(ent, cnt, cen)
        a, _, ca = _run(dent, cnt, cen, tau, 3, True, P, POISONS[0])
        b, _, cb = _run(dent, cnt, cen, tau, 3, True, P, POISONS[1])
        for x, y in zip(a[1:], b[1:]):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
        assert np.array_equal(C.bits(a[0]), C.bits(b[0])) and np.array_equal(ca, cb)


def _text_g(ent, cnt, cen, u_final, w_final):
    """The text's g at the device's own final weights."""
    from flsim.robust import _cclip_z
    x = C.cols_of(ent, cnt).double()
    c = None if cen is None else torch.from_numpy(np.ascontiguousarray(cen, np.float32)).double()
    return _cclip_z(x, c, torch.tensor(float(u_final), dtype=torch.float64),
                    torch.from_numpy(np.ascontiguousarray(w_final))).float().numpy()


@pytest.mark.parametrize("k", (5, 17, 64))
@pytest.mark.parametrize("name", list(KINDS))
def test_update_equals_existing_step_on_the_texts_g(name, k):
    """Two consecutive fused steps (the state carries over; the second runs non-fresh on the
    first's center and on other entries) against the existing k = 1 step on the text's g; arrays
    a kind does not own are passed poisoned to the fused step and stay untouched."""
    from flsim.engine import CClip, aggregate_adam_sum, cclip_step
    o = KINDS[name]
    nstate = _n_state(o)
    P = 3 * _tile(k) + 5
    p0, m0, v0 = _state(P, 7 * k)
    a = [_dev(p0), _dev(m0) if nstate >= 1 else _poisoned(P),
         _dev(v0) if nstate >= 2 else _poisoned(P)]
    b = [_dev(p0), _dev(m0) if nstate >= 1 else None, _dev(v0) if nstate >= 2 else None]
    center = _poisoned(P, C.SNAN)
    cen = None
    for step in (1, 2):
        ent, cnt = C.inputs(k, P, step)
        tau = C.pick_tau(ent, cnt, cen)
        cc = CClip(tau, 2, step == 2, [_dev(e) for e in ent], cnt, center, fresh=step == 1)
        _poison_scratch(cc, P, C.QNAN)
        cclip_step(cc, a[0], a[1], a[2], step, optim=o)
        u, w, d2, s, dead = _outputs(cc)
        g = _text_g(ent, cnt, cen, u[-1], w[-1])
        assert np.isfinite(g).all() and (g != 0).all() and not dead.any()
        assert int((_bits(center) != C.bits(g)).sum()) == 0, (name, step, "center")
        cen = g
        aggregate_adam_sum(_dev(g), 1, b[0], b[1], b[2], step, [P], optim=o)
        for x, y, what in zip(a, b, "pmv"):
            if y is None:
                assert int((_bits(x) != C.QNAN).sum()) == 0, (name, what)
                continue
            bad = int((_bits(x) != _bits(y)).sum())
            assert bad == 0, (name, step, what, bad)
    assert not np.array_equal(_bits(a[0]), C.bits(p0))


@pytest.mark.parametrize("name", ["adam", "sgdm"])
def test_clipped_step_equals_existing_clipped_step(name):
    """k = 16, max_norm below and above the norm: total_norm, coef and p / m / v against
    flsim_aggregate_optim_clip_push fed the same g as a k = 1 rule; g_out and the center receive
    the unclipped g; the scratch is poisoned first."""
    from flsim.engine import CClip, Clip, Rule, aggregate_rule, cclip_step
    k = 16
    P = 3 * _tile(k) + 5
    o = KINDS[name]
    nstate = _n_state(o)
    ent, cnt = C.inputs(k, P)
    dent = [_dev(e) for e in ent]
    cen = C.center(P)
    tau = C.pick_tau(ent, cnt, cen)
    got, _, g = _check(ent, cnt, cen, tau, 3, False, dent, P, "clip")
    assert np.isfinite(g).all() and (g != 0).all()
    exact, norm, dist = CL.exact_norm(g)
    assert dist >= CL.MIN_MIDPOINT_DISTANCE
    for mn in (0.5 * float(norm), 2.0 * float(norm)):
        p0, m0, v0 = _state(P, 11)
        a = [_dev(p0), _dev(m0), _dev(v0) if nstate >= 2 else None]
        b = [_dev(p0), _dev(m0), _dev(v0) if nstate >= 2 else None]
        ca, cb = Clip(mn), Clip(mn)
        ca.c_struct(torch.device(DEV), P)
        for buf in ca._scratch[(DEV, P)]:
            buf.view(torch.int32).fill_(C.QNAN)
        gout = _poisoned(P)
        center = _dev(cen)
        cc = CClip(tau, 3, False, dent, cnt, center)
        _poison_scratch(cc, P, C.QNAN)
        cclip_step(cc, a[0], a[1], a[2], 1, optim=o, clip=ca, g_out=gout)
        aggregate_rule(_dev(g), Rule(1, [], c=1), b[0], b[1], b[2], 1, [P], optim=o, clip=cb)
        assert int((_bits(gout) != C.bits(g)).sum()) == 0
        assert int((_bits(center) != C.bits(g)).sum()) == 0          # the unclipped g
        assert CL.bits(ca.total_norm.cpu().numpy()) == CL.bits(norm)
        assert CL.bits(ca.total_norm.cpu().numpy()) == CL.bits(cb.total_norm.cpu().numpy())
        assert CL.bits(ca.coef.cpu().numpy()) == CL.bits(cb.coef.cpu().numpy())
        assert (float(ca.coef) == 1.0) == (mn > float(norm))
        for x, y, what in zip(a, b, "pmv"):
            if x is not None:
                bad = int((_bits(x) != _bits(y)).sum())
                assert bad == 0, (mn, what, bad)


def test_refusals_on_device_pointers():
    """The center aliasing p, m, g_out, an entry or the scratch; an entry aliasing p; a misaligned
    or missing center; a misaligned p: ValueError, and nothing is launched (p and the center keep
    their bits)."""
    from flsim.engine import CClip, cclip_step
    P = 1000
    rs = np.random.RandomState(1)
    ent = [_dev(e) for e in C.inputs(5, P)[0]]
    cnt = [1, 2, 3, 4, 1]
    buf = _dev(rs.standard_normal(P + 8).astype(np.float32))
    cbuf = _dev(rs.standard_normal(P + 8).astype(np.float32))
    p, m, cen = buf[:P], _dev(np.zeros(P, np.float32)), cbuf[:P]
    before, cbefore = buf.clone(), cbuf.clone()
    o = KINDS["sgdm"]

    def cc(entries=ent, center=cen, iters=3, tau=1.0, fresh=False):
        return CClip(tau, iters, False, entries, cnt, center, fresh=fresh)

    for bad in (p, buf[4:P + 4], m):
        with pytest.raises(ValueError, match="center overlaps p/m/v/g_out"):
            cclip_step(cc(center=bad), p, m, None, 1, P=P, optim=o)
    gout = torch.zeros(P, device=DEV)
    with pytest.raises(ValueError, match="center overlaps p/m/v/g_out"):
        cclip_step(cc(center=gout), p, m, None, 1, optim=o, g_out=gout)
    for fresh in (False, True):
        with pytest.raises(ValueError, match="overlaps the centered-clipping center"):
            cclip_step(cc(ent[:4] + [cen], fresh=fresh), p, m, None, 1, optim=o)
        with pytest.raises(ValueError, match="overlaps the centered-clipping center"):
            cclip_step(cc([cbuf[4:P + 4]] + ent[1:], fresh=fresh), p, m, None, 1, optim=o)
    own = cc()
    own.c_scratch(torch.device(DEV), P)
    with pytest.raises(ValueError, match="center overlaps the centered-clipping scratch"):
        cclip_step(cc(center=own.partials.view(torch.float32)[:P]), p, m, None, 1, optim=o)
    with pytest.raises(ValueError, match="overlaps p/m/v/g_out"):
        cclip_step(cc([ent[0], p] + ent[2:]), p, m, None, 1, optim=o)
    with pytest.raises(ValueError, match="centered-clipping scratch"):
        cclip_step(cc(ent[:4] + [own.partials.view(torch.float32)[:P]]), p, m, None, 1, optim=o)
    with pytest.raises(ValueError, match="center must be 16-byte aligned"):
        cclip_step(cc(center=cbuf[1:P + 1]), p, m, None, 1, optim=o)
    with pytest.raises(ValueError, match="null centered-clipping center"):
        cclip_step(cc(center=None, fresh=True), p, m, None, 1, optim=o)
    for kw, what in ((dict(iters=33), "Invalid iters"), (dict(iters=0), "Invalid iters"),
                     (dict(tau=0.0), "Invalid tau"), (dict(tau=float("inf")), "Invalid tau")):
        with pytest.raises(ValueError, match=what):
            cclip_step(cc(**kw), p, m, None, 1, optim=o)
    with pytest.raises(ValueError, match="16-byte aligned"):
        cclip_step(cc(), buf[1:P + 1], m, None, 1, P=P, optim=o)
    with pytest.raises(ValueError, match="null pointer"):
        cclip_step(cc(), None, m, None, 1, P=P, optim=o)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32))
    assert torch.equal(cbuf.view(torch.int32), cbefore.view(torch.int32))


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


def _sim(pool, tau, **kw):
    from flsim.sim import FLSimulation
    return FLSimulation(N, device=DEV, chunk_workers=CW, pool=pool, dropout=False,
                        semantics="independent", delay=2, robust_rule=("cclip", tau, 2),
                        buckets=6, optimizer="sgd", lr=LR, keep_entries=True, **kw)


def _epoch_checks(sim, tau, t, prev_g):
    """One epoch of `sim`, checked against the text on last_entries / last_center; returns
    (the text's g at the device's weights, the epoch's s as numpy, whether an entry popped)."""
    before = sim.theta.clone()
    sim.epoch()
    ents, counts = sim.last_entries
    cc = sim.last_cclip
    u, w, d2, s, dead = _outputs(cc)
    assert (sim.last_center is None) == (t == 0) and cc.fresh == (t == 0)   # epoch 0 ran fresh
    cen = None if sim.last_center is None else sim.last_center.cpu().numpy()
    if t:       # the center of epoch t + 1 has the bits of epoch t's g
        assert np.array_equal(C.bits(cen), C.bits(prev_g)), t
    host = [e.cpu().numpy() for e in ents]
    g = _text_g(host, counts, cen, u[-1], w[-1])
    assert np.isfinite(g).all() and not dead.any()
    C.stepwise(host, counts, cen, tau, 2, False, (g, u, w, d2, s), t)
    assert int((_bits(sim.center) != C.bits(g)).sum()) == 0, t
    ul, wl, nl = sim.cclip_log()[-1]
    assert ul == float(u[-1]) and wl == [float(x) for x in w[-1]] and nl == int((s[-1] < 1).sum())
    pe = _sgd(g, before.cpu().numpy(), LR)
    bad = int((pe.view(np.uint32) != _bits(sim.theta)).sum())
    assert bad == 0, (t, bad)
    return g, s, bool(sim.trace[-1].stale)


def test_simulation_cclip(pool):
    """buckets = 6, one slow worker with delay 2, ("cclip", tau, 2), tau from a dry first epoch's
    distances: per epoch the stepwise check on last_entries with last_center, the center carried
    bit for bit, theta equal to torch.optim.SGD on the CPU applied to g, cclip_log() equal to the
    device values; at least one pop epoch.  Then a short run under an IPM attack: the entries and
    counts after the attack feed the rule."""
    dry = _sim(pool, 1.0)
    dry.epoch()
    ents, counts = dry.last_entries
    tau = C.pick_tau([e.cpu().numpy() for e in ents], counts, None)
    sim = _sim(pool, tau)
    pops, g, clipped = 0, None, set()
    for t in range(EPOCHS):
        g, s, pop = _epoch_checks(sim, tau, t, g)
        pops += pop
        clipped |= set((s < 1).reshape(-1).tolist())
    assert pops >= 1 and clipped == {True, False}
    assert len(sim.cclip_log()) == EPOCHS
    att = _sim(pool, tau, attack=("ipm", 4), n_byz=3)
    g = None
    for t in range(2):
        g, s, _ = _epoch_checks(att, tau, t, g)
        _, counts = att.last_entries
        _, honest, byz = att.last_attack
        assert sum(byz) == 3 and counts[:len(byz)] == [h + b for h, b in zip(honest, byz)]
    assert [e[0] for e in att.attack_log()] == ["ipm", "ipm"]
