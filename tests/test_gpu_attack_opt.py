"""GPU: the optimised attacks Min-Max and Min-Sum (csrc/server.hip: k_attack_opt_stats, the
pairwise-distance stage, k_attack_opt_finish and k_attack's mix through flsim_attack_opt_entries)
against the text of flsim/robust.py run by torch on the CPU, by the stage-by-stage yardstick of
tests/_attack_opt.py: dist, a_i and q within 2 (P + 2) 2^-53 relative, c_i within that times
sqrt(a_i q) absolute, gamma bit for bit opt_gamma of the device's own sums, b and the entries
equal as numbers to the text evaluated with the device's gamma.

  kernels       both kinds x three directions at k on both sides of every KPAD (of the mix: k; of
                the stats launch: the honest entries, also with every entry honest), P in {1, 2,
                257, E - 1, E, E + 1} for the mix launch's tile E; nothing past P is written;
  several tiles a P with more tiles than either streaming launch has blocks;
  poison        the write-only entries, b_out and the scratch start from two patterns: same bits;
  sub-views     entries at 16-byte-aligned offsets inside one larger buffer: the guards keep
                their bits;
  NaN and inf   propagate as in the text;
  refusals      on device pointers: nothing is launched;
  sim           FLSimulation on PerformantNet1 under minmax x {krum, geomed}, compared with the
                text through keep_entries.
"""
import math

import numpy as np
import pytest
import torch

import _attack as A
import _attack_opt as AO
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

DEV = "cuda:0"
KS = (1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)       # both sides of every KPAD
CASES = [(kind, dirn) for kind in AO.KINDS for dirn in AO.DIRS]
POISONS = (A.QNAN, 0x7F800001)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _poisoned(n, pat=A.QNAN):
    return torch.full((n,), pat, dtype=torch.int32, device=DEV).view(torch.float32)


def _tiles(k, kh):
    from flsim._lib import lib
    return int(lib().flsim_attack_tile_elems(k)), int(lib().flsim_attack_opt_tile_elems(kh))


def _poison_scratch(pat):
    """Every cached scratch buffer of the class takes the pattern (both 32-bit halves)."""
    from flsim.engine import OptAttack
    for bufs in OptAttack._scratch.values():
        for t in bufs:
            t.view(torch.int32).fill_(pat)


def _run(ents, honest, byz, kind, dirn, strength, pat=A.QNAN, b_out=True):
    """The four launches over device copies of the entries (the never-read ones, b_out and the
    scratch start from `pat`) -> a host_twin-style dict; nothing past P is written to b_out."""
    from flsim.engine import OptAttack, opt_attack_entries
    P = len(ents[0])
    dents = [_dev(e) if h else _poisoned(P, pat) for e, h in zip(ents, honest)]
    b = _poisoned(P + 3, pat) if b_out else None
    at = OptAttack(kind, dirn, strength, dents, honest, byz)
    at.c_scratch(DEV, P)
    _poison_scratch(pat)
    opt_attack_entries(at, None if b is None else b[:P], P)
    torch.cuda.synchronize()
    if b is not None:
        assert int((_bits(b[P:]) != pat).sum()) == 0
    return dict(entries=[d.cpu().numpy() for d in dents],
                b=None if b is None else b[:P].cpu().numpy(), gamma=float(at.gamma.cpu()[0]),
                a=at.stats_a.cpu().numpy(), c=at.stats_c.cpu().numpy(),
                q=float(at.stats_q.cpu()[0]), dist=at.dist.cpu().numpy())


@pytest.mark.parametrize("k", KS)
def test_kernels_against_the_text(k):
    """Every (kind, direction) at some P of the list, every P under two of them; both input
    variants (three categories of entries; every entry honest)."""
    E = _tiles(k, k)[0]
    Ps = (1, 2, 257, E - 1, E, E + 1)
    n = 0
    for i, P in enumerate(Ps):
        for full in (False, True):
            ents, honest, byz = AO.inputs(k, P, full=full)
            if k >= 3 and not full:
                assert {(h > 0, c > 0) for h, c in zip(honest, byz)} == \
                    {(True, True), (True, False), (False, True)}
            kind, dirn = CASES[(i + 3 * full) % 6]
            got = _run(ents, honest, byz, kind, dirn, 1.0)
            ref = AO.check_stages(got, ents, honest, byz, kind, dirn, 1.0, (k, P, full))
            assert np.isfinite(ref["b"]).all() and math.isfinite(got["gamma"])
            assert k == 1 or sum(h > 0 for h in honest) == 1 or got["gamma"] > 0
            n += 1
    assert n == 12


@pytest.mark.parametrize("kind,dirn", CASES)
def test_every_kind_and_direction_at_one_shape(kind, dirn):
    """k = 9 (KPAD 16 for the mix, 8 for the stats launch over six honest entries), a P of three
    tiles and a part, strength 0.75."""
    P = 3 * _tiles(9, 6)[0] + 5
    ents, honest, byz = AO.inputs(9, P)
    assert sum(h > 0 for h in honest) == 6
    got = _run(ents, honest, byz, kind, dirn, 0.75)
    AO.check_stages(got, ents, honest, byz, kind, dirn, 0.75, (kind, dirn))
    assert got["gamma"] > 0


@pytest.mark.parametrize("k,kind,dirn", ((4, "minmax", "std"), (64, "minsum", "unit")))
def test_a_block_runs_several_tiles(k, kind, dirn):
    """More tiles than the grid's cap of either streaming launch (2048 blocks at KPAD 4, 512 at
    64), the last one partial: some blocks take two tiles."""
    cap = 2048 if k == 4 else 512
    P = (cap + 3) * max(_tiles(k, k)) + 5
    ents, honest, byz = AO.inputs(k, P, full=True)
    got = _run(ents, honest, byz, kind, dirn, 1.0)
    AO.check_stages(got, ents, honest, byz, kind, dirn, 1.0, (k, P))


@pytest.mark.parametrize("k", (3, 9, 64))
def test_bits_do_not_depend_on_what_is_never_read(k):
    """Two runs whose write-only entries, b_out and scratch start from different patterns, and a
    third without b_out: identical bits in every output."""
    P = 3 * _tiles(k, k)[0] + 5
    ents, honest, byz = AO.inputs(k, P)
    kind, dirn = CASES[k % 6]
    a = _run(ents, honest, byz, kind, dirn, 1.0, POISONS[0])
    for pat, with_b in ((POISONS[0], True), (POISONS[1], True), (POISONS[1], False)):
        c = _run(ents, honest, byz, kind, dirn, 1.0, pat, with_b)
        for key in ("gamma", "q"):
            assert AO.same_f64(a[key], c[key]), key
        for key in ("a", "c", "dist"):
            assert np.array_equal(a[key].view(np.uint64), c[key].view(np.uint64)), key
        if with_b:
            assert np.array_equal(A.bits(a["b"]), A.bits(c["b"]))
        for x, y in zip(a["entries"], c["entries"]):
            assert np.array_equal(A.bits(x), A.bits(y))


def test_sub_views_of_a_larger_buffer():
    """k = 9 entries and b_out as views at 16-byte-aligned offsets (not 256-byte aligned) inside
    one poisoned buffer, four guard words after each: the guards keep their bits."""
    from flsim.engine import OptAttack, opt_attack_entries
    k, P = 9, 2 * _tiles(9, 6)[0] + 37
    ents, honest, byz = AO.inputs(k, P)
    stride = (P + 4 + 3) // 4 * 4
    buf = _poisoned(4 + (k + 1) * stride)
    views = [buf[4 + j * stride:4 + j * stride + P] for j in range(k + 1)]
    assert all(v.data_ptr() % 16 == 0 for v in views) and any(v.data_ptr() % 256 for v in views)
    for v, e, h in zip(views, ents, honest):
        if h:
            v.copy_(_dev(e))
    at = OptAttack("minmax", "std", 1.0, views[:k], honest, byz)
    opt_attack_entries(at, views[k], P)
    torch.cuda.synchronize()
    got = dict(entries=[v.cpu().numpy() for v in views[:k]], b=views[k].cpu().numpy(),
               gamma=float(at.gamma.cpu()[0]), a=at.stats_a.cpu().numpy(),
               c=at.stats_c.cpu().numpy(), q=float(at.stats_q.cpu()[0]), dist=at.dist.cpu().numpy())
    AO.check_stages(got, ents, honest, byz, "minmax", "std", 1.0, "views")
    guard = torch.ones(buf.numel(), dtype=torch.bool, device=DEV)
    for j in range(k + 1):
        guard[4 + j * stride:4 + j * stride + P] = False
    assert int(guard.sum()) >= 4 * (k + 1)
    assert int((buf.view(torch.int32)[guard] != A.QNAN).sum()) == 0


def test_nan_and_inf_propagate_as_in_the_text():
    for i, bad in enumerate((np.nan, np.inf, -np.inf)):
        for kind, dirn in (CASES[i], CASES[i + 3]):
            ents, honest, byz = AO.inputs(8, 1027, 1)
            j = next(i for i, h in enumerate(honest) if h and not byz[i])
            ents[j] = ents[j].copy()
            ents[j][3::7] = bad
            got = _run(ents, honest, byz, kind, dirn, 1.0)
            ref = AO.check_stages(got, ents, honest, byz, kind, dirn, 1.0, bad)
            assert math.isnan(ref["gamma"]) and math.isnan(got["gamma"])
            assert np.isnan(got["b"]).all()


def test_one_honest_entry_and_a_zero_direction():
    e = (np.random.RandomState(5).standard_normal(1027) * 3).astype(np.float32)
    ents, honest, byz = [e, A.poisoned(1027)], [3, 0], [2, 1]
    got = _run(ents, honest, byz, "minmax", "std", 7.0)
    AO.check_stages(got, ents, honest, byz, "minmax", "std", 7.0, "kh = 1")
    assert got["gamma"] == 0.0 and got["dist"].shape == (1, 1)
    z = np.zeros(1027, np.float32)
    ents, honest, byz = [z, z.copy(), z.copy(), A.poisoned(1027)], [1, 1, 1, 0], [0, 1, 0, 2]
    got = _run(ents, honest, byz, "minsum", "sign", 1.0)
    AO.check_stages(got, ents, honest, byz, "minsum", "sign", 1.0, "q = 0")
    assert got["q"] == 0 and got["gamma"] == 0.0 and (got["b"] == 0).all()


def test_refusals_on_device_pointers():
    """Overlapping entries, an entry overlapping b_out or the scratch, a misaligned entry, a
    missing honest entry, an unknown direction: ValueError, and nothing is launched (the buffer
    keeps its bits)."""
    import ctypes
    from flsim._lib import check, lib, ptr, stream_ptr
    from flsim.engine import OptAttack, opt_attack_entries
    P = 1000
    buf = _dev(np.random.RandomState(1).standard_normal(4 * P + 8).astype(np.float32))
    before = buf.clone()
    e = [buf[j * P:(j + 1) * P] for j in range(3)]

    def at(ents=e, honest=(1, 1, 0), byz=(0, 1, 1), kind="minmax", dirn="std", s=1.0):
        return OptAttack(kind, dirn, s, ents, honest, byz)
    with pytest.raises(ValueError, match="entries 0 and 1 overlap"):
        opt_attack_entries(at([e[0], buf[P - 4:2 * P - 4], e[2]]), None, P)
    with pytest.raises(ValueError, match="overlaps b_out"):
        opt_attack_entries(at(), buf[2 * P + 4:3 * P + 4], P)
    with pytest.raises(ValueError, match="16-byte aligned"):
        opt_attack_entries(at([e[0], e[1], buf[2 * P + 1:3 * P + 1]]), None, P)
    with pytest.raises(ValueError, match="nothing to observe"):
        opt_attack_entries(at(honest=(0, 0, 0), byz=(1, 1, 1)), None, P)
    with pytest.raises(ValueError, match="attack strength"):
        opt_attack_entries(at(s=-1.0), None, P)
    with pytest.raises(ValueError, match="attack direction"):
        opt_attack_entries(at(dirn="l2"), None, P)
    with pytest.raises(ValueError, match="attack kind"):
        opt_attack_entries(at(kind="alie"), None, P)
    # the scratch: gamma inside an entry, and partials too small
    a = at()
    s = a.c_scratch(DEV, P)
    s.gamma = e[1].data_ptr()
    with pytest.raises(ValueError, match="entry 1 overlaps the attack scratch"):
        check(lib().flsim_attack_opt_entries(ctypes.byref(a.c_struct()), ctypes.byref(s),
                                             ptr(None), P, stream_ptr()))
    s = a.c_scratch(DEV, P)
    s.n_partials = 4
    with pytest.raises(ValueError, match="n_partials = 4"):
        check(lib().flsim_attack_opt_entries(ctypes.byref(a.c_struct()), ctypes.byref(s),
                                             ptr(None), P, stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32))


# ---- FLSimulation on PerformantNet1 (tests/test_gpu_attack.py's sizes) -------------------------------
N, EPOCHS, LR, CW, B = 12, 3, 0.01, 4, 4   # (the slow worker's first entry pops in the third epoch)


@pytest.fixture(scope="module")
def pool():
    from oracle import oracle as O
    return O.make_pool(0)


@pytest.mark.parametrize("rule,dirn", ((("krum", 0), "std"), (("geomed", 3), "unit")))
def test_simulation_under_minmax(pool, rule, dirn):
    """n = 12, delay 2, 4 buckets, 3 Byzantine workers spread over the 11 fast ones.  Through
    keep_entries: the solve (last_attack_opt) and the attacked entries (last_entries) against the
    text over the honest sums (last_honest) by the stage-by-stage yardstick; theta equals the
    existing rule's step run by hand on last_entries; attack_gamma_log() holds the same gamma."""
    from flsim.engine import GeoMed, Krum, geomed_step, krum_step
    from flsim.sim import FLSimulation
    sim = FLSimulation(N, device=DEV, chunk_workers=CW, pool=pool, dropout=False,
                       semantics="independent", delay=2, robust_rule=rule, buckets=B,
                       optimizer="sgd", lr=LR, keep_entries=True, attack=("minmax", dirn),
                       n_byz=3)
    assert sim.attack == ("minmax", dirn, 1.0)
    pops = 0
    for t in range(EPOCHS):
        before = sim.theta.clone()
        sim.epoch()
        plan = sim.trace[-1]
        ents, counts = sim.last_entries
        b, honest, byz = sim.last_attack
        assert sum(byz) == 3 and len(ents) == B + bool(plan.stale) and min(honest) >= 1
        pops += bool(plan.stale)
        assert sim.attack_log()[-1] == ("minmax", 1.0, 3)
        gamma, a, c, q, dist = (x.cpu() for x in sim.last_attack_opt)
        assert torch.equal(sim.attack_gamma_log()[-1].cpu(), gamma) and float(gamma) > 0
        sums = [h.cpu().numpy() for h in sim.last_honest]
        got = dict(entries=[e.cpu().numpy() for e in ents[:B]], b=b.cpu().numpy(),
                   gamma=float(gamma[0]), a=a.numpy(), c=c.numpy(), q=float(q[0]),
                   dist=dist.numpy())
        AO.check_stages(got, sums, honest, byz, "minmax", dirn, 1.0, t)
        assert counts[:B] == [h + n for h, n in zip(honest, byz)]
        theta = before.clone()
        hand = [e.clone() for e in ents]
        if rule[0] == "krum":
            krum_step(Krum(0, 1, hand, counts), theta, None, None, sim.step, optim=sim.optim)
        else:
            geomed_step(GeoMed(3, 1e-6, False, hand, counts), theta, None, None, sim.step,
                        optim=sim.optim)
        torch.cuda.synchronize()
        bad = int((_bits(theta) != _bits(sim.theta)).sum())
        assert bad == 0, (t, bad)
        assert not torch.equal(theta, before)
    assert pops >= 1 and len(sim.attack_gamma_log()) == EPOCHS
