"""GPU: simulated Byzantine workers (csrc/server.hip: k_attack through flsim_attack_entries) against
the text of flsim/robust.py run by torch on the CPU, "equal as numbers" (tests/_attack.py): the same
32 bits wherever the text's value is neither zero nor NaN, a zero where it gives a zero, a NaN
where it gives a NaN.  No tolerance: the attack is element-wise and every operation of the text is
one correctly rounded IEEE operation.

  kernel        both kinds at k on both sides of every KPAD, P in {1, 255, 256, 257, E - 1, E,
                E + 1, 3 E + 5} for the launch's tile E, honest-only, mixed and fully Byzantine
                entries in every case; entries with byz == 0 keep their bits; b_out equals
                attack_vector; nothing past P is written;
  poison        the write-only entries and b_out start from two different patterns: same bits;
  sub-views     entries at 16-byte-aligned offsets inside one larger buffer: the words between
                them keep their bits;
  several tiles a P with more tiles than the grid has blocks;
  sim           FLSimulation on PerformantNet1 under attack: last_entries equals the text over
                the honest sums, theta equals the existing robust step run by hand on them.
"""
import numpy as np
import pytest
import torch

import _attack as A
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

DEV = "cuda:0"
KS = (1, 4, 5, 8, 9, 16, 17, 32, 33, 64)       # both sides of every KPAD
POISONS = (A.QNAN, 0x7F800001)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _poisoned(n, pat=A.QNAN):
    return torch.full((n,), pat, dtype=torch.int32, device=DEV).view(torch.float32)


def _tile(k):
    from flsim._lib import lib
    return int(lib().flsim_attack_tile_elems(k))


def _ps(k):
    E = _tile(k)
    return (1, 255, 256, 257, E - 1, E, E + 1, 3 * E + 5)


def _run(ents, honest, byz, kind, strength, pat=A.QNAN, b_out=True):
    """One launch over device copies of the entries (the never-read ones and b_out start from the
    pattern `pat`) -> (entries after, b) on the host; nothing past P is written to b_out."""
    from flsim.engine import Attack, attack_entries
    P = len(ents[0])
    dents = [_dev(e) if h else _poisoned(P, pat) for e, h in zip(ents, honest)]
    b = _poisoned(P + 3, pat) if b_out else None
    attack_entries(Attack(kind, strength, dents, honest, byz), None if b is None else b[:P], P)
    torch.cuda.synchronize()
    if b is not None:
        assert int((_bits(b[P:]) != pat).sum()) == 0
    return [d.cpu().numpy() for d in dents], None if b is None else b[:P].cpu().numpy()


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("k", KS)
def test_kernel_equals_the_text(kind, k):
    from flsim.robust import attack_vector
    for P in _ps(k):
        ents, honest, byz = A.inputs(k, P)
        if k >= 3:
            assert {(h > 0, c > 0) for h, c in zip(honest, byz)} == \
                {(True, True), (True, False), (False, True)}
        got, b = _run(ents, honest, byz, kind, A.STRENGTH[kind])
        ref, counts, bt = A.compare(got, b, ents, honest, byz, kind, A.STRENGTH[kind], (k, P))
        sums = [torch.from_numpy(e) if h else None for e, h in zip(ents, honest)]
        vec = attack_vector(sums, honest, kind, A.STRENGTH[kind]).numpy()
        assert A.mismatches(b, vec) == 0 and np.isfinite(vec).all() and (vec != 0).all()


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("k", (3, 9, 64))
def test_bits_do_not_depend_on_what_is_never_read(kind, k):
    """Two runs whose write-only entries and b_out start from different patterns, and a third
    without b_out: identical bits, and identical to a repeat of the first."""
    P = 3 * _tile(k) + 5
    ents, honest, byz = A.inputs(k, P)
    a, ba = _run(ents, honest, byz, kind, A.STRENGTH[kind], POISONS[0])
    for pat, with_b in ((POISONS[0], True), (POISONS[1], True), (POISONS[1], False)):
        c, bc = _run(ents, honest, byz, kind, A.STRENGTH[kind], pat, with_b)
        if with_b:
            assert np.array_equal(A.bits(ba), A.bits(bc))
        for x, y in zip(a, c):
            assert np.array_equal(A.bits(x), A.bits(y))


@pytest.mark.parametrize("kind", A.KINDS)
def test_sub_views_of_a_larger_buffer(kind):
    """k = 9 entries and b_out as views at 16-byte-aligned offsets (not 256-byte aligned) inside
    one poisoned buffer, four guard words after each: the guards keep their bits."""
    from flsim.engine import Attack, attack_entries
    k, P = 9, 2 * _tile(9) + 37
    ents, honest, byz = A.inputs(k, P)
    stride = (P + 4 + 3) // 4 * 4
    buf = _poisoned(4 + (k + 1) * stride)
    views = [buf[4 + j * stride:4 + j * stride + P] for j in range(k + 1)]
    assert all(v.data_ptr() % 16 == 0 for v in views) and any(v.data_ptr() % 256 for v in views)
    for v, e, h in zip(views, ents, honest):
        if h:
            v.copy_(_dev(e))
    attack_entries(Attack(kind, A.STRENGTH[kind], views[:k], honest, byz), views[k], P)
    torch.cuda.synchronize()
    A.compare([v.cpu().numpy() for v in views[:k]], views[k].cpu().numpy(), ents, honest, byz,
              kind, A.STRENGTH[kind], "views")
    guard = torch.ones(buf.numel(), dtype=torch.bool, device=DEV)
    for j in range(k + 1):
        guard[4 + j * stride:4 + j * stride + P] = False
    assert int(guard.sum()) >= 4 * (k + 1)
    assert int((buf.view(torch.int32)[guard] != A.QNAN).sum()) == 0


@pytest.mark.parametrize("k", (4, 64))
def test_a_block_runs_several_tiles(k):
    """More tiles than the grid's cap (2048 blocks at k = 4, 512 at k = 64), the last one partial:
    some blocks take two tiles."""
    cap = 2048 if k == 4 else 512
    P = (cap + 3) * _tile(k) + 5
    ents, honest, byz = A.inputs(k, P)
    got, b = _run(ents, honest, byz, "ipm", A.STRENGTH["ipm"])
    A.compare(got, b, ents, honest, byz, "ipm", A.STRENGTH["ipm"], (k, P))


def test_nan_and_inf_propagate_as_in_the_text():
    for kind in A.KINDS:
        for bad in (np.nan, np.inf, -np.inf):
            ents, honest, byz = A.inputs(8, 1027, 1)
            j = next(i for i, h in enumerate(honest) if h and not byz[i])
            ents[j] = ents[j].copy()
            ents[j][3::7] = bad
            got, b = _run(ents, honest, byz, kind, A.STRENGTH[kind])
            ref, counts, bt = A.compare(got, b, ents, honest, byz, kind, A.STRENGTH[kind], bad)
            assert not np.isfinite(bt[3::7]).any()


def test_refusals_on_device_pointers():
    """Overlapping entries, an entry overlapping b_out, a misaligned entry, a missing honest
    entry: ValueError, and nothing is launched (the buffer keeps its bits)."""
    from flsim.engine import Attack, attack_entries
    P = 1000
    buf = _dev(np.random.RandomState(1).standard_normal(4 * P + 8).astype(np.float32))
    before = buf.clone()
    e = [buf[j * P:(j + 1) * P] for j in range(3)]
    with pytest.raises(ValueError, match="entries 0 and 1 overlap"):
        attack_entries(Attack("ipm", 1.0, [e[0], buf[P - 4:2 * P - 4], e[2]], [1, 1, 0],
                              [0, 1, 1]), None, P)
    with pytest.raises(ValueError, match="overlaps b_out"):
        attack_entries(Attack("ipm", 1.0, e, [1, 1, 0], [0, 1, 1]), buf[2 * P + 4:3 * P + 4], P)
    with pytest.raises(ValueError, match="16-byte aligned"):
        attack_entries(Attack("ipm", 1.0, [e[0], e[1], buf[2 * P + 1:3 * P + 1]], [1, 1, 0],
                              [0, 1, 1]), None, P)
    with pytest.raises(ValueError, match="nothing to observe"):
        attack_entries(Attack("alie", 1.0, e, [0, 0, 0], [1, 1, 1]), None, P)
    with pytest.raises(ValueError, match="attack strength"):
        attack_entries(Attack("alie", -1.0, e, [1, 1, 0], [0, 1, 1]), None, P)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32))


# ---- FLSimulation on PerformantNet1 ----------------------------------------------------------------
N, EPOCHS, LR, CW, B = 12, 3, 0.01, 4, 4   # (the slow worker's first entry pops in the third epoch)


@pytest.fixture(scope="module")
def pool():
    from oracle import oracle as O
    return O.make_pool(0)


@pytest.mark.parametrize("rule", ("median", ("geomed", 3)))
def test_simulation_under_attack(pool, rule):
    """n = 12, delay 2, 4 buckets, 3 Byzantine workers spread over the 11 fast ones, ALIE with the
    paper's z.  Every fresh entry's honest sum is an engine pass over exactly its honest workers;
    last_entries equals the text over the honest sums; theta equals the existing robust step run by
    hand on last_entries."""
    from flsim.engine import GeoMed, PN1Engine, Robust, geomed_step, robust_step, worker_table
    from flsim.robust import alie_z
    from flsim.sim import FLSimulation
    sim = FLSimulation(N, device=DEV, chunk_workers=CW, pool=pool, dropout=False,
                       semantics="independent", delay=2, robust_rule=rule, buckets=B,
                       optimizer="sgd", lr=LR, keep_entries=True, attack="alie", n_byz=3)
    byzset = set(int(i) for i in sim.byz_workers)
    assert len(byzset) == 3
    eng = PN1Engine(DEV, chunk_workers=CW)
    rs = np.random.RandomState(sim.seed)
    pops = 0
    for t in range(EPOCHS):
        before = sim.theta.clone()
        ks = rs.randint(0, N, size=N)
        sim.epoch()
        plan = sim.trace[-1]
        ents, counts = sim.last_entries
        b, honest, byz = sim.last_attack
        fast = [i for i in range(N) if plan.computes[i] and sim.delays[i] == 0]
        bounds = [(j * len(fast)) // B for j in range(B + 1)]
        assert sum(byz) == 3 and len(ents) == B + bool(plan.stale)
        pops += bool(plan.stale)
        z = alie_z(len(fast), 3)
        assert sim.attack_log()[-1] == ("alie", z, 3)
        sums = []
        for j in range(B):
            ws = [i for i in fast[bounds[j]:bounds[j + 1]] if i not in byzset]
            assert honest[j] == len(ws) >= 1
            eng.begin_epoch(before)
            eng.run_chunk(before, sim.pool, worker_table([(t, i, int(ks[i])) for i in ws], DEV),
                          len(ws), N, sim.seed, False, torch.zeros(len(ws), device=DEV))
            S = torch.empty(eng.P, device=DEV)
            eng.end_epoch(S)
            assert int((_bits(S) != _bits(sim.last_honest[j])).sum()) == 0, (t, j)
            sums.append(sim.last_honest[j].cpu().numpy())
        A.compare([e.cpu().numpy() for e in ents[:B]], b.cpu().numpy(), sums, honest, byz, "alie",
                  z, t)
        assert counts[:B] == [h + c for h, c in zip(honest, byz)]
        # the existing robust step by hand on the attacked entries
        theta = before.clone()
        hand = [e.clone() for e in ents]
        if rule == "median":
            robust_step(Robust("median", 0, hand, counts), theta, None, None, sim.step,
                        optim=sim.optim)
        else:
            geomed_step(GeoMed(3, 1e-6, False, hand, counts), theta, None, None, sim.step,
                        optim=sim.optim)
        torch.cuda.synchronize()
        bad = int((_bits(theta) != _bits(sim.theta)).sum())
        assert bad == 0, (t, bad)
        assert not torch.equal(theta, before)
    assert pops >= 1
