"""MI355X: nearest-neighbour mixing of the bucketed entries (Krum's distance launch, k_nnm_finish,
k_nnm_mix through flsim_nnm_entries) against the text of flsim/robust.py run by torch on the CPU
(tests/_nnm.py's comparison: dist within 2 (P + 2) 2^-53 relative, nbr equal after asserting the
text's own cut is 1000 times wider, the mixed entries equal as numbers): k on both sides of every
KPAD, P around the tiles of both launches, blocks that run several tiles, scratch that starts from
different bytes, sub-views, exact ties, poisoned entries, the host twin bit for bit, FLSimulation
on PerformantNet1, and the property the feature exists for.
"""
import numpy as np
import pytest
import torch

import _nnm as M
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

DEV = "cuda:0"
POISONS = (M.QNAN, 0x7F800001)
GUARD = 3


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _poisoned(n, pat=M.QNAN):
    return torch.full((n,), pat, dtype=torch.int32, device=DEV).view(torch.float32)


def _mix_tile(k):
    from flsim._lib import lib
    return int(lib().flsim_nnm_tile_elems(k))


def _ps(k):
    out = []
    for E in (M.krum_tile(k), _mix_tile(k)):
        for P in (1, 3, 255, 256, 257, E - 1, E, E + 1, 3 * E + 5):
            if P not in out:
                out.append(P)
    return out


def _run(ents, counts, f, pat=M.QNAN):
    """One flsim_nnm_entries over device copies of the entries, each allocated with GUARD words
    past P; the scratch (partials, dist, nbr) starts from the pattern `pat`.  -> (mixed [k, P],
    dist [k, k], nbr [k] uint64) on the host; the guard words keep their pattern."""
    from flsim.engine import NNM, nnm_entries
    k, P = len(ents), len(ents[0])
    bufs = []
    for e in ents:
        b = _poisoned(P + GUARD, pat)
        b[:P].copy_(torch.from_numpy(np.ascontiguousarray(e, np.float32)))
        bufs.append(b)
    n = NNM(f, [b[:P] for b in bufs], counts)
    n.c_scratch(bufs[0].device, P)
    for t in NNM._scratch[(str(bufs[0].device), P, k)]:
        t.view(torch.int32).fill_(pat)
    nnm_entries(n, P)
    torch.cuda.synchronize()
    for b in bufs:
        assert int((_bits(b[P:]) != pat).sum()) == 0, "a word past P was written"
    mixed = np.stack([b[:P].cpu().numpy() for b in bufs])
    return mixed, n.dist.cpu().numpy(), n.nbr.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("k", M.KS)
def test_kernel_equals_the_text(k):
    for P in _ps(k):
        ents, counts = M.inputs(k, P)
        for f in M.fs(k):
            mixed, d, nbr = _run(ents, counts, f)
            M.compare(mixed, d, nbr, ents, counts, f, "device")


@pytest.mark.parametrize("k", (4, 64))
def test_blocks_run_several_tiles(k):
    """More mix tiles than the mix grid has blocks (2048 at k = 4, 512 at k = 64) and, at the same
    P, more distance tiles than krum_max_blocks (768, 512); the last tile of either is partial."""
    from flsim._lib import lib
    mix_cap, krum_cap = (2048, 768) if k == 4 else (512, 512)
    P = (mix_cap + 3) * _mix_tile(k) + 5
    assert -(-P // M.krum_tile(k)) > krum_cap and -(-P // _mix_tile(k)) > mix_cap
    # (the partials are then capped: one run of NPB * 16 doubles a block)
    npb = (M.kpad(k) // 4) * (M.kpad(k) // 4 + 1) // 2
    assert lib().flsim_nnm_partials(P, k) == krum_cap * npb * 16
    ents, counts = M.inputs(k, P)
    f = (k - 1) // 2
    mixed, d, nbr = _run(ents, counts, f)
    M.compare(mixed, d, nbr, ents, counts, f, "grid-stride")


@pytest.mark.parametrize("k", (2, 9, 64))
def test_bits_do_not_depend_on_what_is_never_read(k):
    """The scratch starts from two different patterns: identical bits, and identical on a repeat."""
    P = 3 * M.krum_tile(k) + 5
    ents, counts = M.inputs(k, P)
    f = (k - 1) // 2
    a = _run(ents, counts, f, POISONS[0])
    for pat in (POISONS[0], POISONS[1]):
        b = _run(ents, counts, f, pat)
        assert np.array_equal(M.bits(a[0]), M.bits(b[0]))
        assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
        assert np.array_equal(a[2], b[2])


def test_sub_views_of_a_larger_buffer():
    """k = 9 entries as views at 16-byte-aligned offsets (not 256-byte aligned) inside one poisoned
    buffer, four guard words or more between them: the guards keep their bits."""
    from flsim.engine import NNM, nnm_entries
    k, P, f = 9, 2 * _mix_tile(9) + 37, 2
    ents, counts = M.inputs(k, P)
    stride = (P + 4 + 3) // 4 * 4
    buf = _poisoned(4 + k * stride)
    views = [buf[4 + j * stride:4 + j * stride + P] for j in range(k)]
    assert all(v.data_ptr() % 16 == 0 for v in views) and any(v.data_ptr() % 256 for v in views)
    for v, e in zip(views, ents):
        v.copy_(torch.from_numpy(e))
    n = NNM(f, views, counts)
    nnm_entries(n, P)
    torch.cuda.synchronize()
    M.compare(np.stack([v.cpu().numpy() for v in views]), n.dist.cpu().numpy(),
              n.nbr.cpu().numpy().view(np.uint64), ents, counts, f, "views")
    assert n.neighbours() == [[j for j in range(k) if (int(w) >> j) & 1]
                              for w in n.nbr.cpu().numpy().view(np.uint64)]
    guard = torch.ones(buf.numel(), dtype=torch.bool, device=DEV)
    for j in range(k):
        guard[4 + j * stride:4 + j * stride + P] = False
    assert int(guard.sum()) >= 4 * (k + 1)
    assert int((buf.view(torch.int32)[guard] != M.QNAN).sum()) == 0


def test_exact_ties_and_poisoned_entries():
    """The CPU cases (tests/test_cpu_nnm.py) on the device."""
    from test_cpu_nnm import poisoned_inputs, tie_cases, tie_inputs
    for k, groups in tie_cases():
        ents, counts = tie_inputs(k, groups)
        for f in M.fs(k, zero=False):
            mixed, d, nbr = _run(ents, counts, f)
            M.compare(mixed, d, nbr, ents, counts, f, "ties")
            for g in groups:
                assert all(d[a, b] == 0.0 for a in g for b in g)
                assert all(np.array_equal(d[a], d[g[0]]) for a in g)
                assert len({int(nbr[a]) for a in g}) == 1
    ents, counts = tie_inputs(5, [(0, 2, 4)])
    assert [int(w) for w in _run(ents, counts, 2)[2][[0, 2, 4]]] == [0b10101] * 3
    for k in (5, 9):
        for bad in (np.nan, np.inf):
            ents, counts, p = poisoned_inputs(k, bad)
            mixed, d, nbr = _run(ents, counts, 1)
            M.compare(mixed, d, nbr, ents, counts, 1, "poisoned")
            assert (int(nbr[p]) >> p) & 1 and d[p, p] == 0
            hit = np.zeros(257, bool)
            hit[3::7] = True
            assert not np.isfinite(mixed[p][hit]).any() and np.isfinite(mixed[p][~hit]).all()
            if np.isnan(bad):
                assert np.isnan(mixed[p][hit]).all()
            for i in range(k):
                if i != p:
                    assert not (int(nbr[i]) >> p) & 1 and np.isfinite(mixed[i]).all()


@pytest.mark.parametrize("k", (3, 7, 13, 29, 50))
def test_device_equals_the_host_twin(k):
    """One shape per KPAD: nbr and the mixed entries bit for bit (the same selection and element
    code on both sides; the distances differ in their summation order alone, within the bound)."""
    P = 2 * _mix_tile(k) + 77
    ents, counts = M.inputs(k, P)
    f = (k - 1) // 2
    mixed, d, nbr = _run(ents, counts, f)
    hm, hd, hn = M.host_twin(ents, counts, f)
    assert M.cut_gap(hd, f) > M.GAP_FACTOR * M.dist_bound(P)
    assert np.array_equal(nbr, hn)
    assert np.array_equal(M.bits(mixed), M.bits(hm))
    assert (np.abs(d - hd) <= 2 * M.dist_bound(P) * hd).all()


@pytest.mark.parametrize("k", (3, 4, 5, 9, 64))
def test_krum_and_nnm_share_the_matrix(k):
    """Krum (f = 0, m = 1, the rule alone) and NNM (f = 0) over the same entries and counts, both
    scratches starting from QNAN: dist is the same matrix, bit for bit.  KPAD 4, 4, 8, 16 and 64;
    P of one element, one tile + 1 and 3 tiles + 5; then entry 1 holding a NaN (a +inf row and
    column on both sides).  NNM mixes in place, so each side gets its own copies."""
    from flsim.engine import Krum, krum_step
    E = M.krum_tile(k)
    cases = [(P, False) for P in (1, E + 1, 3 * E + 5)] + [(3 * E + 5, True)]
    for P, poison in cases:
        ents, counts = M.inputs(k, P)
        if poison:
            ents[1][P // 2] = np.nan
        dev = [torch.from_numpy(e).to(DEV) for e in ents]
        kr = Krum(0, 1, dev, counts)
        kr.c_scratch(dev[0].device, P)
        for t in Krum._scratch[(str(dev[0].device), P, k)]:
            t.view(torch.int32).fill_(M.QNAN)
        krum_step(kr, None, None, None, 1, optim=False, g_out=torch.empty(P, device=DEV))
        torch.cuda.synchronize()
        dk = kr.dist.cpu().numpy()
        _, dn, _ = _run(ents, counts, 0)
        assert np.array_equal(dk.view(np.uint64), dn.view(np.uint64)), (k, P, poison)
        off = np.arange(k) != 1
        hit = np.isinf(dk[1, off]) & np.isinf(dk[off, 1])
        assert hit.all() if poison else not np.isinf(dk).any()
        assert np.isfinite(dk[off][:, off]).all() and dk[1, 1] == 0


def test_refusals_on_device_pointers():
    """Overlapping entries, a misaligned entry, a bad f, a None entry: ValueError, and nothing is
    launched (the buffer keeps its bits)."""
    from flsim.engine import NNM, nnm_entries
    P = 1000
    buf = torch.from_numpy(np.random.RandomState(1).standard_normal(4 * P + 8)
                           .astype(np.float32)).to(DEV)
    before = buf.clone()
    e = [buf[j * P:(j + 1) * P] for j in range(3)]
    with pytest.raises(ValueError, match="entries 0 and 1 overlap"):
        nnm_entries(NNM(1, [e[0], buf[P - 4:2 * P - 4], e[2]], [1, 1, 1]), P)
    with pytest.raises(ValueError, match="16-byte aligned"):
        nnm_entries(NNM(1, [e[0], e[1], buf[2 * P + 1:3 * P + 1]], [1, 1, 1]), P)
    with pytest.raises(ValueError, match="Invalid NNM f = 2 for k = 3"):
        nnm_entries(NNM(2, e, [1, 1, 1]), P)
    with pytest.raises(ValueError, match="null entry 1"):
        nnm_entries(NNM(1, [e[0], None, e[2]], [1, 1, 1]), P)
    with pytest.raises(ValueError, match="Invalid count 0 of entry 2"):
        nnm_entries(NNM(1, e, [1, 1, 0]), P)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32))


def test_selection_changes_the_outcome():
    """k = 8 entries of which the last 2 are IPM-crafted (eps = 4, the text's attack_flat).  With
    f = 2 no honest row's neighbours contain a Byzantine entry -- asserted on the text first, a
    property of the inputs -- so the mean of the mixed honest entries still points along the honest
    mean, while the plain mean over all 8 points against it."""
    from flsim.robust import attack_flat, nnm_flat
    k, P, f = 8, 1000, 2
    g = torch.Generator().manual_seed(77)
    base = torch.randn(P, generator=g)
    honest, byz = [2, 1, 3, 1, 2, 1, 0, 0], [0, 0, 0, 0, 0, 0, 1, 2]
    sums = [(torch.randn(P, generator=g) * 0.5 + base) * h if h else None for h in honest]
    ents, counts, b = attack_flat(sums, honest, byz, "ipm", 4.0)
    mu = torch.stack([s / h for s, h in zip(sums, honest) if h]).mean(0)
    mixed_t, d_t, nbr_t = nnm_flat(ents, counts, f)
    assert all(not set(nbr_t[i]) & {6, 7} for i in range(6))
    np_ents = [e.numpy() for e in ents]
    mixed, d, nbr = _run(np_ents, counts, f)
    M.compare(mixed, d, nbr, np_ents, counts, f, "ipm")
    assert all(not (int(nbr[i]) >> 6) & 3 for i in range(6))
    means = torch.stack([e / c for e, c in zip(ents, counts)])
    plain = means.mean(0)
    kept = torch.from_numpy(mixed[:6]).mean(0)
    assert not torch.equal(kept, plain)
    assert float(plain @ mu) < 0 < float(kept @ mu)
    assert float((kept - mu).norm()) < 0.2 * float(mu.norm())


# ---- FLSimulation on PerformantNet1 ----------------------------------------------------------------
N, EPOCHS, LR, CW = 12, 3, 0.01, 4      # (the slow worker's first entry pops in the third epoch)


@pytest.fixture(scope="module")
def pool():
    from oracle import oracle as O
    return O.make_pool(0)


@pytest.mark.parametrize("attack", (None, "ipm"))
@pytest.mark.parametrize("rule", ("median", ("krum", 1)))
def test_simulation_with_mixing(pool, rule, attack):
    """n = 12, delay 2, nnm = 1, with and without 3 IPM workers; 4 buckets for the median, 5 for
    Krum (f = 1 needs k >= 5 entries in every epoch).  last_entries is the pre-mix snapshot;
    last_mixed equals the text over it; nnm_log() holds the text's masks; theta equals the
    existing rule step run by hand on last_mixed with counts 1; the recorded config holds nnm."""
    from flsim.engine import Krum, Robust, krum_step, robust_step
    from flsim.sim import FLSimulation
    B = 4 if rule == "median" else 5
    kw = dict(attack=attack, n_byz=3) if attack else {}
    sim = FLSimulation(N, device=DEV, chunk_workers=CW, pool=pool, dropout=False,
                       semantics="independent", delay=2, robust_rule=rule, buckets=B,
                       optimizer="sgd", lr=LR, keep_entries=True, nnm=1, **kw)
    assert sim._stale_config()["nnm"] == 1
    pops = 0
    for t in range(EPOCHS):
        before = sim.theta.clone()
        sim.epoch()
        plan = sim.trace[-1]
        ents, counts = sim.last_entries
        k = B + bool(plan.stale)
        pops += bool(plan.stale)
        assert len(ents) == k == len(sim.last_mixed) and sum(counts) == 11 + bool(plan.stale)
        log = sim.nnm_log()
        assert len(log) == t + 1 and log[-1].is_cuda
        M.compare(np.stack([e.cpu().numpy() for e in sim.last_mixed]), None,
                  log[-1].cpu().numpy().view(np.uint64), [e.cpu().numpy() for e in ents], counts,
                  1, f"sim t={t}")
        theta = before.clone()
        hand = [e.clone() for e in sim.last_mixed]
        if rule == "median":
            robust_step(Robust("median", 0, hand, [1] * k), theta, None, None, sim.step,
                        optim=sim.optim)
        else:
            krum_step(Krum(1, 1, hand, [1] * k), theta, None, None, sim.step, optim=sim.optim)
        torch.cuda.synchronize()
        bad = int((_bits(theta) != _bits(sim.theta)).sum())
        assert bad == 0, (t, bad)
        assert not torch.equal(theta, before)
    assert pops >= 1
