"""CPU: nearest-neighbour mixing (NNM) of the bucketed entries before a robust rule.

The host twin flsim_nnm_eval_host (csrc/nnm.h: the selection and the element code the kernels run,
one host + device function each) against the text (flsim/robust.py: nnm_neighbours, _nnm,
nnm_flat) by tests/_nnm.py's comparison; exact ties; poisoned entries; every refusal of
flsim_nnm_entries (they come before any launch, so made-up device addresses are never read) and
their order; check_nnm and NNM(rule, f) against a hand-written example; the NNM object; and the
refusals of FLSimulation(nnm=...) and main.py --nnm that need no GPU.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import _nnm as M

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "fl-distributed-delay_amd")


@pytest.mark.parametrize("k", M.KS)
def test_host_twin_equals_the_text(k):
    """dist within the bound, nbr equal, the mixed entries equal as numbers; f = 0: every y_i is
    the plain mean of all entries in index order.  out is optional."""
    for P in M.ps_for_tile(M.krum_tile(k)):
        ents, counts = M.inputs(k, P)
        for f in M.fs(k):
            mixed, d, nbr = M.host_twin(ents, counts, f)
            ref, dt, nt = M.compare(mixed, d, nbr, ents, counts, f, "host")
            assert all(bin(int(w)).count("1") == k - f and (int(w) >> i) & 1
                       for i, w in enumerate(nbr))
            if f == 0:
                means = [e / np.float32(c) for e, c in zip(ents, counts)]
                acc = means[0].copy()
                for x in means[1:]:
                    acc = acc + x
                plain = acc / np.float32(k)
                for i in range(k):
                    assert M.mismatches(mixed[i], plain) == 0
        none, d2, nbr2 = M.host_twin(ents, counts, M.fs(k)[-1], out=False)
        assert none is None and np.array_equal(nbr2, nbr) and np.array_equal(d2, d)


def test_the_mix_tile_is_the_attacks_and_the_partials_are_krums():
    from flsim._lib import lib
    L = lib()
    for k in range(1, 65):
        assert L.flsim_nnm_tile_elems(k) == L.flsim_attack_tile_elems(k) >= 256
        for P in (1, 8191, 8192, 8193, 1 << 22):
            assert L.flsim_nnm_partials(P, k) == L.flsim_krum_partials(P, k) > 0
    assert L.flsim_nnm_tile_elems(0) == 0 and L.flsim_nnm_tile_elems(65) == 0
    assert L.flsim_nnm_partials(0, 4) == 0 and L.flsim_nnm_partials(1 << 31, 4) == 0
    assert L.flsim_nnm_partials(64, 0) == 0 and L.flsim_nnm_partials(64, 65) == 0


def tie_cases():
    """(k, the groups of duplicated entries): two and three duplicates."""
    return [(5, [(1, 3)]), (5, [(0, 2, 4)]), (9, [(2, 7)]), (9, [(1, 4, 8)]), (9, [(0, 8), (3, 5)])]


def tie_inputs(k, groups, P=257):
    ents, counts = M.inputs(k, P)
    for g in groups:
        for j in g[1:]:
            ents[j] = ents[g[0]].copy()
            counts[j] = counts[g[0]]
    return ents, counts


@pytest.mark.parametrize("k,groups", tie_cases())
def test_exact_ties_go_to_the_lowest_index(k, groups):
    """Duplicate entries are at distance exactly 0 of each other and at bit-identical distances of
    everything else: the text and the host twin both take the lower index first."""
    ents, counts = tie_inputs(k, groups)
    for f in M.fs(k, zero=False):
        mixed, d, nbr = M.host_twin(ents, counts, f)
        ref, dt, nt = M.compare(mixed, d, nbr, ents, counts, f, "ties")
        for g in groups:
            for a in g:
                for b in g:
                    assert d[a, b] == 0.0
                assert np.array_equal(d[a], d[g[0]])
            # the duplicates have the same neighbours, and they take each other lowest index first
            assert len({int(nbr[a]) for a in g}) == 1
    # a hand-checked case: three equal entries and f = 2 of k = 5: each keeps the three
    ents, counts = tie_inputs(5, [(0, 2, 4)])
    _, _, nbr = M.host_twin(ents, counts, 2)
    assert [int(nbr[j]) for j in (0, 2, 4)] == [0b10101] * 3


def poisoned_inputs(k, bad, P=257):
    ents, counts = M.inputs(k, P)
    p = 2
    ents[p] = ents[p].copy()
    ents[p][3::7] = bad
    return ents, counts, p


@pytest.mark.parametrize("bad", (np.nan, np.inf))
@pytest.mark.parametrize("k", (5, 9))
def test_poisoned_entries(k, bad):
    """f = 1 and one entry with NaNs, or with +infs: its distance to itself is NaN -> +inf and the
    diagonal is zero all the same, so its own row keeps itself; every other row sees it at +inf,
    last, and does not select it; the others' mixed entries are finite and the text's.  The
    poisoned entry's mixed entry is not finite where it was not: NaN for the NaN case; for +inf the
    text's own value there, inf + finite = +inf (asserted as the text gives it, as numbers)."""
    ents, counts, p = poisoned_inputs(k, bad)
    mixed, d, nbr = M.host_twin(ents, counts, 1)
    ref, dt, nt = M.compare(mixed, d, nbr, ents, counts, 1, "poisoned")
    assert (int(nbr[p]) >> p) & 1
    assert d[p, p] == 0 and all(np.isinf(d[p, j]) for j in range(k) if j != p)
    hit = np.zeros(257, bool)
    hit[3::7] = True
    for i in range(k):
        if i == p:
            assert not np.isfinite(mixed[i][hit]).any() and np.isfinite(mixed[i][~hit]).all()
            if np.isnan(bad):
                assert np.isnan(mixed[i][hit]).all()
        else:
            assert not (int(nbr[i]) >> p) & 1
            assert np.isfinite(mixed[i]).all()


# ---- refusals of the entry point (status 1, before any launch) -------------------------------------
F = {name: 0x1000000 * (i + 1) for i, name in enumerate(["part", "dist", "nbr", "e0", "e1", "e2"])}
P = 64
NPART = 16      # flsim_nnm_partials(64, 3): one block, one 4 x 4 pair block


def _call(f=1, counts=(2, 1, 3), ents=None, n=P, k=None, part=F["part"], dist=F["dist"],
          nbr=F["nbr"], n_part=NPART, scratch=True, host=False):
    from flsim._lib import FlsimNnmScratch, lib
    ents = [F["e0"], F["e1"], F["e2"]][:len(counts)] if ents is None else ents
    ents = list(ents) + [0] * (min(len(counts), 64) - len(ents))
    a, _ = M.c_nnm(None, list(counts), f, ptrs=ents, k=k)
    vp = ctypes.c_void_p
    if host:
        rc = lib().flsim_nnm_eval_host(ctypes.byref(a), n, vp(dist), vp(nbr), None)
    else:
        s = FlsimNnmScratch()
        s.partials, s.n_partials, s.dist, s.nbr = part, n_part, dist, nbr
        rc = lib().flsim_nnm_entries(ctypes.byref(a), ctypes.byref(s) if scratch else None, n,
                                     None)
    return rc, lib().flsim_last_error().decode()


N_FIELDS = 10       # the leading REFUSALS that are about flsim_nnm's fields alone
REFUSALS = [
    (dict(counts=()), "NNM over k = 0 entries (1 .. 64)"),
    (dict(counts=(1,) * 65), "NNM over k = 65 entries"),
    (dict(k=-3), "NNM over k = -3 entries"),
    (dict(f=-1), "Invalid NNM f = -1 for k = 3 entries: f >= 0 and 2 * f < k"),
    (dict(f=2), "Invalid NNM f = 2 for k = 3 entries"),
    (dict(f=1, counts=(1, 1)), "Invalid NNM f = 1 for k = 2 entries"),
    (dict(f=32, counts=(1,) * 64), "Invalid NNM f = 32 for k = 64 entries"),
    (dict(counts=(2, 0, 3)), "Invalid count 0 of entry 1: it must be >= 1"),
    (dict(counts=(2, 1, -4)), "Invalid count -4 of entry 2"),
    (dict(f=0, counts=(0,)), "Invalid count 0 of entry 0"),
    # the pointers
    (dict(ents=[F["e0"], 0, F["e2"]]), "null entry 1"),
    (dict(ents=[F["e0"], F["e1"], 0]), "null entry 2"),
    (dict(ents=[F["e0"] + 4, F["e1"], F["e2"]]), "entry 0 must be 16-byte aligned"),
    (dict(ents=[F["e0"], F["e1"], F["e2"] + 8]), "entry 2 must be 16-byte aligned"),
    (dict(n=0), "P = 0 out of range"),
    (dict(n=-5), "out of range"),
    (dict(n=1 << 31), "out of range"),
    (dict(scratch=False), "null NNM scratch"),
    (dict(part=0), "null NNM scratch"),
    (dict(dist=0), "null NNM scratch"),
    (dict(nbr=0), "null NNM scratch"),
    (dict(part=F["part"] + 8), "NNM scratch must be 16-byte aligned"),
    (dict(dist=F["dist"] + 8), "NNM scratch must be 16-byte aligned"),
    (dict(nbr=F["nbr"] + 8), "NNM scratch must be 16-byte aligned"),
    (dict(n_part=NPART - 1), "NNM n_partials = 15, this step writes 16"),
    (dict(ents=[F["e0"], F["e0"], F["e2"]]), "entries 0 and 1 overlap"),
    (dict(ents=[F["e0"], F["e1"], F["e0"] + 4 * (P - 4)]), "entries 0 and 2 overlap"),
    (dict(ents=[F["e0"], F["e2"] - 4 * (P - 4), F["e2"]]), "entries 1 and 2 overlap"),
    (dict(part=F["e1"]), "entry 1 overlaps the NNM scratch"),
    (dict(dist=F["e0"] + 4 * (P - 4)), "entry 0 overlaps the NNM scratch"),
    (dict(nbr=F["e2"] - 16), "entry 2 overlaps the NNM scratch"),
    (dict(dist=F["part"] + 8 * NPART - 16), "NNM scratch buffers overlap each other"),
]


@pytest.mark.parametrize("kw,message", REFUSALS, ids=[f"{i}-{m[:24]}" for i, (_, m) in
                                                       enumerate(REFUSALS)])
def test_entry_point_refusals(kw, message):
    rc, err = _call(**kw)
    assert rc == 1, (rc, err)
    assert message in err, err


@pytest.mark.parametrize("kw,message", REFUSALS[:N_FIELDS + 2])
def test_host_twin_refuses_the_fields_and_a_null_entry(kw, message):
    rc, err = _call(host=True, **kw)
    assert rc == 1 and message in err, (rc, err)


def test_refusal_order_and_python_errors():
    """The fields come before the pointers (everything NULL and misaligned still names k, then f,
    then the counts); among the pointers: NULL / alignment of the entries, P, the scratch
    pointers, their alignment, n_partials, overlapping entries, an entry over the scratch.
    Adjacent buffers do not overlap.  The library's messages arrive as ValueError."""
    from flsim._lib import check, lib
    L = lib()
    bad = dict(ents=[0, 4, 0], n=0, part=0, dist=8, nbr=8, n_part=0)
    order = [dict(k=70, f=-1, counts=(0, 1, 1)),
             dict(f=-1, counts=(0, 1, 1)),
             dict(counts=(0, 1, 1)),
             dict()]
    names = ["k = 70", "Invalid NNM f = -1", "Invalid count 0 of entry 0", "null entry 0"]
    for kw, name in zip(order, names):
        rc, err = _call(**{**bad, **kw})
        assert rc == 1 and name in err, (name, err)
    e = [F["e0"], F["e1"], F["e2"]]
    steps = [(dict(ents=[e[0], e[1] + 4, e[2]], n=0, part=0), "entry 1 must be"),
             (dict(ents=[e[0], e[0], e[2]], n=0, part=0), "out of range"),
             (dict(ents=[e[0], e[0], e[2]], part=0, dist=8), "null NNM scratch"),
             (dict(ents=[e[0], e[0], e[2]], dist=F["dist"] + 8, n_part=0), "16-byte aligned"),
             (dict(ents=[e[0], e[0], e[2]], n_part=0), "n_partials = 0"),
             (dict(ents=[e[0], e[0], e[2]], part=e[2]), "entries 0 and 1 overlap"),
             (dict(part=e[2], dist=e[2]), "entry 2 overlaps the NNM scratch")]
    for kw, name in steps:
        rc, err = _call(**kw)
        assert rc == 1 and name in err, (name, err)
    assert L.flsim_nnm_entries(None, None, P, None) == 1
    assert "null NNM" in L.flsim_last_error().decode()
    # adjacent buffers overlap nothing: every check passes and the host twin runs (host arrays)
    buf = np.zeros(3 * P, np.float32)
    assert buf.ctypes.data % 16 == 0
    d, nbr = np.zeros(9), np.zeros(3, np.uint64)
    rc, err = _call(ents=[buf.ctypes.data + 4 * P * i for i in range(3)], dist=d.ctypes.data,
                    nbr=nbr.ctypes.data, host=True)
    assert rc == 0, err
    # three all-zero entries, every distance 0: ties by index alone, on the diagonal too
    assert [int(w) for w in nbr] == [0b011, 0b011, 0b011]
    with pytest.raises(ValueError, match="Invalid NNM f"):
        check(_call(f=2)[0])
    with pytest.raises(ValueError, match="Invalid count"):
        check(_call(counts=(1, 0, 1))[0])


def test_check_nnm_and_the_rule_wrapper_on_a_hand_written_example():
    from flsim.robust import NNM, check_nnm, median_rule, nnm_flat, nnm_neighbours
    with pytest.raises(IndexError, match="empty weight_ups"):
        check_nnm(0, 0)
    for f, k in ((-1, 3), (2, 3), (1, 2), (1, 1), (32, 64)):
        with pytest.raises(ValueError, match="Invalid NNM f"):
            check_nnm(f, k)
    assert check_nnm(0, 1) == 0 and check_nnm(1, 3) == 1 and check_nnm(31, 64) == 31
    # k = 3, f = 1, two tensors a worker: the whole-model points are 0, 1 and 10 (times ones)
    ups = [[torch.full((2, 2), v), torch.full((3,), v)] for v in (0.0, 1.0, 10.0)]
    cols = torch.stack([torch.cat([u.reshape(-1) for u in w]) for w in ups])
    d, nbr = nnm_neighbours(cols, 1)
    assert nbr == [[0, 1], [0, 1], [1, 2]]
    assert d.tolist() == [[0.0, 7.0, 700.0], [7.0, 0.0, 567.0], [700.0, 567.0, 0.0]]
    seen = []

    def spy(mixed_ups):
        seen.append(mixed_ups)
        return median_rule(mixed_ups)
    out = NNM(spy, f=1)(ups)
    (mixed,) = seen
    assert len(mixed) == 3 and [t.shape for t in mixed[0]] == [(2, 2), (3,)]
    for w, v in zip(mixed, (0.5, 0.5, 5.5)):
        assert all(bool((t == v).all()) for t in w)
    assert [t.shape for t in out] == [(2, 2), (3,)] and all(bool((t == 0.5).all()) for t in out)
    # the flat form over bucket sums: counts 2, 1, 4 of the same means
    flat, d2, nbr2 = nnm_flat([cols[0] * 2, cols[1], cols[2] * 4], [2, 1, 4], 1)
    assert nbr2 == nbr and torch.equal(d2, d)
    assert flat[:, 0].tolist() == [0.5, 0.5, 5.5]
    # None is an all-zero entry
    flat3, _, nbr3 = nnm_flat([None, cols[1], cols[2] * 4], [2, 1, 4], 1)
    assert nbr3 == nbr and torch.equal(flat3, flat)
    with pytest.raises(ValueError, match="Invalid NNM f"):
        NNM(median_rule, f=2)(ups)
    with pytest.raises(ValueError, match="Invalid NNM f"):
        NNM(median_rule, f=-1)
    with pytest.raises(IndexError):
        NNM(median_rule, f=0)([])


def test_nnm_object():
    from flsim.engine import NNM
    e = [torch.zeros(8) for _ in range(3)]
    n = NNM(1, e, [2, 1, 3])
    c = n.c_struct()
    assert (c.f, c.k) == (1, 3) and n.k == 3
    assert list(c.count[:3]) == [2, 1, 3]
    assert c.entries[0] == e[0].data_ptr() and c.entries[2] == e[2].data_ptr()
    assert NNM(1, e, [2, 1, 2 ** 40]).c_struct().count[2] == -1
    with pytest.raises(ValueError, match="counts"):
        NNM(1, e, [1, 1])
    with pytest.raises(ValueError, match="k = 65"):
        NNM(1, [e[0]] * 65, [1] * 65)
    from flsim._lib import lib
    names = [lib().flsim_probe_kernel_name(i).decode()
             for i in range(lib().flsim_probe_kernel_count())]
    assert {"nnm_dist", "nnm_finish", "nnm_mix"} <= set(names)


# ---- FLSimulation on a CPU stand-in (the one of tests/test_cpu_attack.py, with the mixing) ---------
def _stand_in():
    from test_cpu_attack import StandInEngine

    class MixingEngine(StandInEngine):
        def nnm_entries(self, nnm):
            from flsim.robust import nnm_flat
            self.mixed_counts = list(nnm.counts)
            mixed, d, nbr = nnm_flat(nnm.entries, nnm.counts, nnm.f)
            for e, new in zip(nnm.entries, mixed):
                e.copy_(new)
            nnm.dist = d
            nnm.nbr = torch.from_numpy(M.masks(nbr).view(np.int64).copy())
    return MixingEngine()


@pytest.mark.parametrize("attack", (None, ("ipm", 2.5)))
@pytest.mark.parametrize("rule", ("median", ("trimmed_mean", 1), ("krum", 1), ("geomed", 2)))
def test_epoch_with_mixing_on_a_stand_in(rule, attack):
    """n = 12, the last worker slow with delay 2, five buckets, nnm = 1.  The mixing comes after
    the attack and after the popped entry is appended: last_entries is the pre-mix snapshot with
    the real counts, last_mixed the text over exactly those, the rule then reads counts of 1, and
    nnm_log() holds the epoch's masks."""
    from test_cpu_attack import IND, _sim
    from flsim.robust import geomed_flat, krum_flat, nnm_flat, robust_flat
    eng = _stand_in()
    kw = dict(attack=attack, n_byz=3) if attack else {}
    sim = _sim(eng, robust_rule=rule, buckets=5, keep_entries=True, nnm=1, **kw, **IND)
    assert sim.nnm == 1 and sim.last_mixed is None and sim.nnm_log() == []
    pops = 0
    for t in range(4):
        before = sim.theta.clone()
        sim.epoch()
        plan = sim.trace[-1]
        ents, counts = sim.last_entries
        k = 5 + bool(plan.stale)
        pops += bool(plan.stale)
        assert len(ents) == k and eng.mixed_counts == counts and sum(counts) == 11 + bool(plan.stale)
        mixed, d, nbr = nnm_flat(ents, counts, 1)
        assert len(sim.last_mixed) == k
        for got, ref in zip(sim.last_mixed, mixed):
            assert torch.equal(got, ref)
        assert not torch.equal(sim.last_mixed[0], ents[0])
        log = sim.nnm_log()
        assert len(log) == t + 1 and log[-1].dtype == torch.int64
        assert np.array_equal(log[-1].numpy().view(np.uint64), M.masks(nbr))
        one = [1] * k
        if rule == "median" or rule[0] == "trimmed_mean":
            kind, trim = (rule, 0) if rule == "median" else rule
            g = robust_flat(list(mixed), one, kind, trim)
        elif rule[0] == "krum":
            g = krum_flat(list(mixed), one, 1, 1)[0]
        else:
            g = geomed_flat(list(mixed), one, 2, 1e-6, False)[0]
        assert torch.equal(sim.theta, before - 0.125 * g)
    assert pops >= 1
    # f is checked against every epoch's k: 2 * 3 >= 5 + a popped entry at the most
    sim = _sim(_stand_in(), robust_rule="median", buckets=5, nnm=3, **IND)
    with pytest.raises(ValueError, match="Invalid NNM f = 3 for k = 5"):
        sim.epoch()
    # off: the run is today's
    a, b = _sim(robust_rule="median", buckets=4, nnm=None, **IND), \
        _sim(robust_rule="median", buckets=4, **IND)
    for _ in range(3):
        assert a.epoch() == b.epoch()
    assert torch.equal(a.theta, b.theta) and a.nnm_log() == [] and a.last_mixed is None


def test_checkpoint_config_round_trip():
    """The config a checkpoint records holds nnm; a run that differs refuses the checkpoint; a
    checkpoint from before it reads as None.  (nnm needs a robust rule and so the independent-entry
    semantics, whose state no checkpoint holds yet: the recorded config is moved into a
    reference-semantics checkpoint, as tests/test_cpu_attack.py does for the attack.)"""
    from test_cpu_attack import IND, _sim
    a = _sim(robust_rule="median", buckets=4, nnm=2, **IND)
    assert a._stale_config()["nnm"] == 2
    with pytest.raises(NotImplementedError, match="independent"):
        a.checkpoint()
    plain = _sim(buckets=4)
    plain.epoch()
    ck = plain.checkpoint()
    c = ck["config"]
    assert c["nnm"] is None
    _sim(buckets=4).restore(ck)
    with pytest.raises(ValueError, match="nnm"):
        _sim(buckets=4).restore(dict(ck, config=dict(c, nnm=2)))
    old = {k: v for k, v in c.items() if k != "nnm"}
    assert len(old) == len(c) - 1
    back = _sim(buckets=4)
    back.restore(dict(ck, config=old))
    assert torch.equal(back.theta, plain.theta)
    import io
    buf = io.BytesIO()
    torch.save(dict(ck, config=dict(c, nnm=2)), buf)
    buf.seek(0)
    assert torch.load(buf, map_location="cpu", weights_only=True)["config"]["nnm"] == 2


def test_simulation_and_command_line_refusals():
    from flsim.sim import FLSimulation
    kw = dict(device="cpu", semantics="independent")
    with pytest.raises(NotImplementedError, match="nnm needs robust_rule"):
        FLSimulation(8, nnm=1, **kw)
    for bad in (-1, 1.0, 1.5, "1", True, (1,)):
        with pytest.raises(ValueError, match="Invalid NNM f"):
            FLSimulation(8, nnm=bad, robust_rule="median", **kw)
    sys.path.insert(0, PKG)
    try:
        import main
    finally:
        sys.path.remove(PKG)
    base = ['--n_workers', '8', '--delay', '2']
    assert main.parse(base).nnm is None and main.nnm_spec(main.parse(base)) is None
    args = main.parse(base + ['--robust_rule', 'median', '--nnm', '2'])
    assert main.nnm_spec(args) == 2
    assert main.nnm_spec(main.parse(base + ['--robust_rule', 'median', '--nnm', '0'])) == 0
    with pytest.raises(SystemExit, match="needs --robust_rule"):
        main.nnm_spec(main.parse(base + ['--nnm', '2']))
    with pytest.raises(SystemExit, match="F must be >= 0"):
        main.nnm_spec(main.parse(base + ['--robust_rule', 'median', '--nnm', '-1']))
    with pytest.raises(SystemExit):
        main.parse(base + ['--nnm', '1.5'])
