"""CPU: simulated Byzantine workers, the IPM and ALIE attacks on the bucketed entries.

The text (flsim/robust.py: attack_vector, attack_flat) against an independent numpy restatement; the
host twin flsim_attack_eval_host (csrc/attack.h: the element code the kernel runs, one host + device
function) against the text as numbers (tests/_attack.py) over honest-only, mixed and fully
Byzantine entries; the special inputs; alie_z; every refusal of flsim_attack_entries (they come
before any launch, so made-up device addresses are never read) and their order; check_attack /
parse_attack; the Attack object; FLSimulation on a CPU stand-in; and the property the feature exists
for: under IPM the plain mean over buckets points against the honest mean while every robust rule
still points along it.
"""
import ctypes

import numpy as np
import pytest
import torch

import _attack as A

KS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)
PS = (1, 2, 257)


@pytest.mark.parametrize("kind", A.KINDS)
def test_text_equals_a_numpy_restatement(kind):
    """Every operation is one IEEE operation on both sides: as numbers, no tolerance."""
    for k in (1, 2, 5, 16, 33):
        for P in (1, 257):
            ents, honest, byz = A.inputs(k, P)
            ref, counts, b = A.text(ents, honest, byz, kind, A.STRENGTH[kind])
            ref2, counts2, b2 = A.numpy_text(ents, honest, byz, kind, A.STRENGTH[kind])
            assert counts == counts2 == [h + c for h, c in zip(honest, byz)]
            assert A.mismatches(b2, b) == 0
            assert np.isfinite(b).all() and (b != 0).all()
            for j, (x, y) in enumerate(zip(ref, ref2)):
                assert A.mismatches(y, x) == 0, (k, P, j)


@pytest.mark.parametrize("kind", A.KINDS)
@pytest.mark.parametrize("k", KS)
def test_host_twin_equals_the_text(kind, k):
    """Honest-only, mixed and fully Byzantine entries (k >= 3: all three); an entry with byz == 0
    keeps its bits; the never-read entries hold the quiet-NaN pattern and b starts poisoned."""
    for P in PS:
        ents, honest, byz = A.inputs(k, P)
        if k >= 3:
            assert {(h > 0, c > 0) for h, c in zip(honest, byz)} == \
                {(True, True), (True, False), (False, True)}
        got, b = A.host_twin(ents, honest, byz, kind, A.STRENGTH[kind])
        ref, counts, bt = A.compare(got, b, ents, honest, byz, kind, A.STRENGTH[kind], (k, P))
        assert np.isfinite(bt).all()
        # b_out is optional
        got2, none = A.host_twin(ents, honest, byz, kind, A.STRENGTH[kind], b_out=False)
        assert none is None
        for x, y in zip(got, got2):
            assert np.array_equal(A.bits(x), A.bits(y))


@pytest.mark.parametrize("kind", A.KINDS)
def test_never_read_entries_do_not_matter(kind):
    """Two runs whose fully Byzantine entries start from different bytes give the same bits."""
    ents, honest, byz = A.inputs(9, 257)
    other = [e if h else A.poisoned(257, 0x7F800001) for e, h in zip(ents, honest)]
    zero = [e if h else np.zeros(257, np.float32) for e, h in zip(ents, honest)]
    a, ba = A.host_twin(ents, honest, byz, kind, A.STRENGTH[kind])
    for alt in (other, zero):
        c, bc = A.host_twin(alt, honest, byz, kind, A.STRENGTH[kind])
        assert np.array_equal(A.bits(ba), A.bits(bc))
        for x, y in zip(a, c):
            assert np.array_equal(A.bits(x), A.bits(y))


def test_one_honest_entry_has_sigma_zero():
    """kh = 1: the population variance is 0, so ALIE sends mu itself, whatever z."""
    rs = np.random.RandomState(3)
    e = (rs.standard_normal(257) * 3).astype(np.float32)
    ents, honest, byz = [e, A.poisoned(257)], [3, 0], [2, 1]
    mu = (e.astype(np.float64) / 3.0).astype(np.float32)
    for z in (0.0, 0.5, 7.0):
        got, b = A.host_twin(ents, honest, byz, "alie", z)
        A.compare(got, b, ents, honest, byz, "alie", z, z)
        assert np.array_equal(A.bits(b), A.bits(mu))
        assert np.array_equal(A.bits(got[1]), A.bits(mu * np.float32(1)))
        assert np.array_equal(A.bits(got[0]), A.bits(e + mu * np.float32(2)))
    # strength 0: IPM sends a zero, ALIE the mean
    ents, honest, byz = A.inputs(5, 257)
    got, b = A.host_twin(ents, honest, byz, "ipm", 0.0)
    A.compare(got, b, ents, honest, byz, "ipm", 0.0)
    assert (b == 0).all()


@pytest.mark.parametrize("kind", A.KINDS)
def test_nan_and_inf_in_an_honest_entry_propagate(kind):
    """No dead-entry logic: a NaN or an inf at an element of an honest entry makes b what the text
    makes it there (a NaN, or for IPM an inf of the text's sign), and leaves every other element
    alone."""
    for bad in (np.nan, np.inf, -np.inf):
        ents, honest, byz = A.inputs(8, 257, 1)
        j = next(i for i, h in enumerate(honest) if h and not byz[i])
        ents[j] = ents[j].copy()
        ents[j][3::7] = bad
        got, b = A.host_twin(ents, honest, byz, kind, A.STRENGTH[kind])
        ref, counts, bt = A.compare(got, b, ents, honest, byz, kind, A.STRENGTH[kind], bad)
        hit = np.zeros(257, bool)
        hit[3::7] = True
        assert not np.isfinite(bt[hit]).any() and np.isfinite(bt[~hit]).all()
        if kind == "alie" or np.isnan(bad):
            assert np.isnan(b[hit]).all()       # inf - inf in the variance
        else:
            assert (b[hit] == -bad).all()       # -eps * mu


def test_alie_z():
    from flsim.robust import alie_z
    # s = n // 2 + 1 - f, z = the standard normal quantile of (n - s) / n
    assert alie_z(4, 1) == 0.0                                    # 2 / 4
    assert abs(alie_z(10, 2) - 0.2533471031357997) < 1e-12        # 6 / 10
    assert abs(alie_z(8, 3) - 0.6744897501960817) < 1e-12         # 6 / 8
    assert abs(alie_z(20, 9) - 1.2815515655446004) < 1e-12        # 18 / 20
    assert alie_z(11, 3) > 0 and alie_z(64, 16) > alie_z(64, 8) > 0
    for n, f in ((10, 0), (10, 5), (10, 6), (10, -1), (1, 1), (0, 0)):
        with pytest.raises(ValueError, match="Invalid f"):
            alie_z(n, f)


# ---- refusals of the entry point (status 1, before any launch) -------------------------------------
F = {name: 0x1000000 * (i + 1) for i, name in enumerate(["b", "e0", "e1", "e2"])}
P = 64


def _call(kind="ipm", strength=1.0, honest=(2, 1, 0), byz=(0, 1, 2), ents=None, b_out=0, n=P,
          k=None, host=False):
    from flsim._lib import lib
    ents = [F["e0"], F["e1"], F["e2"]][:len(honest)] if ents is None else ents
    ents = list(ents) + [0] * (min(len(honest), 64) - len(ents))
    a, _ = A.c_attack(None, list(honest), list(byz), kind, strength, ptrs=ents, k=k)
    vp = ctypes.c_void_p
    if host:
        rc = lib().flsim_attack_eval_host(ctypes.byref(a), vp(b_out), n)
    else:
        rc = lib().flsim_attack_entries(ctypes.byref(a), vp(b_out), n, None)
    return rc, lib().flsim_last_error().decode()


N_FIELDS = 16       # the leading REFUSALS that are about flsim_attack's fields alone
REFUSALS = [
    (dict(kind=2), "Invalid attack kind 2"),
    (dict(kind=-1), "Invalid attack kind -1"),
    (dict(honest=(), byz=()), "k = 0 entries"),
    (dict(honest=(1,) * 65, byz=(1,) * 65), "k = 65 entries"),
    (dict(k=-3), "k = -3 entries"),
    (dict(strength=-0.5), "Invalid attack strength"),
    (dict(strength=float("nan")), "Invalid attack strength"),
    (dict(strength=float("inf")), "Invalid attack strength"),
    (dict(strength=float("-inf")), "Invalid attack strength"),
    (dict(honest=(2, -1, 0)), "Invalid honest count -1 of entry 1"),
    (dict(byz=(0, 1, -2)), "Invalid Byzantine count -2 of entry 2"),
    (dict(honest=(2, 0, 0), byz=(0, 0, 2)), "entry 1 holds no worker"),
    (dict(honest=(0, 0, 0), byz=(1, 1, 2)), "ValueError: no entry holds an honest worker"),
    (dict(honest=(0,), byz=(4,)), "the attacker has nothing to observe"),
    (dict(honest=(2, 1, 3), byz=(0, 0, 0)), "no entry holds a Byzantine worker"),
    (dict(honest=(1,), byz=(0,)), "no entry holds a Byzantine worker"),
    # the pointers
    (dict(ents=[F["e0"], 0, F["e2"]]), "null entry 1"),
    (dict(ents=[F["e0"], F["e1"], 0]), "null entry 2"),
    (dict(ents=[F["e0"] + 4, F["e1"], F["e2"]]), "entry 0 must be 16-byte aligned"),
    (dict(ents=[F["e0"], F["e1"], F["e2"] + 8]), "entry 2 must be 16-byte aligned"),
    (dict(b_out=F["b"] + 4), "b_out must be 16-byte aligned"),
    (dict(n=0), "P = 0 out of range"),
    (dict(n=-5), "out of range"),
    (dict(n=1 << 31), "out of range"),
    (dict(ents=[F["e0"], F["e0"], F["e2"]]), "entries 0 and 1 overlap"),
    (dict(ents=[F["e0"], F["e1"], F["e0"] + 4 * (P - 4)]), "entries 0 and 2 overlap"),
    (dict(ents=[F["e0"], F["e2"] - 4 * (P - 4), F["e2"]]), "entries 1 and 2 overlap"),
    (dict(b_out=F["e1"]), "entry 1 overlaps b_out"),
    (dict(b_out=F["e2"] + 4 * (P - 4)), "entry 2 overlaps b_out"),
]


@pytest.mark.parametrize("kw,message", REFUSALS, ids=[f"{i}-{m[:24]}" for i, (_, m) in
                                                       enumerate(REFUSALS)])
def test_entry_point_refusals(kw, message):
    for host in (False, True):          # the host twin refuses what the entry point refuses
        rc, err = _call(host=host, **kw)
        assert rc == 1, (rc, err)
        assert message in err, err


def test_refusal_order_tile_and_python_errors():
    """The fields come before the pointers (everything NULL and misaligned still names the kind,
    then k, the strength, the counts); among the pointers: NULL / alignment of the entries, b_out,
    P, overlap.  Adjacent buffers do not overlap.  The library's messages arrive as ValueError."""
    from flsim._lib import check, lib
    L = lib()
    bad = dict(ents=[0, 4, 0], b_out=4, n=0)
    order = [dict(kind=7, k=0, strength=-1.0, honest=(-1, 0, 0), byz=(0, 0, 0)),
             dict(k=70, strength=-1.0, honest=(-1, 0, 0), byz=(0, 0, 0)),
             dict(strength=-1.0, honest=(-1, 0, 0), byz=(0, 0, 0)),
             dict(honest=(-1, 0, 0), byz=(-1, 0, 0)),
             dict(honest=(1, 0, 0), byz=(-1, 0, 0)),
             dict(honest=(1, 0, 0), byz=(0, 0, 0)),
             dict(honest=(0, 0, 0), byz=(1, 1, 1)),
             dict(honest=(1, 1, 1), byz=(0, 0, 0)),
             dict()]
    names = ["attack kind", "k = 70", "attack strength", "honest count", "Byzantine count",
             "entry 1 holds no worker", "honest worker", "Byzantine worker", "null entry 0"]
    for kw, name in zip(order, names):
        rc, err = _call(**{**bad, **kw})
        assert rc == 1 and name in err, (name, err)
    rc, err = _call(ents=[F["e0"], F["e1"] + 4, F["e2"]], b_out=F["b"] + 4, n=0)
    assert "entry 1 must be" in err
    rc, err = _call(b_out=F["b"] + 4, n=0)
    assert "b_out must be" in err
    rc, err = _call(ents=[F["e0"], F["e0"], F["e2"]], n=0)
    assert "out of range" in err
    assert L.flsim_attack_entries(None, None, P, None) == 1
    assert "null attack" in L.flsim_last_error().decode()
    # adjacent buffers overlap nothing: the host twin then runs (host arrays this time)
    buf = np.zeros(4 * P, np.float32)
    assert buf.ctypes.data % 16 == 0
    ptrs = [buf.ctypes.data + 4 * P * i for i in range(3)]
    rc, err = _call(ents=ptrs, b_out=buf.ctypes.data + 12 * P, host=True)
    assert rc == 0, err
    for k in range(1, 65):
        E = L.flsim_attack_tile_elems(k)
        assert E >= 256 and E % 256 == 0
    assert L.flsim_attack_tile_elems(0) == 0 and L.flsim_attack_tile_elems(65) == 0
    with pytest.raises(ValueError, match="nothing to observe"):
        check(_call(honest=(0, 0, 0), byz=(1, 1, 2))[0])
    with pytest.raises(ValueError, match="attack strength"):
        check(_call(strength=-1.0)[0])


def test_check_attack_and_parse_attack():
    from flsim.robust import ATTACK_KINDS, attack_flat, check_attack, parse_attack
    assert ATTACK_KINDS == ("ipm", "alie")
    assert check_attack("ipm", 2, [1, 0], [0, 3]) == ("ipm", 2.0)
    for kw, message in REFUSALS[:N_FIELDS]:
        if "k" in kw or isinstance(kw.get("kind"), int):
            continue
        args = ("ipm", kw.get("strength", 1.0), kw.get("honest", (2, 1, 0)),
                kw.get("byz", (0, 1, 2)))
        with pytest.raises(ValueError, match=message.replace("ValueError: ", "")):
            check_attack(*args)
        with pytest.raises(ValueError):
            attack_flat([torch.zeros(4)] * len(args[2]), args[2], args[3], *args[:2])
    with pytest.raises(ValueError, match="attack kind"):
        check_attack("mimic", 1.0, [1], [1])
    with pytest.raises(ValueError, match="counts"):
        check_attack("ipm", 1.0, [1, 1], [1])
    assert parse_attack(None) is None and parse_attack("none") is None
    assert parse_attack("ipm") == ("ipm", 1.0) and parse_attack(("ipm", 4)) == ("ipm", 4.0)
    assert parse_attack("alie") == ("alie", None) and parse_attack(["alie", 0.5]) == ("alie", 0.5)
    assert parse_attack(("alie", None)) == ("alie", None) and parse_attack(("ipm",)) == ("ipm", 1.0)
    assert parse_attack(("ipm", 0)) == ("ipm", 0.0)
    for bad in ("mimic", ("ipm", -1), ("alie", float("nan")), ("alie", float("inf")),
                ("ipm", 1, 2), ("ipm", "x"), (), ("sign_flip", 1)):
        with pytest.raises(ValueError, match="attack"):
            parse_attack(bad)


def test_attack_object():
    from flsim.engine import Attack
    e = [torch.zeros(8) for _ in range(3)]
    a = Attack("alie", 0.5, e, [2, 1, 0], [0, 1, 2])
    c = a.c_struct()
    assert (c.kind, c.k, c.strength) == (1, 3, 0.5) and a.k == 3
    assert list(c.honest[:3]) == [2, 1, 0] and list(c.byz[:3]) == [0, 1, 2]
    assert c.entries[0] == e[0].data_ptr() and c.entries[2] == e[2].data_ptr()
    assert Attack("ipm", 1, e, [1] * 3, [1] * 3).c_struct().kind == 0
    assert Attack("mimic", 1, e, [1] * 3, [1] * 3).c_struct().kind == -1
    assert Attack("ipm", 1, [None] * 2, [1, 1], [2 ** 40, 1]).c_struct().byz[0] == -1
    with pytest.raises(ValueError, match="counts"):
        Attack("ipm", 1.0, e, [1, 2], [1, 2, 3])
    with pytest.raises(ValueError, match="counts"):
        Attack("ipm", 1.0, e, [1, 2, 3], [1, 2])
    with pytest.raises(ValueError, match="65 entries"):
        Attack("ipm", 1.0, [None] * 65, [1] * 65, [1] * 65)


# ---- FLSimulation on a CPU stand-in (the one of tests/test_cpu_geomed.py, with the attack) ---------
class StandInEngine:
    SIZES = [40, 24]
    STATS_PER_WORKER = 0

    def __init__(self):
        self.P = sum(self.SIZES)
        self.chunk_workers = 3
        self.acc = torch.zeros(self.P, dtype=torch.float64)
        self.ran = []           # every worker record a chunk was run for
        self.passes = 0

    @staticmethod
    def grad(P, i, k):
        return torch.arange(P, dtype=torch.float64).mul_(0.1 * (i + 1)).sin_() + k

    def begin_epoch(self, theta):
        self.acc.zero_()
        self.passes += 1

    def run_chunk(self, theta, pool, workers_dev, n_chunk, n_total, seed, dropout, loss_out,
                  backward=True):
        for j, (t, i, k, _) in enumerate(workers_dev.tolist()):
            self.ran.append((t, i))
            self.acc += self.grad(self.P, i, k)
            loss_out[j] = float(t + 0.001 * i)

    def end_epoch(self, S):
        S.copy_(self.acc.float())

    def aggregate_rule(self, S, rule, theta, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                       S_out=None, optim=None, **kw):
        if S_out is not None:
            S_out[:self.P].copy_(S)
        theta -= 0.125 * S / rule.k

    def attack_entries(self, attack, b_out=None):
        from flsim.robust import attack_flat
        sums = [e if h else None for e, h in zip(attack.entries, attack.honest)]
        out, counts, b = attack_flat(sums, attack.honest, attack.byz, attack.kind,
                                     attack.strength)
        for e, new, c in zip(attack.entries, out, attack.byz):
            if c:
                e.copy_(new)
        if b_out is not None:
            b_out.copy_(b)

    def robust_step(self, r, theta, m, v, step, optim=None, clip=None, **kw):
        from flsim.robust import robust_flat
        theta -= optim.lr * robust_flat(r.entries, r.counts, r.kind, r.trim)

    def krum_step(self, kr, theta, m, v, step, optim=None, clip=None, **kw):
        from flsim.robust import krum_flat
        g, d, s, sel = krum_flat(kr.entries, kr.counts, kr.f, kr.m)
        kr.sel = torch.tensor(sel, dtype=torch.int32)
        theta -= optim.lr * g

    def geomed_step(self, gm, theta, m, v, step, optim=None, clip=None, **kw):
        from flsim.robust import geomed_flat
        g, w, d2, obj = geomed_flat(gm.entries, gm.counts, gm.iters, gm.nu, gm.weighted)
        gm.w, gm.obj = torch.stack(w), torch.stack(obj) if obj else torch.zeros(0)
        theta -= optim.lr * g


def _sim(engine=None, **kw):
    from flsim.sim import FLSimulation
    eng = engine or StandInEngine()
    kw.setdefault("delay", 2)
    return FLSimulation(kw.pop("n", 12), device="cpu", engine=eng, device_pool=object(),
                        theta0=torch.zeros(eng.P), optimizer="sgd", lr=0.125, **kw)


IND = dict(semantics="independent")


def test_constructor_accepts_and_refuses():
    s = _sim(robust_rule="median", attack="ipm", n_byz=2, **IND)
    assert s.attack == ("ipm", 1.0) and s.n_byz == 2 and s.byz_placement == "spread"
    assert _sim(robust_rule="geomed", attack=("alie", 0.5), n_byz=1, byz_placement="block",
                **IND).attack == ("alie", 0.5)
    assert _sim(robust_rule=("trimmed_mean", 0), attack="alie", n_byz=10, **IND).attack == \
        ("alie", None)
    off = _sim(robust_rule="median", **IND)
    assert off.attack is None and off.n_byz == 0 and len(off.byz_workers) == 0
    assert off.attack_log() == []
    with pytest.raises(NotImplementedError, match="robust_rule"):
        _sim(attack="ipm", n_byz=2, **IND)
    with pytest.raises(NotImplementedError, match="robust_rule"):
        _sim(attack="ipm", n_byz=2)
    with pytest.raises(ValueError, match="without an attack"):
        _sim(robust_rule="median", n_byz=1, **IND)
    with pytest.raises(ValueError, match="n_byz = 0"):
        _sim(robust_rule="median", attack="ipm", **IND)
    with pytest.raises(ValueError, match="n_byz"):
        _sim(robust_rule="median", attack="ipm", n_byz=-1, **IND)
    # n = 12 with one slow worker: 11 delay-0 workers, one of which must stay honest
    with pytest.raises(ValueError, match="11 of 11 delay-0 workers"):
        _sim(robust_rule="median", attack="ipm", n_byz=11, **IND)
    with pytest.raises(ValueError, match="delay-0 workers"):
        _sim(robust_rule="median", attack="ipm", n_byz=12, **IND)
    with pytest.raises(ValueError, match="byz_placement"):
        _sim(robust_rule="median", attack="ipm", n_byz=2, byz_placement="random", **IND)
    with pytest.raises(ValueError, match="attack"):
        _sim(robust_rule="median", attack=("ipm", -1), n_byz=2, **IND)
    # everything robust_rule refuses stays refused
    for sem in ("reference", "torch1"):
        with pytest.raises(NotImplementedError, match="independent"):
            _sim(robust_rule="median", attack="ipm", n_byz=2, semantics=sem)
    with pytest.raises(NotImplementedError, match="distributed"):
        _sim(robust_rule="median", attack="ipm", n_byz=2, distributed=True, **IND)
    with pytest.raises(ValueError, match="buckets"):
        _sim(robust_rule="median", attack="ipm", n_byz=2, buckets=0, **IND)


def test_placements():
    """Among the delay-0 workers F[0 .. nF) in index order: "block" F[0 .. n_byz), "spread"
    F[((2q + 1) nF) // (2 n_byz)]; the slow worker is never Byzantine."""
    kw = dict(robust_rule="median", attack="ipm", **IND)
    s = _sim(n_byz=3, byz_placement="block", **kw)
    slow = [i for i in range(12) if s.delays[i] != 0]
    assert len(slow) == 1
    F = [i for i in range(12) if i not in slow]
    assert list(s.byz_workers) == F[:3]
    s = _sim(n_byz=3, **kw)
    assert list(s.byz_workers) == [F[(1 * 11) // 6], F[(3 * 11) // 6], F[(5 * 11) // 6]] == \
        [F[1], F[5], F[9]]
    s = _sim(n_byz=1, **kw)
    assert list(s.byz_workers) == [F[5]]
    s = _sim(n_byz=10, **kw)
    assert len(set(s.byz_workers)) == 10 and not set(s.byz_workers) & set(slow)
    # several slow workers: they are skipped
    d = np.zeros(12, np.int32)
    d[[0, 4]] = 3
    s = _sim(n_byz=4, delays=d, byz_placement="block", **kw)
    assert list(s.byz_workers) == [1, 2, 3, 5]


@pytest.mark.parametrize("placement", ("block", "spread"))
@pytest.mark.parametrize("rule", ("median", ("trimmed_mean", 0), ("krum", 0), ("geomed", 2)))
def test_epoch_under_attack(rule, placement):
    """n = 12, the last worker slow with delay 2, four buckets, three Byzantine workers.  The
    Byzantine workers never reach run_chunk and have no loss; the bucket boundaries are those of
    all eleven fast workers ("block": the first bucket is fully Byzantine and runs no pass);
    last_entries and the counts equal the text over the honest sums, theta follows the rule over
    the attacked entries, attack_log() holds Python values."""
    from flsim.robust import attack_flat, geomed_flat, krum_flat, robust_flat
    n, B, nb = 12, 4, 3
    eng = StandInEngine()
    sim = _sim(eng, n=n, robust_rule=rule, buckets=B, keep_entries=True, attack=("ipm", 2.5),
               n_byz=nb, byz_placement=placement, **IND)
    assert sim.last_attack is None and sim.attack_log() == []
    byzset = set(int(i) for i in sim.byz_workers)
    fast = [i for i in range(n) if sim.delays[i] == 0]
    bounds = [(j * len(fast)) // B for j in range(B + 1)]
    rs = np.random.RandomState(sim.seed)
    pops = 0
    for t in range(4):
        before = sim.theta.clone()
        ks = rs.randint(0, n, size=n)
        passes0 = eng.passes
        loss = sim.epoch()
        plan = sim.trace[-1]
        ents, counts = sim.last_entries
        b, honest, byz = sim.last_attack
        sums = []
        for j in range(B):
            ws = fast[bounds[j]:bounds[j + 1]]
            hs = [i for i in ws if i not in byzset]
            assert honest[j] == len(hs) and byz[j] == len(ws) - len(hs)
            sums.append(sum(eng.grad(eng.P, i, int(ks[i])) for i in hs).float() if hs else None)
        if placement == "block":
            assert honest == [0, 2, 3, 3] and byz == [2, 1, 0, 0]
        else:
            assert honest == [1, 3, 2, 2] and byz == [1, 0, 1, 1]
        # one pass per bucket with an honest worker, one for the slow worker's class
        slow = int(sum(bool(plan.computes[i]) for i in range(n) if sim.delays[i] != 0))
        assert eng.passes - passes0 == sum(h > 0 for h in honest) + slow
        for j in range(B):
            if sums[j] is None:
                assert sim.last_honest[j] is None
            else:
                assert torch.equal(sim.last_honest[j], sums[j])
        out, cnt, bt = attack_flat(sums, honest, byz, "ipm", 2.5)
        assert torch.equal(b, bt)
        assert counts[:B] == cnt == [h + c for h, c in zip(honest, byz)]
        assert len(ents) == B + bool(plan.stale)
        pops += bool(plan.stale)
        for j in range(B):
            assert torch.equal(ents[j], out[j]), (t, j)
        if plan.stale:          # the popped entry stays honest: the slow worker's own gradient
            assert counts[B] == 1 and not torch.equal(ents[B], out[0])
        if rule == "median" or rule[0] == "trimmed_mean":
            kind, trim = (rule, 0) if rule == "median" else rule
            g = robust_flat(ents, counts, kind, trim)
        elif rule[0] == "krum":
            g = krum_flat(ents, counts, 0, 1)[0]
        else:
            g = geomed_flat(ents, counts, 2, 1e-6, False)[0]
        assert torch.equal(sim.theta, before - 0.125 * g)
        # 'Avg. Loss' is the mean over the honest fast workers alone
        hf = [i for i in fast if i not in byzset]
        assert abs(loss - np.mean([np.float32(t + 0.001 * i) for i in hf])) < 1e-6
        assert sim.rank_worker_steps[-1] == len(hf) + slow
        assert sim.attack_log()[-1] == ("ipm", 2.5, nb)
        assert [type(x) for x in sim.attack_log()[-1]] == [str, float, int]
    assert pops >= 1 and len(sim.attack_log()) == 4
    assert not {i for _, i in eng.ran} & byzset
    assert {i for _, i in eng.ran} == set(range(n)) - byzset


def test_alie_default_strength_no_honest_worker_and_no_keep():
    """ALIE without a strength takes alie_z(fast workers, Byzantine among them) per epoch; without
    keep_entries nothing is kept; an epoch with Byzantine workers but no honest fast worker raises
    the library's ValueError; an epoch whose fast set holds no Byzantine worker runs no attack."""
    from flsim.robust import alie_z
    sim = _sim(robust_rule="median", buckets=4, attack="alie", n_byz=3, **IND)
    sim.epoch()
    assert sim.attack_log() == [("alie", alie_z(11, 3), 3)]
    assert sim.last_attack is None and sim.last_entries is None and sim.last_honest is None
    # 2 f < n does not hold: alie_z refuses the default
    sim = _sim(robust_rule="median", buckets=4, attack="alie", n_byz=6, **IND)
    with pytest.raises(ValueError, match="Invalid f"):
        sim.epoch()
    _sim(robust_rule="median", buckets=4, attack=("alie", 1.0), n_byz=6, **IND).epoch()
    # every fast worker of the epoch Byzantine: the attacker has nothing to observe
    sim = _sim(n=3, robust_rule="median", buckets=2, attack="ipm", n_byz=1, **IND)
    sim.byz_workers = np.asarray([0, 1], np.int64)
    with pytest.raises(ValueError, match="nothing to observe"):
        sim.epoch()
    # no Byzantine worker in the epoch's fast set: no attack, the entries are today's
    sim = _sim(robust_rule="median", buckets=4, keep_entries=True, attack="ipm", n_byz=3, **IND)
    ref = _sim(robust_rule="median", buckets=4, keep_entries=True, **IND)
    sim.byz_workers = np.zeros(0, np.int64)
    sim.epoch()
    ref.epoch()
    assert sim.attack_log() == [("ipm", None, 0)] and sim.last_attack is None
    assert torch.equal(sim.theta, ref.theta) and sim.last_entries[1] == ref.last_entries[1]


def test_attack_off_is_todays_run():
    """With no attack the epoch runs the same chunks in the same order as a run built without the
    new arguments."""
    a_eng, b_eng = StandInEngine(), StandInEngine()
    a = _sim(a_eng, robust_rule="geomed", buckets=4, attack=None, n_byz=0, **IND)
    b = _sim(b_eng, robust_rule="geomed", buckets=4, **IND)
    for _ in range(3):
        assert a.epoch() == b.epoch()
    assert a_eng.ran == b_eng.ran and a_eng.passes == b_eng.passes
    assert torch.equal(a.theta, b.theta) and a.attack_log() == []


def test_checkpoint_config_round_trip():
    """The config a checkpoint records holds attack, n_byz and byz_placement; a run that differs
    refuses the checkpoint; a checkpoint from before them reads as None, 0, "spread".  (An attack
    needs a robust rule and so the independent-entry semantics, whose state no checkpoint holds
    yet: the recorded config is moved into a reference-semantics checkpoint.)"""
    kw = dict(robust_rule="median", buckets=4, **IND)
    a = _sim(attack=("ipm", 4), n_byz=3, byz_placement="block", **kw)
    cfg = a._stale_config()
    assert (cfg["attack"], cfg["n_byz"], cfg["byz_placement"]) == (["ipm", 4.0], 3, "block")
    assert _sim(attack="alie", n_byz=2, **kw)._stale_config()["attack"] == ["alie", None]
    with pytest.raises(NotImplementedError, match="independent"):
        a.checkpoint()
    plain = _sim(buckets=4)
    plain.epoch()
    ck = plain.checkpoint()
    c = ck["config"]
    assert (c["attack"], c["n_byz"], c["byz_placement"]) == (None, 0, "spread")
    _sim(buckets=4).restore(ck)
    for key, val in (("attack", ["ipm", 4.0]), ("n_byz", 3), ("byz_placement", "block")):
        with pytest.raises(ValueError, match=key):
            _sim(buckets=4).restore(dict(ck, config=dict(c, **{key: val})))
    # an old-style config without the new keys
    old = {k: v for k, v in c.items() if k not in ("attack", "n_byz", "byz_placement")}
    assert len(old) == len(c) - 3
    back = _sim(buckets=4)
    back.restore(dict(ck, config=old))
    assert torch.equal(back.theta, plain.theta)
    # torch.save / weights_only load keeps the recorded values as they are
    import io
    buf = io.BytesIO()
    torch.save(dict(ck, config=dict(c, attack=cfg["attack"], n_byz=3)), buf)
    buf.seek(0)
    back = torch.load(buf, map_location="cpu", weights_only=True)
    assert back["config"]["attack"] == ["ipm", 4.0] and back["config"]["n_byz"] == 3


def test_main_arguments():
    import main
    a = main.parse([])
    assert main.attack_spec(a) is None and a.n_byz == 0 and a.byz_placement == "spread"
    a = main.parse(["--attack", "ipm"])
    assert main.attack_spec(a) == "ipm"
    a = main.parse(["--robust_rule", "geomed", "--attack", "ipm", "--attack_strength", "4",
                    "--n_byz", "16", "--byz_placement", "block", "--byz_f", "2"])
    assert main.attack_spec(a) == ("ipm", 4.0) and a.n_byz == 16 and a.byz_placement == "block"
    assert a.byz_f == 2                       # (Krum's tolerated count: another flag)
    a = main.parse(["--attack", "alie", "--n_byz", "3"])
    assert main.attack_spec(a) == "alie"
    from flsim.robust import parse_attack
    assert parse_attack(main.attack_spec(a)) == ("alie", None)
    with pytest.raises(SystemExit):
        main.parse(["--attack", "mimic"])
    with pytest.raises(SystemExit):
        main.parse(["--byz_placement", "random"])


# ---- the property the feature exists for ---------------------------------------------------------
def _property_inputs():
    """8 entries of one worker each: 6 honest, y_j = base + noise_j with |noise_j| < |base| / 2
    element-wise (every honest value has the sign of mu), and 2 fully Byzantine."""
    g = torch.Generator().manual_seed(2020)
    Pn = 257
    base = torch.randn(Pn, generator=g)
    base = torch.where(base.abs() < 0.05, torch.full_like(base, 0.05), base)
    noise = (torch.rand(6, Pn, generator=g) - 0.5) * 0.98 * base.abs()
    assert bool((noise.abs() < base.abs() / 2).all())
    sums = [(base + noise[j]).contiguous() for j in range(6)] + [None, None]
    return sums, [1] * 6 + [0, 0], [0] * 6 + [1, 1]


def test_ipm_defeats_the_mean_and_not_the_robust_rules():
    """IPM with eps = 4 and 2 Byzantine of 8 entries: the plain mean over the attacked entries
    ("trimmed_mean", 0) is (6 mu - 8 mu) / 8 = -mu / 4, a strictly negative inner product with mu;
    the median (per coordinate the two Byzantine values are the two extremes on one side, so the
    lower median of eight is an honest value), the trimmed mean (trim 2), Krum (f = 2) and the
    geometric median each keep a strictly positive one.  On the text and on the host twin."""
    from flsim.robust import attack_flat, attack_vector, geomed_flat, krum_flat, robust_flat
    sums, honest, byz = _property_inputs()
    mu = torch.stack(sums[:6]).double().mean(0)
    assert bool((torch.stack(sums[:6]).sign() == mu.sign().float()).all())
    text_entries, counts, b = attack_flat(sums, honest, byz, "ipm", 4.0)
    assert counts == [1] * 8
    assert torch.equal(b, attack_vector(sums, honest, "ipm", 4.0))
    np_ents = [s.numpy() if s is not None else A.poisoned(257) for s in sums]
    twin, tb = A.host_twin(np_ents, honest, byz, "ipm", 4.0)
    A.compare(twin, tb, np_ents, honest, byz, "ipm", 4.0)
    for entries in (text_entries, [torch.from_numpy(e) for e in twin]):
        def dot(g):
            return float((g.double() * mu).sum())
        mean = robust_flat(entries, counts, "trimmed_mean", 0)
        assert dot(mean) < 0
        np.testing.assert_allclose(mean.double().numpy(), (-mu / 4).numpy(), rtol=1e-5,
                                   atol=1e-7)
        assert dot(robust_flat(entries, counts, "median", 0)) > 0
        assert dot(robust_flat(entries, counts, "trimmed_mean", 2)) > 0
        g, d, s, sel = krum_flat(entries, counts, 2, 1)
        assert dot(g) > 0 and sel[0] < 6
        assert dot(geomed_flat(entries, counts, 3, 1e-6, False)[0]) > 0
        # coordinate by coordinate the median is an honest value
        med = robust_flat(entries, counts, "median", 0)
        assert bool((med.sign() == mu.sign().float()).all())
