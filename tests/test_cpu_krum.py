"""CPU: Krum and Multi-Krum over bucket means.

The host twin flsim_krum_eval_host sums every distance in element order and then runs the score /
selection code the finish kernel runs (csrc/krum.h, one host + device function); here it is compared
with the rule text (flsim/robust.py: krum_select, _krum) within the derived bound of tests/_krum.py
(dist, score) and exactly (sel, g).  Then every refusal of flsim_krum_optim_step (they come before
any launch, so made-up device addresses are never read), check / parse_rule, and FLSimulation on a
CPU stand-in.
"""
import ctypes

import numpy as np
import pytest
import torch

import _krum as K

PS = (1, 5, 255, 257, 1027)


@pytest.mark.parametrize("k", K.KS)
def test_host_twin_equals_the_text(k):
    """The whole (f, m) grid at P in {1, 5, 255, 257, 1027}: dist and score within the bound, the
    selection equal, g bit for bit; the text's scores at the cut are >= 1000 bounds apart."""
    for P in PS:
        ent, cnt = K.inputs(k, P)
        assert set(cnt) <= {1, 2, 3, 4}
        for f, m in K.grid(k):
            g, d, s, sel = K.text(ent, cnt, f, m)
            assert K.score_gap(s, m) >= 1000 * K.dist_bound(P), (P, f, m)    # input condition
            g2, d2, s2, sel2 = K.host_twin(ent, cnt, f, m)
            assert K.outside(d2, d, K.dist_bound(P)) == 0, (P, f, m)
            assert K.outside(s2, s, 2 * K.dist_bound(P)) == 0, (P, f, m)
            assert sel2 == sel and len(sel) == m and sel == sorted(sel), (P, f, m)
            assert K.g_mismatches(g2, g) == 0, (P, f, m)
            assert np.array_equal(d2, d2.T) and (np.diag(d2) == 0).all()


def test_exact_tie_lowest_index_wins():
    """k = 3, f = 0: a score is the distance to the nearest neighbour, so both ends of the closest
    pair tie exactly (the matrix is symmetric bitwise); the lower index is selected."""
    for seed in range(6):
        ent, cnt = K.inputs(3, 257, seed)
        ent = [ent[j] for j in np.random.RandomState(seed).permutation(3)]
        g, d, s, sel = K.text(ent, cnt, 0, 1)
        g2, d2, s2, sel2 = K.host_twin(ent, cnt, 0, 1)
        assert np.array_equal(d2.view(np.uint64), d2.T.copy().view(np.uint64))
        off = d2 + np.diag([np.inf] * 3)
        i, j = sorted(np.unravel_index(np.argmin(off), off.shape))
        assert s2[i] == s2[j] and s2[i] == off[i, j] and s2[3 - i - j] > s2[i]
        assert sel2 == [int(i)] == sel
        assert K.g_mismatches(g2, g) == 0
        _, _, _, sel_m2 = K.host_twin(ent, cnt, 0, 2)
        assert sel_m2 == [int(i), int(j)]


@pytest.mark.parametrize("k", (5, 9, 16, 33))
def test_special_inputs(k):
    P = 255
    f = 1
    off = ~np.eye(k, dtype=bool)
    for bad in (np.nan, np.inf, -np.inf):
        for m in (1, k - f):
            ent, cnt = K.inputs(k, P, 1)
            j = k // 2
            ent[j] = ent[j].copy()
            ent[j][3::7] = bad
            g, d, s, sel = K.text(ent, cnt, f, m)
            g2, d2, s2, sel2 = K.host_twin(ent, cnt, f, m)
            assert j not in sel2 and sel2 == sel, (bad, m)
            assert np.isinf(d2[j][off[j]]).all() and np.isinf(s2[j]) and d2[j, j] == 0
            assert K.outside(d2[off], d[off], K.dist_bound(P)) == 0
            assert K.outside(s2, s, 2 * K.dist_bound(P)) == 0
            assert np.isfinite(g2).all() and K.g_mismatches(g2, g) == 0
    # every entry NaN: every distance +inf, every score ties, the lowest indices are taken
    ent = [np.full(P, np.nan, np.float32) for _ in range(k)]
    for m in (1, 3):
        g, d, s, sel = K.text(ent, [1] * k, f, m)
        g2, d2, s2, sel2 = K.host_twin(ent, [1] * k, f, m)
        assert sel2 == list(range(m)) == sel and np.isnan(g2).all()
        assert np.isinf(d2[off]).all() and np.isinf(s2).all()
    # a duplicate pointer: distance exactly 0, and the pair is each other's nearest neighbour
    ent, cnt = K.inputs(k, P, 2)
    r, keep = K.c_krum(ent, cnt, f, 1)
    r.entries[1] = r.entries[0]
    r.count[1] = r.count[0]
    from flsim._lib import check, lib
    d2, s2, sel2 = np.zeros((k, k)), np.zeros(k), np.zeros(1, np.int32)
    vp = ctypes.c_void_p
    check(lib().flsim_krum_eval_host(ctypes.byref(r), P, d2.ctypes.data_as(vp),
                                     s2.ctypes.data_as(vp), sel2.ctypes.data_as(vp), None))
    assert d2[0, 1] == 0.0 and d2[1, 0] == 0.0 and (d2[0, 2:] > 0).all()
    dup = [ent[0]] + [ent[0]] + ent[2:]
    _, d, s, sel = K.text(dup, [cnt[0], cnt[0]] + cnt[2:], f, 1)
    assert K.outside(d2, d, K.dist_bound(P)) == 0 and [int(sel2[0])] == sel
    # a NULL entry is all zero
    ent, cnt = K.inputs(k, P, 3)
    ent[2] = None
    g, d, s, sel = K.text(ent, cnt, f, 2)
    g2, d2, s2, sel2 = K.host_twin(ent, cnt, f, 2)
    assert K.outside(d2, d, K.dist_bound(P)) == 0 and sel2 == sel
    assert K.g_mismatches(g2, g) == 0


@pytest.mark.parametrize("k,f", [(5, 1), (9, 3), (16, 2), (64, 30)])
def test_outliers_are_never_selected(k, f):
    """An honest cluster (a common mean plus small noise) and f far outliers: no m selects an
    outlier, and Multi-Krum with m = k - f selects exactly the honest set."""
    P = 257
    rs = np.random.RandomState(40 + k)
    mean = rs.standard_normal(P).astype(np.float32)
    cnt = [int(c) for c in rs.randint(1, 5, k)]
    outl = sorted(int(j) for j in rs.permutation(k)[:f])
    ent = []
    for j in range(k):
        x = mean + 0.05 * rs.standard_normal(P).astype(np.float32)
        if j in outl:
            x = x + (10.0 + j) * rs.choice([-1.0, 1.0], P).astype(np.float32)
        ent.append(np.ascontiguousarray(x * np.float32(cnt[j])))
    honest = [j for j in range(k) if j not in outl]
    for m in sorted({1, 2, k - f}):
        g, d, s, sel = K.text(ent, cnt, f, m)
        g2, d2, s2, sel2 = K.host_twin(ent, cnt, f, m)
        assert sel2 == sel and not set(sel2) & set(outl), (m, sel2, outl)
        assert K.g_mismatches(g2, g) == 0
    assert sel2 == honest


def test_rules_over_the_flattened_model():
    """flsim/robust.py itself: the list forms are what Agg(rule) calls; the distances are over all
    tensors together, the input shapes are kept; Krum returns one of the updates."""
    from FL.agents import Agg
    from flsim.robust import check, krum_flat, krum_rule, multi_krum_rule
    gen = torch.Generator().manual_seed(5)
    ups = [[torch.randn(4, 3, generator=gen), torch.randn(5, generator=gen)] for _ in range(7)]
    ups[3] = [u + 50 for u in ups[3]]
    one = Agg(lambda u: krum_rule(u, 1)).rule(ups)
    flat = [torch.cat([t.reshape(-1) for t in u]) for u in ups]
    g, d, s, sel = krum_flat(flat, [1] * 7, 1, 1)
    assert sel != [3] and all(torch.equal(a, b) for a, b in zip(one, ups[sel[0]]))
    assert [t.shape for t in one] == [t.shape for t in ups[0]]
    many = Agg(lambda u: multi_krum_rule(u, 1, 3)).rule(ups)
    g3, _, _, sel3 = krum_flat(flat, [1] * 7, 1, 3)
    assert torch.equal(torch.cat([t.reshape(-1) for t in many]), g3) and 3 not in sel3
    acc = flat[sel3[0]].clone()
    for j in sel3[1:]:
        acc += flat[j]
    assert torch.equal(g3, acc / 3)
    assert check("multi_krum", (1, 3), 7) == (1, 3) and check("krum", (0, 1), 3) == (0, 1)
    with pytest.raises(IndexError):
        krum_rule([], 0)
    for f, m, k, what in ((-1, 1, 9, "Invalid f"), (1, 1, 4, "Invalid f"), (3, 1, 8, "Invalid f"),
                          (1, 0, 5, "Invalid m"), (1, 5, 5, "Invalid m"), (0, 4, 3, "Invalid m")):
        with pytest.raises(ValueError, match=what):
            check("multi_krum", (f, m), k)
    with pytest.raises(ValueError, match="Invalid f"):
        multi_krum_rule(ups, 3, 1)


def test_parse_rule():
    from flsim.robust import parse_rule
    assert parse_rule(("krum", 2)) == ("krum", 2, 1)
    assert parse_rule(["multi_krum", 1, 3]) == ("multi_krum", 1, 3)
    assert parse_rule("median") == ("median", 0) and parse_rule(None) is None
    for bad in ("krum", "multi_krum", ("krum",), ("krum", 1, 2), ("multi_krum", 1),
                ("multi_krum", 1, 2, 3), ("krum", -1), ("multi_krum", 0, 0)):
        with pytest.raises(ValueError, match="robust_rule"):
            parse_rule(bad)


# ---- refusals of the entry point (status 1, before any launch) -------------------------------------
F = {name: 0x1000000 * (i + 1) for i, name in enumerate(
    ["p", "m", "v", "g", "G", "D", "O", "e0", "e1", "e2", "sp", "sd", "ss", "sl"])}
P = 64


def _optim(**kw):
    from flsim.engine import Optim
    return Optim(**kw).c_struct()


def _clip(max_norm=1.0, G=None, partials=None, n=1 << 20, out=None):
    from flsim._lib import FlsimClip
    c = FlsimClip()
    c.max_norm = max_norm
    c.G = F["G"] if G is None else G
    c.partials = F["D"] if partials is None else partials
    c.n_partials = n
    c.out = F["O"] if out is None else out
    return c


def _scratch(partials=None, n=1 << 20, dist=None, score=None, sel=None):
    from flsim._lib import FlsimKrumScratch
    s = FlsimKrumScratch()
    s.partials = F["sp"] if partials is None else partials
    s.n_partials = n
    s.dist = F["sd"] if dist is None else dist
    s.score = F["ss"] if score is None else score
    s.sel = F["sl"] if sel is None else sel
    return s


def _call(f=0, m=1, counts=(1, 3, 4), ents=None, scratch="default", clip=None, g_out=0, p=None,
          mm=0, v=0, n=P, step=1, optim="sgd"):
    from flsim._lib import lib
    ents = [F["e0"], F["e1"], F["e2"]][:len(counts)] if ents is None else ents
    ents = list(ents) + [0] * (min(len(counts), 64) - len(ents))
    r, _ = K.c_krum(None, list(counts), f, m, ptrs=ents)
    r.k = len(counts)
    s = _scratch() if scratch == "default" else scratch
    o = None if optim is None else (optim if not isinstance(optim, str) else
                                     _optim(kind=optim, lr=0.1))
    vp = ctypes.c_void_p
    rc = lib().flsim_krum_optim_step(
        ctypes.byref(r), None if s is None else ctypes.byref(s),
        None if clip is None else ctypes.byref(clip), vp(g_out), vp(F["p"] if p is None else p),
        vp(mm), vp(v), n, step, None if o is None else ctypes.byref(o), None)
    return rc, lib().flsim_last_error().decode()


REFUSALS = [
    (dict(counts=()), "k = 0 entries"),
    (dict(counts=(1, 1)), "k = 2 entries"),
    (dict(counts=(1,) * 65), "k = 65 entries"),
    (dict(f=-1), "Invalid f = -1"),
    (dict(f=1), "Invalid f = 1 for k = 3"),
    (dict(f=1, counts=(1,) * 4), "Invalid f = 1 for k = 4"),
    (dict(f=31, counts=(1,) * 64), "Invalid f = 31 for k = 64"),
    (dict(m=0), "Invalid m = 0"),
    (dict(m=-2), "Invalid m = -2"),
    (dict(m=4), "Invalid m = 4 for k = 3"),
    (dict(f=1, m=5, counts=(1,) * 5), "Invalid m = 5 for k = 5 entries and f = 1"),
    (dict(counts=(1, 0, 3)), "Invalid count 0 of entry 1"),
    (dict(counts=(1, 3, -5)), "Invalid count -5 of entry 2"),
    # what check_optim / check_clip refuse, still before any pointer (p = NULL everywhere)
    (dict(optim=_optim(kind="sgd", lr=-1.0), p=0, scratch=None), "Invalid learning rate"),
    (dict(optim=_optim(kind="sgd", lr=0.1, momentum=-0.5), p=0), "Invalid momentum"),
    (dict(optim=_optim(kind="adam", weight_decay=-1.0), p=0), "Invalid weight_decay"),
    (dict(optim=_optim(kind="yogi", betas=(1.0, 0.9)), p=0), "Invalid beta parameter at index 0"),
    (dict(optim=_optim(kind="adagrad", lr_decay=-1.0), p=0), "Invalid lr_decay"),
    (dict(clip=_clip(max_norm=0.0), p=0), "max_norm"),
    (dict(clip=_clip(max_norm=float("nan")), p=0, scratch=None), "max_norm"),
    (dict(optim=None), "null optimizer"),
    (dict(optim=None, g_out=F["g"], clip=_clip()), "null optimizer"),
    # the pointers
    (dict(p=0), "null pointer"),
    (dict(optim="adam", mm=F["m"]), "null pointer"),
    (dict(optim=_optim(kind="sgd", lr=0.1, momentum=0.9)), "null pointer"),
    (dict(p=F["p"] + 4), "16-byte aligned"),
    (dict(g_out=F["g"] + 8), "16-byte aligned"),
    (dict(n=0), "out of range"),
    (dict(n=1 << 31), "out of range"),
    (dict(step=0), "step must be >= 1"),
    (dict(g_out=F["p"]), "overlap each other"),
    (dict(scratch=None), "null Krum scratch"),
    (dict(scratch=_scratch(partials=0)), "null Krum scratch"),
    (dict(scratch=_scratch(dist=0)), "null Krum scratch"),
    (dict(scratch=_scratch(score=0)), "null Krum scratch"),
    (dict(scratch=_scratch(sel=0)), "null Krum scratch"),
    (dict(scratch=_scratch(partials=F["sp"] + 8)), "Krum scratch must be 16-byte aligned"),
    (dict(scratch=_scratch(dist=F["sd"] + 8)), "Krum scratch must be 16-byte aligned"),
    (dict(scratch=_scratch(score=F["ss"] + 8)), "Krum scratch must be 16-byte aligned"),
    (dict(scratch=_scratch(sel=F["sl"] + 4)), "Krum scratch must be 16-byte aligned"),
    (dict(scratch=_scratch(n=15)), "Krum n_partials = 15, this step writes 16"),
    (dict(scratch=_scratch(dist=F["sp"] + 64)), "Krum scratch buffers overlap"),
    (dict(scratch=_scratch(sel=F["p"] + 16)), "Krum scratch overlaps p/m/v/g_out"),
    (dict(scratch=_scratch(score=F["G"] + 16), clip=_clip()), "Krum scratch overlaps clip G"),
    (dict(ents=[F["e0"], F["e1"] + 2, F["e2"]]), "entry 1 must be 4-byte aligned"),
    (dict(ents=[F["e0"], F["p"], F["e2"]]), "entry 1 overlaps"),
    (dict(ents=[F["p"] + 4 * (P - 1), F["e1"], F["e2"]]), "entry 0 overlaps"),
    (dict(ents=[F["e0"], F["e1"], F["p"] - 4 * (P - 1)]), "entry 2 overlaps"),
    (dict(optim="adam", mm=F["m"], v=F["v"], ents=[F["m"] + 16, F["e1"], F["e2"]]),
     "entry 0 overlaps"),
    (dict(optim="adam", mm=F["m"], v=F["v"], ents=[F["e0"], F["v"], F["e2"]]), "entry 1 overlaps"),
    (dict(g_out=F["g"], ents=[F["e0"], F["e1"], F["g"] + 32]), "entry 2 overlaps"),
    (dict(clip=_clip(), ents=[F["G"] + 4, F["e1"], F["e2"]]), "entry 0 overlaps clip G"),
    (dict(ents=[F["sp"] + 8, F["e1"], F["e2"]]), "entry 0 overlaps the Krum scratch"),
    (dict(ents=[F["e0"], F["sd"] - 4 * (P - 1), F["e2"]]), "entry 1 overlaps the Krum scratch"),
    (dict(ents=[F["e0"], F["e1"], F["ss"] + 16]), "entry 2 overlaps the Krum scratch"),
    (dict(ents=[F["e0"], F["e1"], F["sl"]]), "entry 2 overlaps the Krum scratch"),
    (dict(clip=_clip(G=0)), "null clip buffer"),
    (dict(clip=_clip(G=F["G"] + 4)), "16-byte aligned"),
    (dict(clip=_clip(G=F["p"] + 16)), "clip G overlaps"),
    (dict(clip=_clip(n=0)), "n_partials"),
]


@pytest.mark.parametrize("kw,message", REFUSALS, ids=[f"{i}-{m[:24]}" for i, (_, m) in
                                                       enumerate(REFUSALS)])
def test_entry_point_refusals(kw, message):
    rc, err = _call(**kw)
    assert rc == 1, (rc, err)
    assert message in err, err


def test_refusal_order_partials_and_host_twin_refusals():
    """Hyper-parameters come before pointers (everything NULL still names f); adjacent buffers do
    not overlap, so the next check is reached; flsim_krum_partials is what the step asks for."""
    from flsim._lib import lib
    L = lib()
    rc, err = _call(f=5, p=0, ents=[0, 0, 0], scratch=None)
    assert rc == 1 and "Invalid f = 5" in err
    rc, err = _call(ents=[F["p"] - 4 * P, F["p"] + 4 * P, F["e2"]], clip=_clip(n=0))
    assert rc == 1 and "n_partials" in err
    for k in (3, 4, 5, 8, 9, 16, 17, 32, 33, 64):
        E = L.flsim_krum_tile_elems(k)
        assert E >= 4 and E % 4 == 0
        for n in (1, E - 1, E, E + 1, 3 * E + 5, 5596090, (1 << 31) - 1):
            need = L.flsim_krum_partials(n, k)
            assert need >= k * (k - 1) // 2 and need % 16 == 0
            rc, err = _call(counts=(1,) * k, n=n, scratch=_scratch(n=need - 1))
            assert rc == 1 and f"this step writes {need}" in err, err
        assert L.flsim_krum_partials(E, k) < L.flsim_krum_partials(E + 1, k)
    assert L.flsim_krum_partials(0, 8) == 0 and L.flsim_krum_partials(8, 65) == 0
    assert L.flsim_krum_tile_elems(0) == 0
    vp = ctypes.c_void_p
    d, s, sel = np.zeros(64 * 64), np.zeros(64), np.zeros(64, np.int32)
    a = (d.ctypes.data_as(vp), s.ctypes.data_as(vp), sel.ctypes.data_as(vp), None)
    for kw, message in REFUSALS[:13]:
        counts = list(kw.get("counts", (1, 3, 4)))
        ent = [np.ones(4, np.float32) for _ in counts[:64]]
        r, keep = K.c_krum(ent, counts, kw.get("f", 0), kw.get("m", 1))
        r.k = len(counts)
        assert L.flsim_krum_eval_host(ctypes.byref(r), 4, *a) == 1
        assert message in L.flsim_last_error().decode()
    r, keep = K.c_krum([np.ones(4, np.float32)] * 3, [1] * 3, 0, 1)
    assert L.flsim_krum_eval_host(ctypes.byref(r), 0, *a) == 1
    assert L.flsim_krum_eval_host(ctypes.byref(r), 4, None, a[1], a[2], None) == 1
    assert L.flsim_krum_eval_host(None, 4, *a) == 1
    assert L.flsim_krum_eval_host(ctypes.byref(r), 4, *a) == 0


def test_krum_object():
    from flsim.engine import Krum
    e = [torch.zeros(8) for _ in range(3)]
    r = Krum(0, 2, e, [1, 3, 4])
    c = r.c_struct()
    assert (c.f, c.m, c.k) == (0, 2, 3) and list(c.count[:3]) == [1, 3, 4]
    assert c.entries[0] == e[0].data_ptr() and r.k == 3
    assert Krum(0, 1, [None] * 3, [4] * 3).c_struct().entries[0] is None
    with pytest.raises(ValueError, match="counts"):
        Krum(0, 1, e, [1, 2])
    with pytest.raises(ValueError, match="65 entries"):
        Krum(0, 1, [None] * 65, [1] * 65)


# ---- FLSimulation on a CPU stand-in (mirrors the one of tests/test_cpu_robust.py) ----------------------
class StandInEngine:
    SIZES = [40, 24]
    STATS_PER_WORKER = 0

    def __init__(self):
        self.P = sum(self.SIZES)
        self.chunk_workers = 3
        self.acc = torch.zeros(self.P, dtype=torch.float64)

    def begin_epoch(self, theta):
        self.acc.zero_()

    def run_chunk(self, theta, pool, workers_dev, n_chunk, n_total, seed, dropout, loss_out,
                  backward=True):
        for j, (t, i, k, _) in enumerate(workers_dev.tolist()):
            self.acc += torch.arange(self.P, dtype=torch.float64).mul_(0.1 * (i + 1)).sin_() + k
            loss_out[j] = float(t + 0.001 * i)

    def end_epoch(self, S):
        S.copy_(self.acc.float())

    def aggregate_rule(self, S, rule, theta, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                       S_out=None, optim=None, **kw):
        if S_out is not None:
            S_out[:self.P].copy_(S)
        theta -= 0.125 * S / rule.k

    def robust_step(self, robust, theta, m, v, step, optim=None, clip=None, **kw):
        from flsim.robust import robust_flat
        theta -= optim.lr * robust_flat(robust.entries, robust.counts, robust.kind, robust.trim)

    def krum_step(self, krum, theta, m, v, step, optim=None, clip=None, **kw):
        from flsim.robust import krum_flat
        g, d, s, sel = krum_flat(krum.entries, krum.counts, krum.f, krum.m)
        krum.dist, krum.score, krum.sel = d, s, torch.tensor(sel, dtype=torch.int32)
        theta -= optim.lr * g


class BNStandIn(StandInEngine):
    STATS_PER_WORKER = 8


def _sim(engine=None, **kw):
    from flsim.sim import FLSimulation
    eng = engine or StandInEngine()
    kw.setdefault("delay", 2)
    return FLSimulation(kw.pop("n", 6), device="cpu", engine=eng, device_pool=object(),
                        theta0=torch.zeros(eng.P), optimizer="sgd", lr=0.125, **kw)


def test_constructor_accepts_and_refuses():
    ind = dict(semantics="independent")
    assert _sim(robust_rule=("krum", 1), **ind).robust == ("krum", 1, 1)
    assert _sim(robust_rule=("multi_krum", 1, 3), **ind).robust == ("multi_krum", 1, 3)
    for bad in ("krum", "multi_krum", ("multi_krum", 1), ("krum", -1)):
        with pytest.raises(ValueError, match="robust_rule"):
            _sim(robust_rule=bad, **ind)
    rule = ("krum", 0)
    for sem in ("reference", "torch1"):
        with pytest.raises(NotImplementedError, match="independent"):
            _sim(robust_rule=rule, semantics=sem)
    with pytest.raises(NotImplementedError, match="distributed"):
        _sim(robust_rule=rule, distributed=True, **ind)
    with pytest.raises(NotImplementedError, match="staleness discount"):
        _sim(robust_rule=rule, stale_weight=("poly", 0.5), **ind)
    with pytest.raises(NotImplementedError, match="delay compensation"):
        _sim(robust_rule=rule, delay_comp=0.5, **ind)
    with pytest.raises(NotImplementedError, match="batch_size"):
        _sim(robust_rule=rule, batch_size=64, **ind)
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        _sim(BNStandIn(), robust_rule=rule, **ind)
    with pytest.raises(ValueError, match="buckets"):
        _sim(robust_rule=rule, buckets=0, **ind)


def test_epoch_entries_selection_and_refusals():
    """n = 6, worker 5 slow with delay 2, four buckets: the entries are the buckets of the five fast
    workers, then a popped class slot; last_selected and theta follow the text over last_entries;
    an f, m or k that the epoch's entry count does not allow is refused."""
    from flsim.robust import krum_flat
    sim = _sim(robust_rule=("multi_krum", 0, 2), buckets=4, keep_entries=True,
               semantics="independent")
    assert sim.last_selected is None
    pops = 0
    for t in range(5):
        before = sim.theta.clone()
        sim.epoch()
        ents, counts = sim.last_entries
        plan = sim.trace[-1]
        assert counts[:4] == [1, 1, 1, 2] and len(ents) == 4 + bool(plan.stale)
        pops += bool(plan.stale)
        g, d, s, sel = krum_flat(ents, counts, 0, 2)
        assert sim.last_selected == sel and all(type(j) is int for j in sim.last_selected)
        assert torch.equal(sim.theta, before - 0.125 * g)
    assert pops >= 1
    ind = dict(semantics="independent")
    with pytest.raises(ValueError, match="Invalid f = 1 for k = 4"):
        _sim(robust_rule=("krum", 1), buckets=4, **ind).epoch()
    with pytest.raises(ValueError, match="Invalid m = 5 for k = 4"):
        _sim(robust_rule=("multi_krum", 0, 5), buckets=4, **ind).epoch()
    with pytest.raises(ValueError, match="k = 2 entries"):
        _sim(robust_rule=("krum", 0), buckets=2, **ind).epoch()
    big = _sim(n=70, robust_rule=("krum", 0), buckets=65, **ind)
    with pytest.raises(ValueError, match="65 entries"):
        big.epoch()
    # without keep_entries nothing is read back
    quiet = _sim(robust_rule=("krum", 0), buckets=4, **ind)
    quiet.epoch()
    assert quiet.last_selected is None and quiet.last_entries is None


def test_checkpoint_config_round_trip():
    """The config a checkpoint records holds the rule as (kind, f, m); a run whose rule differs
    refuses the checkpoint.  (A robust run needs the independent-entry semantics, whose state no
    checkpoint holds yet: the recorded config is moved into a reference-semantics checkpoint.)"""
    kw = dict(buckets=4, semantics="independent")
    a = _sim(robust_rule=("krum", 2), **kw)
    assert a._stale_config()["robust_rule"] == ["krum", 2, 1]
    cfg = _sim(robust_rule=("multi_krum", 1, 3), **kw)._stale_config()
    assert cfg["robust_rule"] == ["multi_krum", 1, 3] and cfg["buckets"] == 4
    with pytest.raises(NotImplementedError, match="independent"):
        a.checkpoint()
    plain = _sim(buckets=4)
    plain.epoch()
    ck = plain.checkpoint()
    assert ck["config"]["robust_rule"] is None
    _sim(buckets=4).restore(ck)
    for rule in (["krum", 2, 1], ["multi_krum", 1, 3]):
        with pytest.raises(ValueError, match="robust_rule"):
            _sim(buckets=4).restore(dict(ck, config=dict(ck["config"], robust_rule=rule)))
    # torch.save / weights_only load keeps the recorded list as it is
    import io
    buf = io.BytesIO()
    torch.save(dict(ck, config=dict(ck["config"], robust_rule=cfg["robust_rule"])), buf)
    buf.seek(0)
    back = torch.load(buf, map_location="cpu", weights_only=True)
    assert back["config"]["robust_rule"] == ["multi_krum", 1, 3]
