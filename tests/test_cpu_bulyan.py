"""CPU: Bulyan over bucket means.

The host twin flsim_bulyan_eval_host sums every distance in element order, then runs the selection
code the finish kernel runs and the window / sum code the apply kernel runs (csrc/bulyan.h, host +
device functions); here it is compared with the rule text (flsim/robust.py: bulyan_order,
_bulyan_coord) stage by stage at its own outputs (tests/_bulyan.py), with no tolerance after the
distances.  Then every refusal of flsim_bulyan_optim_step (they come before any launch, so made-up
device addresses are never read), check_bulyan / parse_rule, the ABI, and FLSimulation on a CPU
stand-in.
"""
import ctypes

import numpy as np
import pytest
import torch

import _bulyan as B
import _krum as K

def _ps(k):
    """The grid's P: 1, 257, E + 1 and 4099, E the distance launch's tile at k entries."""
    from flsim._lib import lib
    return (1, 257, int(lib().flsim_krum_tile_elems(k)) + 1, 4099)


@pytest.mark.parametrize("k", B.KS)
def test_host_twin_equals_the_text(k):
    """Every f of the grid at P in {1, 257, E + 1, 4099}: dist within the bound of the text's;
    order, the winning scores (bit for bit) and sel equal bulyan_order run on the twin's own dist; g
    equals _bulyan_coord on the twin's own sel, bit for bit."""
    for P in _ps(k):
        ent, cnt = K.inputs(k, P)
        for f in B.fs(k):
            got = B.host_twin(ent, cnt, f)
            g_t, d_t, o_t, w_t, s_t = B.text(ent, cnt, f)
            assert K.outside(got[1], d_t, K.dist_bound(P)) == 0, (P, f)
            B.stage_check(got, ent, cnt, f, P, (P, f))
            assert len(got[2]) == k - 2 * f and got[4] == sorted(got[2])


def test_f_zero_is_the_mean_in_sorted_order():
    """f = 0: every entry is selected and the window is all of them, so g is the values added in
    ascending order over k -- the trimmed mean with trim 0, the text of flsim_robust."""
    from flsim.robust import robust_flat
    for k in (3, 4, 9, 33, 64):
        ent, cnt = K.inputs(k, 257, 1)
        g, d, order, win, sel = B.host_twin(ent, cnt, 0)
        assert sel == list(range(k)) and sorted(order) == sel
        ref = robust_flat([torch.from_numpy(e) for e in ent], cnt, "trimmed_mean", 0)
        assert K.g_mismatches(g, ref.numpy()) == 0
        assert K.g_mismatches(B.text(ent, cnt, 0)[0], ref.numpy()) == 0


def test_exact_ties_go_to_the_lowest_index():
    """Rounds with n = 1: the two ends of the closest pair share one matrix element, so their scores
    tie exactly and the lower index wins; the twin follows the text through every such round."""
    for k, f in ((3, 0), (4, 0), (7, 1), (9, 0)):
        for seed in range(4):
            ent, cnt = K.inputs(k, 257, seed)
            got = B.host_twin(ent, cnt, f)
            B.stage_check(got, ent, cnt, f, 257, (k, f, seed))
            ref = B.text(ent, cnt, f)
            assert got[2] == ref[2] and got[4] == ref[4]
    # k = 3, f = 0: the first winner is the lower end of the closest pair
    ent, cnt = K.inputs(3, 257, 2)
    g, d, order, win, sel = B.host_twin(ent, cnt, 0)
    off = d + np.diag([np.inf] * 3)
    i, j = sorted(np.unravel_index(np.argmin(off), off.shape))
    assert order[0] == i and win[0] == off[i, j] and win[2] == 0.0


@pytest.mark.parametrize("k", (7, 16, 33))
def test_special_inputs(k):
    P, f = 257, 1
    off = ~np.eye(k, dtype=bool)
    # one poisoned entry is never selected; g stays finite and equals the text bit for bit
    for bad in (np.nan, np.inf, -np.inf):
        ent, cnt = K.inputs(k, P, 1)
        j = k // 2
        ent[j] = ent[j].copy()
        ent[j][3::7] = bad
        got = B.host_twin(ent, cnt, f)
        ref = B.text(ent, cnt, f)
        assert j not in got[4] and got[4] == ref[4] and got[2] == ref[2], bad
        assert np.isinf(got[1][j][off[j]]).all() and got[1][j, j] == 0
        assert np.isfinite(got[0]).all() and K.g_mismatches(got[0], ref[0]) == 0
        B.stage_check(got, ent, cnt, f, P, bad)
    # +-inf and +-0 scattered in two entries: g equals the text as numbers
    ent, cnt = K.inputs(k, P, 2)
    rs = np.random.RandomState(k)
    for j in (0, k - 1):
        ent[j] = ent[j].copy()
        idx = rs.permutation(P)[:40]
        ent[j][idx] = rs.choice([np.inf, -np.inf, 0.0, -0.0], 40).astype(np.float32)
    got = B.host_twin(ent, cnt, f)
    assert got[4] == B.text(ent, cnt, f)[4]
    assert B.g_differs(got[0], B.coord(ent, cnt, got[4], f)) == 0
    # specials in most entries (some are then selected): the window code on NaN, +-inf, +-0
    for dense in (3, 12):
        ent, cnt = K.inputs(k, P, 4)
        for j in range(k):
            ent[j] = ent[j].copy()
            idx = rs.permutation(P)[:P // dense]
            ent[j][idx] = rs.choice([np.nan, np.inf, -np.inf, 0.0, -0.0],
                                    len(idx)).astype(np.float32)
        for ff in B.fs(k):
            got = B.host_twin(ent, cnt, ff)
            g_t = B.coord(ent, cnt, got[4], ff)
            assert B.g_differs(got[0], g_t) == 0, (dense, ff)
            assert got[2] == B.order_of(got[1], ff)[0]
    # every entry NaN: every distance +inf, every round ties, the lowest indices leave first
    ent = [np.full(P, np.nan, np.float32) for _ in range(k)]
    g, d, order, win, sel = B.host_twin(ent, [1] * k, f)
    assert order == list(range(k - 2 * f)) == sel and np.isnan(g).all()
    assert np.isinf(d[off]).all() and np.isinf(win).all()
    # a duplicate pointer (distance exactly 0) and a NULL entry (all zero)
    ent, cnt = K.inputs(k, P, 3)
    ent[2] = None
    ent[1], cnt[1] = ent[0], cnt[0]
    got = B.host_twin(ent, cnt, f)
    assert got[1][0, 1] == 0.0 and got[1][1, 0] == 0.0
    ref = B.text(ent, cnt, f)
    assert got[2] == ref[2] and K.g_mismatches(got[0], ref[0]) == 0
    B.stage_check(got, ent, cnt, f, P, "dup")


@pytest.mark.parametrize("k,f", [(7, 1), (16, 3), (64, 15)])
def test_outliers_are_never_selected(k, f):
    """An honest cluster and f far outliers: no outlier is selected, and g stays within the
    honest values' range in every coordinate."""
    P = 257
    rs = np.random.RandomState(70 + k)
    mean = rs.standard_normal(P).astype(np.float32)
    outl = sorted(int(j) for j in rs.permutation(k)[:f])
    ent = []
    for j in range(k):
        x = mean + 0.05 * rs.standard_normal(P).astype(np.float32)
        if j in outl:
            x = x + (10.0 + j) * rs.choice([-1.0, 1.0], P).astype(np.float32)
        ent.append(np.ascontiguousarray(x))
    got = B.host_twin(ent, [1] * k, f)
    assert not set(got[4]) & set(outl)
    hon = np.stack([ent[j] for j in range(k) if j not in outl])
    assert (got[0] >= hon.min(0)).all() and (got[0] <= hon.max(0)).all()
    B.stage_check(got, ent, [1] * k, f, P, (k, f))


def test_rule_over_the_flattened_model_check_and_parse():
    from FL.agents import Agg
    from flsim.robust import bulyan_flat, bulyan_rule, check_bulyan, parse_rule
    gen = torch.Generator().manual_seed(5)
    ups = [[torch.randn(4, 3, generator=gen), torch.randn(5, generator=gen)] for _ in range(7)]
    ups[3] = [u + 50 for u in ups[3]]
    out = Agg(lambda u: bulyan_rule(u, 1)).rule(ups)
    flat = [torch.cat([t.reshape(-1) for t in u]) for u in ups]
    g, d, order, win, sel = bulyan_flat(flat, [1] * 7, 1)
    assert 3 not in sel and len(sel) == 5 and sel == sorted(order) and len(win) == 5
    assert torch.equal(torch.cat([t.reshape(-1) for t in out]), g)
    assert [t.shape for t in out] == [t.shape for t in ups[0]]
    assert check_bulyan(1, 7) == 1 and check_bulyan(0, 3) == 0 and check_bulyan(15, 64) == 15
    with pytest.raises(IndexError):
        bulyan_rule([], 0)
    with pytest.raises(IndexError):
        check_bulyan(0, 0)
    for f, k in ((-1, 9), (1, 6), (2, 10), (16, 64), (0, 2)):
        with pytest.raises(ValueError, match=f"Invalid f = {f} for k = {k} entries: f >= 0 and "
                                             r"k >= 4 \* f \+ 3"):
            check_bulyan(f, k)
    assert parse_rule(("bulyan", 2)) == ("bulyan", 2) and parse_rule(["bulyan", 0]) == ("bulyan", 0)
    for bad in ("bulyan", ("bulyan",), ("bulyan", 1, 2), ("bulyan", -1)):
        with pytest.raises(ValueError, match="robust_rule"):
            parse_rule(bad)
    # the other rules' specs are untouched
    assert parse_rule(("krum", 2)) == ("krum", 2, 1) and parse_rule("median") == ("median", 0)


def test_abi_structs_exports_and_probe_names():
    from flsim import _lib
    L = _lib.lib()
    assert {"flsim_bulyan_partials", "flsim_bulyan_optim_step",
            "flsim_bulyan_eval_host"} <= set(_lib.EXPORTS)
    assert ctypes.sizeof(_lib.FlsimBulyan) == 8 + 8 * 64 + 4 * 64
    assert (_lib.FlsimBulyan.f.offset, _lib.FlsimBulyan.k.offset) == (0, 4)
    assert _lib.FlsimBulyan.entries.offset == 8 and _lib.FlsimBulyan.count.offset == 520
    assert ctypes.sizeof(_lib.FlsimBulyanScratch) == 6 * 8
    assert [getattr(_lib.FlsimBulyanScratch, n).offset for n in
            ("partials", "n_partials", "dist", "score", "order", "sel")] == [0, 8, 16, 24, 32, 40]
    names = [L.flsim_probe_kernel_name(i).decode() for i in range(L.flsim_probe_kernel_count())]
    assert names[-3:] == ["bulyan_dist", "bulyan_finish", "bulyan_apply"]
    assert names.index("nnm_mix") == len(names) - 4          # appended: nothing reordered
    for k in (3, 9, 64):
        for n in (1, 257, 5596090):
            assert L.flsim_bulyan_partials(n, k) == L.flsim_krum_partials(n, k) > 0
    assert L.flsim_bulyan_partials(0, 8) == 0 and L.flsim_bulyan_partials(8, 65) == 0


# ---- refusals of the entry point (status 1, before any launch) -------------------------------------
F = {name: 0x1000000 * (i + 1) for i, name in enumerate(
    ["p", "m", "v", "g", "G", "D", "O", "e0", "e1", "e2", "sp", "sd", "ss", "so", "sl"])}
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


def _scratch(partials=None, n=1 << 20, dist=None, score=None, order=None, sel=None):
    from flsim._lib import FlsimBulyanScratch
    s = FlsimBulyanScratch()
    s.partials = F["sp"] if partials is None else partials
    s.n_partials = n
    s.dist = F["sd"] if dist is None else dist
    s.score = F["ss"] if score is None else score
    s.order = F["so"] if order is None else order
    s.sel = F["sl"] if sel is None else sel
    return s


def _call(f=0, counts=(1, 3, 4), ents=None, scratch="default", clip=None, g_out=0, p=None, mm=0,
          v=0, n=P, step=1, optim="sgd"):
    from flsim._lib import lib
    ents = [F["e0"], F["e1"], F["e2"]][:len(counts)] if ents is None else ents
    ents = list(ents) + [0] * (min(len(counts), 64) - len(ents))
    r, _ = B.c_bulyan(None, list(counts), f, ptrs=ents)
    s = _scratch() if scratch == "default" else scratch
    o = None if optim is None else (optim if not isinstance(optim, str) else
                                     _optim(kind=optim, lr=0.1))
    vp = ctypes.c_void_p
    rc = lib().flsim_bulyan_optim_step(
        ctypes.byref(r), None if s is None else ctypes.byref(s),
        None if clip is None else ctypes.byref(clip), vp(g_out), vp(F["p"] if p is None else p),
        vp(mm), vp(v), n, step, None if o is None else ctypes.byref(o), None)
    return rc, lib().flsim_last_error().decode()


REFUSALS = [
    (dict(counts=()), "Bulyan over k = 0 entries (3 .. 64)"),
    (dict(counts=(1, 1)), "Bulyan over k = 2 entries"),
    (dict(counts=(1,) * 65), "Bulyan over k = 65 entries"),
    (dict(f=-1), "Invalid f = -1 for k = 3 entries: f >= 0 and k >= 4 * f + 3"),
    (dict(f=1), "Invalid f = 1 for k = 3"),
    (dict(f=1, counts=(1,) * 6), "Invalid f = 1 for k = 6"),
    (dict(f=16, counts=(1,) * 64), "Invalid f = 16 for k = 64"),
    (dict(f=0x7FFFFFFF, counts=(1,) * 64), "Invalid f = 2147483647"),
    (dict(counts=(1, 0, 3)), "Invalid count 0 of entry 1"),
    (dict(counts=(1, 3, -5)), "Invalid count -5 of entry 2"),
    # what check_optim / check_clip refuse, still before any pointer (p = NULL everywhere)
    (dict(optim=_optim(kind="sgd", lr=-1.0), p=0, scratch=None), "Invalid learning rate"),
    (dict(optim=_optim(kind="adam", weight_decay=-1.0), p=0), "Invalid weight_decay"),
    (dict(clip=_clip(max_norm=0.0), p=0), "max_norm"),
    (dict(clip=_clip(max_norm=float("nan")), p=0, scratch=None), "max_norm"),
    (dict(optim=None), "null optimizer"),
    (dict(optim=None, g_out=F["g"], clip=_clip()), "null optimizer"),
    # the pointers
    (dict(p=0), "null pointer"),
    (dict(optim="adam", mm=F["m"]), "null pointer"),
    (dict(p=F["p"] + 4), "16-byte aligned"),
    (dict(g_out=F["g"] + 8), "16-byte aligned"),
    (dict(n=0), "out of range"),
    (dict(n=1 << 31), "out of range"),
    (dict(step=0), "step must be >= 1"),
    (dict(g_out=F["p"]), "overlap each other"),
    (dict(scratch=None), "null Bulyan scratch"),
    (dict(scratch=_scratch(partials=0)), "null Bulyan scratch"),
    (dict(scratch=_scratch(dist=0)), "null Bulyan scratch"),
    (dict(scratch=_scratch(score=0)), "null Bulyan scratch"),
    (dict(scratch=_scratch(order=0)), "null Bulyan scratch"),
    (dict(scratch=_scratch(sel=0)), "null Bulyan scratch"),
    (dict(scratch=_scratch(partials=F["sp"] + 8)), "Bulyan scratch must be 16-byte aligned"),
    (dict(scratch=_scratch(order=F["so"] + 4)), "Bulyan scratch must be 16-byte aligned"),
    (dict(scratch=_scratch(sel=F["sl"] + 4)), "Bulyan scratch must be 16-byte aligned"),
    (dict(scratch=_scratch(n=15)), "Bulyan n_partials = 15, this step writes 16"),
    (dict(scratch=_scratch(dist=F["sp"] + 64)), "Bulyan scratch buffers overlap"),
    (dict(scratch=_scratch(order=F["sl"])), "Bulyan scratch buffers overlap"),
    (dict(scratch=_scratch(sel=F["p"] + 16)), "Bulyan scratch overlaps p/m/v/g_out"),
    (dict(scratch=_scratch(score=F["G"] + 16), clip=_clip()), "Bulyan scratch overlaps clip G"),
    (dict(ents=[F["e0"], F["e1"] + 2, F["e2"]]), "entry 1 must be 4-byte aligned"),
    (dict(ents=[F["e0"], F["p"], F["e2"]]), "entry 1 overlaps"),
    (dict(ents=[F["p"] + 4 * (P - 1), F["e1"], F["e2"]]), "entry 0 overlaps"),
    (dict(g_out=F["g"], ents=[F["e0"], F["e1"], F["g"] + 32]), "entry 2 overlaps"),
    (dict(clip=_clip(), ents=[F["G"] + 4, F["e1"], F["e2"]]), "entry 0 overlaps clip G"),
    (dict(ents=[F["sp"] + 8, F["e1"], F["e2"]]), "entry 0 overlaps the Bulyan scratch"),
    (dict(ents=[F["e0"], F["sd"] - 4 * (P - 1), F["e2"]]), "entry 1 overlaps the Bulyan scratch"),
    (dict(ents=[F["e0"], F["e1"], F["ss"] + 16]), "entry 2 overlaps the Bulyan scratch"),
    (dict(ents=[F["e0"], F["e1"], F["so"]]), "entry 2 overlaps the Bulyan scratch"),
    (dict(ents=[F["e0"], F["e1"], F["sl"] + 8]), "entry 2 overlaps the Bulyan scratch"),
    (dict(clip=_clip(G=0)), "null clip buffer"),
    (dict(clip=_clip(G=F["p"] + 16)), "clip G overlaps"),
    (dict(clip=_clip(n=0)), "n_partials"),
]


@pytest.mark.parametrize("kw,message", REFUSALS, ids=[f"{i}-{m[:24]}" for i, (_, m) in
                                                       enumerate(REFUSALS)])
def test_entry_point_refusals(kw, message):
    rc, err = _call(**kw)
    assert rc == 1, (rc, err)
    assert message in err, err


def test_refusal_order_and_host_twin_refusals():
    """Hyper-parameters come before pointers (everything NULL still names f); the partials asked for
    are flsim_bulyan_partials; the twin refuses what the entry point refuses about the rule."""
    from flsim._lib import lib
    L = lib()
    rc, err = _call(f=5, p=0, ents=[0, 0, 0], scratch=None)
    assert rc == 1 and "Invalid f = 5" in err
    rc, err = _call(ents=[F["p"] - 4 * P, F["p"] + 4 * P, F["e2"]], clip=_clip(n=0))
    assert rc == 1 and "n_partials" in err
    for k in (3, 9, 33, 64):
        for n in (1, 257, 5596090):
            need = L.flsim_bulyan_partials(n, k)
            rc, err = _call(counts=(1,) * k, n=n, scratch=_scratch(n=need - 1))
            assert rc == 1 and f"this step writes {need}" in err, err
    vp = ctypes.c_void_p
    d, s = np.zeros(64 * 64), np.zeros(64)
    o, sel = np.zeros(64, np.int32), np.zeros(64, np.int32)
    a = (d.ctypes.data_as(vp), s.ctypes.data_as(vp), o.ctypes.data_as(vp), sel.ctypes.data_as(vp),
         None)
    for kw, message in REFUSALS[:10]:
        counts = list(kw.get("counts", (1, 3, 4)))
        ent = [np.ones(4, np.float32) for _ in counts[:64]]
        r, keep = B.c_bulyan(ent, counts, kw.get("f", 0))
        assert L.flsim_bulyan_eval_host(ctypes.byref(r), 4, *a) == 1
        assert message in L.flsim_last_error().decode()
    r, keep = B.c_bulyan([np.ones(4, np.float32)] * 3, [1] * 3, 0)
    assert L.flsim_bulyan_eval_host(ctypes.byref(r), 0, *a) == 1
    assert L.flsim_bulyan_eval_host(ctypes.byref(r), 4, None, *a[1:]) == 1
    assert L.flsim_bulyan_eval_host(ctypes.byref(r), 4, a[0], a[1], None, a[3], None) == 1
    assert L.flsim_bulyan_eval_host(None, 4, *a) == 1
    assert L.flsim_bulyan_eval_host(ctypes.byref(r), 4, *a) == 0


def test_bulyan_object():
    from flsim.engine import Bulyan
    e = [torch.zeros(8) for _ in range(7)]
    r = Bulyan(1, e, [1, 3, 4, 1, 1, 2, 2])
    c = r.c_struct()
    assert (c.f, c.k) == (1, 7) and list(c.count[:3]) == [1, 3, 4] and r.k == 7
    assert c.entries[0] == e[0].data_ptr() and c.entries[6] == e[6].data_ptr()
    assert Bulyan(0, [None] * 3, [4] * 3).c_struct().entries[0] is None
    assert Bulyan(2 ** 40, e, [1] * 7).c_struct().f == -1
    with pytest.raises(ValueError, match="counts"):
        Bulyan(0, e, [1, 2])
    with pytest.raises(ValueError, match="Bulyan over k = 65 entries"):
        Bulyan(0, [None] * 65, [1] * 65)


# ---- FLSimulation on a CPU stand-in (the one of tests/test_cpu_attack.py, with Bulyan) -------------
def _stand_in():
    import _nnm as M
    from test_cpu_attack import StandInEngine

    class BulyanEngine(StandInEngine):
        def bulyan_step(self, bul, theta, m, v, step, optim=None, clip=None, **kw):
            from flsim.robust import bulyan_flat
            g, d, order, win, sel = bulyan_flat(bul.entries, bul.counts, bul.f)
            bul.dist, bul.score = d, win
            bul.order = torch.tensor(order, dtype=torch.int32)
            bul.sel = torch.tensor(sel, dtype=torch.int32)
            theta -= optim.lr * g

        def nnm_entries(self, nnm):
            from flsim.robust import nnm_flat
            mixed, d, nbr = nnm_flat(nnm.entries, nnm.counts, nnm.f)
            for e, new in zip(nnm.entries, mixed):
                e.copy_(new)
            nnm.dist = d
            nnm.nbr = torch.from_numpy(M.masks(nbr).view(np.int64).copy())
    return BulyanEngine()


@pytest.mark.parametrize("nnm", (None, 1))
@pytest.mark.parametrize("attack", (None, ("ipm", 2.5), ("alie", 1.5)))
def test_epochs_on_a_stand_in(attack, nnm):
    """n = 12, the last worker slow with delay 2, seven buckets, ("bulyan", 1): last_selected and
    theta follow the text over last_entries (after the attack; over the mixed entries with count 1
    under nnm); selections() holds lists of ints."""
    from test_cpu_attack import IND, _sim
    from flsim.robust import bulyan_flat, nnm_flat
    kw = dict(attack=attack, n_byz=2) if attack else {}
    sim = _sim(_stand_in(), robust_rule=("bulyan", 1), buckets=7, keep_entries=True, nnm=nnm, **kw,
               **IND)
    assert sim.robust == ("bulyan", 1) and sim.last_selected is None
    pops = 0
    for t in range(4):
        before = sim.theta.clone()
        sim.epoch()
        ents, counts = sim.last_entries
        plan = sim.trace[-1]
        k = 7 + bool(plan.stale)
        pops += bool(plan.stale)
        assert len(ents) == k
        if nnm is not None:
            ents, counts = list(nnm_flat(ents, counts, nnm)[0]), [1] * k
        g, d, order, win, sel = bulyan_flat(ents, counts, 1)
        assert sim.last_selected == sel and len(sel) == k - 2
        assert all(type(j) is int for j in sim.last_selected)
        assert sim.selections()[-1] == sel and len(sim.selections()) == t + 1
        assert torch.equal(sim.theta, before - 0.125 * g)
    assert pops >= 1


def test_constructor_epoch_refusals_and_main_arguments():
    from test_cpu_attack import IND, _sim
    for bad in ("bulyan", ("bulyan",), ("bulyan", -1), ("bulyan", 1, 2)):
        with pytest.raises(ValueError, match="robust_rule"):
            _sim(_stand_in(), robust_rule=bad, **IND)
    rule = ("bulyan", 0)
    for sem in ("reference", "torch1"):
        with pytest.raises(NotImplementedError, match="independent"):
            _sim(_stand_in(), robust_rule=rule, semantics=sem)
    with pytest.raises(NotImplementedError, match="distributed"):
        _sim(_stand_in(), robust_rule=rule, distributed=True, **IND)
    # f against the epoch's k
    with pytest.raises(ValueError, match="Invalid f = 1 for k = 6 entries: f >= 0 and k >= 4"):
        _sim(_stand_in(), robust_rule=("bulyan", 1), buckets=6, **IND).epoch()
    quiet = _sim(_stand_in(), robust_rule=rule, buckets=4, **IND)
    quiet.epoch()
    assert quiet.last_selected is None and quiet.selections() == [[0, 1, 2, 3]]
    assert quiet._stale_config()["robust_rule"] == ["bulyan", 0]
    import main
    a = main.parse(["--robust_rule", "bulyan", "--byz_f", "2"])
    assert main.robust_spec(a) == ("bulyan", 2)
    with pytest.raises(SystemExit, match="--byz_f"):
        main.robust_spec(main.parse(["--robust_rule", "bulyan"]))
    assert main.robust_spec(main.parse(["--robust_rule", "krum", "--byz_f", "1"])) == ("krum", 1)
