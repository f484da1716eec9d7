"""CPU: the optimised attacks Min-Max and Min-Sum (Shejwalkar and Houmansadr 2021) on the bucketed
entries.

The text (flsim/robust.py: opt_attack_flat, opt_gamma) against an independent numpy restatement;
opt_gamma against a bisection of the paper's form; the budget met at strength 1 and strictly inside
it at 0.5; kh = 1 and q = 0; NaN and inf; the host twin flsim_attack_opt_eval_host (csrc/attack_opt.h:
the element and scalar code the kernels run) against the text by the stage-by-stage yardstick of
tests/_attack_opt.py; every refusal of flsim_attack_opt_entries (they come before any launch, so
made-up device addresses are never read) and their order; parse_attack and main.py's flags; the
OptAttack object; FLSimulation on the CPU stand-in of tests/test_cpu_attack.py.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import _attack as A
import _attack_opt as AO

KS = (1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)       # both sides of every KPAD
PS = (1, 2, 257)
CASES = [(kind, dirn) for kind in AO.KINDS for dirn in AO.DIRS]
E52 = 2.0 ** -52


@pytest.mark.parametrize("kind,dirn", CASES)
def test_text_equals_a_numpy_restatement(kind, dirn):
    """The element-wise part and gamma's scalar code are one IEEE operation each on both sides
    and every sum over elements is sequential on both sides: a, c, q and gamma bit for bit, b and
    the entries as numbers.  dist is torch's sum against numpy's: the stage's bound."""
    for k in (1, 2, 5, 16, 33):
        for P in (1, 257):
            ents, honest, byz = AO.inputs(k, P)
            ref = AO.text(ents, honest, byz, kind, dirn, 0.75)
            alt = AO.numpy_text(ents, honest, byz, kind, dirn, 0.75)
            assert ref["counts"] == [h + c for h, c in zip(honest, byz)]
            assert AO.within(alt["dist"], ref["dist"],
                             2 * (P + 2) * AO.U53 * np.abs(ref["dist"])) == 0
            assert np.array_equal(alt["a"].view(np.uint64), ref["a"].view(np.uint64)), (k, P)
            assert AO.within(alt["c"], ref["c"], 0.0) == 0 and AO.same_f64(alt["q"], ref["q"])
            from flsim.robust import opt_gamma
            g = opt_gamma(kind, ref["a"].tolist(), ref["c"].tolist(), ref["q"],
                          alt["dist"].tolist())
            assert AO.same_f64(g, alt["gamma"]), (k, P, g, alt["gamma"])
            out, _, b = AO.text_mix(ents, honest, byz, dirn, 0.75, alt["gamma"])
            assert A.mismatches(alt["b"], b) == 0
            for x, y in zip(alt["entries"], out):
                assert A.mismatches(x, y) == 0, (k, P)
            assert np.isfinite(ref["b"]).all()


def _budget(kind, y, b64):
    """(the attack's quantity at b64, the honest entries' own): max_i |b - y_i|^2 against D, or
    sum_i |b - y_i|^2 against S, in fp64 (math.fsum: exact sums of the rounded squares)."""
    d = [[math.fsum(((s - t) ** 2).tolist()) for t in y] for s in y]
    v = [math.fsum(((b64 - t) ** 2).tolist()) for t in y]
    if kind == "minmax":
        return max(v), max(max(r) for r in d)
    return math.fsum(v), max(math.fsum(r) for r in d)


@pytest.mark.parametrize("kind,dirn", CASES)
def test_budget_is_met_at_strength_one_and_strictly_inside_at_half(kind, dirn):
    """At strength 1 the active constraint holds with equality to 8 * 2^-52 relative, on the fp64
    b before its fp32 rounding; at strength 0.5 strictly.  (y_j in fp64 here: one worker per
    entry, so the fp32 means the distances are taken over are the y_j themselves.)"""
    for kh, P in ((2, 257), (3, 1), (3, 2), (8, 257), (33, 257)):
        g = torch.Generator().manual_seed(100 * kh + P)
        ents = [(torch.randn(P, generator=g) * 0.5 + 0.25).numpy() for _ in range(kh)] + \
            [A.poisoned(P)]
        honest, byz = [1] * kh + [0], [0] * kh + [2]
        one = AO.numpy_text(ents, honest, byz, kind, dirn, 1.0)
        assert one["gamma"] > 0 and math.isfinite(one["gamma"])
        got, lim = _budget(kind, one["y"], one["b64"])
        print(kind, dirn, kh, P, "at 1:", got / lim - 1)
        assert lim * (1 - 8 * E52) <= got <= lim * (1 + 8 * E52), (kh, P, got, lim)
        half = AO.numpy_text(ents, honest, byz, kind, dirn, 0.5)
        got, lim = _budget(kind, half["y"], half["b64"])
        assert got < lim, (kh, P, got, lim)
        # and the text is that restatement
        ref = AO.text(ents, honest, byz, kind, dirn, 1.0)
        assert AO.same_f64(ref["gamma"], one["gamma"]) or \
            abs(ref["gamma"] - one["gamma"]) <= 4 * (P + 2) * AO.U53 * one["gamma"]


@pytest.mark.parametrize("kind,dirn", CASES)
def test_opt_gamma_equals_a_bisection_of_the_papers_form(kind, dirn):
    """The paper's search: the largest gamma whose constraint holds, bracketed by doubling and
    halved 60 times.  The bracket [lo, hi] found by doubling has hi <= 2 * gamma_true and width
    <= gamma_true, so after 60 halvings lo is within gamma * 2^-60 of the root of the evaluated
    constraint; evaluating the quadratic itself in fp64 moves that root by a few ulps (its slope
    at the root is >= sqrt(q r) > 0 here).  Bound: 2^-48 relative."""
    from flsim.robust import opt_gamma
    for kh, P in ((2, 257), (3, 2), (8, 257), (33, 257)):
        ents, honest, byz = AO.inputs(kh, P, full=True)
        ref = AO.text(ents, honest, byz, kind, dirn, 1.0)
        a, c, q = ref["a"].tolist(), ref["c"].tolist(), ref["q"]
        dist = ref["dist"].tolist()
        D = max(max(r) for r in dist)
        S = max(math.fsum(r) for r in dist)

        def holds(g):
            if kind == "minmax":
                return all(q * g * g + 2 * c[i] * g + a[i] <= D for i in range(len(a)))
            return len(a) * q * g * g + 2 * math.fsum(c) * g + math.fsum(a) <= S
        assert holds(0.0)
        hi = 1e-3
        while holds(hi):
            hi *= 2
        lo = hi / 2 if hi > 1e-3 else 0.0
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if holds(mid) else (lo, mid)
        g = opt_gamma(kind, a, c, q, dist)
        print(kind, dirn, kh, P, "gamma", g, "bisection", lo, "rel", abs(g - lo) / g)
        assert abs(g - lo) <= 2.0 ** -48 * g, (kh, P, g, lo)
        assert AO.same_f64(g, ref["gamma"])


def test_one_honest_entry_and_a_zero_direction_give_gamma_zero():
    """kh = 1: D = S = 0 and a_0 = 0, so gamma = 0 and b = mu, whatever the strength.  q = 0 (a
    zero direction): all-zero honest entries for unit and sign, identical ones for std."""
    rs = np.random.RandomState(5)
    e = (rs.standard_normal(257) * 3).astype(np.float32)
    mu = (e.astype(np.float64) / 3.0).astype(np.float32)
    for kind, dirn in CASES:
        ents, honest, byz = [e, A.poisoned(257)], [3, 0], [2, 1]
        got = AO.host_twin(ents, honest, byz, kind, dirn, 7.0)
        ref = AO.check_stages(got, ents, honest, byz, kind, dirn, 7.0, (kind, dirn))
        assert ref["gamma"] == 0.0 and got["gamma"] == 0.0 and got["a"][0] == 0
        assert got["dist"].shape == (1, 1) and got["dist"][0, 0] == 0
        assert np.array_equal(A.bits(got["b"]), A.bits(mu))
        assert np.array_equal(A.bits(got["entries"][0]), A.bits(e + mu * np.float32(2)))
        same = e if dirn == "std" else np.zeros(257, np.float32)
        ents, honest, byz = [same.copy(), same.copy(), same.copy(), A.poisoned(257)], \
            [1, 1, 1, 0], [0, 1, 0, 2]
        got = AO.host_twin(ents, honest, byz, kind, dirn, 1.0)
        ref = AO.check_stages(got, ents, honest, byz, kind, dirn, 1.0, (kind, dirn, "q"))
        assert ref["q"] == 0 and got["q"] == 0 and ref["gamma"] == 0.0 and got["gamma"] == 0.0
        assert A.mismatches(got["b"], same) == 0
    # strength 0: b = mu too
    ents, honest, byz = AO.inputs(5, 257)
    got = AO.host_twin(ents, honest, byz, "minmax", "std", 0.0)
    AO.check_stages(got, ents, honest, byz, "minmax", "std", 0.0)
    assert got["gamma"] > 0
    from flsim.robust import attack_vector
    assert A.mismatches(got["b"], attack_vector(AO._tensors(ents, honest), honest, "alie",
                                                0.0).numpy()) == 0


@pytest.mark.parametrize("kind,dirn", CASES)
def test_nan_and_inf_in_an_honest_entry_propagate(kind, dirn):
    """No dead-entry logic: a NaN or an inf at elements of one honest entry makes that entry's
    a_i a NaN (e_i = mu - y_i is inf - inf for an inf), so gamma and the whole of b are NaN; dist
    shows the entry at +inf."""
    for bad in (np.nan, np.inf, -np.inf):
        ents, honest, byz = AO.inputs(8, 257, 1)
        j = next(i for i, h in enumerate(honest) if h and not byz[i])
        ents[j] = ents[j].copy()
        ents[j][3::7] = bad
        got = AO.host_twin(ents, honest, byz, kind, dirn, 1.0)
        ref = AO.check_stages(got, ents, honest, byz, kind, dirn, 1.0, bad)
        ji = sum(1 for h in honest[:j] if h)
        assert math.isnan(ref["gamma"]) and math.isnan(got["gamma"])
        assert np.isnan(ref["a"][ji]) and np.isnan(ref["b"]).all() and np.isnan(got["b"]).all()
        assert np.isinf(got["dist"][ji]).sum() == got["dist"].shape[0] - 1
        assert got["dist"][ji, ji] == 0


@pytest.mark.parametrize("kind,dirn", CASES)
@pytest.mark.parametrize("k", KS)
def test_host_twin_equals_the_text(kind, dirn, k):
    """Honest-only, mixed and fully Byzantine entries (k >= 3: all three), and the variant in
    which every entry is read (kh = k); an entry with byz == 0 keeps its bits; the never-read
    entries hold the quiet-NaN pattern and every output starts poisoned."""
    for P in PS:
        for full in (False, True):
            ents, honest, byz = AO.inputs(k, P, full=full)
            if k >= 3 and not full:
                assert {(h > 0, c > 0) for h, c in zip(honest, byz)} == \
                    {(True, True), (True, False), (False, True)}
            got = AO.host_twin(ents, honest, byz, kind, dirn, 1.0)
            ref = AO.check_stages(got, ents, honest, byz, kind, dirn, 1.0, (k, P, full))
            assert np.isfinite(ref["b"]).all() and math.isfinite(got["gamma"])
    # b_out is optional
    got2 = AO.host_twin(ents, honest, byz, kind, dirn, 1.0, b_out=False)
    assert got2["b"] is None and AO.same_f64(got2["gamma"], got["gamma"])
    for x, y in zip(got["entries"], got2["entries"]):
        assert np.array_equal(A.bits(x), A.bits(y))


def test_never_read_entries_do_not_matter():
    ents, honest, byz = AO.inputs(9, 257)
    other = [e if h else A.poisoned(257, 0x7F800001) for e, h in zip(ents, honest)]
    for kind, dirn in CASES:
        a = AO.host_twin(ents, honest, byz, kind, dirn, 1.0)
        c = AO.host_twin(other, honest, byz, kind, dirn, 1.0)
        assert AO.same_f64(a["gamma"], c["gamma"])
        assert np.array_equal(A.bits(a["b"]), A.bits(c["b"]))
        for x, y in zip(a["entries"], c["entries"]):
            assert np.array_equal(A.bits(x), A.bits(y))


# ---- refusals of the entry point (status 1, before any launch) -------------------------------------
F = {name: 0x1000000 * (i + 1) for i, name in enumerate(
    ["b", "e0", "e1", "e2", "sp", "sd", "ss", "sg"])}
P = 64


def _call(kind="minmax", dirn="std", strength=1.0, honest=(2, 1, 0), byz=(0, 1, 2), ents=None,
          b_out=0, n=P, k=None, host=False, scratch=None, n_partials=None, no_scratch=False):
    from flsim._lib import FlsimAttackOptScratch, lib
    L = lib()
    ents = [F["e0"], F["e1"], F["e2"]][:len(honest)] if ents is None else ents
    ents = list(ents) + [0] * (min(len(honest), 64) - len(ents))
    a, _ = AO.c_attack_opt(None, list(honest), list(byz), kind, dirn, strength, ptrs=ents, k=k)
    vp = ctypes.c_void_p
    if host:
        rc = L.flsim_attack_opt_eval_host(ctypes.byref(a), vp(F["sd"]), vp(F["ss"]), vp(F["sg"]),
                                          vp(b_out), n)
        return rc, L.flsim_last_error().decode()
    s = FlsimAttackOptScratch()
    sc = {**dict(partials=F["sp"], dist=F["sd"], stats=F["ss"], gamma=F["sg"]), **(scratch or {})}
    s.partials, s.dist, s.stats, s.gamma = sc["partials"], sc["dist"], sc["stats"], sc["gamma"]
    s.n_partials = 1 << 20 if n_partials is None else n_partials
    rc = L.flsim_attack_opt_entries(ctypes.byref(a), None if no_scratch else ctypes.byref(s),
                                    vp(b_out), n, None)
    return rc, L.flsim_last_error().decode()


FIELD_REFUSALS = [
    (dict(kind=0), "Invalid attack kind 0"),
    (dict(kind=4), "Invalid attack kind 4"),
    (dict(dirn=3), "Invalid attack direction 3"),
    (dict(dirn=-1), "Invalid attack direction -1"),
    (dict(honest=(), byz=()), "k = 0 entries"),
    (dict(honest=(1,) * 65, byz=(1,) * 65), "k = 65 entries"),
    (dict(strength=-0.5), "Invalid attack strength"),
    (dict(strength=float("nan")), "Invalid attack strength"),
    (dict(strength=float("inf")), "Invalid attack strength"),
    (dict(honest=(2, -1, 0)), "Invalid honest count -1 of entry 1"),
    (dict(byz=(0, 1, -2)), "Invalid Byzantine count -2 of entry 2"),
    (dict(honest=(2, 0, 0), byz=(0, 0, 2)), "entry 1 holds no worker"),
    (dict(honest=(0, 0, 0), byz=(1, 1, 2)), "ValueError: no entry holds an honest worker"),
    (dict(honest=(2, 1, 3), byz=(0, 0, 0)), "no entry holds a Byzantine worker"),
]
POINTER_REFUSALS = [
    (dict(ents=[F["e0"], 0, F["e2"]]), "null entry 1"),
    (dict(ents=[F["e0"] + 4, F["e1"], F["e2"]]), "entry 0 must be 16-byte aligned"),
    (dict(b_out=F["b"] + 4), "b_out must be 16-byte aligned"),
    (dict(n=0), "P = 0 out of range"),
    (dict(n=1 << 31), "out of range"),
    (dict(ents=[F["e0"], F["e0"], F["e2"]]), "entries 0 and 1 overlap"),
    (dict(b_out=F["e2"] + 4 * (P - 4)), "entry 2 overlaps b_out"),
]
SCRATCH_REFUSALS = [
    (dict(no_scratch=True), "null attack scratch"),
    (dict(scratch=dict(partials=0)), "null attack scratch"),
    (dict(scratch=dict(dist=0)), "null attack scratch"),
    (dict(scratch=dict(stats=0)), "null attack scratch"),
    (dict(scratch=dict(gamma=0)), "null attack scratch"),
    (dict(scratch=dict(gamma=F["sg"] + 8)), "attack scratch must be 16-byte aligned"),
    (dict(n_partials=3), "attack n_partials = 3, this step writes"),
    (dict(b_out=F["ss"]), "b_out overlaps the attack scratch"),
    (dict(scratch=dict(stats=F["e2"] + 4 * (P - 4))), "entry 2 overlaps the attack scratch"),
    (dict(scratch=dict(gamma=F["e0"])), "entry 0 overlaps the attack scratch"),
    (dict(scratch=dict(gamma=F["ss"] + 8 * 128)), "attack scratch buffers overlap each other"),
    (dict(scratch=dict(dist=F["sp"] + 16)), "attack scratch buffers overlap each other"),
]
REFUSALS = FIELD_REFUSALS + POINTER_REFUSALS + SCRATCH_REFUSALS


@pytest.mark.parametrize("kw,message", REFUSALS, ids=[f"{i}-{m[:24]}" for i, (_, m) in
                                                       enumerate(REFUSALS)])
def test_entry_point_refusals(kw, message):
    rc, err = _call(**kw)
    assert rc == 1, (rc, err)
    assert message in err, err
    if (kw, message) not in SCRATCH_REFUSALS:       # the host twin refuses what concerns it
        rc, err = _call(host=True, **kw)
        assert rc == 1 and message in err, (rc, err)


def test_refusal_order_sizes_and_python_errors():
    """The fields come before the pointers, the kind before the direction, then flsim_attack's
    order; among the pointers the entries, b_out, P, the overlaps, then the scratch.  The host twin
    runs on adjacent host buffers.  flsim_attack_opt_partials covers every kh <= k."""
    from flsim._lib import check, lib
    L = lib()
    bad = dict(ents=[0, 4, 0], b_out=4, n=0, scratch=dict(partials=0, gamma=8))
    order = [dict(kind=7, dirn=9, k=0, strength=-1.0, honest=(-1, 0, 0), byz=(0, 0, 0)),
             dict(dirn=9, k=0, strength=-1.0, honest=(-1, 0, 0), byz=(0, 0, 0)),
             dict(k=70, strength=-1.0, honest=(-1, 0, 0), byz=(0, 0, 0)),
             dict(strength=-1.0, honest=(-1, 0, 0), byz=(0, 0, 0)),
             dict(honest=(-1, 0, 0), byz=(-1, 0, 0)),
             dict(honest=(1, 0, 0), byz=(-1, 0, 0)),
             dict(honest=(1, 0, 0), byz=(0, 0, 0)),
             dict(honest=(0, 0, 0), byz=(1, 1, 1)),
             dict(honest=(1, 1, 1), byz=(0, 0, 0)),
             dict()]
    names = ["attack kind", "attack direction", "k = 70", "attack strength", "honest count",
             "Byzantine count", "entry 1 holds no worker", "honest worker", "Byzantine worker",
             "null entry 0"]
    for kw, name in zip(order, names):
        rc, err = _call(**{**bad, **kw})
        assert rc == 1 and name in err, (name, err)
    rc, err = _call(b_out=F["b"] + 4, n=0, scratch=dict(partials=0))
    assert "b_out must be" in err
    rc, err = _call(n=0, scratch=dict(partials=0))
    assert "out of range" in err
    rc, err = _call(ents=[F["e0"], F["e0"], F["e2"]], scratch=dict(partials=0))
    assert "entries 0 and 1 overlap" in err
    rc, err = _call(scratch=dict(partials=0, gamma=F["sg"] + 8), n_partials=0)
    assert "null attack scratch" in err
    rc, err = _call(scratch=dict(gamma=F["sg"] + 8), n_partials=0)
    assert "16-byte aligned" in err
    rc, err = _call(n_partials=0, b_out=F["ss"])
    assert "n_partials" in err
    assert L.flsim_attack_opt_entries(None, None, None, P, None) == 1
    assert "null attack" in L.flsim_last_error().decode()
    buf = np.zeros(4 * P, np.float32)
    ptrs = [buf.ctypes.data + 4 * P * i for i in range(3)]
    d, s, g = np.zeros(4), np.zeros(129), np.zeros(1)
    a, _ = AO.c_attack_opt(None, [2, 1, 0], [0, 1, 2], "minsum", "sign", 1.0, ptrs=ptrs)
    vp = ctypes.c_void_p
    assert L.flsim_attack_opt_eval_host(ctypes.byref(a), d.ctypes.data_as(vp),
                                        s.ctypes.data_as(vp), g.ctypes.data_as(vp),
                                        vp(buf.ctypes.data + 12 * P), P) == 0
    assert L.flsim_attack_opt_eval_host(ctypes.byref(a), None, s.ctypes.data_as(vp),
                                        g.ctypes.data_as(vp), None, P) == 1
    for k in range(1, 65):
        E = L.flsim_attack_opt_tile_elems(k)
        assert E >= 256 and E % 256 == 0
        for n in (1, 257, 5596090):
            need = L.flsim_attack_opt_partials(n, k)
            assert need > L.flsim_krum_partials(n, k)
            assert k == 1 or need >= L.flsim_attack_opt_partials(n, k - 1)
    assert L.flsim_attack_opt_tile_elems(0) == 0 and L.flsim_attack_opt_tile_elems(65) == 0
    assert L.flsim_attack_opt_partials(0, 8) == 0 and L.flsim_attack_opt_partials(8, 65) == 0
    with pytest.raises(ValueError, match="nothing to observe"):
        check(_call(honest=(0, 0, 0), byz=(1, 1, 2))[0])
    with pytest.raises(ValueError, match="attack direction"):
        check(_call(dirn=5)[0])


def test_abi_structs_and_exports():
    from flsim import _lib
    assert {"flsim_attack_opt_partials", "flsim_attack_opt_tile_elems",
            "flsim_attack_opt_entries", "flsim_attack_opt_eval_host"} <= set(_lib.EXPORTS)
    T = _lib.FlsimAttackOpt
    assert ctypes.sizeof(T) == 24 + 8 * 64 + 4 * 64 + 4 * 64
    assert [getattr(T, n).offset for n in ("kind", "dir", "k", "strength", "entries", "honest",
                                           "byz")] == [0, 4, 8, 16, 24, 536, 792]
    S = _lib.FlsimAttackOptScratch
    assert [getattr(S, n).offset for n in ("partials", "n_partials", "dist", "stats", "gamma")] == \
        [0, 8, 16, 24, 32]
    assert _lib.ATTACK_OPT_STATS == 129
    # the existing struct keeps its layout
    assert ctypes.sizeof(_lib.FlsimAttack) == 16 + 8 * 64 + 4 * 64 + 4 * 64


def test_check_and_parse():
    from flsim.robust import (ATTACK_KINDS, OPT_ATTACK_DIRS, OPT_ATTACK_KINDS, check_opt_attack,
                              opt_attack_flat, parse_attack)
    assert ATTACK_KINDS == ("ipm", "alie")
    assert OPT_ATTACK_KINDS == ("minmax", "minsum") and OPT_ATTACK_DIRS == ("unit", "std", "sign")
    assert check_opt_attack("minsum", "sign", 2, [1, 0], [0, 3]) == ("minsum", "sign", 2.0)
    for kw, message in FIELD_REFUSALS:
        if isinstance(kw.get("kind"), int) or isinstance(kw.get("dirn"), int):
            continue
        args = ("minmax", "std", kw.get("strength", 1.0), kw.get("honest", (2, 1, 0)),
                kw.get("byz", (0, 1, 2)))
        with pytest.raises(ValueError, match=message.replace("ValueError: ", "")):
            check_opt_attack(*args)
        with pytest.raises(ValueError):
            opt_attack_flat([torch.zeros(4)] * len(args[3]), args[3], args[4], *args[:3])
    with pytest.raises(ValueError, match="attack kind"):
        check_opt_attack("ipm", "std", 1.0, [1], [1])
    with pytest.raises(ValueError, match="attack direction"):
        check_opt_attack("minmax", "l2", 1.0, [1], [1])
    with pytest.raises(ValueError, match="attack kind"):          # the kind before the direction
        check_opt_attack("alie", "l2", -1.0, [1], [1])
    assert parse_attack("minmax") == ("minmax", "std", 1.0)
    assert parse_attack(("minsum",)) == ("minsum", "std", 1.0)
    assert parse_attack(("minmax", "unit")) == ("minmax", "unit", 1.0)
    assert parse_attack(["minsum", "sign", 2]) == ("minsum", "sign", 2.0)
    assert parse_attack(("minmax", None, None)) == ("minmax", "std", 1.0)
    assert parse_attack(("minmax", "std", 0)) == ("minmax", "std", 0.0)
    for bad in (("minmax", "l2"), ("minmax", 1.0), ("minsum", "std", -1),
                ("minsum", "std", float("nan")), ("minmax", "std", "x"),
                ("minmax", "std", 1, 2)):
        with pytest.raises(ValueError, match="attack"):
            parse_attack(bad)
    # what parse_attack accepted or refused before stays
    assert parse_attack(None) is None and parse_attack("ipm") == ("ipm", 1.0)
    assert parse_attack(("alie", 0.5)) == ("alie", 0.5) and parse_attack("alie") == ("alie", None)
    for bad in ("mimic", ("sign_flip", 1), ("ipm", 1, 2), ()):
        with pytest.raises(ValueError, match=r"supported: None, 'ipm', \('ipm', eps\), 'alie'"):
            parse_attack(bad)


def test_opt_attack_object():
    from flsim.engine import Attack, OptAttack, _BucketRule
    e = [torch.zeros(8) for _ in range(3)]
    a = OptAttack("minsum", "sign", 0.5, e, [2, 1, 0], [0, 1, 2])
    assert isinstance(a, _BucketRule) and isinstance(a, Attack)
    c = a.c_struct()
    assert (c.kind, c.dir, c.k, c.strength) == (3, 2, 3, 0.5) and a.k == 3 and a.kh == 2
    assert list(c.honest[:3]) == [2, 1, 0] and list(c.byz[:3]) == [0, 1, 2]
    assert c.entries[0] == e[0].data_ptr() and c.entries[2] == e[2].data_ptr()
    assert OptAttack("minmax", "unit", 1, e, [1] * 3, [1] * 3).c_struct().kind == 2
    assert OptAttack("ipm", "std", 1, e, [1] * 3, [1] * 3).c_struct().kind == -1
    assert OptAttack("minmax", "l2", 1, e, [1] * 3, [1] * 3).c_struct().dir == -1
    tail, rows = a._scratch_rows(3)
    assert tail == () and [r[0] for r in rows] == ["dist", "stats", "gamma"]
    assert rows[0][4] == (2, 2) and rows[0][3] >= 9 and rows[1][4] == (129,) and rows[2][4] == (1,)
    with pytest.raises(ValueError, match="counts"):
        OptAttack("minmax", "std", 1.0, e, [1, 2], [1, 2, 3])
    with pytest.raises(ValueError, match="65 entries"):
        OptAttack("minmax", "std", 1.0, [None] * 65, [1] * 65, [1] * 65)


def test_main_arguments():
    import main
    from flsim.robust import parse_attack
    a = main.parse(["--attack", "minmax"])
    assert main.attack_spec(a) == ("minmax", "std") and a.attack_dir == "std"
    assert parse_attack(main.attack_spec(a)) == ("minmax", "std", 1.0)
    a = main.parse(["--robust_rule", "krum", "--byz_f", "2", "--attack", "minsum", "--attack_dir",
                    "sign", "--attack_strength", "0.5", "--n_byz", "16"])
    assert main.attack_spec(a) == ("minsum", "sign", 0.5)
    a = main.parse(["--attack", "ipm", "--attack_dir", "unit"])      # the direction is theirs alone
    assert main.attack_spec(a) == "ipm"
    assert main.attack_spec(main.parse([])) is None
    with pytest.raises(SystemExit):
        main.parse(["--attack", "minmax", "--attack_dir", "l2"])
    assert "minmax" in main.__doc__ and "--attack_dir" in main.__doc__


# ---- FLSimulation on the CPU stand-in of tests/test_cpu_attack.py ------------------------------------
def _stand_in():
    from test_cpu_attack import StandInEngine

    class Engine(StandInEngine):
        def attack_entries(self, attack, b_out=None):
            from flsim.engine import OptAttack
            from flsim.robust import opt_attack_flat
            if not isinstance(attack, OptAttack):
                return super().attack_entries(attack, b_out)
            sums = [e if h else None for e, h in zip(attack.entries, attack.honest)]
            out, counts, b, gamma, a, c, q, dist = opt_attack_flat(
                sums, attack.honest, attack.byz, attack.kind, attack.dir, attack.strength)
            for e, new, n in zip(attack.entries, out, attack.byz):
                if n:
                    e.copy_(new)
            if b_out is not None:
                b_out.copy_(b)
            attack.gamma = torch.tensor([gamma], dtype=torch.float64)
            attack.stats = torch.zeros(129, dtype=torch.float64)
            attack.stats[:len(a)], attack.stats[64:64 + len(c)], attack.stats[128] = a, c, q
            attack.dist = dist
    return Engine()


def _sim(engine, **kw):
    from flsim.sim import FLSimulation
    kw.setdefault("delay", 2)
    return FLSimulation(kw.pop("n", 12), device="cpu", engine=engine, device_pool=object(),
                        theta0=torch.zeros(engine.P), optimizer="sgd", lr=0.125, **kw)


IND = dict(semantics="independent")


@pytest.mark.parametrize("spec", ("minmax", ("minsum", "unit", 0.5)))
def test_simulation_on_the_stand_in(spec):
    """n = 12, four buckets, three Byzantine workers: last_entries equals the text over the honest
    sums, theta follows the rule over the attacked entries, attack_log() keeps its triple with
    the strength used, attack_gamma_log() and last_attack_opt hold the solve."""
    from flsim.robust import opt_attack_flat, parse_attack, robust_flat
    kind, dirn, strength = parse_attack(spec)
    eng = _stand_in()
    sim = _sim(eng, robust_rule="median", buckets=4, keep_entries=True, attack=spec, n_byz=3,
               **IND)
    assert sim.attack == (kind, dirn, strength)
    assert sim.attack_gamma_log() == [] and sim.last_attack_opt is None
    for t in range(3):
        before = sim.theta.clone()
        sim.epoch()
        ents, counts = sim.last_entries
        b, honest, byz = sim.last_attack
        out, cnt, bt, gamma, a, c, q, dist = opt_attack_flat(sim.last_honest, honest, byz, kind,
                                                             dirn, strength)
        assert torch.equal(b, bt) and counts[:4] == cnt
        for j in range(4):
            assert torch.equal(ents[j], out[j]), (t, j)
        assert torch.equal(sim.theta, before - 0.125 * robust_flat(ents, counts, "median", 0))
        assert sim.attack_log()[-1] == (kind, strength, 3)
        assert [type(x) for x in sim.attack_log()[-1]] == [str, float, int]
        g = sim.attack_gamma_log()[-1]
        assert g.dtype == torch.float64 and g.shape == (1,) and float(g) == gamma > 0
        lg, la, lc, lq, ld = sim.last_attack_opt
        assert float(lg) == gamma and torch.equal(la, a) and torch.equal(lc, c)
        assert float(lq) == float(q) and torch.equal(ld, dist)
    assert len(sim.attack_gamma_log()) == 3
    cfg = sim._stale_config()
    assert cfg["attack"] == [kind, dirn, strength] and cfg["n_byz"] == 3


def test_simulation_refusals_checkpoint_and_off():
    eng = _stand_in()
    with pytest.raises(NotImplementedError, match="robust_rule"):
        _sim(eng, attack="minmax", n_byz=2, **IND)
    with pytest.raises(ValueError, match="n_byz = 0"):
        _sim(eng, robust_rule="median", attack="minsum", **IND)
    with pytest.raises(ValueError, match="attack"):
        _sim(eng, robust_rule="median", attack=("minmax", "l2"), n_byz=2, **IND)
    # no Byzantine worker in the epoch's fast set: no attack, no gamma
    sim = _sim(eng, robust_rule="median", buckets=4, keep_entries=True, attack="minmax", n_byz=3,
               **IND)
    sim.byz_workers = np.zeros(0, np.int64)
    sim.epoch()
    assert sim.attack_log() == [("minmax", None, 0)] and sim.attack_gamma_log() == []
    # a run under the earlier attacks logs no gamma; a checkpoint from before the new kinds reads
    old = _sim(_stand_in(), robust_rule="median", buckets=4, attack="ipm", n_byz=3, **IND)
    old.epoch()
    assert old.attack_gamma_log() == [] and old.last_attack_opt is None
    assert old._stale_config()["attack"] == ["ipm", 1.0]
    plain = _sim(_stand_in(), buckets=4)
    plain.epoch()
    ck = plain.checkpoint()
    assert ck["config"]["attack"] is None
    _sim(_stand_in(), buckets=4).restore(ck)
    with pytest.raises(ValueError, match="attack"):
        _sim(_stand_in(), buckets=4).restore(
            dict(ck, config=dict(ck["config"], attack=["minmax", "std", 1.0])))
