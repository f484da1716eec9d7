"""CPU: the robust rules (coordinate-wise median, trimmed mean over bucket means).

The host twin flsim_robust_eval_host runs the sorting network and the select / sum code the kernel
runs (csrc/robust.h, one host + device template); here it is compared with the rule text
(flsim/robust.py: torch sort, sequential adds, one division) as numbers (tests/_robust.py).  Then
every refusal of flsim_robust_optim_step (they come before any launch, so made-up device addresses
are never read), and the constructor and checkpoint checks of FLSimulation on a CPU stand-in.
"""
import ctypes

import numpy as np
import pytest
import torch

import _robust as R

PS = (1, 255, 1027)


@pytest.mark.parametrize("k", R.KS)
def test_host_twin_equals_the_text(k):
    """Nonzero normal random sums, mixed counts in {1, 3, 128}, P in {1, 255, 1027}, the median and
    every valid trim: no zero and no NaN in the text's value (asserted), so every word is equal."""
    for kind, trim in R.rules(k):
        for P in PS:
            rs = np.random.RandomState(1000 * k + 10 * trim + P)
            ent, cnt = R.values(rs, k, P), R.counts_for(k)
            assert k < 3 or set(cnt) == set(R.COUNTS)
            ref = R.text(ent, cnt, kind, trim)
            assert np.isfinite(ref).all() and (ref != 0).all()          # input condition
            got = R.host_twin(ent, cnt, kind, trim)
            assert int((R.bits(got) != R.bits(ref)).sum()) == 0, (kind, trim, P)


@pytest.mark.parametrize("k", R.KS)
def test_host_twin_special_values(k):
    """Duplicated values across entries; +-inf and NaN in 1, ceil(k / 2) and k entries; one NULL
    entry; a -0.0 / +0.0 tie (compared by value): equal as numbers."""
    for kind, trim in R.rules(k):
        for name, (ent, cnt) in R.special_cases(k, 255).items():
            ref = R.text(ent, cnt, kind, trim)
            got = R.host_twin(ent, cnt, kind, trim)
            assert R.mismatches(got, ref) == 0, (kind, trim, name)
            if name == "zero_tie":
                assert (ref == 0).all() and (got == 0).all()
            if name.startswith("special"):                  # input condition: all three are there
                x = np.stack(ent)
                bad = {"special1": 1, "special_half": -(-k // 2), "special_all": k}[name]
                assert int(np.isnan(x).any(1).sum()) == bad
                assert (x == np.inf).any() and (x == -np.inf).any()
            if name == "duplicates":
                assert int((R.bits(got) != R.bits(ref)).sum()) == 0


def test_median_is_torch_median_and_rules_run_per_tensor():
    """flsim/robust.py itself: the lower median is torch.median on NaN-free input; the list forms
    are what Agg(rule) calls (one tensor per parameter, the input shapes kept)."""
    from FL.agents import Agg
    from flsim.robust import bucket_means, median_rule, trimmed_mean_rule
    g = torch.Generator().manual_seed(3)
    ups = [[torch.randn(4, 3, generator=g), torch.randn(5, generator=g)] for _ in range(6)]
    med = Agg(median_rule).rule(ups)
    tm = Agg(lambda u: trimmed_mean_rule(u, 1)).rule(ups)
    for i in range(2):
        st = torch.stack([u[i] for u in ups])
        assert torch.equal(med[i], st.median(0).values) and med[i].shape == ups[0][i].shape
        s = st.sort(0).values[1:5]
        acc = s[0].clone()
        for r in s[1:]:
            acc += r
        assert torch.equal(tm[i], acc / 4)
    assert torch.equal(bucket_means([ups[0][1] * 3], [3])[0], ups[0][1] * 3 / 3)
    with pytest.raises(IndexError):
        median_rule([])
    with pytest.raises(ValueError, match="trim"):
        trimmed_mean_rule(ups, 3)


# ---- refusals of the entry point (status 1, before any launch) -------------------------------------
F = {name: 0x100000 * (i + 1) for i, name in enumerate(
    ["p", "m", "v", "g", "G", "D", "O", "e0", "e1", "e2"])}
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


def _call(kind="median", trim=0, counts=(1, 3, 128), ents=None, clip=None, g_out=0, p=None, m=0,
          v=0, n=P, step=1, optim="sgd"):
    from flsim._lib import lib
    ents = [F["e0"], F["e1"], F["e2"]][:len(counts)] if ents is None else ents
    ents = list(ents) + [0] * (min(len(counts), 64) - len(ents))
    r, _ = R.c_robust(None, list(counts), kind, trim, ptrs=ents)
    r.k = len(counts)
    o = None if optim is None else (optim if not isinstance(optim, str) else
                                     _optim(kind=optim, lr=0.1))
    vp = ctypes.c_void_p
    rc = lib().flsim_robust_optim_step(
        ctypes.byref(r), None if clip is None else ctypes.byref(clip), vp(g_out),
        vp(F["p"] if p is None else p), vp(m), vp(v), n, step,
        None if o is None else ctypes.byref(o), None)
    return rc, lib().flsim_last_error().decode()


REFUSALS = [
    (dict(kind=2), "unknown robust rule kind"),
    (dict(kind=-1), "unknown robust rule kind"),
    (dict(counts=()), "k = 0 entries"),
    (dict(counts=(1,) * 65), "k = 65 entries"),
    (dict(kind="trimmed_mean", trim=-1), "Invalid trim -1"),
    (dict(kind="trimmed_mean", trim=2, counts=(1, 1, 1, 1)), "Invalid trim 2 for k = 4"),
    (dict(kind="trimmed_mean", trim=1, counts=(1, 1)), "Invalid trim 1 for k = 2"),
    (dict(kind="median", trim=1), "the median takes no trim"),
    (dict(counts=(1, 0, 3)), "Invalid count 0 of entry 1"),
    (dict(counts=(1, 3, -5)), "Invalid count -5 of entry 2"),
    # what check_optim / check_clip refuse, still before any pointer (p = NULL everywhere)
    (dict(optim=_optim(kind="sgd", lr=-1.0), p=0), "Invalid learning rate"),
    (dict(optim=_optim(kind="sgd", lr=0.1, momentum=-0.5), p=0), "Invalid momentum"),
    (dict(optim=_optim(kind="adam", weight_decay=-1.0), p=0), "Invalid weight_decay"),
    (dict(optim=_optim(kind="yogi", betas=(1.0, 0.9)), p=0), "Invalid beta parameter at index 0"),
    (dict(optim=_optim(kind="adagrad", lr_decay=-1.0), p=0), "Invalid lr_decay"),
    (dict(clip=_clip(max_norm=0.0), p=0), "max_norm"),
    (dict(clip=_clip(max_norm=float("nan")), p=0), "max_norm"),
    (dict(optim=None), "null optimizer"),
    (dict(optim=None, g_out=F["g"], clip=_clip()), "null optimizer"),
    # the pointers
    (dict(p=0), "null pointer"),
    (dict(optim="adam", m=F["m"]), "null pointer"),
    (dict(optim=_optim(kind="sgd", lr=0.1, momentum=0.9)), "null pointer"),
    (dict(p=F["p"] + 4), "16-byte aligned"),
    (dict(g_out=F["g"] + 8), "16-byte aligned"),
    (dict(optim="adam", m=F["m"] + 4, v=F["v"]), "16-byte aligned"),
    (dict(n=0), "out of range"),
    (dict(n=1 << 31), "out of range"),
    (dict(step=0), "step must be >= 1"),
    (dict(ents=[F["e0"], F["e1"] + 2, F["e2"]]), "entry 1 must be 4-byte aligned"),
    (dict(ents=[F["e0"], F["p"], F["e2"]]), "entry 1 overlaps"),
    (dict(ents=[F["p"] + 4 * (P - 1), F["e1"], F["e2"]]), "entry 0 overlaps"),
    (dict(ents=[F["e0"], F["e1"], F["p"] - 4 * (P - 1)]), "entry 2 overlaps"),
    (dict(optim="adam", m=F["m"], v=F["v"], ents=[F["m"] + 16, F["e1"], F["e2"]]),
     "entry 0 overlaps"),
    (dict(optim="adam", m=F["m"], v=F["v"], ents=[F["e0"], F["v"], F["e2"]]), "entry 1 overlaps"),
    (dict(g_out=F["g"], ents=[F["e0"], F["e1"], F["g"] + 32]), "entry 2 overlaps"),
    (dict(clip=_clip(), ents=[F["G"] + 4, F["e1"], F["e2"]]), "entry 0 overlaps clip G"),
    (dict(g_out=F["p"]), "overlap each other"),
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


def test_refusal_order_and_adjacent_buffers():
    """Hyper-parameters come before pointers (everything NULL still names the kind); an entry that
    ends where p begins does not overlap, so the next check is reached."""
    rc, err = _call(kind=7, p=0, ents=[0, 0, 0])
    assert rc == 1 and "unknown robust rule kind 7" in err
    rc, err = _call(ents=[F["p"] - 4 * P, F["p"] + 4 * P, F["e2"]], clip=_clip(n=0))
    assert rc == 1 and "n_partials" in err
    # the partials a clipped robust step writes fit the bound the Clip object allocates
    from flsim._lib import lib
    for n in (1, 255, 256, 257, 4101, 300000, 5596090, (1 << 31) - 1):
        assert lib().flsim_clip_partials(n) >= -(-n // 256)


def test_host_twin_refusals():
    from flsim._lib import lib
    out = np.zeros(4, np.float32)
    for kw, message in REFUSALS[:10]:
        counts = list(kw.get("counts", (1, 3, 128)))
        ent = [np.ones(4, np.float32) for _ in counts[:64]]
        r, keep = R.c_robust(ent, counts, kw.get("kind", "median"), kw.get("trim", 0))
        r.k = len(counts)
        rc = lib().flsim_robust_eval_host(ctypes.byref(r), 4, out.ctypes.data_as(ctypes.c_void_p))
        assert rc == 1 and message in lib().flsim_last_error().decode()
    r, keep = R.c_robust([np.ones(4, np.float32)], [1], "median", 0)
    assert lib().flsim_robust_eval_host(ctypes.byref(r), 4, None) == 1
    assert lib().flsim_robust_eval_host(ctypes.byref(r), 0, out.ctypes.data_as(ctypes.c_void_p)) == 1


def test_robust_object():
    from flsim.engine import Robust
    e = [torch.zeros(8) for _ in range(3)]
    r = Robust("trimmed_mean", 1, e, [1, 3, 128])
    c = r.c_struct()
    assert (c.kind, c.trim, c.k) == (1, 1, 3) and list(c.count[:3]) == [1, 3, 128]
    assert c.entries[0] == e[0].data_ptr() and r.k == 3
    assert Robust("nope", 0, e, [1, 1, 1]).c_struct().kind == -1
    assert Robust("median", 0, [None], [4]).c_struct().entries[0] is None
    with pytest.raises(ValueError, match="counts"):
        Robust("median", 0, e, [1, 2])
    with pytest.raises(ValueError, match="65 entries"):
        Robust("median", 0, [None] * 65, [1] * 65)


# ---- FLSimulation: constructor refusals and the checkpoint config ------------------------------
class StandInEngine:
    """A CPU stand-in with the engine's interface, as tests/test_dist_cpu.py uses."""
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
        self.last = robust
        theta -= optim.lr * robust_flat(robust.entries, robust.counts, robust.kind, robust.trim)


class BNStandIn(StandInEngine):
    STATS_PER_WORKER = 8


def _sim(engine=None, **kw):
    from flsim.sim import FLSimulation
    eng = engine or StandInEngine()
    kw.setdefault("delay", 2)
    return FLSimulation(kw.pop("n", 6), device="cpu", engine=eng, device_pool=object(),
                        theta0=torch.zeros(eng.P), optimizer="sgd", lr=0.125, **kw)


def test_constructor_refusals():
    ind = dict(semantics="independent")
    assert _sim(robust_rule=None).robust is None and _sim(robust_rule="none").robust is None
    assert _sim(robust_rule="median", **ind).robust == ("median", 0)
    assert _sim(robust_rule=("trimmed_mean", 2), **ind).robust == ("trimmed_mean", 2)
    for sem in ("reference", "torch1"):
        with pytest.raises(NotImplementedError, match="independent"):
            _sim(robust_rule="median", semantics=sem)
    with pytest.raises(NotImplementedError, match="distributed"):
        _sim(robust_rule="median", distributed=True, **ind)
    with pytest.raises(NotImplementedError, match="staleness discount"):
        _sim(robust_rule="median", stale_weight=("poly", 0.5), **ind)
    with pytest.raises(NotImplementedError, match="delay compensation"):
        _sim(robust_rule="median", delay_comp=0.5, **ind)
    with pytest.raises(NotImplementedError, match="batch_size"):
        _sim(robust_rule="median", batch_size=64, **ind)
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        _sim(BNStandIn(), robust_rule="median", **ind)
    with pytest.raises(ValueError, match="robust_rule"):
        _sim(robust_rule="krum", **ind)
    with pytest.raises(ValueError, match="robust_rule"):
        _sim(robust_rule=("median", 1), **ind)
    with pytest.raises(ValueError, match="buckets"):
        _sim(robust_rule="median", buckets=0, **ind)


def test_epoch_entries_buckets_then_popped_slots():
    """n = 6, worker 5 slow with delay 2, three buckets: the fresh entries are the contiguous
    buckets of the fast workers (count = bucket size), a popped class slot follows (count = the
    popped workers sharing it); theta follows the text over last_entries; k > 64 and a trim too
    large for the epoch's k are refused."""
    from flsim.robust import robust_flat
    sim = _sim(robust_rule=("trimmed_mean", 1), buckets=3, keep_entries=True,
               semantics="independent")
    pops = 0
    for t in range(5):
        before = sim.theta.clone()
        sim.epoch()
        ents, counts = sim.last_entries
        plan = sim.trace[-1]
        assert counts[:3] == [1, 2, 2] and len(ents) == 3 + bool(plan.stale)   # 5 fast workers
        if plan.stale:
            pops += 1
            assert counts[3] == 1
        g = robust_flat(ents, counts, "trimmed_mean", 1)
        assert torch.equal(sim.theta, before - 0.125 * g)
    assert pops >= 1
    with pytest.raises(ValueError, match="trim"):
        _sim(robust_rule=("trimmed_mean", 1), buckets=2, semantics="independent").epoch()
    big = _sim(n=70, robust_rule="median", buckets=65, semantics="independent")
    with pytest.raises(ValueError, match="65 entries"):
        big.epoch()
    # more buckets than fast workers: the empty ones are dropped
    few = _sim(n=3, robust_rule="median", buckets=8, keep_entries=True, semantics="independent")
    few.epoch()
    assert few.last_entries[1] == [1, 1]


def test_checkpoint_config_records_the_rule():
    a = _sim()
    a.epoch()
    ck = a.checkpoint()
    assert ck["config"]["robust_rule"] is None and ck["config"]["buckets"] == 8
    _sim().restore(ck)
    with pytest.raises(ValueError, match="buckets"):
        _sim(buckets=4).restore(ck)
    ck2 = dict(ck, config=dict(ck["config"], robust_rule=["median", 0]))
    with pytest.raises(ValueError, match="robust_rule"):
        _sim().restore(ck2)
    # a checkpoint from before the robust rules existed: off, the default bucket count
    old = dict(ck, config={k: v for k, v in ck["config"].items()
                           if k not in ("robust_rule", "buckets")})
    _sim().restore(old)
