"""GPU: engine results do not depend on what the raw buffers held before, nor on earlier epochs
and chunks ("buffer contents and history").

`gradstate`, `workspace` and `workspace2` come from torch.empty, PerformantNet1's begin_epoch does
not clear its 1.9 GB of weight-gradient slabs (host bookkeeping decides which slab rows a chunk
stores into, accumulates into and which the epoch sum reads: EpochRows, wsplit, EpiSlabAcc::zinit,
SlabSeg::zlim, plan_in_use in csrc/pn1_net.hip), and workspace rows past the current chunk hold the
last, larger chunk's values.  A fresh process gets zero pages and a long pytest process finite
leftovers of similar tensors, so the other tests cannot see a read of a stale value.  Here every
scenario is a fixed script of engine calls (one theta, fixed (t, i, k) items, dropout on) run on
engines whose buffers tests/_poison.py filled first:

  fill invariance       every output of a script (per-worker losses, every S, p / m / v and S_out
                        of a fused step, bn_stats, the running buffers, predictions) is
                        bit-identical for the ZERO, QNAN and PI fills, and finite;
  history independence  an epoch's S on an engine that ran other epochs before it equals, bit for
                        bit, the S of a freshly QNAN-filled engine that runs only that epoch;
  order swap            S([A, B]) == S([B, A]) bit for bit for chunks of different sizes: a slab
                        row receives at most two addends and the head slab 0 + a + b (two-term
                        fp32 sums commute), the row sum's order is fixed.  vgg11_bn's BatchNorm
                        weight / bias gradients are the exception: k_bn_gacc (csrc/bn_kernels.h)
                        adds a chunk's workers to ONE accumulator in worker order, ((0 + a1) +
                        a2) + b against ((0 + b) + a1) + a2; those tensors are checked against
                        exactly that fp32 sequence of the single-worker gradients instead;
  growing order         [1 worker, then 3 workers] -- the only order in which a later chunk stores
                        into some slab rows and accumulates into others -- against the fp64
                        reference of tests/_flips.py, per chunk (end_epoch mid-epoch);
  empty epoch           begin_epoch, a forward-only chunk, end_epoch: S is exactly zero.

Nothing here has a tolerance of its own: bit-identity, finiteness, exact zero, _flips' bounds.
"""
import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

DEV = "cuda:0"
NTOT = 4                                      # workers of the simulated run (the batch draw's n)
CW = {"PerformantNet1": 8, "vgg11": 3, "vgg11_bn": 3}
# small_chunk_samples() is 256: one or two workers run on the small tiles, three on the large
# ones; one, three and eight workers use different wsplit row counts
ITEMS8 = [(5, 0, 1), (5, 1, 3), (5, 2, 0), (5, 3, 2), (6, 0, 0), (6, 1, 1), (6, 2, 3), (6, 3, 3)]
A3 = [(7, 0, 1), (7, 2, 3), (7, 3, 0)]
B1 = [(7, 1, 2)]
C2 = [(8, 0, 3), (8, 3, 1)]
GROUP = 1 << 20                               # dropout key stride of a batch's 128-sample groups
FILLS = ["qnan", "pi"]


class _Ctx:
    """The pool, one theta per model and the explicit batches, uploaded once."""

    def __init__(self):
        from flsim.data import DevicePool, make_test_pool
        from oracle import model_ref as MR
        from oracle import oracle as O
        self.pool = O.make_pool(0)
        self.dpool = DevicePool(DEV, 0, self.pool)
        self.dtest = DevicePool(DEV, 0, make_test_pool(0, size=400))
        self.theta_np = {m: MR.init_params(0, m) for m in CW}
        self.theta = {m: torch.from_numpy(a).to(DEV) for m, a in self.theta_np.items()}
        rs = np.random.RandomState(11)
        idx = rs.randint(0, self.pool[0].shape[0], 384)
        self.X = torch.from_numpy(O.normalize_lut()[self.pool[0][idx]]).to(DEV)
        self.Y = torch.from_numpy(self.pool[1][idx]).to(DEV)
        # the fused step's inputs (PerformantNet1): one stale entry, Adam state of a third step
        g = torch.Generator(device="cpu").manual_seed(3)
        P = self.theta["PerformantNet1"].numel()
        self.stale = (torch.randn(P + 64, generator=g) * 1e-3).to(DEV)
        self.m0 = (torch.randn(P, generator=g) * 1e-4).to(DEV)
        self.v0 = (torch.rand(P, generator=g) * 1e-6).to(DEV)
        # vgg11_bn evaluation: running buffers that are not the initial 0 / 1
        rs = np.random.RandomState(3)
        self.running = torch.from_numpy(np.concatenate(
            [np.concatenate([rs.normal(0, 0.3, c), rs.uniform(0.5, 2.0, c)])
             for c in MR.VGG_BN_CHANNELS]).astype(np.float32)).to(DEV)
        self._theta_eval = {}

    def theta_eval(self, model):
        """The evaluate script's theta: centred for images [3, 303) of the 400-image test pool
        (vgg11_bn: on the running buffers above, _theta.random_running's)."""
        import _theta
        if model not in self._theta_eval:
            case = _theta.eval_case(model, first=3, n=300, size=400)
            self._theta_eval[model] = torch.from_numpy(case.theta.copy()).to(DEV)
        return self._theta_eval[model]


class _Script:
    """The calls the scripts share; every output is kept under a name in `out`."""

    def __init__(self, eng, ctx):
        self.eng, self.ctx, self.out = eng, ctx, {}
        self.theta = ctx.theta[eng.MODEL]

    def begin(self):
        self.eng.begin_epoch(self.theta)

    def _stats(self, n):
        if not self.eng.STATS_PER_WORKER:
            return None
        return torch.zeros(n, self.eng.STATS_PER_WORKER, device=DEV)

    def _keep_stats(self, name, stats, n):
        if stats is not None:                  # nn.BatchNorm2d's running update, worker order
            self.out[name + ".bn_stats"] = stats
            self.eng.update_running(stats, n)
            self.out[name + ".running"] = self.eng.running.clone()

    def chunk(self, name, items, backward=True, slot=None):
        from flsim.engine import worker_table
        n = len(items)
        loss = torch.zeros(n, device=DEV)
        wt = worker_table(items, DEV)
        if slot is not None:
            self.eng.run_chunk_async(self.theta, self.ctx.dpool, wt, n, NTOT, 0, True, loss, slot)
        else:
            stats = self._stats(n)
            self.eng.run_chunk(self.theta, self.ctx.dpool, wt, n, NTOT, 0, True, loss,
                               backward=backward, stats_out=stats)
            self._keep_stats(name, stats, n)
        self.out[name + ".loss"] = loss

    def groups(self, n, t=9, index=2):
        """WorkerRec rows of an n-sample batch: group g's dropout key is (t, index + g * 2^20)."""
        from flsim.engine import worker_table
        k = -(-n // 128)
        return k, worker_table([(t, index + g * GROUP, 0) for g in range(k)], DEV)

    def batch(self, name, n):
        k, wt = self.groups(n)
        loss = torch.zeros(k, device=DEV)
        stats = self._stats(k)
        self.eng.run_input(self.theta, self.ctx.X[:n], self.ctx.Y[:n], wt, 0, True, loss,
                           stats_out=stats)
        self._keep_stats(name, stats, k)
        self.out[name + ".loss"] = loss

    def end(self, name):
        S = torch.zeros(self.eng.P + 64, device=DEV)     # (the streaming step reads whole float4s)
        self.eng.end_epoch(S)
        self.out[name] = S[:self.eng.P]
        return S


# ---- PerformantNet1 (chunk_workers = 8) -----------------------------------------------------
PN1_EPOCHS = [[ITEMS8], [B1], [A3, B1], [B1, A3]]


def pn1_sync(s, fused=True, only=None, hook=None):
    """Scenario 1.  Epochs [8], [1], [3][1], [1][3], then the empty epoch; epoch 3 ends with the
    fused server step (S_out set, copies of p / m / v) or, fused=False, end_epoch + the streaming
    step.  only=e: that epoch alone, by end_epoch (epoch 3: after each chunk, hook(j, S))."""
    from flsim.engine import Rule
    eng, c = s.eng, s.ctx
    for e, chunks in enumerate(PN1_EPOCHS):
        if only is not None and e != only:
            continue
        s.begin()
        for j, items in enumerate(chunks):
            s.chunk(f"e{e}.c{j}", items)
            if only == 3:
                S = s.end(f"S3.c{j}")
                if hook is not None:
                    hook(j, S)
        if only is not None:
            if only != 3:
                s.end(f"S{e}")
        elif e < 3:
            s.end(f"S{e}")
        else:
            rule = Rule(6, [c.stale], c=5)
            p, m, v = s.theta.clone(), c.m0.clone(), c.v0.clone()
            if fused:
                S = torch.full((eng.P + 64,), float("nan"), device=DEV)
                eng.server_step(S, rule, p, m, v, 3)
                s.out["S3"] = S[:eng.P]
            else:
                eng.aggregate_rule(s.end("S3"), rule, p, m, v, 3)
            s.out["p"], s.out["m"], s.out["v"] = p, m, v
    if only is None:
        s.begin()
        s.chunk("e4.c0", B1, backward=False)
        s.end("S4")


def pn1_chunks(s, pipelined=True):
    """Scenario 2.  One epoch of chunks [1, 3, 2], pipelined on alternating slots or not."""
    s.begin()
    for j, items in enumerate([B1, A3, C2]):
        s.chunk(f"c{j}", items, slot=j if pipelined else None)
    s.end("S")


def pn1_rows(s):
    """Scenario 3.  Deferred rows: three staged calls, their batched forward, one backward over
    384 rows (rows 384 .. 1023 keep the fill); then a ragged 100-sample batch over 128 rows."""
    eng, c = s.eng, s.ctx
    s.begin()
    for g in range(3):
        eng.load_rows(c.X[128 * g:128 * (g + 1)], c.Y[128 * g:128 * (g + 1)], 128 * g, 0)
    k, wt = s.groups(384)
    loss = torch.zeros(k, device=DEV)
    eng.forward_loaded_rows(s.theta, 0, 384, wt, 0, True, loss, 0)
    eng.backward_rows(s.theta, 384, True, 0)
    s.out["e0.loss"] = loss
    s.end("S0")
    s.begin()
    k, wt = s.groups(100)
    loss = torch.zeros(k, device=DEV)
    eng.forward_rows(s.theta, c.X[:100], c.Y[:100], wt, 0, True, loss, 0, 0)
    eng.backward_rows(s.theta, 128, True, 0)
    s.out["e1.loss"] = loss
    s.end("S1")


def pn1_input(s):
    """Scenario 4.  Explicit batches of 100 and 200 samples (two groups, 72 valid in the second)."""
    for n in (100, 200):
        s.begin()
        s.batch(f"n{n}", n)
        s.end(f"S.n{n}")


def evaluate(s):
    """Scenarios 5 and 9.  A ragged evaluation chunk: 300 images from image 3 on, at the model's
    centred theta for those images (tests/_theta.py): the predictions depend on the forward."""
    if s.eng.STATS_PER_WORKER:
        s.eng.running.copy_(s.ctx.running)
    s.out["pred"] = s.eng.evaluate(s.ctx.theta_eval(s.eng.MODEL), s.ctx.dtest, first=3,
                                   n_images=300)


# ---- vgg11 / vgg11_bn (chunk_workers = 3) ---------------------------------------------------
A2 = A3[:2]


def vgg_sync(s):
    """Scenario 6.  Epochs [2][1] and [1][2]; vgg11_bn: also each worker alone (the addends of
    k_bn_gacc's accumulator, for the order-swap test)."""
    epochs = [[A2, B1], [B1, A2]]
    if s.eng.STATS_PER_WORKER:
        epochs += [[A2[:1]], [A2[1:]], [B1]]
    for e, chunks in enumerate(epochs):
        s.begin()
        for j, items in enumerate(chunks):
            s.chunk(f"e{e}.c{j}", items)
        s.end(f"S{e}")


def vgg_input(s):
    """Scenario 7.  Explicit batches: 128 samples; vgg11 also the ragged 100 and 200."""
    for n in (128,) if s.eng.STATS_PER_WORKER else (128, 100, 200):
        s.begin()
        s.batch(f"n{n}", n)
        s.end(f"S.n{n}")


def vgg_rows(s):
    """Scenario 8.  Deferred rows: two staged calls, one forward + backward over 256 of the 384
    workspace rows."""
    eng, c = s.eng, s.ctx
    s.begin()
    for g in range(2):
        eng.load_rows(c.X[128 * g:128 * (g + 1)], c.Y[128 * g:128 * (g + 1)], 128 * g, 0)
    k, wt = s.groups(256)
    loss = torch.zeros(k, device=DEV)
    stats = s._stats(k)
    eng.fwd_bwd_loaded_rows(s.theta, 256, wt, 0, True, loss, *(() if stats is None else (stats,)))
    s._keep_stats("rows", stats, k)
    s.out["rows.loss"] = loss
    s.end("S")


class _Lab:
    """Runs a script on a freshly filled engine; the ZERO runs are kept (the baselines)."""

    def __init__(self):
        self.ctx = _Ctx()
        self.base = {}

    def run(self, model, script, fill, **kw):
        import _poison
        from flsim.engine import engine_class
        eng = engine_class(model)(DEV, chunk_workers=CW[model])
        _poison.fill(eng, _poison.PATTERNS[fill])
        s = _Script(eng, self.ctx)
        script(s, **kw)
        torch.cuda.synchronize()
        out = {k: v.detach().cpu().numpy() for k, v in s.out.items()}
        del s, eng
        return out

    def zero(self, model, script):
        key = (model, script.__name__)
        if key not in self.base:
            out = self.base[key] = self.run(model, script, "zero")
            _assert_finite(out, key)
        return self.base[key]


@pytest.fixture(scope="module")
def lab():
    return _Lab()


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _diff(a, b):
    """Number of elements of a and b that differ as bit patterns."""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    return int((_bits(a) != _bits(b)).sum())


def _assert_finite(out, what):
    bad = {k: int((~np.isfinite(v)).sum()) for k, v in out.items() if v.dtype == np.float32}
    assert not any(bad.values()), (what, {k: n for k, n in bad.items() if n})


def _assert_same(out, base, what):
    assert out.keys() == base.keys(), (what, sorted(out.keys() ^ base.keys()))
    bad = {k: _diff(out[k], base[k]) for k in out}
    assert not any(bad.values()), (what, {k: n for k, n in bad.items() if n})


def _fill_invariance(lab, model, script, fill):
    base = lab.zero(model, script)
    out = lab.run(model, script, fill)
    _assert_finite(out, (model, script.__name__, fill))
    _assert_same(out, base, (model, script.__name__, fill))
    return out, base


# ---- scenario 1 -------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", FILLS)
def test_pn1_sync_fill_invariance_and_empty_epoch(lab, fill):
    out, base = _fill_invariance(lab, "PerformantNet1", pn1_sync, fill)
    for o in (out, base):
        assert not o["S4"].any(), int(np.count_nonzero(o["S4"]))      # the empty epoch
        assert o["S0"].any() and o["S3"].any()


@pytest.mark.parametrize("epoch", [1, 2])
def test_pn1_epoch_is_independent_of_history(lab, epoch):
    """The epoch after a larger one ([1] after [8], [3][1] after [1]) against the same epoch on
    an engine without history whose buffers hold NaNs."""
    base = lab.zero("PerformantNet1", pn1_sync)
    fresh = lab.run("PerformantNet1", pn1_sync, "qnan", only=epoch)
    _assert_finite(fresh, epoch)
    assert set(fresh) <= set(base)
    _assert_same(fresh, {k: base[k] for k in fresh}, ("history", epoch))


def test_pn1_growing_order_reference_and_history(lab):
    """[1 worker, then 3 workers] on a NaN-filled engine without history, end_epoch after each
    chunk: S after the first chunk and the difference of the two S against _flips' fp64 reference
    (scale 1/128); the same epoch at the end of the long script (fused step's S_out) and the
    epoch [1] of the long script give the same bits."""
    import _flips
    from oracle import model_ref as MR
    c = lab.ctx
    sim = MR.OracleSim(NTOT, delay=2, pool=c.pool)
    theta_np = c.theta_np["PerformantNet1"]
    assert np.array_equal(sim.theta, theta_np)
    prev = [np.zeros(theta_np.size, np.float64)]
    eng_of = []

    def hook(j, S):
        items = (B1, A3)[j]
        xs, ys = zip(*[sim.batch(*it, dtype=torch.float64) for it in items])
        x, y = torch.cat(xs), torch.cat(ys)
        noise = _flips.noise_groups([(t, i) for (t, i, _) in items], x.shape[0])
        torch.cuda.synchronize()
        g = S[:theta_np.size].cpu().numpy().astype(np.float64)
        _flips.check_worker_step(g - prev[0], eng_of[0], theta_np, x, y, noise, 1.0 / 128)
        prev[0] = g

    def script(s):
        eng_of.append(s.eng)
        pn1_sync(s, only=3, hook=hook)

    fresh = lab.run("PerformantNet1", script, "qnan")
    eng_of.clear()
    _assert_finite(fresh, "growing order")
    base = lab.zero("PerformantNet1", pn1_sync)
    bad = {"S3": _diff(fresh["S3.c1"], base["S3"]), "S1": _diff(fresh["S3.c0"], base["S1"]),
           "loss.c0": _diff(fresh["e3.c0.loss"], base["e3.c0.loss"]),
           "loss.c1": _diff(fresh["e3.c1.loss"], base["e3.c1.loss"])}
    assert not any(bad.values()), bad


def test_pn1_chunk_order_swap(lab):
    """S([3 workers][1 worker]) == S([1 worker][3 workers]), the losses too."""
    base = lab.zero("PerformantNet1", pn1_sync)
    bad = {"S": _diff(base["S2"], base["S3"]),
           "loss3": _diff(base["e2.c0.loss"], base["e3.c1.loss"]),
           "loss1": _diff(base["e2.c1.loss"], base["e3.c0.loss"])}
    assert not any(bad.values()), bad


def test_pn1_fused_step_equals_reduce_then_stream_after_history(lab):
    """The two end-of-epoch paths share EpochRows: the fused server step at the end of the long
    script against end_epoch + the streaming step in a second pass of it (NaN-filled)."""
    base = lab.zero("PerformantNet1", pn1_sync)
    out = lab.run("PerformantNet1", pn1_sync, "qnan", fused=False)
    _assert_finite(out, "unfused")
    _assert_same(out, base, "fused vs end_epoch + aggregate_rule")


# ---- scenarios 2 - 5 --------------------------------------------------------------------------
@pytest.mark.parametrize("fill", FILLS)
def test_pn1_pipelined_fill_invariance(lab, fill):
    _fill_invariance(lab, "PerformantNet1", pn1_chunks, fill)


def test_pn1_pipelined_equals_synchronous(lab):
    base = lab.zero("PerformantNet1", pn1_chunks)
    out = lab.run("PerformantNet1", pn1_chunks, "qnan", pipelined=False)
    _assert_finite(out, "synchronous")
    _assert_same(out, base, "pipelined vs synchronous")


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("script", [pn1_rows, pn1_input, evaluate], ids=lambda f: f.__name__)
def test_pn1_fill_invariance(lab, script, fill):
    out, _ = _fill_invariance(lab, "PerformantNet1", script, fill)
    if script is evaluate:
        assert out["pred"].shape == (300,) and out["pred"].min() >= 0 and out["pred"].max() <= 9


# ---- scenarios 6 - 9 --------------------------------------------------------------------------
@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("script", [vgg_sync, vgg_input, vgg_rows, evaluate],
                         ids=lambda f: f.__name__)
@pytest.mark.parametrize("model", ["vgg11", "vgg11_bn"])
def test_vgg_fill_invariance(lab, model, script, fill):
    out, _ = _fill_invariance(lab, model, script, fill)
    if script is evaluate:
        assert out["pred"].shape == (300,) and out["pred"].min() >= 0 and out["pred"].max() <= 9


def _bn_affine_mask():
    """True at the BatchNorm weight / bias gradients of vgg11_bn's flat parameter vector."""
    from flsim.engine import VGG11_BN_SHAPES
    mask, conv = [], set()
    for name, shp in VGG11_BN_SHAPES:
        if len(shp) == 4:
            conv.add(name.rsplit(".", 2)[1])
        feat = name.startswith("features.") and name.rsplit(".", 2)[1] not in conv
        mask.append(np.full(int(np.prod(shp)), feat))
    return np.concatenate(mask)


@pytest.mark.parametrize("model", ["vgg11", "vgg11_bn"])
def test_vgg_chunk_order_swap(lab, model):
    """S([2 workers][1 worker]) == S([1 worker][2 workers]) bit for bit.  vgg11_bn's BatchNorm
    weight / bias gradients have one accumulator that k_bn_gacc (csrc/bn_kernels.h) adds the
    chunk's workers to in worker order: those equal exactly that fp32 sequence of the three
    single-worker gradients, ((a1 + a2) + b) and ((b + a1) + a2)."""
    base = lab.zero(model, vgg_sync)
    S0, S1 = base["S0"], base["S1"]
    bad = {"loss2": _diff(base["e0.c0.loss"], base["e1.c1.loss"]),
           "loss1": _diff(base["e0.c1.loss"], base["e1.c0.loss"])}
    if model == "vgg11":
        bad["S"] = _diff(S0, S1)
    else:
        bn = _bn_affine_mask()
        assert bn.sum() == 2 * 2752 and bn.size == S0.size
        a1, a2, b = (base[f"S{e}"][bn] for e in (2, 3, 4))
        bad["S"] = _diff(S0[~bn], S1[~bn])
        bad["bn [2][1]"] = _diff(S0[bn], (a1 + a2) + b)
        bad["bn [1][2]"] = _diff(S1[bn], (b + a1) + a2)
        bad["bn_stats2"] = _diff(base["e0.c0.bn_stats"], base["e1.c1.bn_stats"])
        bad["bn_stats1"] = _diff(base["e0.c1.bn_stats"], base["e1.c0.bn_stats"])
    print("MEASURED", bad)
    assert not any(bad.values()), bad
