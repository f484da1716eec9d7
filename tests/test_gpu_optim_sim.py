"""GPU: FLSimulation and the FL.agents facade with torch.optim.SGD as the central optimizer.

The simulation is replayed on the host from its own kept S_t and schedule trace: the oracle's
cascade mean over [S_t] * c_t + the stale entries, then torch.optim.SGD itself on CPU tensors.
theta and the momentum buffer are compared bit for bit after every epoch; the fused, streaming and
resumed runs must end bit-identical to that run.
"""
import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

DEV = "cuda:0"
N, DELAY, EPOCHS = 4, 2, 5
OPT = dict(optimizer="sgd", momentum=0.9, weight_decay=5e-4)
LR = 0.01


@pytest.fixture(scope="module")
def pool():
    from oracle import oracle as O
    return O.make_pool(0)


def _sim(pool, **kw):
    from flsim.sim import FLSimulation
    return FLSimulation(N, delay=DELAY, throttle=True, device=DEV, chunk_workers=2, pool=pool,
                        lr=LR, **{**OPT, **kw})


def _mean(entries, sizes):
    from oracle import oracle as O
    g = np.empty_like(entries[0])
    off = 0
    for n in sizes:
        g[off:off + n] = O.cascade_mean([e[off:off + n] for e in entries])
        off += n
    return g


@pytest.fixture(scope="module")
def straight(pool):
    """The keep_S run: per epoch (S_t, theta, buffer), its trace and theta_0."""
    sim = _sim(pool, keep_S=True)
    assert sim.v is None and sim.m is not None
    theta0 = sim.theta.cpu().numpy().copy()
    rec = []
    for _ in range(EPOCHS):
        sim.epoch()
        rec.append((sim.comm[:sim.P].cpu().numpy().copy(), sim.theta.cpu().numpy().copy(),
                    sim.m.cpu().numpy().copy()))
    return dict(theta0=theta0, rec=rec, trace=list(sim.trace), sizes=list(sim.engine.SIZES),
                losses=sim.losses())


def test_simulation_replays_on_host_bit_exact(straight):
    tp = torch.nn.Parameter(torch.from_numpy(straight["theta0"].copy()))
    opt = torch.optim.SGD([tp], lr=LR, momentum=0.9, weight_decay=5e-4)
    ticks = []
    for t, (plan, (S, theta, buf)) in enumerate(zip(straight["trace"], straight["rec"])):
        if plan.pushed:
            ticks.append(t)
        ents = [S] * plan.c_t + [straight["rec"][src][0] for (_, src) in plan.stale]
        tp.grad = torch.from_numpy(_mean(ents, straight["sizes"]))
        opt.step()
        bad_p = int((tp.detach().numpy().view(np.uint32) != theta.view(np.uint32)).sum())
        bad_m = int((opt.state[tp]["momentum_buffer"].numpy().view(np.uint32) !=
                     buf.view(np.uint32)).sum())
        print(t, plan.c_t, plan.stale, bad_p, bad_m)
        assert (bad_p, bad_m) == (0, 0), (t, bad_p, bad_m)
    assert ticks == [0, 2, 4]           # the slow worker computes at t = 0, 2, 4: pops at 2 and 4
    assert [t for t, pl in enumerate(straight["trace"]) if pl.stale] == [2, 4]


@pytest.mark.parametrize("kw", [dict(), dict(fused=False)], ids=["fused", "streaming"])
def test_epoch_paths_end_bit_identical(pool, straight, kw):
    sim = _sim(pool, **kw)
    for _ in range(EPOCHS):
        sim.epoch()
    assert sim.v is None
    assert np.array_equal(sim.theta.cpu().numpy().view(np.uint32),
                          straight["rec"][-1][1].view(np.uint32))
    assert np.array_equal(sim.m.cpu().numpy().view(np.uint32),
                          straight["rec"][-1][2].view(np.uint32))
    assert sim.losses() == straight["losses"]


def test_checkpoint_resume_and_mismatch(pool, straight, tmp_path):
    from flsim.sim import FLSimulation
    a = _sim(pool)
    for _ in range(3):
        a.epoch()
    path = tmp_path / "ck.pt"
    a.save_checkpoint(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["config"]["optimizer"] == "sgd" and ck["config"]["momentum"] == 0.9
    assert "v" not in ck
    b = _sim(pool)
    b.restore(path)
    for _ in range(3, EPOCHS):
        b.epoch()
    assert np.array_equal(b.theta.cpu().numpy().view(np.uint32),
                          straight["rec"][-1][1].view(np.uint32))
    assert np.array_equal(b.m.cpu().numpy().view(np.uint32),
                          straight["rec"][-1][2].view(np.uint32))
    adam = FLSimulation(N, delay=DELAY, throttle=True, device=DEV, chunk_workers=2, pool=pool,
                        lr=LR, optimizer="adam")
    with pytest.raises(ValueError, match="optimizer"):
        adam.restore(path)
    # a checkpoint from before the optimizer was recorded restores as Adam without weight decay
    ck_adam = adam.checkpoint()
    for k in ("optimizer", "weight_decay", "momentum", "dampening", "nesterov"):
        del ck_adam["config"][k]
    FLSimulation(N, delay=DELAY, throttle=True, device=DEV, chunk_workers=2, pool=pool,
                 lr=LR).restore(ck_adam)
    with pytest.raises(ValueError, match="optimizer"):
        _sim(pool).restore(ck_adam)


def _facade_loop(pool, read_grads):
    """The loop of test_gpu_parity.test_reference_api_facade_loop (main.py:126-188 against the
    drop-in FL.agents API) with torch.optim.SGD; read_grads reads the epoch's .grad before every
    update_model (then Central takes the buffered path, otherwise the fused one).  Returns the
    model, the optimizer, the Central, per-epoch theta and (read_grads) per-epoch (entry epochs,
    S_t)."""
    import torch.nn as nn
    from FL.agents import Agg, Central, Worker, rule
    from FL.models import PerformantNet1
    from oracle import oracle as O
    n, d, ep = 3, 2, 4
    torch.manual_seed(0)
    model = PerformantNet1().to(DEV)
    optimizer = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9)
    central = Central(model, optimizer)
    workers = [Worker(nn.CrossEntropyLoss()) for _ in range(n)]
    agg = Agg(rule)
    rs = np.random.RandomState(0)
    lists = O.class_lists(pool[1])
    lut = O.normalize_lut()
    pesky, window, gone = [], 0, False
    thetas, reads = [], []
    for t in range(ep):
        weight_ups, srcs = [], []
        model.train()
        for i in range(n):
            k = rs.randint(0, n)
            idx = O.batch_indices(0, t, i, k, n, lists)
            x = torch.from_numpy(lut[pool[0][idx]]).to(DEV)
            y = torch.from_numpy(pool[1][idx]).to(DEV)
            if i == n - 1:
                gone = False
                ups = src = None
                if t == 0 or t % d == 0:
                    workers[i].model = central.model
                    ups, _ = workers[i].fwd_bkwd(x, y)
                    pesky.append((ups, t))
                    ups = None
                    if t != 0:
                        ups, src = pesky.pop(0)
                if ups is not None:
                    weight_ups.append(ups)
                    srcs.append(src)
                    gone = True
            elif window <= 0:
                workers[i].model = central.model
                ups, _ = workers[i].fwd_bkwd(x, y)
                weight_ups.append(ups)
                srcs.append(t)
                window = 1 if gone else 2
            if window > 0:
                window -= 1
        if read_grads:
            cur = weight_ups[srcs.index(t)]
            S = torch.cat([u.detach().reshape(-1) for u in cur]).cpu().numpy().copy()
            reads.append((srcs, S))
        central.update_model(agg.rule(weight_ups))
        thetas.append(torch.cat([p.detach().reshape(-1) for p in model.parameters()])
                      .cpu().numpy().copy())
    return model, optimizer, central, thetas, reads


def test_facade_sgd_buffered_fused_and_host_replay(pool):
    from flsim.engine import PN1_SIZES
    torch.manual_seed(0)
    from FL.models import PerformantNet1
    theta0 = torch.cat([p.detach().reshape(-1) for p in PerformantNet1().parameters()]).numpy()
    model_a, optim_a, central_a, th_a, reads = _facade_loop(pool, True)
    _, _, central_b, th_b, _ = _facade_loop(pool, False)
    for t, (x, y) in enumerate(zip(th_a, th_b)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), t
    ma = central_a.ctx.m[:central_a.ctx.P]
    assert torch.equal(ma, central_b.ctx.m[:central_b.ctx.P])
    # host replay from the gradients the buffered run read
    tp = torch.nn.Parameter(torch.from_numpy(theta0.copy()))
    opt = torch.optim.SGD([tp], lr=0.01, momentum=0.9)
    assert any(len(set(srcs)) > 1 for srcs, _ in reads)          # a stale entry took part
    for t, (srcs, _) in enumerate(reads):
        tp.grad = torch.from_numpy(_mean([reads[s][1] for s in srcs], PN1_SIZES))
        opt.step()
        bad = int((tp.detach().numpy().view(np.uint32) != th_a[t].view(np.uint32)).sum())
        print(t, srcs, bad)
        assert bad == 0, (t, bad)
    assert np.array_equal(opt.state[tp]["momentum_buffer"].numpy().view(np.uint32),
                          ma.cpu().numpy().view(np.uint32))
    # optim.state is what torch itself would hold: momentum_buffer views of the engine's buffer
    off = 0
    for p in model_a.parameters():
        st = optim_a.state[p]
        assert set(st) == {"momentum_buffer"}
        assert st["momentum_buffer"].shape == p.shape
        assert torch.equal(st["momentum_buffer"].reshape(-1), ma[off:off + p.numel()])
        assert st["momentum_buffer"].data_ptr() == ma[off:].data_ptr()
        off += p.numel()
    fresh_model = PerformantNet1()
    fresh = torch.optim.SGD(fresh_model.parameters(), lr=0.01, momentum=0.9)
    fresh.load_state_dict(optim_a.state_dict())
    p0 = next(fresh_model.parameters())
    assert torch.equal(fresh.state[p0]["momentum_buffer"].reshape(-1),
                       ma[:p0.numel()].cpu())


def test_facade_plain_sgd_and_adamw_accepted(pool):
    """Plain SGD publishes no optimizer state; AdamW publishes the Adam family's."""
    import torch.nn as nn
    from FL.agents import Agg, Central, Worker, rule
    from FL.models import PerformantNet1
    from oracle import oracle as O
    idx = O.batch_indices(0, 0, 0, 0, 2, O.class_lists(pool[1]))
    x = torch.from_numpy(O.normalize_lut()[pool[0][idx]]).to(DEV)
    y = torch.from_numpy(pool[1][idx]).to(DEV)
    for make, keys in ((lambda ps: torch.optim.SGD(ps, lr=0.01), set()),
                       (lambda ps: torch.optim.AdamW(ps, lr=1e-3, weight_decay=1e-2),
                        {"step", "exp_avg", "exp_avg_sq"})):
        torch.manual_seed(0)
        model = PerformantNet1().to(DEV)
        before = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).clone()
        optimizer = make(model.parameters())
        central = Central(model, optimizer)
        w = Worker(nn.CrossEntropyLoss())
        w.model = central.model
        ups, _ = w.fwd_bkwd(x, y)
        central.update_model(Agg(rule).rule([ups]))
        after = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
        assert not torch.equal(before, after)
        p0 = next(model.parameters())
        assert set(optimizer.state.get(p0, {})) == keys


def test_facade_still_refuses_other_optimizers():
    from FL.agents import Central
    from FL.models import PerformantNet1
    model = PerformantNet1()
    with pytest.raises(NotImplementedError, match="SGD"):
        Central(model, torch.optim.Adam(model.parameters(), amsgrad=True))
    with pytest.raises(NotImplementedError, match="SGD"):
        Central(model, torch.optim.RMSprop(model.parameters()))
    with pytest.raises(NotImplementedError):
        Central(model, torch.optim.SGD(model.parameters(), lr=0.1, maximize=True))
