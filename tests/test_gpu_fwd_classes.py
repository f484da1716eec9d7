"""The conv2-6 forwards in tap-class row order (csrc/rowmap.h, DESIGN 8b "forward tap classes").

Every PerformantNet1 convolution is 3x3 with padding 2.  The forwards group their GEMM rows by the
filter taps that fall inside the input, and every block runs only the k-steps of its class's taps;
the k-steps left out contributed exact zeros and the others keep their order, so every stored value
must come out bit-identical to the canonical row order (FLSIM_DEBUG_FWD_ROWS=canonical, read per
call, runs that order in the same process).

Sizes: 128 samples (one worker, small tiles: the smallest shape at which every class of every layer
exists, the corner classes less than one large tile), 256 (the small-tile limit) and 384 (large
tiles, three workers' dropout streams), dropout on.  Before every pass the whole workspace is
poisoned (tests/_poison.py, QNAN and PI): a row the map never reaches keeps the pattern, a row it
reaches twice or in the wrong place differs from the canonical pass.

Independent of the canonical path (a bug shared by the map's consumers would pass the above): at
128 samples with dropout off, a3 and a5 against a float64 convolution of the engine's own d1 and
d2.  The error is measured per element in units of 2^-24 (sum |x w| + |b|); the bound is 1.5 x the
largest value this file measured on the parent commit's library (DESIGN 7a's rule), and a dropped
or misplaced tap is an error of a whole product, orders of magnitude above it.
"""
import os

import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

DEV = "cuda:0"
SIZES = (1, 2, 3)                 # workers of 128 samples
ORDERS = ("classes", "canonical")

# name -> (per-sample shape, dtype); d1, a3, d2, a5 are stored split (HM + L parts), d3 is fp32
FLOATS = {"d1": (18, 18, 48), "a3": (20, 20, 96), "d2": (11, 11, 96), "a5": (13, 13, 192),
          "d3": (9408,)}
ARGMAX = {"i1": 18 * 18 * 48, "i2": 11 * 11 * 96, "i3": 7 * 7 * 192}

# largest error of a3 / a5 against float64 on the parent commit's library, in units of
# 2^-24 (sum |x w| + |b|) (test_a3_a5_against_float64 prints it; the class order prints the same
# digits, being bit-identical)
PARENT_MAX_UNITS = {"a3": 4.086175641519433, "a5": 4.688170859385126}


def _set_order(order):
    if order == "canonical":
        os.environ["FLSIM_DEBUG_FWD_ROWS"] = "canonical"
    else:
        os.environ.pop("FLSIM_DEBUG_FWD_ROWS", None)


def _raw(eng, which, nbytes):
    """The first nbytes of workspace tensor `which`, as stored."""
    return eng._workspace_bytes_at(which, nbytes).clone()


def _forward(eng, dpool, theta, table, nw, dropout, pattern):
    """One poisoned forward pass of nw workers; the stored tensors of its samples, as raw words."""
    import _poison
    _poison.fill(eng, pattern)
    eng.begin_epoch(theta)
    loss = torch.zeros(nw, device=DEV)
    eng.run_chunk(theta, dpool, table, nw, 1024, 0, dropout, loss, backward=False)
    torch.cuda.synchronize()
    n = 128 * nw
    ids = {name: eng.WORKSPACE.index(name) for name in eng.WORKSPACE}
    out = {"loss": loss.clone().view(torch.int32).cpu(),
           "loss_s": _raw(eng, ids["loss_s"], 4 * n).view(torch.int32).cpu()}
    for name, shp in FLOATS.items():
        numel = n * int(np.prod(shp))
        lpart = eng.split_part(ids[name])
        out[name] = _raw(eng, ids[name], 4 * numel).view(torch.int32).cpu()
        if lpart >= 0:
            out[name + ".l"] = _raw(eng, lpart, 2 * numel).view(torch.int32).cpu()
    for name, per in ARGMAX.items():
        out[name] = _raw(eng, ids[name], n * per).cpu()
    return out


@pytest.fixture(scope="module")
def setup():
    from flsim.data import DevicePool
    from flsim.engine import PN1Engine
    from oracle import model_ref as MR
    from oracle import oracle as O
    pool = O.make_pool(0)
    sim = MR.OracleSim(1024, delay=50, pool=pool)
    eng = PN1Engine(DEV, chunk_workers=max(SIZES))
    theta = torch.from_numpy(sim.theta.copy()).to(DEV)
    return sim, eng, DevicePool(DEV, 0, pool), theta


@pytest.fixture(scope="module")
def passes(setup):
    """{(nw, order, pattern): stored tensors}, computed once; nothing below changes it."""
    import _poison
    from flsim.engine import worker_table
    _, eng, dpool, theta = setup
    out = {}
    old = os.environ.get("FLSIM_DEBUG_FWD_ROWS")
    try:
        for nw in SIZES:
            rng = np.random.RandomState(200 + nw)
            items = [(5, 2 * i, int(rng.randint(0, 1023))) for i in range(nw)]      # (t, i, k)
            table = worker_table(items, DEV)
            for pname in ("qnan", "pi"):
                for order in ORDERS:
                    _set_order(order)
                    out[nw, order, pname] = _forward(eng, dpool, theta, table, nw, True,
                                                     _poison.PATTERNS[pname])
    finally:
        _set_order("classes")
        if old is not None:
            os.environ["FLSIM_DEBUG_FWD_ROWS"] = old
    return out


@pytest.mark.parametrize("nw", SIZES)
def test_class_order_is_bit_identical_to_canonical(passes, nw):
    """d1, a3, d2, a5 (both split parts), d3, the argmax bytes i1-i3, the per-sample and the
    per-worker losses: equal bit for bit between the two row orders, under both poisons."""
    ref = passes[nw, "canonical", "qnan"]
    for order in ORDERS:
        for pname in ("qnan", "pi"):
            got = passes[nw, order, pname]
            assert got.keys() == ref.keys()
            for name in ref:
                assert torch.equal(got[name], ref[name]), (nw, order, pname, name)
    assert torch.isfinite(ref["loss"].view(torch.float32)).all()


@pytest.mark.parametrize("nw", SIZES)
def test_no_stored_element_keeps_the_poison(passes, nw):
    """Every word of the stored tensors of the pass's samples was written by the pass: none holds
    the pattern the workspace was filled with (as a 32-bit word of the stored form)."""
    import _poison
    for order in ORDERS:
        for pname in ("qnan", "pi"):
            pat = _poison.PATTERNS[pname]
            pat = pat - (1 << 32) if pat >= 1 << 31 else pat
            got = passes[nw, order, pname]
            for name in list(FLOATS) + [k for k in got if k.endswith(".l")] + ["loss_s"]:
                left = int((got[name] == pat).sum())
                assert left == 0, (nw, order, pname, name, left)
    # the argmax bytes are zeroed by the fill: every window position occurs, so they were written
    for name in ARGMAX:
        vals = passes[nw, "classes", "qnan"][name]
        assert int(vals.max()) == 3 and int(vals.min()) == 0, name


def _conv64_units(x, w, b, got):
    """Largest |got - relu(conv64(x, w) + b)| per element in units of 2^-24 (sum |x w| + |b|).
    x [n][IH][IW][ci] and got [n][OH][OW][co] fp32 on the device, w [co][ci][3][3], b [co]."""
    co = w.shape[0]
    w64 = w.double().reshape(co, -1).to(DEV)
    b64 = b.double().to(DEV)
    worst = 0.0
    for r in range(0, x.shape[0], 32):
        xr = x[r:r + 32].permute(0, 3, 1, 2).double()
        col = torch.nn.functional.unfold(xr, 3, padding=2)                  # [32][ci * 9][L]
        ref = torch.relu(torch.matmul(w64, col) + b64[None, :, None])      # [32][co][L]
        mag = torch.matmul(w64.abs(), col.abs()) + b64.abs()[None, :, None]
        g = got[r:r + 32].permute(0, 3, 1, 2).reshape(ref.shape).double()
        err = (g - ref).abs()
        units = torch.where(err > 0, err / (mag * 2.0 ** -24), torch.zeros_like(err))
        assert torch.isfinite(units).all()
        worst = max(worst, float(units.max()))
    return worst


def test_a3_a5_against_float64(setup):
    """a3 = relu(conv3(d1)) and a5 = relu(conv5(d2)) of 128 samples, dropout off, against float64
    on the engine's own d1 and d2: within 1.5 x the parent commit's largest error."""
    from flsim.engine import PN1_SHAPES, worker_table
    sim, eng, dpool, theta = setup
    _set_order("classes")
    offs = np.concatenate([[0], np.cumsum([int(np.prod(s)) for _, s in PN1_SHAPES])])
    part = lambda j: torch.from_numpy(                                       # noqa: E731
        sim.theta[offs[j]:offs[j + 1]].copy()).view(PN1_SHAPES[j][1])
    eng.begin_epoch(theta)
    loss = torch.zeros(1, device=DEV)
    eng.run_chunk(theta, dpool, worker_table([(5, 0, 17)], DEV), 1, 1024, 0, False, loss,
                  backward=False)
    torch.cuda.synchronize()
    ids = {name: eng.WORKSPACE.index(name) for name in eng.WORKSPACE}
    W = lambda name: eng.workspace_view(ids[name], (128,) + FLOATS[name])    # noqa: E731
    measured = {"a3": _conv64_units(W("d1"), part(4), part(5), W("a3")),
                "a5": _conv64_units(W("d2"), part(8), part(9), W("a5"))}
    for name, units in measured.items():
        print("MEASURED", name, "max error", repr(units), "x 2^-24 (sum |x w| + |b|), parent",
              PARENT_MAX_UNITS[name])
    for name, units in measured.items():
        assert units <= 1.5 * PARENT_MAX_UNITS[name], (name, units)
