"""The dense conv2-6 weight gradients (csrc/net_kernels.h conv_wgrad_dense): reduced over the
S IH IW input pixels instead of the S OH OW padded output pixels (conv3-6 in the product, conv2
behind its switch), the bias gradient from the unshifted tap's dZ tiles plus the ring of the map
they leave out (loaders.h TapRowsKM::bias_ring): every stored dZ pixel once.

References as in test_gpu_survey_chunk.py::_conv_refs, on the GPU's own layer input and dZ from
the workspace: unfold + float64 matmul, and torch-CPU `convolution_backward` per worker as the fp32
port.  Criterion, per tensor T:
    ||g - g64|| <= 2 ||g_cpu32 - g64|| + 1e-7 ||g64||.

Sizes: 1 worker (128 samples) and 3 workers (384 samples) in one chunk.  S is always a multiple of
128, so S IH IW is a multiple of the 16-pixel k-step for every layer (IH IW = 1156, 324, 400, 121,
169) and the reduction has no K tail to cover.  384 samples put image and row boundaries at every
residue inside the k-steps of conv5 (121 pixels per image) and conv6 (169): 121 and 169 are odd,
so the first pixel of image i sits at residue (i * 121) % 16, which takes all 16 values over 16
consecutive images.
"""
import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

DEV = "cuda:0"
LAYERS = ("conv2", "conv3", "conv4", "conv5", "conv6")
SIZES = (1, 3)


@pytest.fixture(scope="module")
def runs():
    """{nw: dict(S=[S of two identical epochs], refs={layer: _conv_refs tuple}, x=..., dz=...)}
    computed once; nothing below changes it."""
    import test_gpu_survey_chunk as T
    from flsim.data import DevicePool
    from flsim.engine import PN1_SHAPES, PN1Engine, worker_table
    from oracle import model_ref as MR
    from oracle import oracle as O
    pool = O.make_pool(0)
    sim = MR.OracleSim(1024, delay=50, pool=pool)
    eng = PN1Engine(DEV, chunk_workers=max(SIZES))
    dpool = DevicePool(DEV, 0, pool)
    theta = torch.from_numpy(sim.theta.copy()).to(DEV)
    offs = np.concatenate([[0], np.cumsum([int(np.prod(s)) for _, s in PN1_SHAPES])])
    tparts = [torch.from_numpy(sim.theta[offs[j]:offs[j + 1]].copy()).view(s)
              for j, (_, s) in enumerate(PN1_SHAPES)]
    out = {}
    for nw in SIZES:
        rng = np.random.RandomState(100 + nw)
        items = [(7, 2 * i, int(rng.randint(0, 1023))) for i in range(nw)]      # (t, i, k)
        table = worker_table(items, DEV)
        n = 128 * nw
        refs, xs, dzs = {}, {}, {}
        for stop in (5, 3, 0):
            T._run(eng, dpool, theta, [table], [nw], stop)
            for name in LAYERS:
                st, xi, xshape, di, dshape, _ = T.CONV[name]
                if st != stop:
                    continue
                refs[name] = T._conv_refs(eng, name, n, tparts)
                xs[name] = eng.workspace_view(xi, (eng.max_samples,) + xshape)[:n].clone()
                dzs[name] = eng.workspace_view(di, (eng.max_samples,) + dshape)[:n].clone()
        S = [T._run(eng, dpool, theta, [table], [nw], 0).clone() for _ in range(2)]
        out[nw] = dict(S=S, refs=refs, x=xs, dz=dzs, offs=offs, shapes=PN1_SHAPES,
                       index={name: T.CONV[name][-1] for name in LAYERS})
    return out


def _bound(c32, r64):
    """SURVEY 8(c)'s right-hand side."""
    return 2 * np.linalg.norm(c32 - r64) + 1e-7 * np.linalg.norm(r64)


def _gpu(run, name, part):
    j = run["index"][name] + part
    return run["S"][0][run["offs"][j]:run["offs"][j + 1]].double().cpu().numpy()


@pytest.mark.parametrize("nw", SIZES)
def test_dense_weight_and_bias_gradients_meet_survey_8c(runs, nw):
    """conv2-6 weight and bias gradients of 128 / 384 samples meet SURVEY 8(c) against fp64 and the
    CPU fp32 port on the GPU's own inputs."""
    import _flips
    run = runs[nw]
    gpu, c32, r64, shapes = [], [], [], []
    for name in LAYERS:
        ref = run["refs"][name]
        for part in (0, 1):                      # weight, bias
            gpu.append(_gpu(run, name, part))
            r64.append(ref[part].numpy())
            c32.append(ref[2 + part].numpy())
            shapes.append(run["shapes"][run["index"][name] + part])
    ratios = _flips.survey_ratios(np.concatenate(gpu), np.concatenate(c32), np.concatenate(r64),
                                  shapes)
    _flips.assert_survey(ratios, f"pn1_wgrad_dense_nw{nw}")


@pytest.mark.parametrize("nw", SIZES)
def test_bias_gradient_sums_every_output_pixel(runs, nw):
    """The bias gradient is the fp64 sum over ALL stored dZ pixels.  dZ's border rows and columns
    (0, 1, OH-2, OH-1; conv6's compact 14 x 14 map of a 15 x 15 output: 0, 1, 13, its row and
    column 14 are structurally zero) hold non-zero entries, and the sum over any single tap's
    IH x IW window misses the bound by itself, so a bias that summed one window would fail."""
    run = runs[nw]
    for name in LAYERS:
        dz = run["dz"][name].double()                       # [n][DH][DH][co]
        dh = dz.shape[1]
        ih = run["x"][name].shape[1]
        border = (0, 1, dh - 2, dh - 1) if dh == ih + 2 else (0, 1, dh - 1)
        for b in border:
            assert dz[:, b].abs().sum().item() > 0, (name, "row", b)
            assert dz[:, :, b].abs().sum().item() > 0, (name, "column", b)
        b64, b32 = run["refs"][name][1].numpy(), run["refs"][name][3].numpy()
        full = dz.sum((0, 1, 2)).cpu().numpy()
        assert np.allclose(full, b64, rtol=1e-12, atol=0), name    # the reference IS the full sum
        bound = _bound(b32, b64)
        for kh in range(3):
            for kw in range(3):
                win = dz[:, 2 - kh:2 - kh + ih, 2 - kw:2 - kw + ih].sum((0, 1, 2)).cpu().numpy()
                assert np.linalg.norm(win - b64) > bound, (name, kh, kw)
        err = np.linalg.norm(_gpu(run, name, 1) - b64)
        print("MEASURED", name, "bias err", err, "bound", bound)
        assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("nw", SIZES)
def test_conv6_compact_edge_reads_zero(runs, nw):
    """conv6's dZ is stored compact (14 x 14 of 15 x 15): taps kh == 0 / kw == 0 reach row / column
    14 from input row / column 12, which must read as zero and not as the next row or image.  The
    weight-gradient slices of those taps meet the criterion on their own against the reference
    whose dZ row and column 14 are zero; the input's row and column 12 and the dZ pixels an
    unmasked read would hit (the next row's / image's first pixels) are non-zero, so a missing
    mask would show."""
    run = runs[nw]
    x, dz = run["x"]["conv6"], run["dz"]["conv6"]
    assert x[:, 12].abs().sum().item() > 0 and x[:, :, 12].abs().sum().item() > 0
    assert dz[:, :, 0].abs().sum().item() > 0 and dz[:, 0].abs().sum().item() > 0
    g64, _, g32, _ = run["refs"]["conv6"]
    shp = (192, 192, 3, 3)
    g = _gpu(run, "conv6", 0).reshape(shp)
    g64, g32 = g64.numpy().reshape(shp), g32.numpy().reshape(shp)
    for sl in ((slice(None), slice(None), 0), (slice(None), slice(None), slice(None), 0)):
        err = np.linalg.norm(g[sl] - g64[sl])
        bound = _bound(g32[sl], g64[sl])
        print("MEASURED conv6 edge taps err", err, "bound", bound)
        assert err <= bound, (err, bound)


@pytest.mark.parametrize("nw", SIZES)
def test_two_runs_are_bit_identical(runs, nw):
    """Two epochs of the same chunk give bit-identical slab-summed gradients (fixed-order sums, no
    atomics), weight and bias of every layer."""
    a, b = runs[nw]["S"]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
