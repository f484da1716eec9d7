"""CPU: the conditions the GPU tests at tests/_theta.py's thetas rest on, on the oracle alone.

The GPU evaluation tests (tests/test_gpu_eval.py) require the engine's prediction on every
decisive image to be the fp64 oracle's.  That is a check of the forward only if, at the centred
theta, the predictions depend on the image (spread), most images are decisive (share), the CPU
fp32 port itself passes (agreement), and a small indexing error changes many of them (mutant).
K = 100 is a condition on the theta, not a measurement of the GPU: were a seed change to break
the share, the seed changes, not K.

The golden fixtures pin vgg_forward / vgg_bn_forward to the reference at the init theta only,
where every conv bias is 0 and BatchNorm is the identity map's affine part; the last tests pin
them to the nn.Module's own forward at trained_like.
"""
import numpy as np
import pytest
import torch

import _theta
from oracle import model_ref as MR

MODELS = ["PerformantNet1", "vgg11", "vgg11_bn"]
VGGS = ["vgg11", "vgg11_bn"]


@pytest.mark.parametrize("model", VGGS)
def test_trained_like_recipe(model):
    """Every conv bias and BatchNorm weight / bias is off its init value, channel 0 of every
    BatchNorm weight is exactly 0, an eighth of the others negative; the rest is the init."""
    init, th = MR.init_params(0, model), _theta.trained_like(model)
    assert np.array_equal(th, _theta.trained_like(model)) and th.dtype == np.float32
    off = 0
    for name, shp in MR.param_shapes(model):
        n = int(np.prod(shp))
        a, b = th[off:off + n], init[off:off + n]
        off += n
        if not name.startswith("features.") or len(shp) == 4:
            assert np.array_equal(a, b), name
        elif (b == 1).all():                         # a BatchNorm weight
            assert a[0] == 0 and (a[1:] != 0).all(), name
            assert (a < 0).sum() in (n // 8 - 1, n // 8) and (np.abs(a[1:]) >= 0.5).all(), name
        else:                                        # conv / BatchNorm bias: zeros at init
            assert not b.any() and (a != 0).all(), name


@pytest.mark.parametrize("model", MODELS)
def test_centred_theta_conditions(model):
    """Spread: every class gets at least 3 % of the images.  Decisive share: fp64 margin >
    K * E32 on at least 0.9 of them.  Agreement: the fp32 oracle predicts the fp64 class on every
    decisive image.  Only the last bias differs from the base theta."""
    c = _theta.eval_case(model)
    n = _theta.EVAL_IMAGES[model]
    assert c.l64.shape == (n, 10) and c.theta.dtype == np.float32
    counts = np.bincount(c.ref, minlength=10)
    print("MEASURED", dict(model=model, per_class=(int(counts.min()), int(counts.max())),
                           e32=c.e32, median_margin=float(np.median(c.margin)),
                           decisive=float(c.decisive.mean())))
    assert counts.min() >= 0.03 * n, counts
    # centred: what the fp32 rounding of the shift leaves is far below the margins
    assert np.abs(c.l64.mean(0)).max() <= 1e-2 * np.median(c.margin)
    assert c.decisive.mean() >= 0.9, c.decisive.mean()
    assert np.array_equal(c.ref32[c.decisive], c.ref[c.decisive])
    base = MR.init_params(0, model) if model == "PerformantNet1" else _theta.trained_like(model)
    assert np.array_equal(c.theta[:-10], base[:-10])


@pytest.mark.parametrize("model", VGGS)
def test_uncentred_theta_predicts_one_class(model):
    """What the centring is for: at trained_like itself the last bias decides the argmax."""
    c = _theta.eval_case(model)
    pred = _theta.logits(_theta.trained_like(model), model, c.images[:100],
                         torch.float32, c.running).argmax(1)
    assert len(set(pred.tolist())) <= 2, np.bincount(pred)


@pytest.mark.parametrize("model", VGGS)
def test_bias_slip_mutant_changes_predictions(model):
    """features.0.bias[0:4] copied over [4:8] in the oracle changes at least a quarter of the
    decisive predictions."""
    c = _theta.eval_case(model)
    mut = _theta.logits(_theta.bias_slip(c.theta, model), model, c.images, torch.float64,
                        c.running).argmax(1)
    changed = float((mut[c.decisive] != c.ref[c.decisive]).mean())
    print("MEASURED", dict(model=model, changed=changed))
    assert changed >= 0.25, changed


def _module(model, theta, running):
    """models.py's module in fp64 with theta (and the running buffers) loaded; the classifier's
    Dropouts in eval mode (the oracle takes its dropout masks as an input)."""
    from FL.models import vgg11, vgg11_bn
    mod = (vgg11_bn if model == "vgg11_bn" else vgg11)().double()
    with torch.no_grad():
        for p, a in zip(mod.parameters(), MR.split_flat(theta.astype(np.float64), model)):
            p.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        bns = [m for m in mod.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        st = MR.BNState(torch.float64)
        st.load_flat(running, torch.float64)
        for m, (rm, rv) in zip(bns, st.bufs):
            m.running_mean.copy_(rm)
            m.running_var.copy_(rv)
    return mod, bns, st


@pytest.mark.parametrize("model", VGGS)
def test_oracle_forward_matches_module_at_trained_like(model):
    """vgg_forward / vgg_bn_forward against the module's own forward at trained_like, fp64,
    rtol 1e-12: train mode on 128 images (vgg11_bn: batch statistics, and the running buffers
    advanced from random ones) and eval mode (the random running buffers)."""
    from oracle import oracle as O
    theta = _theta.trained_like(model)
    imgs = _theta.eval_case(model).images[:128]
    x = torch.from_numpy(O.normalize_lut()[imgs]).double()
    params = [torch.from_numpy(np.ascontiguousarray(a))
              for a in MR.split_flat(theta.astype(np.float64), model)]
    mod, bns, st = _module(model, theta, _theta.random_running())
    fwd = (lambda: MR.vgg_bn_forward(params, x, None, st)) if bns else \
        (lambda: MR.vgg_forward(params, x, None))
    for training in (False, True):             # eval first: train mode moves the buffers
        mod.train(training)
        for m in mod.modules():
            if isinstance(m, torch.nn.Dropout):
                m.eval()
        st.training = training
        with torch.no_grad():
            got, ref = fwd().numpy(), mod(x).numpy()
        assert np.ptp(ref, 0).min() > 0                 # the logits depend on the image
        np.testing.assert_allclose(got, ref, rtol=1e-12)
    if bns:
        assert st.num_batches_tracked == int(bns[0].num_batches_tracked) == 1
        run = torch.cat([torch.cat([m.running_mean, m.running_var]) for m in bns]).numpy()
        assert not np.allclose(run, _theta.random_running().astype(np.float64), rtol=1e-3)
        np.testing.assert_allclose(st.flat(), run, rtol=1e-12)
