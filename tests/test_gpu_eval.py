"""GPU: device evaluation (util.py:31-45: eval mode, dropout off, BatchNorm on the running
buffers) of the three networks, at thetas where the prediction depends on the forward.

At an init theta the last layer's bias decides the argmax: every image gets the same one or two
classes and a forward that returned zeros for the last hidden layer would pass.  Here each model
runs at its centred theta (tests/_theta.py: the per-class mean logit of the image set removed
from the last bias; vgg11 / vgg11_bn from trained_like, vgg11_bn on random running buffers), and
the engine's prediction must equal the fp64 oracle's on every decisive image -- fp64 top-2 margin
> 100 x E32, E32 the CPU fp32 port's own worst logit error.  tests/test_cpu_theta.py checks on
the oracle alone that these cases have spread, that >= 0.9 of the images are decisive, that the
CPU fp32 port passes, and that a four-channel bias slip in one layer changes >= 25 % of them.

  flsim_<net>_eval_pool   the whole pool (chunks of 256 and a ragged tail), a ragged inner range
  flsim_<net>_eval_input  the same images as an explicit fp32 batch: the pool path's predictions

The last hidden layer (`e2`, the last chunk's rows in the workspace) against the fp64 oracle's,
next to the CPU fp32 port's, is logged as a MEASURED line and named in a failure: a decisive
image that disagrees is a wrong forward, not a tolerance.
"""
import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs an MI355X")]

DEV = "cuda:0"
CHUNK = 256                                   # chunk_workers = 2
MODELS = ["PerformantNet1", "vgg11", "vgg11_bn"]
AGREE = {"PerformantNet1": 0.995, "vgg11": 0.99, "vgg11_bn": 0.99}
# evaluate_input: a ragged second piece; vgg11_bn's explicit batches are whole 128-sample groups
N_INPUT = {"PerformantNet1": 300, "vgg11": 300, "vgg11_bn": 256}


def _rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


class _Run:
    """One engine per model at its centred theta, the pool uploaded, evaluated once."""

    def __init__(self, model):
        import _theta
        from flsim.data import DevicePool, make_test_pool
        from flsim.engine import engine_class
        self.case = c = _theta.eval_case(model)
        self.eng = engine_class(model)(DEV, chunk_workers=CHUNK // 128)
        if c.running is not None:
            self.eng.running.copy_(torch.from_numpy(c.running))
        n = len(c.images)
        test = make_test_pool(0, size=n)
        assert np.array_equal(test[0], c.images)
        self.dpool = DevicePool(DEV, 0, test)
        self.theta = torch.from_numpy(c.theta.copy()).to(DEV)
        self.pred = self.eng.evaluate(self.theta, self.dpool).cpu().numpy()
        self.e2 = self._e2(n - (n - 1) // CHUNK * CHUNK)

    def _e2(self, rows):
        """rel-L2 of the last chunk's last hidden layer against the fp64 oracle's: the GPU's
        (workspace `e2`) and the CPU fp32 port's."""
        c, eng = self.case, self.eng
        ids = {name: j for j, name in enumerate(eng.WORKSPACE)}
        h64, h32 = c.h64[-rows:], c.h32[-rows:]
        got = eng.workspace_view(ids["e2"], (CHUNK, h64.shape[1])).cpu().numpy()[:rows]
        return dict(rows=rows, gpu=_rel_l2(got.astype(np.float64), h64),
                    cpu32=_rel_l2(h32.astype(np.float64), h64))


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(model):
        if model not in cache:
            cache[model] = _Run(model)
        return cache[model]
    return get


@pytest.mark.parametrize("model", MODELS)
def test_evaluate_pool_decisive_predictions(runs, model):
    """evaluate over the whole pool: the fp64 oracle's class on every decisive image, and the
    former tests' overall agreement with the fp32 oracle's predictions."""
    import _flips
    r = runs(model)
    c = r.case
    assert r.pred.shape == (len(c.images),) and r.pred.dtype == np.int32
    bad = np.nonzero(c.decisive & (r.pred != c.ref))[0]
    agree = float((r.pred == c.ref32).mean())
    _flips.log_measured("eval_" + model, e2=r.e2, decisive=int(c.decisive.sum()),
                        decisive_wrong=int(bad.size), agree32=agree, e32=c.e32,
                        classes=np.bincount(r.pred, minlength=10).tolist())
    assert bad.size == 0, (bad[:10], r.pred[bad[:10]], c.ref[bad[:10]], c.margin[bad[:10]], r.e2)
    assert agree >= AGREE[model], (r.pred != c.ref32).sum()


@pytest.mark.parametrize("model", MODELS)
def test_evaluate_inner_range(runs, model):
    """evaluate(first=100, n_images=37) is that slice of the whole pool's predictions."""
    r = runs(model)
    pred = r.eng.evaluate(r.theta, r.dpool, first=100, n_images=37).cpu().numpy()
    assert len(set(r.pred[100:137].tolist())) >= 5
    assert np.array_equal(pred, r.pred[100:137])


@pytest.mark.parametrize("model", MODELS)
def test_evaluate_input_equals_pool_path(runs, model):
    """flsim_<net>_eval_input on fp32 lut[images] gives the pool path's predictions exactly."""
    from oracle import oracle as O
    r = runs(model)
    n = N_INPUT[model]
    x = torch.from_numpy(O.normalize_lut()[r.case.images[:n]])
    pred = r.eng.evaluate_input(r.theta, x).cpu().numpy()
    assert pred.shape == (n,) and len(set(pred.tolist())) == 10
    assert np.array_equal(pred, r.pred[:n])
