"""Thetas and evaluation cases at which a wrong kernel shows (test helper, CPU only).

The reference's init zeroes every conv bias of the VGG nets (models.py:70-71) and leaves
BatchNorm at weight 1, bias 0: at MR.init_params a wrong layer offset into the biases, a channel
slip in an epilogue, a dropped `* gamma` or a beta that is never added change nothing.  And at
any init theta the argmax of the logits is decided by the last layer's bias alone (the logits'
spread over images is orders of magnitude below their spread over classes), so a prediction test
passes on a forward that returns zeros.

  trained_like      init theta with non-trivial conv biases and BatchNorm weights / biases
  last_hidden, logits  the oracle's eval-mode forward in fp64 / fp32
  centred_for_eval  theta whose last bias has the per-class mean logit of a given image set
                    removed: the prediction then depends on the image
  eval_case         the evaluation case of a model (images, centred theta, running buffers, the
                    fp64 and fp32 oracle logits, the decisive images), computed once per process
                    and shared by tests/test_cpu_theta.py (the conditions) and the GPU tests

An image is decisive when its fp64 top-2 margin exceeds K times E32 = max |logit32 - logit64|,
the CPU fp32 port's own error over the whole image set: an fp32 implementation that is within
K / 2 times the port's error of fp64 must predict the fp64 class there.
"""
import functools

import numpy as np
import torch

from oracle import model_ref as MR
from oracle import oracle as O

K = 100
# images per model: PerformantNet1 keeps the 1000 of its former evaluation test (3 chunks of 256
# and a ragged 232), the VGG nets their 600 (2 chunks and a ragged 88)
EVAL_IMAGES = {"PerformantNet1": 1000, "vgg11": 600, "vgg11_bn": 600}
BASE_THETA = {"PerformantNet1": "init", "vgg11": "trained_like", "vgg11_bn": "trained_like"}
BIAS_STD = {"vgg11": 0.2, "vgg11_bn": 1.0}


@functools.lru_cache(maxsize=None)
def _trained_like(model, seed):
    theta = MR.init_params(0, model).copy()
    rs = np.random.RandomState(seed)
    off, kind = 0, None
    for name, shp in MR.param_shapes(model):
        n = int(np.prod(shp))
        if name.endswith(".weight"):
            kind = ("conv" if len(shp) == 4 else "bn") if name.startswith("features.") else "fc"
        if kind == "conv" and name.endswith(".bias"):
            theta[off:off + n] = rs.normal(0, BIAS_STD[model], n)
        elif kind == "bn" and name.endswith(".weight"):
            g = rs.uniform(0.5, 1.5, n)
            g[rs.permutation(n)[:n // 8]] *= -1
            g[0] = 0.0
            theta[off:off + n] = g
        elif kind == "bn":
            theta[off:off + n] = rs.normal(0, 0.5, n)
        off += n
    assert off == theta.size
    theta.setflags(write=False)
    return theta


def trained_like(model, seed=20):
    """MR.init_params(0, model) of vgg11 / vgg11_bn with, drawn from RandomState(seed) in
    named_parameters order: conv biases N(0, 0.2) (vgg11) or N(0, 1.0) (vgg11_bn: a per-channel
    mean comparable to the std, so the mean subtraction subtracts something); BatchNorm weights
    U(0.5, 1.5), the sign flipped on a random eighth of the channels and channel 0 exactly 0;
    BatchNorm biases N(0, 0.5).  Conv and classifier weights stay as initialised."""
    assert model in BIAS_STD, model
    return _trained_like(model, seed).copy()


def random_running(seed=3):
    """vgg11_bn running buffers that are not the initial (0, 1): [mean | var] per layer."""
    rs = np.random.RandomState(seed)
    return np.concatenate([np.concatenate([rs.normal(0, 0.3, c), rs.uniform(0.5, 2.0, c)])
                           for c in MR.VGG_BN_CHANNELS]).astype(np.float32)


def last_hidden(theta, model, images_u8, dtype=torch.float64, running=None, batch=200):
    """The oracle's eval-mode input of the last Linear (the engines' `e2`; util.py:31-45:
    dropout off, BatchNorm on the running buffers `running`, a flat [mean | var] per layer
    array, None = the initial (0, 1)): the model's forward with an identity as its last layer."""
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    params = [torch.from_numpy(np.ascontiguousarray(a))
              for a in MR.split_flat(np.asarray(theta).astype(np_dt), model)]
    width = params[-2].shape[1]
    params[-2:] = [torch.eye(width, dtype=dtype), torch.zeros(width, dtype=dtype)]
    fwd = MR.NETS[model].forward
    if model in MR.HAS_BN:
        st = MR.BNState(dtype)
        if running is not None:
            st.load_flat(running, dtype)
        st.training = False
        fwd = lambda p, x, noise: MR.vgg_bn_forward(p, x, noise, st)   # noqa: E731
    lut = O.normalize_lut()
    out = []
    with torch.no_grad():
        for s in range(0, len(images_u8), batch):
            x = torch.from_numpy(lut[images_u8[s:s + batch]]).to(dtype)
            out.append(fwd(params, x, None).numpy())
    return np.concatenate(out)


def head(theta, model, hidden):
    """The last Linear of theta on last_hidden's output (in its dtype): the logits."""
    w, b = (torch.from_numpy(np.ascontiguousarray(a).astype(hidden.dtype))
            for a in MR.split_flat(np.asarray(theta), model)[-2:])
    return torch.nn.functional.linear(torch.from_numpy(hidden), w, b).numpy()


def logits(theta, model, images_u8, dtype=torch.float64, running=None):
    """The oracle's eval-mode logits."""
    return head(theta, model, last_hidden(theta, model, images_u8, dtype, running))


def centred_for_eval(theta, model, images_u8, running=None, hidden=None):
    """theta with the per-class mean of its fp64 eval-mode logits over images_u8, rounded to
    fp32, subtracted from the last layer's bias -> (theta, fp64 logits, fp32 logits at it).
    Centring removes the constant that decides the argmax at an init-like theta.  Only the last
    bias changes, so the last hidden layer (hidden = (fp64, fp32), computed here when not given)
    is that of theta."""
    theta = np.array(theta, np.float32)
    h64, h32 = hidden if hidden is not None else (
        last_hidden(theta, model, images_u8, dt, running) for dt in (torch.float64, torch.float32))
    shift = head(theta, model, h64).mean(0).astype(np.float32)
    theta[-shift.size:] -= shift
    return theta, head(theta, model, h64), head(theta, model, h32)


def margins(l64):
    """fp64 top-2 margin per image."""
    s = np.sort(l64, 1)
    return s[:, -1] - s[:, -2]


class EvalCase:
    """images: uint8 [n, 3, 32, 32]; theta: centred fp32; running: flat fp32 or None; h64 / h32,
    l64 / l32: the oracle's last hidden layer and logits; e32 = max |l32 - l64|; ref: fp64
    predictions; decisive: margin > K * e32."""

    def __init__(self, model, images, base=None):
        self.model, self.images = model, images
        self.running = random_running() if model in MR.HAS_BN else None
        if base is None:
            base = MR.init_params(0, model) if BASE_THETA[model] == "init" else trained_like(model)
        self.h64, self.h32 = (last_hidden(base, model, images, dt, self.running)
                              for dt in (torch.float64, torch.float32))
        self.theta, self.l64, self.l32 = centred_for_eval(base, model, images, self.running,
                                                          (self.h64, self.h32))
        self.e32 = float(np.abs(self.l32 - self.l64).max())
        self.margin = margins(self.l64)
        self.decisive = self.margin > K * self.e32
        self.ref = self.l64.argmax(1).astype(np.int32)
        self.ref32 = self.l32.argmax(1).astype(np.int32)
        for a in (self.theta, self.l64, self.l32, self.ref, self.decisive):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def eval_case(model, first=0, n=None, size=None):
    """The model's evaluation case over images [first, first + n) of make_test_pool(0, size)
    (defaults: the whole pool of EVAL_IMAGES[model] images), computed once per process."""
    from flsim.data import make_test_pool
    size = EVAL_IMAGES[model] if size is None else size
    imgs = make_test_pool(0, size=size)[0]
    return EvalCase(model, imgs[first:] if n is None else imgs[first:first + n])


def bias_slip(theta, model):
    """The mutant of the conditions: features.0.bias[0:4] copied over [4:8] (a one-layer,
    four-channel index slip)."""
    theta = np.array(theta, np.float32)
    off = 0
    for name, shp in MR.param_shapes(model):
        if name == "features.0.bias":
            theta[off + 4:off + 8] = theta[off:off + 4]
            return theta
        off += int(np.prod(shp))
    raise KeyError(model)
