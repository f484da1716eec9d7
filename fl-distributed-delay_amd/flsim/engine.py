"""Worker-batched network engines: device buffers + the C-ABI calls of one epoch.

  begin_epoch(theta)      pack theta_t, zero the gradient slabs        (start of main.py:126)
  run_chunk(...)          worker-batched fwd/bwd of a chunk of workers (agents.py:32-40, xN)
  end_epoch(S)            S_t = sum of the epoch's gradients           (agents.py:35 accumulation)
  aggregate_adam(...)     fused rule() + Central.update_model          (main.py:23-25,184,188)

PN1Engine runs models.py:PerformantNet1 (the model main.py:97 builds) through flsim_pn1_*;
VGG11Engine runs models.py:vgg11() (models.py:50-103, configs[4]'s larger CNN) through
flsim_vgg11_*; VGG11BNEngine runs vgg11_bn() (models.py:106-108) through flsim_vgg11_bn_* and
keeps its BatchNorm running buffers.  Both entry-point families share one contract (include/flsim.h).
"""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np
import torch

import math

from ._lib import (ATTACK_KINDS, ATTACK_OPT_STATS, MAX_ARRAYS, OPT_ATTACK_DIRS, OPT_ATTACK_KINDS,
                   OPT_KINDS, ROBUST_KINDS, FlsimAttack, FlsimAttackOpt, FlsimAttackOptScratch,
                   FlsimBulyan,
                   FlsimBulyanScratch, FlsimCclip,
                   FlsimCclipScratch, FlsimClip, FlsimGeomed, FlsimGeomedScratch, FlsimKrum,
                   FlsimKrumScratch, FlsimNnm, FlsimNnmScratch, FlsimOptim,
                   FlsimRobust, FlsimRule, FlsimRuleComp, FlsimRuleWeights, WorkerRec, check, lib,
                   ptr, stream_ptr)

# named_parameters() order of models.py:PerformantNet1 (models.py:13-25)
PN1_SHAPES = [
    ("conv1.weight", (48, 3, 3, 3)), ("conv1.bias", (48,)),
    ("conv2.weight", (48, 48, 3, 3)), ("conv2.bias", (48,)),
    ("conv3.weight", (96, 48, 3, 3)), ("conv3.bias", (96,)),
    ("conv4.weight", (96, 96, 3, 3)), ("conv4.bias", (96,)),
    ("conv5.weight", (192, 96, 3, 3)), ("conv5.bias", (192,)),
    ("conv6.weight", (192, 192, 3, 3)), ("conv6.bias", (192,)),
    ("linear1.weight", (512, 9408)), ("linear1.bias", (512,)),
    ("linear2.weight", (256, 512)), ("linear2.bias", (256,)),
    ("linear3.weight", (10, 256)), ("linear3.bias", (10,)),
]
# named_parameters() order of models.py:vgg11() (features = make_layers(cfg 'A'),
# models.py:80-98; classifier models.py:57-65)
VGG11_SHAPES = [
    ("features.0.weight", (64, 3, 3, 3)), ("features.0.bias", (64,)),
    ("features.3.weight", (128, 64, 3, 3)), ("features.3.bias", (128,)),
    ("features.6.weight", (256, 128, 3, 3)), ("features.6.bias", (256,)),
    ("features.8.weight", (256, 256, 3, 3)), ("features.8.bias", (256,)),
    ("features.11.weight", (512, 256, 3, 3)), ("features.11.bias", (512,)),
    ("features.13.weight", (512, 512, 3, 3)), ("features.13.bias", (512,)),
    ("features.16.weight", (512, 512, 3, 3)), ("features.16.bias", (512,)),
    ("features.18.weight", (512, 512, 3, 3)), ("features.18.bias", (512,)),
    ("classifier.1.weight", (512, 512)), ("classifier.1.bias", (512,)),
    ("classifier.4.weight", (512, 512)), ("classifier.4.bias", (512,)),
    ("classifier.6.weight", (10, 512)), ("classifier.6.bias", (10,)),
]
# named_parameters() order of models.py:vgg11_bn() (make_layers(cfg 'A', batch_norm=True):
# Conv2d, BatchNorm2d, ReLU per conv, models.py:88-89) and its BatchNorm buffers
_BN_IDX = (0, 4, 8, 11, 15, 18, 22, 25)      # conv module index in features; BatchNorm = +1
VGG11_BN_SHAPES = []
for _j, (_, _shp) in enumerate(VGG11_SHAPES[:16:2]):
    _co = _shp[0]
    VGG11_BN_SHAPES += [(f"features.{_BN_IDX[_j]}.weight", _shp),
                        (f"features.{_BN_IDX[_j]}.bias", (_co,)),
                        (f"features.{_BN_IDX[_j] + 1}.weight", (_co,)),
                        (f"features.{_BN_IDX[_j] + 1}.bias", (_co,))]
VGG11_BN_SHAPES += VGG11_SHAPES[16:]
VGG11_BN_BUFFERS = [(f"features.{i + 1}", int(shp[0]))
                    for i, (_, shp) in zip(_BN_IDX, VGG11_SHAPES[:16:2])]
PN1_SIZES = [int(np.prod(s)) for _, s in PN1_SHAPES]
VGG11_SIZES = [int(np.prod(s)) for _, s in VGG11_SHAPES]
SAMPLES_PER_WORKER = 128


# a kind's conventional defaults where they differ from Optim's own (torch.optim.Adagrad; Yogi as
# Zaheer et al. 2018 and flsim.optim.Yogi state them)
OPTIM_DEFAULTS = {
    "adagrad": dict(lr=1e-2, eps=1e-10, initial_accumulator_value=0.0),
    "yogi": dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-3, initial_accumulator_value=1e-6),
}


def optim_defaults(kind):
    """The conventional hyper-parameters of `kind` as a dict of Optim fields (lr, betas, eps,
    initial_accumulator_value): torch's for "adam", "adamw", "sgd" (lr 1e-3 as main.py:106) and
    "adagrad", the Yogi paper's for "yogi"."""
    if kind not in OPT_KINDS:
        raise ValueError(f"optimizer {kind!r} (supported: {sorted(OPT_KINDS)})")
    d = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, initial_accumulator_value=0.0)
    d.update(OPTIM_DEFAULTS.get(kind, {}))
    return d


@dataclasses.dataclass(frozen=True)
class Optim:
    """flsim_optim (include/flsim.h): the update rule of a server step, torch's hyper-parameter
    names.  kind "adam" = torch.optim.Adam (weight_decay: coupled L2), "adamw" = torch.optim.AdamW
    (decoupled), "sgd" = torch.optim.SGD (momentum, dampening, weight_decay, nesterov), "adagrad" =
    torch.optim.Adagrad (lr_decay, weight_decay, eps; FedAdagrad with beta1 = 0), "yogi" =
    flsim.optim.Yogi (betas, eps, weight_decay; FedYogi, no bias correction).
    initial_accumulator_value is what the caller fills the state array with before step 1
    (Adagrad: m = sum; Yogi: v = exp_avg_sq); the library never initialises state."""
    kind: str = "adam"
    lr: float = 1e-3
    betas: tuple = (0.9, 0.999)
    eps: float = 1e-8
    weight_decay: float = 0.0
    momentum: float = 0.0
    dampening: float = 0.0
    nesterov: bool = False
    lr_decay: float = 0.0
    initial_accumulator_value: float = 0.0

    @property
    def n_state(self):
        """State arrays the kind owns: 2 (m, v), 1 (the momentum buffer or Adagrad's sum in m)
        or 0."""
        if self.kind == "adagrad":
            return 1
        if self.kind != "sgd":
            return 2
        return 1 if self.momentum != 0 else 0

    def validate(self):
        """The ValueErrors torch's constructors raise (the library refuses the same cases)."""
        if self.kind not in OPT_KINDS:
            raise ValueError(f"optimizer {self.kind!r} (supported: {sorted(OPT_KINDS)})")
        if not self.lr >= 0:
            raise ValueError(f"Invalid learning rate: {self.lr}")
        if not self.weight_decay >= 0:
            raise ValueError(f"Invalid weight_decay value: {self.weight_decay}")
        # (momentum, dampening and nesterov act for "sgd" only; they are checked for every kind)
        if not self.momentum >= 0:
            raise ValueError(f"Invalid momentum value: {self.momentum}")
        if self.nesterov and (self.momentum <= 0 or self.dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        if self.kind == "adagrad" and not self.lr_decay >= 0:
            raise ValueError(f"Invalid lr_decay value: {self.lr_decay}")
        if self.kind in ("adagrad", "yogi"):
            if not self.initial_accumulator_value >= 0:
                raise ValueError("Invalid initial_accumulator_value value: "
                                 f"{self.initial_accumulator_value}")
            if not self.eps >= 0:
                raise ValueError(f"Invalid epsilon value: {self.eps}")
        if self.kind == "yogi":
            for i, b in enumerate(self.betas):
                if not 0.0 <= b < 1.0:
                    raise ValueError(f"Invalid beta parameter at index {i}: {b}")
        return self

    def c_struct(self):
        o = FlsimOptim()
        o.kind = OPT_KINDS.get(self.kind, -1)
        o.nesterov = int(bool(self.nesterov))
        o.lr = float(self.lr)
        o.beta1, o.beta2 = float(self.betas[0]), float(self.betas[1])
        o.eps = float(self.eps)
        o.weight_decay = float(self.weight_decay)
        o.momentum = float(self.momentum)
        o.dampening = float(self.dampening)
        o.lr_decay = float(self.lr_decay)
        return o


def as_optim(optim):
    """An Optim from an Optim or a dict of its fields."""
    return optim if isinstance(optim, Optim) else Optim(**dict(optim))


def _batch(x, y):
    """An explicit batch as the entry points read it: x contiguous, y contiguous int64."""
    return x.contiguous(), y.to(torch.int64).contiguous()


def padded(n, q=64):
    return (n + q - 1) // q * q


def split_views(flat, shapes=PN1_SHAPES):
    out, off = [], 0
    for _, shp in shapes:
        n = int(np.prod(shp))
        out.append(flat[off:off + n].view(shp))
        off += n
    return out


class NetEngine:
    """Gradient state + chunk workspace of one network on one device; PREFIX selects the C-ABI
    family (flsim_<PREFIX>_*), SHAPES its named_parameters layout."""

    PREFIX = None
    MODEL = None
    SHAPES = None
    FLOP_PER_WORKER_STEP = None     # algorithmic fwd + dgrad + wgrad FLOPs of 128 samples
    STATS_PER_WORKER = 0            # per-call statistics the model's buffers need (BatchNorm)

    def __init__(self, device, chunk_workers=32):
        self.device = torch.device(device)
        self.SIZES = [int(np.prod(s)) for _, s in self.SHAPES]
        self.P = int(self._fn("param_count")())
        assert self.P == sum(self.SIZES)
        self.chunk_workers = int(chunk_workers)
        self.max_samples = self.chunk_workers * SAMPLES_PER_WORKER
        self.gradstate = torch.empty(int(self._fn("gradstate_bytes")()), dtype=torch.uint8,
                                     device=self.device)
        self.workspace = torch.empty(int(self._fn("workspace_bytes")(self.max_samples)),
                                     dtype=torch.uint8, device=self.device)

    def _fn(self, name):
        return getattr(lib(), f"flsim_{self.PREFIX}_{name}")

    def __del__(self):
        # the caching allocator may give this gradstate's address to a later engine: the
        # library's slab-row table for it must not outlive the buffer (flsim_pn1_release)
        gs = getattr(self, "gradstate", None)
        try:
            if gs is not None and hasattr(lib(), f"flsim_{self.PREFIX}_release"):
                self._fn("release")(ptr(gs))
        except Exception:      # interpreter teardown: the library may already be gone
            pass

    # -- per-epoch gradient --------------------------------------------------------------------
    def begin_epoch(self, theta):
        check(self._fn("begin_epoch")(ptr(self.gradstate), ptr(theta), stream_ptr()))

    def _stats_arg(self, stats_out):
        """The extra bn_stats argument of a BatchNorm model's entry points (none otherwise)."""
        if not self.STATS_PER_WORKER:
            return ()
        return (ptr(stats_out) if stats_out is not None else None,)

    def run_chunk(self, theta, pool, workers_dev, n_chunk, n_workers_total, seed, dropout,
                  loss_out, backward=True, stats_out=None):
        """stats_out (BatchNorm models): device float[n_chunk][STATS_PER_WORKER] for the
        per-call statistics that update_running() folds into the running buffers."""
        self.last_workspace = self.workspace
        check(self._fn("fwd_bwd_chunk")(
            ptr(self.gradstate), ptr(self.workspace), self.max_samples, ptr(theta),
            ptr(pool.imgs), ptr(pool.labels), ptr(pool.list_a), int(pool.list_a.numel()),
            ptr(pool.list_b), int(pool.list_b.numel()), ptr(pool.lut), ptr(workers_dev),
            int(n_chunk), int(n_workers_total), ctypes.c_uint64(seed), int(bool(dropout)),
            int(bool(backward)), ptr(loss_out), *self._stats_arg(stats_out), stream_ptr()))

    # pipelined chunks (PN1Engine): chunk i's forward on the current stream overlaps chunk i-1's
    # backward on the library's backward stream; two workspaces alternate
    PIPELINE = False

    def run_chunk_async(self, theta, pool, workers_dev, n_chunk, n_workers_total, seed, dropout,
                        loss_out, slot):
        ws = self._slot_workspace(slot)
        self.last_workspace = ws
        check(lib().flsim_pn1_fwd_bwd_chunk_async(
            ptr(self.gradstate), ptr(ws), self.max_samples, ptr(theta),
            ptr(pool.imgs), ptr(pool.labels), ptr(pool.list_a), int(pool.list_a.numel()),
            ptr(pool.list_b), int(pool.list_b.numel()), ptr(pool.lut), ptr(workers_dev),
            int(n_chunk), int(n_workers_total), ctypes.c_uint64(seed), int(bool(dropout)),
            ptr(loss_out), stream_ptr()))

    def run_input_async(self, theta, x, y, workers_dev, seed, dropout, loss_out, slot):
        """run_input with the backward pipelined (PN1Engine): the loss is ready on the current
        stream after the forward; the gradient is complete for every later entry point."""
        ws = self._slot_workspace(slot)
        self.last_workspace = ws
        x, y = _batch(x, y)
        check(lib().flsim_pn1_fwd_bwd_input_async(
            ptr(self.gradstate), ptr(ws), self.max_samples, ptr(theta), ptr(x), ptr(y),
            int(x.shape[0]), ptr(workers_dev), ctypes.c_uint64(seed), int(bool(dropout)),
            ptr(loss_out), stream_ptr()))

    def _slot_workspace(self, slot):
        if getattr(self, "workspace2", None) is None:
            self.workspace2 = torch.empty_like(self.workspace)
        return self.workspace if slot % 2 == 0 else self.workspace2

    def forward_rows(self, theta, x, y, workers_dev, seed, dropout, loss_out, row0, slot):
        """The facade's deferred backward (PN1Engine): forward + loss of an explicit batch into
        workspace rows [row0, row0 + ceil(n/128)*128) of workspace `slot`; the loss is ready on
        the current stream.  backward_rows() later runs the backward of all rows at once."""
        ws = self._slot_workspace(slot)
        self.last_workspace = ws
        x, y = _batch(x, y)
        check(lib().flsim_pn1_fwd_rows(
            ptr(self.gradstate), ptr(ws), self.max_samples, int(row0), ptr(theta), ptr(x), ptr(y),
            int(x.shape[0]), ptr(workers_dev), ctypes.c_uint64(seed), int(bool(dropout)),
            ptr(loss_out), stream_ptr()))

    def load_rows(self, x, y, row0, slot):
        """The facade's deferred forward (PN1Engine): stage an explicit batch into workspace rows
        [row0, row0 + ceil(n/128)*128) of workspace `slot`; nothing is computed yet."""
        ws = self._slot_workspace(slot)
        self.last_workspace = ws
        x, y = _batch(x, y)
        check(self._fn("load_rows")(ptr(self.gradstate), ptr(ws), self.max_samples, int(row0),
                                    ptr(x), ptr(y), int(x.shape[0]), stream_ptr()))

    def forward_loaded_rows(self, theta, row0, n_rows, workers_dev, seed, dropout, loss_out,
                            slot):
        """Forward + loss of the staged rows [row0, row0 + n_rows) of workspace `slot` as one
        batched pass (every 128-row group one whole batch): loss_out[g] = group g's mean loss."""
        ws = self._slot_workspace(slot)
        check(lib().flsim_pn1_fwd_loaded_rows(
            ptr(self.gradstate), ptr(ws), self.max_samples, int(row0), int(n_rows), ptr(theta),
            ptr(workers_dev), ctypes.c_uint64(seed), int(bool(dropout)), ptr(loss_out),
            stream_ptr()))

    def backward_rows(self, theta, n_rows, dropout, slot):
        """The backward of rows [0, n_rows) of workspace `slot` (forward_rows) into the epoch's
        slabs, on the library's backward stream (the next slot's forwards overlap it)."""
        check(lib().flsim_pn1_bwd_rows(ptr(self.gradstate), ptr(self._slot_workspace(slot)),
                                       self.max_samples, int(n_rows), ptr(theta),
                                       int(bool(dropout)), stream_ptr()))

    def evaluate_input(self, theta, x):
        """Predictions for an explicit NCHW fp32 batch (util.py:31-45's model(images) in eval
        mode): device int32 tensor of argmax indices."""
        x = x.to(self.device, torch.float32).contiguous()
        n = int(x.shape[0])
        pred = torch.empty(n, dtype=torch.int32, device=self.device)
        extra = (ptr(self.running),) if self.STATS_PER_WORKER else ()
        self.last_workspace = self.workspace
        check(self._fn("eval_input")(ptr(self.gradstate), ptr(self.workspace), self.max_samples,
                                     ptr(theta), ptr(x), n, *extra, ptr(pred), stream_ptr()))
        return pred

    def run_input(self, theta, x, y, workers_dev, seed, dropout, loss_out, backward=True,
                  stats_out=None):
        x, y = _batch(x, y)
        self.last_workspace = self.workspace
        check(self._fn("fwd_bwd_input")(
            ptr(self.gradstate), ptr(self.workspace), self.max_samples, ptr(theta), ptr(x), ptr(y),
            int(x.shape[0]), ptr(workers_dev), ctypes.c_uint64(seed), int(bool(dropout)),
            int(bool(backward)), ptr(loss_out), *self._stats_arg(stats_out), stream_ptr()))

    def evaluate(self, theta, pool, first=0, n_images=None):
        """Predictions (argmax of the logits, dropout off) for pool images [first, first + n):
        util.print_test_accuracy's forward (util.py:31-45).  Returns a device int32 tensor."""
        n = int(pool.imgs.shape[0]) - first if n_images is None else int(n_images)
        pred = torch.empty(n, dtype=torch.int32, device=self.device)
        extra = (ptr(self.running),) if self.STATS_PER_WORKER else ()
        self.last_workspace = self.workspace
        check(self._fn("eval_pool")(
            ptr(self.gradstate), ptr(self.workspace), self.max_samples, ptr(theta), ptr(pool.imgs),
            int(first), n, ptr(pool.lut), *extra, ptr(pred), stream_ptr()))
        return pred

    # -- model buffers (BatchNorm running statistics; none for the other models) ----------------
    def update_running(self, stats, n_workers):
        """nn.BatchNorm2d's per-call running update for n_workers calls in worker order."""

    def buffer_state(self):
        """The model's buffers as state_dict entries (OrderedDict order of models.py)."""
        return []

    def load_buffers(self, state):
        """Restore buffer_state() output (names -> tensors)."""

    def end_epoch(self, grad_out):
        check(self._fn("end_epoch")(ptr(self.gradstate), ptr(grad_out), stream_ptr()))

    def server_step(self, S_out, rule, theta, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                    optim=None, theta_out=None):
        """world = 1: the epoch's slabs -> S_t [-> S_out] -> rule() + Adam in one launch
        (flsim_<net>_server_step).  rule: a Rule.  optim (an Optim or a dict of its fields): that
        update rule instead (flsim_<net>_server_step_optim); m / v may be None where the kind
        owns no such array.  A rule with weights runs the staleness-weighted step
        (flsim_<net>_server_step_wrule).  A rule with snapshots, or theta_out (the pre-update
        theta is also written there: the snapshot of the entry pushed into S_out), runs the
        delay-compensated step (flsim_<net>_server_step_crule)."""
        if rule.c_comp is not None or theta_out is not None:
            o = (as_optim(optim) if optim is not None else
                 Optim(lr=lr, betas=tuple(betas), eps=eps)).c_struct()
            check(self._fn("server_step_crule")(
                ptr(self.gradstate), ptr(S_out), ptr(theta_out), ctypes.byref(rule.c_rule),
                _byref(rule.c_weights), _byref(rule.c_comp), ptr(theta), ptr(m), ptr(v),
                int(step), ctypes.byref(o), stream_ptr()))
            return
        if rule.c_weights is not None:
            o = (as_optim(optim) if optim is not None else
                 Optim(lr=lr, betas=tuple(betas), eps=eps)).c_struct()
            check(self._fn("server_step_wrule")(
                ptr(self.gradstate), ptr(S_out), ctypes.byref(rule.c_rule),
                ctypes.byref(rule.c_weights), ptr(theta), ptr(m), ptr(v), int(step),
                ctypes.byref(o), stream_ptr()))
            return
        if optim is not None:
            o = as_optim(optim).c_struct()
            check(self._fn("server_step_optim")(
                ptr(self.gradstate), ptr(S_out), ctypes.byref(rule.c_rule), ptr(theta), ptr(m),
                ptr(v), int(step), ctypes.byref(o), stream_ptr()))
            return
        check(self._fn("server_step")(
            ptr(self.gradstate), ptr(S_out), ctypes.byref(rule.c_rule), ptr(theta), ptr(m), ptr(v),
            int(step), float(lr), float(betas[0]), float(betas[1]), float(eps), stream_ptr()))

    def _workspace_bytes_at(self, which, n):
        off = ctypes.c_long()
        check(self._fn("workspace_offset")(which, self.max_samples, ctypes.byref(off)))
        ws = getattr(self, "last_workspace", None)      # the last pass's (pipelined: alternating)
        ws = self.workspace if ws is None else ws
        return ws[off.value:off.value + n]

    def workspace_view(self, which, shape, dtype=torch.float32, samples=None):
        """Debug view of a workspace tensor by id (PN1Engine.WORKSPACE / VGG11Engine.WORKSPACE).
        A tensor the engine stores in the split-bf16 form (HM + L parts, csrc/split.h) comes back
        as its fp32 values, (h + m) + l, which is exact: a copy, not a view."""
        n = int(np.prod(shape)) * torch.tensor([], dtype=dtype).element_size()
        lpart = self.split_part(which)
        if lpart < 0 or dtype != torch.float32:
            return self._workspace_bytes_at(which, n).view(dtype).view(shape)
        units = int(np.prod(shape)) // 4
        hm = self._workspace_bytes_at(which, n).view(torch.int16).view(units, 2, 4)
        lo = self._workspace_bytes_at(lpart, n // 2).view(torch.int16).view(units, 4)

        def f32(b):         # bf16 bits -> fp32 (exact)
            return (b.to(torch.int32) << 16).view(torch.float32)
        vals = (f32(hm[:, 0]) + f32(hm[:, 1])) + f32(lo)
        if self.slice_major(which):
            # stored [N][C/16][H][W][16] (loaders.h XsSrcSM): back to [N][H][W][C]
            n, h, w, c = shape
            return vals.view(n, c // 16, h, w, 16).permute(0, 2, 3, 1, 4).reshape(shape)
        return vals.view(shape)

    def slice_major(self, which):
        """True when workspace tensor `which` is stored channel-slice-major (PN1's a1, d1, a3)."""
        try:
            fn = self._fn("workspace_slice_major")
        except AttributeError:
            return False
        return bool(fn(which))

    def split_part(self, which):
        """Workspace id of tensor `which`'s L part when it is stored split, else -1."""
        fn = getattr(self, "_split_fn", None)
        if fn is None:
            try:
                fn = self._fn("workspace_split_part")
            except AttributeError:
                fn = lambda w: -1      # noqa: E731  (networks whose tensors are all fp32)
            self._split_fn = fn
        return int(fn(which))

    # -- server step ------------------------------------------------------------------------------
    def aggregate_adam(self, S, c, stale, theta, m, v, step, lr=1e-3, betas=(0.9, 0.999),
                       eps=1e-8, optim=None):
        """stale: list of device tensors (or None = zero entry)."""
        aggregate_adam(S, c, stale, theta, m, v, step, self.SIZES, lr, betas, eps, optim=optim)

    def aggregate_adam_sum(self, S, k, theta, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                           optim=None, clip=None):
        aggregate_adam_sum(S, k, theta, m, v, step, self.SIZES, lr, betas, eps, optim=optim,
                           clip=clip)

    def aggregate_rule(self, S, rule, theta, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                       S_out=None, optim=None, theta_out=None, clip=None):
        """rule() + Adam (or the update rule `optim`) from S_t in a buffer; S_out (optional): S_t
        is also written there in the same pass (the FIFO slot of a tick epoch at world > 1);
        theta_out (optional): so is the pre-update theta (that slot's snapshot); clip (a Clip):
        the rule's output is clipped to clip.max_norm before the update."""
        aggregate_rule(S, rule, theta, m, v, step, self.SIZES, lr, betas, eps, S_out=S_out,
                       optim=optim, theta_out=theta_out, clip=clip)

    def robust_step(self, robust, theta, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                    optim=None, clip=None, g_out=None):
        """A robust rule (a Robust: median / trimmed mean over bucket sums) + Adam (or the update
        rule `optim`) over this network's P parameters; clip (a Clip) and g_out as robust_step."""
        robust_step(robust, theta, m, v, step, self.P, lr, betas, eps, optim=optim, clip=clip,
                    g_out=g_out)

    def krum_step(self, krum, theta, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                  optim=None, clip=None, g_out=None):
        """Krum / Multi-Krum (a Krum over bucket sums) + Adam (or the update rule `optim`) over
        this network's P parameters; clip (a Clip) and g_out as krum_step."""
        krum_step(krum, theta, m, v, step, self.P, lr, betas, eps, optim=optim, clip=clip,
                  g_out=g_out)

    def bulyan_step(self, bulyan, theta, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                    optim=None, clip=None, g_out=None):
        """Bulyan (a Bulyan over bucket sums) + Adam (or the update rule `optim`) over this
        network's P parameters; clip (a Clip) and g_out as bulyan_step."""
        bulyan_step(bulyan, theta, m, v, step, self.P, lr, betas, eps, optim=optim, clip=clip,
                    g_out=g_out)

    def geomed_step(self, geomed, theta, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                    optim=None, clip=None, g_out=None):
        """The geometric median (a GeoMed over bucket sums) + Adam (or the update rule `optim`)
        over this network's P parameters; clip (a Clip) and g_out as geomed_step."""
        geomed_step(geomed, theta, m, v, step, self.P, lr, betas, eps, optim=optim, clip=clip,
                    g_out=g_out)

    def cclip_step(self, cclip, theta, m, v, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                   optim=None, clip=None, g_out=None):
        """Centered clipping (a CClip over bucket sums and its carried center) + Adam (or the
        update rule `optim`) over this network's P parameters; clip (a Clip) and g_out as
        cclip_step."""
        cclip_step(cclip, theta, m, v, step, self.P, lr, betas, eps, optim=optim, clip=clip,
                   g_out=g_out)

    def attack_entries(self, attack, b_out=None):
        """Simulated Byzantine workers (an Attack over bucket sums) over this network's P
        parameters: the crafted vector is mixed into the entries in place; b_out as
        attack_entries.  An OptAttack (Min-Max / Min-Sum) takes opt_attack_entries."""
        if isinstance(attack, OptAttack):
            opt_attack_entries(attack, b_out, self.P)
        else:
            attack_entries(attack, b_out, self.P)

    def nnm_entries(self, nnm):
        """Nearest-neighbour mixing (an NNM over bucket sums) over this network's P parameters:
        the entries become their mixed means in place, as nnm_entries."""
        nnm_entries(nnm, self.P)


class PN1Engine(NetEngine):
    PREFIX = "pn1"
    MODEL = "PerformantNet1"
    PIPELINE = True
    SHAPES = PN1_SHAPES
    FLOP_PER_WORKER_STEP = 147_641_499_648
    WORKSPACE = ("x0 a1 a2 d1 a3 a4 d2 a5 a6 d3 e1 e2 dh1 dh2 gx gy loss_s dlog y i1 i2 i3").split()


class VGG11Engine(NetEngine):
    PREFIX = "vgg11"
    MODEL = "vgg11"
    SHAPES = VGG11_SHAPES
    FLOP_PER_WORKER_STEP = 117_276_672_000          # 916,224,000 FLOP/sample x 128
    WORKSPACE = ("x0 d1 d2 a3 d4 a5 d6 a7 f0 e1 e2 dh1 dh2 ga gb gy loss_s dlog y "
                 "i1 i2 i4 i6 i8").split()

    def _slot_workspace(self, slot):
        return self.workspace                 # one workspace: the vgg11 facade has no pipeline

    def fwd_bwd_loaded_rows(self, theta, n_rows, workers_dev, seed, dropout, loss_out):
        """The facade's deferred fwd_bkwd: forward, loss and backward of the staged rows
        [0, n_rows) (load_rows) as one batched chunk; loss_out[g] = call g's loss."""
        check(lib().flsim_vgg11_fwd_bwd_loaded_rows(
            ptr(self.gradstate), ptr(self.workspace), self.max_samples, int(n_rows), ptr(theta),
            ptr(workers_dev), ctypes.c_uint64(seed), int(bool(dropout)), ptr(loss_out),
            stream_ptr()))


class VGG11BNEngine(NetEngine):
    """models.py:106-108 vgg11_bn() through flsim_vgg11_bn_*.  Holds the model's BatchNorm
    buffers: `running` = [running_mean | running_var] per layer on the device (zeros / ones at
    construction, nn.BatchNorm2d's init) and the num_batches_tracked counter (the same for every
    layer: each fwd_bkwd call updates all of them)."""
    PREFIX = "vgg11_bn"
    MODEL = "vgg11_bn"
    SHAPES = VGG11_BN_SHAPES
    FLOP_PER_WORKER_STEP = 117_276_672_000          # the GEMMs of vgg11 (BatchNorm is streaming)
    STATS_PER_WORKER = 5504
    WORKSPACE = ("x0 d1 d2 a3 d4 a5 d6 a7 f0 e1 e2 dh1 dh2 ga gb gy loss_s dlog y "
                 "i1 i2 i4 i6 i8 " + " ".join(f"z{j}" for j in range(8)) + " " +
                 " ".join(f"bmean{j}" for j in range(8)) + " " +
                 " ".join(f"binv{j}" for j in range(8))).split()

    def __init__(self, device, chunk_workers=32):
        super().__init__(device, chunk_workers)
        assert int(lib().flsim_vgg11_bn_stats_per_worker()) == self.STATS_PER_WORKER
        self.running = torch.cat([torch.cat([torch.zeros(c), torch.ones(c)])
                                  for _, c in VGG11_BN_BUFFERS]).to(self.device)
        self.num_batches_tracked = 0

    def _slot_workspace(self, slot):
        return self.workspace                 # one workspace: the vgg11_bn facade has no pipeline

    def fwd_bwd_loaded_rows(self, theta, n_rows, workers_dev, seed, dropout, loss_out,
                            stats_out):
        """The facade's deferred fwd_bkwd: forward, loss and backward of the staged rows
        [0, n_rows) as one batched chunk; stats_out[g] = call g's BatchNorm statistics (for
        update_running), loss_out[g] = its loss."""
        check(lib().flsim_vgg11_bn_fwd_bwd_loaded_rows(
            ptr(self.gradstate), ptr(self.workspace), self.max_samples, int(n_rows), ptr(theta),
            ptr(workers_dev), ctypes.c_uint64(seed), int(bool(dropout)), ptr(loss_out),
            ptr(stats_out), stream_ptr()))

    def update_running(self, stats, n_workers):
        n = int(n_workers)
        if n:
            check(lib().flsim_vgg11_bn_update_running(ptr(self.running), ptr(stats), n,
                                                      stream_ptr()))
        self.num_batches_tracked += n

    def running_views(self):
        """[(name, running_mean view, running_var view)] per BatchNorm layer."""
        out, off = [], 0
        for name, c in VGG11_BN_BUFFERS:
            out.append((name, self.running[off:off + c], self.running[off + c:off + 2 * c]))
            off += 2 * c
        return out

    def buffer_state(self):
        out = []
        for name, rm, rv in self.running_views():
            out += [(f"{name}.running_mean", rm.detach().cpu().clone()),
                    (f"{name}.running_var", rv.detach().cpu().clone()),
                    (f"{name}.num_batches_tracked",
                     torch.tensor(self.num_batches_tracked, dtype=torch.int64))]
        return out

    def load_buffers(self, state):
        for name, rm, rv in self.running_views():
            rm.copy_(state[f"{name}.running_mean"].to(self.device))
            rv.copy_(state[f"{name}.running_var"].to(self.device))
        self.num_batches_tracked = int(state[f"{VGG11_BN_BUFFERS[0][0]}.num_batches_tracked"])


ENGINES = {"PerformantNet1": PN1Engine, "vgg11": VGG11Engine, "vgg11_bn": VGG11BNEngine}


def engine_class(model):
    if model not in ENGINES:
        raise NotImplementedError(f"model {model!r}: the HIP engine implements {sorted(ENGINES)}")
    return ENGINES[model]


def engine_for_parameters(names):
    """The engine class whose named_parameters layout is `names` (a models.py module)."""
    names = list(names)
    for cls in ENGINES.values():
        if names == [n for n, _ in cls.SHAPES]:
            return cls
    raise NotImplementedError("the HIP engine implements FL.models.PerformantNet1, vgg11 and "
                              "vgg11_bn")


def aggregate_adam(S, c, stale, theta, m, v, step, sizes, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                   optim=None):
    """Fused rule() + Adam (main.py:23-25 + agents.py:9-21) over a flat parameter vector whose
    tensors have numel `sizes` (named_parameters order).  stale: device tensors or None (zeros).
    optim: the update rule instead of Adam(lr, betas, eps) (see aggregate_rule)."""
    ns = len(stale)
    if optim is not None:
        if not (c >= 0 and ns <= 8):
            raise ValueError(f"bad entry counts c={c} ns={ns}")
        if c + ns == 0:
            raise IndexError("empty weight_ups (reference: IndexError in rule, main.py:25)")
        aggregate_rule(S, Rule(c + ns, stale, c=c), theta, m, v, step, sizes, optim=optim)
        return
    arr = (ctypes.c_void_p * max(1, ns))(*[(t.data_ptr() if t is not None else None)
                                           for t in stale])
    csz = (ctypes.c_long * len(sizes))(*[int(n) for n in sizes])
    check(lib().flsim_aggregate_adam(
        ptr(S), int(c), arr, ns, ptr(theta), ptr(m), ptr(v), sum(int(n) for n in sizes), csz, len(sizes),
        int(step), float(lr), float(betas[0]), float(betas[1]), float(eps), stream_ptr()))


def aggregate_adam_sum(S, k, theta, m, v, step, sizes, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                       optim=None, clip=None):
    """Independent-entry semantics: S = the sum of the k distinct weight_ups entries; mean = S / k
    then the same Adam step (flsim_aggregate_adam_sum), or the update rule `optim`; clip (a Clip):
    the mean is clipped first (the same stream with the sum rule)."""
    if optim is not None or clip is not None:
        if k <= 0:
            raise IndexError("empty weight_ups (reference: IndexError in rule, main.py:25)")
        aggregate_rule(S, Rule(k, [], c=1), theta, m, v, step, sizes, lr, betas, eps, optim=optim,
                       clip=clip)
        return
    csz = (ctypes.c_long * len(sizes))(*[int(n) for n in sizes])
    check(lib().flsim_aggregate_adam_sum(
        ptr(S), int(k), ptr(theta), ptr(m), ptr(v), sum(int(n) for n in sizes), csz, len(sizes),
        int(step), float(lr), float(betas[0]), float(betas[1]), float(eps), stream_ptr()))


def cascade_program(k, events):
    """rule()'s summation program (host, flsim_cascade_program) for k entries whose non-S_t
    entries are events = [(position, array index)] (positions increasing).  -> (int32 words,
    info[4]).  The words are the device's macro form (csrc/cascade.h): (lo, hi) pairs."""
    ev = np.asarray(events, np.int32).reshape(-1, 2)
    pos = np.ascontiguousarray(ev[:, 0])
    arr = np.ascontiguousarray(ev[:, 1])
    cap = 2 * (72 + 40 * (len(ev) + 8))    # macro pairs (lo, hi) + the fetch-pad pair
    prog = np.zeros(cap, np.int32)
    info = np.zeros(4, np.int32)
    vp = ctypes.c_void_p
    check(lib().flsim_cascade_program(int(k), pos.ctypes.data_as(vp), arr.ctypes.data_as(vp),
                                      len(ev), prog.ctypes.data_as(vp), cap,
                                      info.ctypes.data_as(vp)))
    return prog[:2 * (info[0] + 1)].copy(), info      # with the padding pair


class Rule:
    """weight_ups of one rule() call (flsim_rule): k entries (the mean's divisor); either the
    reference order [S_t] * c + arrays, or a general order given as events [(position, array
    index)] whose program is built on the host and staged to the device (`stager`).  arrays:
    device tensors or None (a zero entry, torch-1.x).

    weights (one Python float per array; None = the plain mean) make it the staleness-weighted
    rule sum_j w_j * entry_j / divisor with w = 1.0 for every S_t entry: divisor defaults to the
    sum of all k weights ("weights" normalisation; pass k for "count").  A weight must be finite
    and >= 0 (ValueError), the divisor > 0 (ZeroDivisionError).

    snapshots (one device tensor or None per array) with delay_comp = lambda make it the
    delay-compensated rule (DC-ASGD): array j enters as x + (x * x) * lambda * (theta_now -
    snapshots[j]) with theta_now the parameters before the step; None leaves an array as it
    stands.  Compensation comes before the weight.  lambda must be finite and >= 0 (ValueError).
    An entry is S_src, a sum over that epoch's workers, so x * x grows with the square of the
    worker count: choose lambda with that in mind."""

    def __init__(self, k, arrays=(), c=None, events=None, stager=None, weights=None,
                 divisor=None, snapshots=None, delay_comp=None):
        arrays = list(arrays)
        self.weights, self.divisor, self.c_weights = None, None, None
        self.snapshots, self.delay_comp, self.c_comp = None, None, None
        if snapshots is not None or delay_comp is not None:
            snapshots = [None] * len(arrays) if snapshots is None else list(snapshots)
            if len(snapshots) != len(arrays):
                raise ValueError(f"{len(snapshots)} snapshots for {len(arrays)} arrays")
            lam = 0.0 if delay_comp is None else float(delay_comp)
            if not (lam >= 0 and math.isfinite(lam)):
                raise ValueError(f"Invalid delay compensation lambda {lam}: it must be finite "
                                 "and >= 0")
            self.snapshots, self.delay_comp = snapshots, lam
        if weights is None and divisor is not None:
            weights = [1.0] * len(arrays)
        if weights is not None:
            weights = [float(w) for w in weights]
            if len(weights) != len(arrays):
                raise ValueError(f"{len(weights)} weights for {len(arrays)} arrays")
            for w in weights:
                if not (w >= 0 and math.isfinite(w)):
                    raise ValueError(f"Invalid weight {w}: a weight must be finite and >= 0")
            if divisor is None:
                # float(sum(weights)) over the k entries in weight_ups order: the S_t entries weigh
                # 1.0 each, every other entry its array's weight
                if events is None:
                    full = [1.0] * int(c) + weights
                else:
                    full = [1.0] * int(k)
                    for pos, j in events:
                        full[pos] = weights[j]
                divisor = float(sum(full))
            divisor = float(divisor)
            if divisor != divisor or math.isinf(divisor):
                raise ValueError(f"Invalid divisor {divisor}")
            if not divisor > 0:
                raise ZeroDivisionError(f"weighted rule divisor {divisor}")
            self.weights, self.divisor = weights, divisor
        if len(arrays) > MAX_ARRAYS:
            raise NotImplementedError(f"{len(arrays)} distinct weight_ups arrays in one step "
                                      f"(max {MAX_ARRAYS})")
        r = FlsimRule()
        r.k = int(k)
        r.n_arrays = len(arrays)
        for q, a in enumerate(arrays):
            r.arrays[q] = a.data_ptr() if a is not None else None
        self.arrays = arrays            # keep the tensors alive with the rule
        self.k, self.c, self.events = int(k), c, events
        if events is None:
            r.c = int(c)
            r.prog = None
            self.prog_dev = None
        else:
            words, info = cascade_program(k, events)
            self.prog_dev = stager.upload(words)
            r.c = -1
            r.prog = self.prog_dev.data_ptr()
            for j in range(4):
                r.info[j] = int(info[j])
        self.c_rule = r
        if self.weights is not None and len(arrays) <= MAX_ARRAYS:
            cw = FlsimRuleWeights()
            cw.n = len(arrays)
            for q, w in enumerate(self.weights):
                cw.w[q] = w
            cw.divisor = self.divisor
            self.c_weights = cw
        if self.snapshots is not None and len(arrays) <= MAX_ARRAYS:
            cc = FlsimRuleComp()
            cc.n = len(arrays)
            cc.lam = self.delay_comp
            for q, t in enumerate(self.snapshots):      # (the rule keeps the tensors alive)
                cc.theta_src[q] = t.data_ptr() if t is not None else None
            self.c_comp = cc


def staleness_weight(spec):
    """The discount s(tau) of a stale entry of age tau epochs as a function tau -> float (host,
    double).  spec: None (no discount: 1.0), a callable (returned as it is), or
      ("poly", a)      (1.0 + tau) ** (-a)                                   (FedAsync)
      ("hinge", a, b)  1.0 if tau <= b else 1.0 / (a * (tau - b) + 1.0)      (FedAsync)
      ("const", a)     a"""
    if spec is None:
        return lambda tau: 1.0
    if callable(spec):
        return spec
    spec = tuple(spec)
    kind, args = spec[0], [float(x) for x in spec[1:]]
    if kind == "poly" and len(args) == 1:
        a, = args
        return lambda tau: (1.0 + tau) ** (-a)
    if kind == "hinge" and len(args) == 2:
        a, b = args
        return lambda tau: 1.0 if tau <= b else 1.0 / (a * (tau - b) + 1.0)
    if kind == "const" and len(args) == 1:
        a, = args
        return lambda tau: a
    raise ValueError(f"stale weight {spec!r} (supported: ('poly', a), ('hinge', a, b), "
                     "('const', a) or a callable)")


class ProgramStager:
    """Pinned host -> device staging of rule programs, double-buffered.  The host waits only for
    the copy out of a pinned buffer two uploads ago; the device buffer is rewritten two uploads
    later, behind (stream order) the launch that reads it now."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.cap = 0
        self.i = 0

    def upload(self, words):
        n = int(words.size)
        if n > self.cap:
            self.cap = max(1024, 2 * n)
            pin = self.device.type == "cuda"
            self.host = [torch.empty(self.cap, dtype=torch.int32, pin_memory=pin) for _ in range(2)]
            self.dev = [torch.empty(self.cap, dtype=torch.int32, device=self.device)
                        for _ in range(2)]
            self.ev = [None, None]
        j = self.i = self.i ^ 1
        if self.ev[j] is not None:
            self.ev[j].synchronize()
        self.host[j][:n].numpy()[:] = words
        self.dev[j][:n].copy_(self.host[j][:n], non_blocking=True)
        if self.device.type == "cuda":
            ev = torch.cuda.Event()
            ev.record()
            self.ev[j] = ev
        return self.dev[j]


def _byref(struct):
    return ctypes.byref(struct) if struct is not None else None


class Clip:
    """Global-norm gradient clipping of a server step (flsim_clip, include/flsim.h): what
    torch.nn.utils.clip_grad_norm_(parameters, max_norm) does between `p.grad = ...` and
    optim.step(), on the rule's output.  max_norm > 0; float("inf") clips nothing and only reports
    the norm.  The object owns its scratch per device (the rule's output G, the per-block partial
    sums, the two result scalars), allocated at the first step on that device.  After a step,
    total_norm (the correctly rounded 2-norm of the rule's output) and coef (the factor the
    gradient was multiplied by) are 0-d device tensors; reading them needs no synchronisation
    beyond the stream's order, and the next step overwrites them (clone to keep)."""

    def __init__(self, max_norm):
        self.max_norm = float(max_norm)
        if not self.max_norm > 0:
            raise ValueError(f"Invalid clipping max_norm {self.max_norm}: it must be > 0")
        self._scratch = {}
        self.total_norm = None
        self.coef = None

    def c_struct(self, device, P):
        """flsim_clip over this device's scratch for a step over P elements."""
        key = (str(device), int(P))
        if key not in self._scratch:
            n = int(lib().flsim_clip_partials(int(P)))
            self._scratch[key] = (torch.empty(padded(int(P)), device=device),
                                  torch.empty(n, dtype=torch.float64, device=device),
                                  torch.empty(4, device=device))
        G, partials, out = self._scratch[key]
        c = FlsimClip()
        c.max_norm = self.max_norm
        c.G = G.data_ptr()
        c.partials = partials.data_ptr()
        c.n_partials = int(partials.numel())
        c.out = out.data_ptr()
        self.total_norm, self.coef = out[0], out[1]
        return c


def aggregate_rule(S, rule, theta, m, v, step, sizes, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                   S_out=None, optim=None, theta_out=None, clip=None):
    """rule() + Adam from S_t in a buffer (flsim_aggregate_adam_rule_push; S_out may be None).
    optim (an Optim or a dict of its fields): that update rule instead of Adam(lr, betas, eps)
    (flsim_aggregate_optim_rule_push); m / v may be None where the kind owns no such array (SGD
    and Adagrad: v; SGD without momentum: m and v) and are left untouched when given.  clip (a Clip): the
    rule's output is clipped to clip.max_norm before the update
    (flsim_aggregate_optim_clip_push); clip.total_norm and clip.coef hold the step's norm and
    factor afterwards."""
    csz = (ctypes.c_long * len(sizes))(*[int(n) for n in sizes])
    if clip is not None:
        o = (as_optim(optim) if optim is not None else
             Optim(lr=lr, betas=tuple(betas), eps=eps)).c_struct()
        P = sum(int(n) for n in sizes)
        c = clip.c_struct(theta.device, P)
        check(lib().flsim_aggregate_optim_clip_push(
            ptr(S), ptr(S_out), ptr(theta_out), ctypes.byref(rule.c_rule), _byref(rule.c_weights),
            _byref(rule.c_comp), ctypes.byref(c), ptr(theta), ptr(m), ptr(v), P, csz, len(sizes),
            int(step), ctypes.byref(o), stream_ptr()))
        return
    if rule.c_comp is not None or theta_out is not None:
        # the delay-compensated rule (rule.snapshots) and / or the snapshot write (theta_out: the
        # pre-update theta, in the same pass)
        o = (as_optim(optim) if optim is not None else
             Optim(lr=lr, betas=tuple(betas), eps=eps)).c_struct()
        check(lib().flsim_aggregate_optim_crule_push(
            ptr(S), ptr(S_out), ptr(theta_out), ctypes.byref(rule.c_rule), _byref(rule.c_weights),
            _byref(rule.c_comp), ptr(theta), ptr(m), ptr(v), sum(int(n) for n in sizes), csz,
            len(sizes), int(step), ctypes.byref(o), stream_ptr()))
        return
    if rule.c_weights is not None:      # the staleness-weighted rule
        o = (as_optim(optim) if optim is not None else
             Optim(lr=lr, betas=tuple(betas), eps=eps)).c_struct()
        check(lib().flsim_aggregate_optim_wrule_push(
            ptr(S), ptr(S_out), ctypes.byref(rule.c_rule), ctypes.byref(rule.c_weights),
            ptr(theta), ptr(m), ptr(v), sum(int(n) for n in sizes), csz, len(sizes), int(step),
            ctypes.byref(o), stream_ptr()))
        return
    if optim is not None:
        o = as_optim(optim).c_struct()
        check(lib().flsim_aggregate_optim_rule_push(
            ptr(S), ptr(S_out), ctypes.byref(rule.c_rule), ptr(theta), ptr(m), ptr(v),
            sum(int(n) for n in sizes), csz, len(sizes), int(step), ctypes.byref(o), stream_ptr()))
        return
    check(lib().flsim_aggregate_adam_rule_push(
        ptr(S), ptr(S_out), ctypes.byref(rule.c_rule), ptr(theta), ptr(m), ptr(v),
        sum(int(n) for n in sizes), csz, len(sizes), int(step), float(lr), float(betas[0]),
        float(betas[1]), float(eps), stream_ptr()))


class _BucketRule:
    """What the objects over bucket / class sums share (the four rules, Attack, NNM): the entries
    and their counts, checked as every rule checks them (_what and _kmin: the object's words in
    the message), their fields in the C struct, and the scratch of those that have one.  center:
    the rule that has one overrides it.

    A class with scratch names its C struct (_scratch_struct) and the library function that sizes
    the partials (_partials), and describes the other buffers in _scratch_rows; c_scratch allocates
    them per key in the class's own _scratch dictionary, as (partials, *rows)."""
    _what, _kmin = None, 1
    _bad_count = 0      # what a count the int32 field cannot hold becomes: the library refuses it
    _scratch_struct = _partials = None
    center = None

    def _set_entries(self, entries, counts):
        entries, counts = list(entries), [int(c) for c in counts]
        if len(entries) != len(counts):
            raise ValueError(f"{len(counts)} counts for {len(entries)} entries")
        if len(entries) > MAX_ARRAYS:
            raise ValueError(f"{self._what} over k = {len(entries)} entries "
                             f"({self._kmin} .. {MAX_ARRAYS})")
        self.entries, self.counts = entries, counts     # (the rule keeps the tensors alive)

    @property
    def k(self):
        return len(self.entries)

    def _fill_entries(self, r, **counts):
        """k, entries[] and the count fields of the C struct r (count = self.counts unless other
        fields are named); returns r."""
        r.k = len(self.entries)
        for j, e in enumerate(self.entries):
            r.entries[j] = e.data_ptr() if e is not None else None
        for field, cs in (counts or {"count": self.counts}).items():
            for j, c in enumerate(cs):
                # (an int32 field: a count it cannot hold becomes one the library refuses)
                getattr(r, field)[j] = c if -2 ** 31 <= c < 2 ** 31 else self._bad_count
        return r

    def _scratch_rows(self, k):
        """-> (the key's tail after (device, P, k), rows); a row is (the struct's field, the
        object's attribute, dtype, elements allocated, the shape of the view exposed)."""
        raise NotImplementedError

    def c_scratch(self, device, P):
        """The class's scratch struct over this device's scratch for a call over P elements (None
        for a class that has none); the views of its rows become the object's attributes."""
        if self._scratch_struct is None:
            return None
        k = len(self.entries)
        tail, rows = self._scratch_rows(k)
        cache, key = type(self)._scratch, (str(device), int(P), k) + tail
        if key not in cache:
            n = max(int(getattr(lib(), self._partials)(int(P), k)), 2)
            cache[key] = (torch.empty(n, dtype=torch.float64, device=device),
                          *(torch.empty(alloc, dtype=dt, device=device)
                            for _, _, dt, alloc, _ in rows))
        s = self._scratch_struct()
        self.partials = cache[key][0]
        s.partials = self.partials.data_ptr()
        s.n_partials = int(self.partials.numel())
        for (field, attr, _, _, shape), buf in zip(rows, cache[key][1:]):
            setattr(s, field, buf.data_ptr())
            setattr(self, attr, buf[:math.prod(shape)].view(shape))
        return s


def _bucket_step(fn, rule, theta, m, v, step, P, lr, betas, eps, optim, clip, g_out):
    """The call of a bucketed rule's entry point `fn` (after the rule and its scratch, where it has
    one, every one takes clip, g_out, theta, m, v, P, step, optim and the stream)."""
    if optim is False:
        o = None
    else:
        o = ctypes.byref((as_optim(optim) if optim is not None else
                          Optim(lr=lr, betas=tuple(betas), eps=eps)).c_struct())
    if P is None:
        P = int((theta if theta is not None else g_out).numel())
    r = rule.c_struct()
    dev = next((t.device for t in (theta, g_out, rule.center, *rule.entries) if t is not None),
               None)
    s = rule.c_scratch(dev, int(P))
    c = ctypes.byref(clip.c_struct(dev, int(P))) if clip is not None else None
    check(getattr(lib(), fn)(
        ctypes.byref(r), *(() if s is None else (ctypes.byref(s),)), c, ptr(g_out), ptr(theta),
        ptr(m), ptr(v), int(P), int(step), o, stream_ptr()))


class Robust(_BucketRule):
    """A robust rule over bucket / class sums (flsim_robust, include/flsim.h): kind "median" (the
    coordinate-wise lower median) or "trimmed_mean" (per coordinate the `trim` lowest and highest
    values dropped, the rest averaged), over the k = len(entries) values entries[j] / counts[j].
    entries: flat fp32 device tensors of the same length, or None (an all-zero entry); counts: the
    number of workers summed into each (>= 1).  flsim/robust.py is the rule's text."""
    _what = "robust rule"

    def __init__(self, kind, trim, entries, counts):
        self._set_entries(entries, counts)
        self.kind, self.trim = kind, int(trim)

    def c_struct(self):
        r = FlsimRobust()
        r.kind = ROBUST_KINDS.get(self.kind, -1)
        r.trim = self.trim
        return self._fill_entries(r)


def robust_step(robust, theta, m, v, step, P=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                optim=None, clip=None, g_out=None):
    """The robust rule + Adam(lr, betas, eps), or the update rule `optim` (an Optim or a dict of its
    fields), in one launch (flsim_robust_optim_step); m / v may be None where the kind owns no such
    array.  clip (a Clip): the rule's output is clipped to clip.max_norm before the update.  g_out
    (optional): the rule's output is also written there; optim=False with g_out runs the rule
    alone and touches none of theta / m / v (theta may then be None)."""
    _bucket_step("flsim_robust_optim_step", robust, theta, m, v, step, P, lr, betas, eps, optim,
                 clip, g_out)


class Krum(_BucketRule):
    """Krum / Multi-Krum over bucket / class sums (flsim_krum, include/flsim.h): of the k =
    len(entries) values entries[j] / counts[j], the mean of the m whose summed squared distance
    to their k - f - 2 nearest neighbours is lowest (m = 1: Krum).  entries, counts as for Robust.
    The object owns its scratch per (device, P, k), allocated at the first step; after a step
    dist ([k, k] fp64), score ([k] fp64) and sel ([m] int32, ascending) are device tensors, read
    with no synchronisation beyond the stream's order; the next step overwrites them.
    flsim/robust.py is the rule's text."""
    _scratch = {}       # (device, P, k) -> buffers, shared by the objects of a run
    _what, _kmin = "Krum", 3
    _scratch_struct, _partials = FlsimKrumScratch, "flsim_krum_partials"

    def __init__(self, f, m, entries, counts):
        self._set_entries(entries, counts)
        self.f, self.m = int(f), int(m)
        self.dist = self.score = self.sel = None

    def c_struct(self):
        r = FlsimKrum()
        r.f, r.m = self.f, self.m
        return self._fill_entries(r)

    def _scratch_rows(self, k):
        f64 = torch.float64
        return (), (("dist", "dist", f64, k * k + 2, (k, k)),
                    ("score", "score", f64, k + 2, (k,)),
                    ("sel", "sel", torch.int32, MAX_ARRAYS, (max(min(self.m, MAX_ARRAYS), 0),)))


def krum_step(krum, theta, m, v, step, P=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
              optim=None, clip=None, g_out=None):
    """Krum / Multi-Krum + Adam(lr, betas, eps), or the update rule `optim`, in three launches
    (flsim_krum_optim_step); m / v, clip, g_out and optim=False as robust_step."""
    _bucket_step("flsim_krum_optim_step", krum, theta, m, v, step, P, lr, betas, eps, optim, clip,
                 g_out)


class Bulyan(_BucketRule):
    """Bulyan over bucket / class sums (flsim_bulyan, include/flsim.h): of the k = len(entries)
    values entries[j] / counts[j], Krum's selection is repeated until theta = k - 2f are chosen,
    then per coordinate the mean of the beta = k - 4f values closest to the median of the chosen
    ones (k >= 4f + 3).  entries, counts as for Robust.  The object owns its scratch per (device,
    P, k), allocated at the first step; after a step dist ([k, k] fp64), score ([theta] fp64:
    the winning scores in round order), order ([theta] int32: the winners in round order) and sel
    ([theta] int32, ascending) are device tensors, read with no synchronisation beyond the
    stream's order; the next step overwrites them.  flsim/robust.py is the rule's text."""
    _scratch = {}       # (device, P, k) -> buffers, shared by the objects of a run
    _what, _kmin = "Bulyan", 3
    _scratch_struct, _partials = FlsimBulyanScratch, "flsim_bulyan_partials"

    def __init__(self, f, entries, counts):
        self._set_entries(entries, counts)
        self.f = int(f)
        self.dist = self.score = self.order = self.sel = None

    def c_struct(self):
        r = FlsimBulyan()
        r.f = self.f if -2 ** 31 <= self.f < 2 ** 31 else -1
        return self._fill_entries(r)

    def _scratch_rows(self, k):
        f64, i32 = torch.float64, torch.int32
        theta = max(min(k - 2 * self.f, MAX_ARRAYS), 0)     # (an f the library refuses: no views)
        return (), (("dist", "dist", f64, k * k + 2, (k, k)),
                    ("score", "score", f64, MAX_ARRAYS, (theta,)),
                    ("order", "order", i32, MAX_ARRAYS, (theta,)),
                    ("sel", "sel", i32, MAX_ARRAYS, (theta,)))


def bulyan_step(bulyan, theta, m, v, step, P=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                optim=None, clip=None, g_out=None):
    """Bulyan + Adam(lr, betas, eps), or the update rule `optim`, in three launches
    (flsim_bulyan_optim_step); m / v, clip, g_out and optim=False as robust_step."""
    _bucket_step("flsim_bulyan_optim_step", bulyan, theta, m, v, step, P, lr, betas, eps, optim,
                 clip, g_out)


class GeoMed(_BucketRule):
    """The geometric median over bucket / class sums by smoothed Weiszfeld iterations
    (flsim_geomed, include/flsim.h; "RFA"): of the k = len(entries) values entries[j] /
    counts[j], `iters` iterations from their alpha-weighted mean, alpha = 1 or (weighted) the
    counts.  entries, counts as for Robust.  The object owns its scratch per (device, P, k,
    iters), allocated at the first step; after a step w ([iters + 1, k] fp64), d2 ([iters, k]
    fp64), obj ([iters] fp64) and dead ([k] int32) are device tensors, read with no
    synchronisation beyond the stream's order; the next step overwrites them.
    flsim/robust.py is the rule's text."""
    _scratch = {}       # (device, P, k, iters) -> buffers, shared by the objects of a run
    _what = "geometric median"
    _scratch_struct, _partials = FlsimGeomedScratch, "flsim_geomed_partials"

    def __init__(self, iters, nu, weighted, entries, counts):
        self._set_entries(entries, counts)
        self.iters, self.nu, self.weighted = int(iters), float(nu), bool(weighted)
        self.w = self.d2 = self.obj = self.dead = None

    def c_struct(self):
        r = FlsimGeomed()
        r.iters, r.weighted = self.iters, int(self.weighted)
        r.nu = self.nu
        return self._fill_entries(r)

    def _scratch_rows(self, k):
        it, f64 = max(min(self.iters, 32), 0), torch.float64
        return (it,), (("w", "w", f64, (it + 1) * k + 2, (it + 1, k)),
                       ("d2", "d2", f64, it * k + 2, (it, k)),
                       ("obj", "obj", f64, it + 2, (it,)),
                       ("state", "dead", torch.int32, k + 4 + 4, (k,)))


def geomed_step(geomed, theta, m, v, step, P=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                optim=None, clip=None, g_out=None):
    """The geometric median (RFA) + Adam(lr, betas, eps), or the update rule `optim`, in
    2 * (iters + 1) + 1 launches (flsim_geomed_optim_step); m / v, clip, g_out and optim=False
    as robust_step."""
    _bucket_step("flsim_geomed_optim_step", geomed, theta, m, v, step, P, lr, betas, eps, optim,
                 clip, g_out)


class CClip(_BucketRule):
    """Centered clipping over bucket / class sums around a carried center (flsim_cclip,
    include/flsim.h; Karimireddy, He and Jaggi 2021): `iters` iterations of v <- v + sum_j lam_j
    min(1, tau / ||x_j - v||) (x_j - v) from v = center over the k = len(entries) values
    entries[j] / counts[j], lam = alpha / sum alpha, alpha = 1 or (weighted) the counts.  center:
    a flat fp32 device tensor of P elements, read (unless fresh: it then counts as all zero and is
    not read) and overwritten with the aggregate g, the next step's center.  entries, counts as
    for Robust.  The object owns its scratch per (device, P, k, iters), allocated at the first
    step; after a step u ([iters + 1] fp64), w ([iters + 1, k] fp64), d2 and s ([iters, k] fp64)
    and dead ([k] int32) are device tensors, read with no synchronisation beyond the stream's
    order; the next step overwrites them.  flsim/robust.py is the rule's text."""
    _scratch = {}       # (device, P, k, iters) -> buffers, shared by the objects of a run
    _what = "centered clipping"
    _scratch_struct, _partials = FlsimCclipScratch, "flsim_cclip_partials"

    def __init__(self, tau, iters, weighted, entries, counts, center, fresh=False):
        self._set_entries(entries, counts)
        self.tau, self.iters, self.weighted = float(tau), int(iters), bool(weighted)
        self.center, self.fresh = center, bool(fresh)
        self.u = self.w = self.d2 = self.s = self.dead = None

    def c_struct(self):
        r = FlsimCclip()
        r.iters, r.weighted = self.iters, int(self.weighted)
        r.fresh, r.tau = int(self.fresh), self.tau
        r.center = self.center.data_ptr() if self.center is not None else None
        return self._fill_entries(r)

    def _scratch_rows(self, k):
        it, f64 = max(min(self.iters, 32), 1), torch.float64
        return (it,), (("u", "u", f64, it + 1 + 2, (it + 1,)),
                       ("w", "w", f64, (it + 1) * k + 2, (it + 1, k)),
                       ("d2", "d2", f64, it * k + 2, (it, k)),
                       ("s", "s", f64, it * k + 2, (it, k)),
                       ("state", "dead", torch.int32, k + 4 + 4, (k,)))


def cclip_step(cclip, theta, m, v, step, P=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
               optim=None, clip=None, g_out=None):
    """Centered clipping + Adam(lr, betas, eps), or the update rule `optim`, in 2 * iters + 1
    launches (flsim_cclip_optim_step); cclip.center then holds the (unclipped) aggregate.  m / v,
    clip, g_out and optim=False as robust_step."""
    _bucket_step("flsim_cclip_optim_step", cclip, theta, m, v, step, P, lr, betas, eps, optim,
                 clip, g_out)


class Attack(_BucketRule):
    """Simulated Byzantine workers over bucket sums (flsim_attack, include/flsim.h): kind "ipm"
    (every Byzantine worker sends -strength * mu) or "alie" (mu - strength * sigma), mu and sigma
    the coordinate-wise mean and population standard deviation of entries[j] / honest[j] over the
    entries with honest[j] >= 1.  entries: flat fp32 device tensors of the same length, updated in
    place where byz[j] >= 1 (never read where honest[j] == 0); honest, byz: the workers of either
    side summed into each.  flsim/robust.py (attack_flat) is the text."""
    _what, _bad_count = "attack", -1

    def __init__(self, kind, strength, entries, honest, byz):
        entries, honest, byz = list(entries), list(honest), [int(c) for c in byz]
        if len(entries) != len(honest) or len(entries) != len(byz):
            raise ValueError(f"{len(honest)} honest and {len(byz)} Byzantine counts for "
                             f"{len(entries)} entries")
        self._set_entries(entries, honest)      # (its counts are the honest side's)
        self.kind, self.strength = kind, float(strength)
        self.honest, self.byz = self.counts, byz

    def c_struct(self):
        a = FlsimAttack()
        a.kind = ATTACK_KINDS.get(self.kind, -1)
        a.strength = self.strength
        return self._fill_entries(a, honest=self.honest, byz=self.byz)


def attack_entries(attack, b_out=None, P=None):
    """Mix the attack's crafted vector into its entries in place, in one launch
    (flsim_attack_entries); b_out (optional, [P] fp32) receives the vector itself."""
    if P is None:
        P = int(next(e for e in attack.entries if e is not None).numel())
    a = attack.c_struct()
    check(lib().flsim_attack_entries(ctypes.byref(a), ptr(b_out), int(P), stream_ptr()))


class OptAttack(Attack):
    """The optimised attacks over bucket sums (flsim_attack_opt, include/flsim.h; Shejwalkar and
    Houmansadr 2021): kind "minmax" or "minsum", every Byzantine worker sends mu + gamma * strength
    * p with p the direction `dir` ("unit": -mu, "std": -sigma, "sign": -sign(mu)) and gamma solved
    on the device from the honest entries.  entries, honest and byz as Attack.  The object owns
    its scratch per (device, P, k), allocated at the first call and shared by the objects of a
    run; after a call gamma ([1] fp64), stats_a and stats_c ([kh] fp64), stats_q ([1]) and dist
    ([kh, kh] fp64, kh the entries with honest >= 1) are device tensors, read with no
    synchronisation beyond the stream's order; the next call overwrites them.  flsim/robust.py
    (opt_attack_flat) is the text."""
    _scratch = {}       # (device, P, k) -> buffers
    _scratch_struct, _partials = FlsimAttackOptScratch, "flsim_attack_opt_partials"

    def __init__(self, kind, dir, strength, entries, honest, byz):
        super().__init__(kind, strength, entries, honest, byz)
        self.dir = dir
        self.kh = sum(1 for h in self.honest if h >= 1)
        self.dist = self.stats = self.gamma = None

    def c_struct(self):
        a = FlsimAttackOpt()
        a.kind = OPT_ATTACK_KINDS.get(self.kind, -1)
        a.dir = OPT_ATTACK_DIRS.get(self.dir, -1)
        a.strength = self.strength
        return self._fill_entries(a, honest=self.honest, byz=self.byz)

    def _scratch_rows(self, k):
        kh = max(self.kh, 1)
        return (), (("dist", "dist", torch.float64, k * k + 2, (kh, kh)),
                    ("stats", "stats", torch.float64, ATTACK_OPT_STATS + 1, (ATTACK_OPT_STATS,)),
                    ("gamma", "gamma", torch.float64, 2, (1,)))

    @property
    def stats_a(self):
        return self.stats[:self.kh]

    @property
    def stats_c(self):
        return self.stats[MAX_ARRAYS:MAX_ARRAYS + self.kh]

    @property
    def stats_q(self):
        return self.stats[2 * MAX_ARRAYS:]


def opt_attack_entries(attack, b_out=None, P=None):
    """Solve the OptAttack's gamma on the device and mix the crafted vector into its entries in
    place, in four launches (flsim_attack_opt_entries); b_out (optional, [P] fp32) receives the
    vector itself; attack.gamma, .stats and .dist then hold the solve."""
    ref = next((e for e in attack.entries if e is not None), None)
    if P is None:
        P = int(ref.numel())
    a = attack.c_struct()
    s = attack.c_scratch(ref.device if ref is not None else "cpu", P)
    check(lib().flsim_attack_opt_entries(ctypes.byref(a), ctypes.byref(s), ptr(b_out), int(P),
                                         stream_ptr()))


class NNM(_BucketRule):
    """Nearest-neighbour mixing over bucket sums (flsim_nnm, include/flsim.h; Allouah et al.
    2023): every entry becomes the mean of the k - f of the k = len(entries) values entries[j] /
    counts[j] nearest to its own, itself included; a rule then reads the entries with counts 1.
    entries: flat fp32 device tensors of the same length, all updated in place (no None here);
    counts: the workers summed into each (>= 1).  The object owns its scratch per (device, P, k),
    allocated at the first call and shared by the objects of a run; after a call dist ([k, k]
    fp64) and nbr ([k] int64: bit j of nbr[i] = entry j is a neighbour of i) are device tensors,
    read with no synchronisation beyond the stream's order; the next call overwrites them.
    flsim/robust.py (nnm_flat) is the text."""
    _scratch = {}       # (device, P, k) -> buffers
    _what, _bad_count = "NNM", -1
    _scratch_struct, _partials = FlsimNnmScratch, "flsim_nnm_partials"

    def __init__(self, f, entries, counts):
        self._set_entries(entries, counts)
        self.f = int(f)
        self.dist = self.nbr = None

    def c_struct(self):
        a = FlsimNnm()
        a.f = self.f if -2 ** 31 <= self.f < 2 ** 31 else -1
        return self._fill_entries(a)

    def _scratch_rows(self, k):
        return (), (("dist", "dist", torch.float64, k * k + 2, (k, k)),
                    ("nbr", "nbr", torch.int64, k + 2, (k,)))

    def neighbours(self):
        """nbr read back as k ascending lists of entry indices (synchronises)."""
        return [[j for j in range(self.k) if (int(w) >> j) & 1] for w in self.nbr.tolist()]


def nnm_entries(nnm, P=None):
    """Replace the NNM's entries by their mixed means in place, in three launches
    (flsim_nnm_entries); nnm.dist and nnm.nbr then hold the distances and the neighbour masks."""
    ref = next((e for e in nnm.entries if e is not None), None)
    if P is None:
        P = int(ref.numel())
    a = nnm.c_struct()
    s = nnm.c_scratch(ref.device if ref is not None else "cpu", P)
    check(lib().flsim_nnm_entries(ctypes.byref(a), ctypes.byref(s), int(P), stream_ptr()))


def worker_table(recs, device):
    """recs: sequence of (t, i, k) -> device tensor of WorkerRec (uint32 x4)."""
    a = np.zeros((len(recs), 4), np.uint32)
    if len(recs):
        a[:, :3] = np.asarray(recs, np.int64).astype(np.uint32)
    return torch.from_numpy(a).to(device, non_blocking=True)
