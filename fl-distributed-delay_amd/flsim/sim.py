"""FLSimulation: the server loop of main.py:126-188 on MI355X.

Per epoch t (one "server step"):
  1. schedule scan on the host (flsim_sched_epoch; main.py:137-181) and the dataset draws
     k_i = np.random.randint(0, n) for every worker (main.py:138, seeded stream);
  2. the workers that compute this epoch are split into contiguous blocks, one per rank
     (torch.distributed; one process per GPU), and each rank runs its block as worker-batched
     chunks of `chunk_workers` x 128 samples through the HIP forward/backward; all of them use
     theta_t, so their gradients simply add (agents.py:35) -- S_t;
  3. world > 1: ONE all-reduce (RCCL) of [S_t partial | per-worker losses | per-worker BatchNorm
     statistics (vgg11_bn)]; BatchNorm running buffers advance over every computing worker's
     call in worker order;
  4. a slow worker that computed stores S_t in its FIFO (main.py:156,161: the entry is an alias
     of the epoch's .grad tensors, so under torch >= 2 it holds S_t); popped entries (main.py:162)
     are the stale gradients S_{t-d};
  5. fused rule() + Adam on the device: c_t copies of S_t and the stale entries (main.py:184,188);
  6. 'Avg. Loss' = np.mean of the fast workers' losses (main.py:172,185).

stale_weight (None, ("poly", a), ("hinge", a, b), ("const", a) or a callable tau -> float) discounts
a popped FIFO entry by its age tau = t - (the epoch it was pushed) before the average (FedAsync's
alternative to the throttle): rule() becomes sum_j w_j * entry_j / W, w = 1.0 for every S_t entry,
W = the sum of the weights (stale_normalize="weights") or the entry count ("count").

delay_comp (None or lambda >= 0) compensates a popped FIFO entry for the distance the model has
moved since the entry was pushed (DC-ASGD, Zheng et al. 2017), before any discount: x becomes
x + (x * x) * lambda * (theta_t - theta_src).  Every pushed slot carries the theta it was pushed
at; the server step writes that snapshot in its own pass.  An entry is S_src, a sum over that
epoch's workers, so x * x grows with the square of the worker count: choose lambda accordingly.

clip_grad_norm (None or max_norm > 0) clips the rule's output to that global 2-norm before the
update, what torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) does between `p.grad = ...`
and optim.step() (engine.Clip; float("inf") clips nothing and only records the norm).  It comes
after the all-reduce and is replicated, so it adds no collective; at world = 1 the epoch then ends
with the slab reduction and the clipped streaming step (three launches) instead of the one fused
launch.  grad_norms() returns the norm of every epoch's aggregate.

attack (None, "ipm", ("ipm", eps), "alie", ("alie", z)) with n_byz and byz_placement ("spread",
"block") turns n_byz of the delay-0 workers into simulated Byzantine workers that mount an
omniscient attack on the epoch's fresh bucket entries (flsim/robust.py: attack_flat; needs
robust_rule, ("trimmed_mean", 0) being the undefended mean over buckets).  They compute nothing:
one launch mixes the crafted vector into the bucket sums before the robust step reads them.
attack_log() returns every epoch's (kind, strength used, Byzantine workers present).
attack may also be "minmax" or "minsum", ("minmax", dir) or ("minmax", dir, strength) with dir
"unit", "std" (default) or "sign": the optimised attacks of Shejwalkar and Houmansadr 2021
(flsim/robust.py: opt_attack_flat), whose coefficient gamma is solved on the device from the
epoch's honest entries in four launches; strength (default 1) scales it.  attack_gamma_log()
returns every attacked epoch's gamma as a device tensor.

nnm (None or f >= 0; needs robust_rule) puts nearest-neighbour mixing (NNM, Allouah et al. 2023;
flsim/robust.py: nnm_flat) in front of the robust rule: after the attack, every entry of the epoch
(fresh buckets and popped slots alike) is replaced in place by the mean of its k - f nearest
entries, itself included, and the rule reads the mixed entries with count 1 each.  f is the number
of Byzantine ENTRIES assumed (2 f < this epoch's k).  With weights "count" the geometric median
and centered clipping therefore see equal weights.  nnm_log() returns every epoch's neighbour
masks.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .data import DevicePool, make_test_pool
from .engine import (PN1_SIZES, Clip, Optim, ProgramStager, Rule, engine_class, optim_defaults,
                     padded, split_views, staleness_weight)
from .robust import (BULYAN_KIND, CCLIP_KIND, GEOMED_KIND, KRUM_KINDS, OPT_ATTACK_KINDS, alie_z,
                     check_bulyan, check_krum, check_nnm, parse_attack, parse_rule)
from .schedule import Schedule, reference_delays

SEMANTICS = ("reference", "torch1", "independent")
# arrays of a weighted or compensated rule the fused step takes (csrc/slabstep.h: STEP_MAX_WARR,
# STEP_MAX_CARR)
STEP_MAX_WARR = 16
# checkpoint format: 2 records the model, the optimizer hyper-parameters and the throttle cap, and
# the reference's --delay 0 slow worker as DELAY_ZERO (restore() migrates format 1)
CKPT_FORMAT = "flsim-checkpoint-2"


def default_theta(seed=0, model="PerformantNet1"):
    """torch default init of the model (PerformantNet1 as main.py:97 builds it, or vgg11) under
    torch.manual_seed(seed) (CPU RNG), flattened in named_parameters order."""
    from FL import models
    torch.manual_seed(seed)
    m = models.PerformantNet1() if model == "PerformantNet1" else getattr(models, model)()
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()])


def load_model_file(path, model="PerformantNet1"):
    """--model_file (main.py:49-50,98-100): `model.load_state_dict(torch.load(path))` on the
    models.py module, then the flat theta0 in named_parameters order and the module's buffers
    (vgg11_bn running statistics; empty for the others).  The file is a plain state_dict, so it
    is read with weights_only=True; a missing or mismatched key raises load_state_dict's
    RuntimeError exactly as the reference would."""
    from FL import models
    m = getattr(models, model)()
    m.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))
    theta0 = torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    return theta0, dict(m.named_buffers())


class FLSimulation:
    def __init__(self, n_workers, delay=100, delays=None, throttle=False, lr=1e-3, seed=0,
                 semantics="reference", dropout=True, chunk_workers=128, device=None, theta0=None,
                 group=None, max_throttle=32, pool=None, betas=None, eps=None,
                 engine=None, device_pool=None, test_pool=None, model="PerformantNet1",
                 fused=True, keep_S=False, batch_size=128, distributed=None,
                 collective="torch", optimizer="adam", weight_decay=0.0, momentum=0.0,
                 dampening=0.0, nesterov=False, stale_weight=None, stale_normalize="weights",
                 delay_comp=None, clip_grad_norm=None, lr_decay=0.0,
                 initial_accumulator_value=None, robust_rule=None, buckets=8,
                 keep_entries=False, attack=None, n_byz=0, byz_placement="spread", nnm=None):
        if semantics not in SEMANTICS:
            raise NotImplementedError(f"semantics {semantics!r} (supported: {SEMANTICS})")
        # a robust rule in place of the mean (None: off; today's code paths exactly): (kind, trim),
        # ("krum" | "multi_krum", f, m), ("bulyan", f), ("geomed", iters, nu, weights), or ("cclip",
        # tau, iters, weights)
        self.robust = parse_rule(robust_rule)
        self.buckets = int(buckets)
        self.keep_entries = bool(keep_entries)
        self.last_entries = None
        self.last_selected = None       # Krum family with keep_entries: the entries chosen
        self.sel_log = []               # per epoch: list of ints (read back) or a device tensor
        self.last_geomed = None         # the geometric median with keep_entries: the epoch's GeoMed
        self.geomed_entries = []        # per epoch: (obj, final w), device tensors or read back
        # centered clipping: the carried center ([P] device tensor; None before the first step),
        # with keep_entries the epoch's CClip and a clone of the center before the step (None:
        # the step ran fresh); per epoch (final u, final w, last s), device tensors or read back
        self.center = None
        self.last_cclip = None
        self.last_center = None
        self.cclip_entries = []
        # simulated Byzantine workers (None: off; today's code paths exactly): (kind, strength) of
        # the attack n_byz of the delay-0 workers mount on the epoch's fresh entries
        self.attack = parse_attack(attack)
        self.n_byz = int(n_byz)
        self.byz_placement = byz_placement
        self.byz_workers = np.zeros(0, np.int64)
        self.last_attack = None         # with keep_entries: (b, honest, byz) of the last attack
        self.last_honest = None         # ... and the fresh entries' honest sums before it
        self.attack_entries_log = []    # per epoch: (kind, strength used, Byzantine present)
        # Min-Max / Min-Sum: (kind, dir, strength); gamma per attacked epoch, a cloned device tensor
        self.attack_gamma_entries = []
        self.last_attack_opt = None     # with keep_entries: (gamma, a, c, q, dist) of the last one
        if byz_placement not in ("spread", "block"):
            raise ValueError(f"byz_placement {byz_placement!r} (supported: 'spread', 'block')")
        if self.attack is not None and self.robust is None:
            # the bucketed path is the only place where entries exist
            raise NotImplementedError("an attack needs robust_rule: the bucketed entries are what "
                                      "it acts on (robust_rule=('trimmed_mean', 0) is the "
                                      "undefended mean over buckets)")
        if self.n_byz < 0:
            raise ValueError(f"n_byz = {self.n_byz}: it must be >= 0")
        # nearest-neighbour mixing of the entries before the rule (None: off; today's code paths
        # exactly): f, the Byzantine entries assumed; checked against every epoch's k
        if nnm is not None:
            if isinstance(nnm, bool) or not isinstance(nnm, (int, np.integer)):
                raise ValueError(f"Invalid NNM f = {nnm!r}: it must be an integer >= 0")
            if nnm < 0:
                raise ValueError(f"Invalid NNM f = {nnm}: it must be an integer >= 0")
            if self.robust is None:
                raise NotImplementedError("nnm needs robust_rule: the bucketed entries are what "
                                          "it acts on (robust_rule=('trimmed_mean', 0) is the "
                                          "mean over the mixed buckets)")
        self.nnm = None if nnm is None else int(nnm)
        self.last_mixed = None          # with keep_entries: clones of the mixed entries
        self.nnm_entries_log = []       # per epoch: the neighbour masks, a cloned device tensor
        if self.n_byz >= 1 and self.attack is None:
            raise ValueError(f"n_byz = {self.n_byz} Byzantine workers without an attack")
        if self.attack is not None and self.n_byz == 0:
            raise ValueError(f"attack {self.attack[0]!r} with n_byz = 0: no worker mounts it")
        if self.robust is not None:
            if self.buckets < 1:
                raise ValueError(f"buckets = {self.buckets}: it must be >= 1")
            if semantics != "independent":
                # under the reference's aliasing weight_ups is [S_t] * c + the stale entries: its
                # median is trivially S_t
                raise NotImplementedError(f"robust_rule with semantics {semantics!r}: the entries "
                                          "must be distinct (semantics='independent')")
        # delay compensation's lambda (None: off); theta is replicated, so at world > 1 every rank
        # keeps the same snapshots locally
        self.delay_comp = None if delay_comp is None else float(delay_comp)
        if self.delay_comp is not None:
            if not (self.delay_comp >= 0 and np.isfinite(self.delay_comp)):
                raise ValueError(f"Invalid delay compensation lambda {self.delay_comp}: it must "
                                 "be finite and >= 0")
            if semantics == "independent":
                # its popped slots are added with a torch add_ before the all-reduce: another path
                raise NotImplementedError("independent entries with delay compensation")
        # global-norm clipping of the aggregate (None: off; today's code paths exactly)
        self.clip_grad_norm = None if clip_grad_norm is None else float(clip_grad_norm)
        self.clip = None if clip_grad_norm is None else Clip(self.clip_grad_norm)
        self.norm_log = []        # per epoch: float (read back) or a 0-d device tensor
        # the discount of a popped entry's age; a replicated host computation (every rank derives
        # the same weights from the schedule)
        if stale_normalize not in ("weights", "count"):
            raise ValueError(f"stale_normalize {stale_normalize!r} (supported: 'weights', 'count')")
        if isinstance(stale_weight, str):
            stale_weight = None if stale_weight == "none" else (stale_weight,)
        self.stale_weight = stale_weight if stale_weight is None or callable(stale_weight) \
            else tuple(stale_weight)
        self.stale_normalize = stale_normalize
        self._stale_fn = None if stale_weight is None else staleness_weight(self.stale_weight)
        if self._stale_fn is not None and semantics == "independent":
            raise NotImplementedError("independent entries with a staleness discount")
        self.n = int(n_workers)
        if self.n < 1:
            raise ValueError("n_workers must be >= 1")
        self.delays = np.asarray(delays if delays is not None else reference_delays(self.n, delay),
                                 np.int32)
        self.delay_arg = delay
        if self.attack is not None:
            # the Byzantine set, fixed for the run, among the delay-0 workers in index order; slow
            # workers are never Byzantine
            F = np.nonzero(self.delays == 0)[0].astype(np.int64)
            nF, nb = len(F), self.n_byz
            if nb >= nF:
                raise ValueError(f"n_byz = {nb} of {nF} delay-0 workers: at least one of them "
                                 "must stay honest")
            pick = list(range(nb)) if byz_placement == "block" else \
                [((2 * q + 1) * nF) // (2 * nb) for q in range(nb)]
            self.byz_workers = F[pick]
        self.throttle = bool(throttle)
        # betas / eps / initial_accumulator_value None: the kind's conventional value (for "adam",
        # "adamw" and "sgd" (0.9, 0.999), 1e-8 and 0)
        dflt = optim_defaults(str(optimizer))
        betas = dflt["betas"] if betas is None else betas
        eps = dflt["eps"] if eps is None else eps
        if initial_accumulator_value is None:
            initial_accumulator_value = dflt["initial_accumulator_value"]
        self.lr, self.betas, self.eps = float(lr), tuple(betas), float(eps)
        # Central(model, optim)'s optimizer (main.py:106 builds Adam(lr)): "adam" (weight_decay:
        # coupled L2), "adamw" (decoupled), "sgd" (momentum, dampening, weight_decay, nesterov),
        # "adagrad" (lr_decay, weight_decay, initial_accumulator_value; FedAdagrad) or "yogi"
        # (betas, weight_decay, initial_accumulator_value; FedYogi);
        # refused here, before any device use, where torch's constructor raises ValueError
        self.optim = Optim(kind=str(optimizer), lr=self.lr, betas=self.betas, eps=self.eps,
                           weight_decay=float(weight_decay), momentum=float(momentum),
                           dampening=float(dampening), nesterov=bool(nesterov),
                           lr_decay=float(lr_decay),
                           initial_accumulator_value=float(initial_accumulator_value)).validate()
        # plain Adam keeps the flsim_aggregate_adam* / flsim_*_server_step entry points
        self._optim_arg = None if (self.optim.kind == "adam" and self.optim.weight_decay == 0) \
            else self.optim
        self.seed = int(seed)
        self.semantics = semantics
        self.dropout = bool(dropout)
        # fused: at world = 1 the epoch ends in ONE launch, slabs -> S_t -> rule() + Adam
        # (flsim_<net>_server_step); keep_S also writes S_t into comm[:P] (tests, debugging)
        self.fused = bool(fused)
        self.keep_S = bool(keep_S)
        # pipelined chunks (PN1), FLSIM_PIPELINE=1: off by default -- +0.4 % on the headline
        # (961 -> 965 worker-steps/s, profiles/r03d) but the per-kernel live timing then measures
        # overlapped kernels
        self.pipeline = os.environ.get("FLSIM_PIPELINE", "0") != "0"
        self.group = group
        self.model = model
        # --batch_size B (main.py:43-44): every worker-step is G = ceil(B/128) 128-sample groups
        # (the engine's unit; WorkerRec.pad = B, include/flsim.h), the last one padded
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self.G = -(-self.batch_size // 128)
        if self.batch_size != 128 and semantics == "independent":
            raise NotImplementedError("independent entries with --batch_size != 128")
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized():
            self.rank = dist.get_rank(group)
            self.world = dist.get_world_size(group)
        else:
            self.rank, self.world = 0, 1
        # distributed: the world > 1 code path (sharding, the one all-reduce per epoch, the
        # streaming server step after it).  Default: on iff world > 1; True at world = 1 runs that
        # path over a one-rank process group (bench.py --force-dist: RCCL on a single GPU)
        self.distributed = self.world > 1 if distributed is None else bool(distributed)
        if self.robust is not None and (self.distributed or self.world > 1):
            raise NotImplementedError("robust_rule with distributed runs: the epoch's entries "
                                      "would need an all-gather")
        if self.distributed and not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("distributed=True needs an initialised torch.distributed group")
        # the epoch's one all-reduce: "torch" = torch.distributed (RCCL with the nccl backend);
        # "flsim" = the C-ABI's flsim_allreduce_sum over RCCL (include/flsim.h), its unique id
        # shipped over the process group; "flsim-local" (world 1) = the C-ABI's one-rank
        # communicator, which never touches RCCL
        if collective not in ("torch", "flsim", "flsim-local"):
            raise ValueError(f"collective {collective!r}")
        if collective == "flsim-local" and self.world != 1:
            raise ValueError("collective='flsim-local' is the one-rank communicator")
        self.collective = collective
        self._comm = None
        if self.distributed and collective != "torch":
            from .comm import Comm
            if collective == "flsim":
                box = [Comm.unique_id() if self.rank == 0 else None]
                dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0)
                                           if group is not None else 0, group=group)
                self._comm = Comm(self.world, self.rank, box[0])
            else:
                self._comm = Comm()
        self.device = torch.device(device) if device is not None else \
            torch.device("cuda", torch.cuda.current_device())
        # engine / device_pool are injectable only so tests can drive the sharding and
        # collective logic with a CPU stand-in (gloo); the product path always builds PN1Engine
        # a chunk never needs more workers than the run has (the workspace scales with it)
        self.engine = engine if engine is not None else \
            engine_class(model)(self.device, min(int(chunk_workers), self.n * self.G))
        if self.batch_size != 128 and getattr(self.engine, "STATS_PER_WORKER", 0):
            raise NotImplementedError("BatchNorm models: one BatchNorm batch is one 128-sample "
                                      "fwd_bkwd call (--batch_size 128)")
        self.pool = device_pool if device_pool is not None else \
            DevicePool(self.device, self.seed, pool)
        self.max_throttle = int(max_throttle)
        self.sched = Schedule(self.n, self.delays, self.throttle, max_throttle)
        self.rs = np.random.RandomState(self.seed)   # main.py:138 np.random stream
        P = self.engine.P
        self.P = P
        self.Ppad = padded(P)
        th = default_theta(self.seed, model) if theta0 is None else torch.as_tensor(theta0)
        self.theta = th.to(self.device, torch.float32).contiguous().clone()
        # optimizer state: Adam family m = exp_avg, v = exp_avg_sq; SGD with momentum m = the
        # momentum buffer and no v; SGD without momentum neither; Adagrad m = sum and no v, Yogi as
        # Adam -- their accumulator (Adagrad's sum, Yogi's exp_avg_sq) starts at
        # initial_accumulator_value
        self.m = torch.zeros_like(self.theta) if self.optim.n_state >= 1 else None
        self.v = torch.zeros_like(self.theta) if self.optim.n_state >= 2 else None
        if self.optim.kind == "adagrad":
            self.m.fill_(self.optim.initial_accumulator_value)
        elif self.optim.kind == "yogi":
            self.v.fill_(self.optim.initial_accumulator_value)
        self.step = 0
        # [S_t | losses of the computing workers | their per-call BatchNorm statistics (vgg11_bn)]
        # -- one all-reduce per epoch when world > 1 (each rank fills only its workers' rows)
        self.nstat = int(getattr(self.engine, "STATS_PER_WORKER", 0))
        if self.nstat and semantics == "independent":
            raise NotImplementedError("independent entries with BatchNorm models")
        self.stats_off = self.Ppad + padded(self.n * self.G)
        self.comm = torch.zeros(self.stats_off + self.n * self.nstat, device=self.device)
        self._stager = ProgramStager(self.device)
        self.stale_store = {}     # epoch -> [slot tensor, refcount]
        self.stale_theta = {}     # epoch -> the slot's theta snapshot (delay_comp only)
        self.free_slots = []
        self.free_snaps = []
        self.trace = []
        self.loss_log = []        # per epoch: float (synced) or (device tensor, fast mask)
        self._test_src = test_pool  # (imgs, labels) of the test split, or None = synthetic
        self._test = None
        # measurement (bench.py): worker-steps this rank executed per epoch, and when enabled the
        # per-epoch collective bracketed by events on the compute stream (RCCL's own stream is
        # joined back into it by the blocking all_reduce, so the pair spans the collective and the
        # wait for the slowest rank)
        self.rank_worker_steps = []
        self.time_collective = False
        self.coll_events = []

    # ---------------------------------------------------------------------------------------------
    def _slot(self, n=None):
        """A FIFO slot of >= n floats (default Ppad): a released one when one is large enough."""
        n = self.Ppad if n is None else n
        for j in range(len(self.free_slots) - 1, -1, -1):
            if self.free_slots[j].numel() >= n:
                return self.free_slots.pop(j)
        slot = torch.empty(n, device=self.device)
        slot[self.P:].zero_()     # the [P, Ppad) padding and the tail enter the all-reduce
        return slot

    def _snap(self):
        """A theta snapshot buffer for a pushed slot (delay_comp); recycled with the slot."""
        return self.free_snaps.pop() if self.free_snaps else \
            torch.empty(self.Ppad, device=self.device)

    def _worker_table(self, t, workers, ks):
        """WorkerRec (t, i, k, 0) of this rank's computing workers, copied host->device from a
        pinned staging buffer (asynchronous: the host never waits for the GPU here).  With
        --batch_size B != 128 each worker is G records (t, i + g * 2^20, k, B), g < G."""
        G = self.G
        if G > 1 or self.batch_size != 128:
            workers = np.repeat(np.asarray(workers, np.int64), G)
            grp = np.tile(np.arange(G, dtype=np.int64), len(workers) // G)
        n = len(workers)
        if getattr(self, "_wt_cap", 0) < max(1, n):
            cap = max(1, n)
            pin = self.device.type == "cuda"
            self._wt_host = [torch.empty((cap, 4), dtype=torch.int32, pin_memory=pin)
                             for _ in range(2)]
            self._wt_dev = torch.empty((cap, 4), dtype=torch.int32, device=self.device)
            self._wt_ev = [None, None]
            self._wt_cap = cap
            self._wt_i = 0
        j = self._wt_i = self._wt_i ^ 1
        if self._wt_ev[j] is not None:
            self._wt_ev[j].synchronize()          # staging buffer j free again (2 epochs ago)
        h = self._wt_host[j][:n].numpy()
        h[:, 0] = t
        h[:, 2] = ks[workers]
        if G > 1 or self.batch_size != 128:
            h[:, 1] = workers + (grp << 20)
            h[:, 3] = self.batch_size
        else:
            h[:, 1] = workers
            h[:, 3] = 0
        dev = self._wt_dev[:n]
        if n:
            dev.copy_(self._wt_host[j][:n], non_blocking=True)
        if self.device.type == "cuda":
            ev = torch.cuda.Event()
            ev.record()
            self._wt_ev[j] = ev
        return dev

    def _reduce(self, buf):
        if self._comm is not None:
            self._comm.all_reduce_sum(buf)          # flsim_allreduce_sum (C-ABI, RCCL)
        else:
            torch.distributed.all_reduce(buf, group=self.group)

    def _all_reduce(self, buf):
        """The epoch's one collective (RCCL over xGMI: the nccl backend or the C-ABI's)."""
        if self.time_collective and self.device.type == "cuda":
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self._reduce(buf)
            e1.record()
            self.coll_events.append((e0, e1))
        else:
            self._reduce(buf)

    def collective_ms(self):
        """Per-epoch collective times (ms) recorded since the last call (synchronises)."""
        if not self.coll_events:
            return []
        self.coll_events[-1][1].synchronize()
        out = [a.elapsed_time(b) for a, b in self.coll_events]
        self.coll_events = []
        return out

    def _rule(self, plan, stale):
        """weight_ups of this epoch as a Rule: k = c_t + s_t entries, the stale ones in append
        (worker-index) order; identical arrays (several FIFOs popping the same epoch) share one
        array index."""
        k = plan.c_t + plan.s_t
        order = self._entry_order(plan)
        ws = self._entry_weights(plan)      # per popped entry, or None: the plain mean
        # delay compensation: the snapshot of every popped entry (None: as it stands -- a zero
        # entry, or this epoch's own S_t, for which theta has not moved)
        snaps = self._entry_snapshots(plan)
        if order is None:       # reference order: c_t copies of S_t, then the stale entries
            ckw = {} if snaps is None else dict(snapshots=snaps, delay_comp=self.delay_comp)
            if ws is None:
                return Rule(k, stale, c=plan.c_t, **ckw)
            full = [1.0] * plan.c_t + ws
            return Rule(k, stale, c=plan.c_t, **self._weighted(k, full, ws), **ckw)
        uniq, ev, uw, usn = [], [], [], []
        for j0, (pos, a) in enumerate(zip(order[0], stale)):
            # entries of one source epoch share an array, and their age, hence their weight (the
            # torch-1.x zero entries share one null array: a zero stays zero under any weight,
            # and the divisor below is summed over the entries, not the arrays)
            j = next((q for q, u in enumerate(uniq) if u is a), None)
            if j is None:
                uniq.append(a)
                uw.append(None if ws is None else ws[j0])
                usn.append(None if snaps is None else snaps[j0])   # ... and their snapshot
                j = len(uniq) - 1
            ev.append((pos, j))
        arrays = uniq
        ckw = {} if snaps is None else dict(snapshots=usn, delay_comp=self.delay_comp)
        if ws is None:
            return Rule(k, arrays, events=ev, stager=self._stager, **ckw)
        full = [1.0] * k
        for (pos, _), w in zip(ev, ws):
            full[pos] = w
        return Rule(k, arrays, events=ev, stager=self._stager, **self._weighted(k, full, uw),
                    **ckw)

    def _entry_snapshots(self, plan):
        """theta_src of every popped FIFO entry in append order (None for an entry that is not
        compensated); None when the epoch's rule carries no compensation at all."""
        if self.delay_comp is None or self.semantics != "reference" or not plan.stale:
            return None
        snaps = [None if int(src) == int(plan.t) else self.stale_theta[src]
                 for (_, src) in plan.stale]
        return None if all(x is None for x in snaps) else snaps

    def _entry_weights(self, plan):
        """s(tau) of every popped FIFO entry in append order, tau = t - (the epoch it was
        pushed); None when the epoch's rule is the plain mean: no discount, nothing popped, or
        all weights 1.0 (then the divisor is k under either normalisation)."""
        if self._stale_fn is None or not plan.stale:
            return None
        ws = [float(self._stale_fn(int(plan.t) - int(src))) for (_, src) in plan.stale]
        for w in ws:
            if not (w >= 0 and np.isfinite(w)):
                raise ValueError(f"Invalid weight {w}: a weight must be finite and >= 0")
        return None if all(w == 1.0 for w in ws) else ws

    def _weighted(self, k, full, weights):
        """Rule's weights / divisor arguments: full = the k entries' weights in weight_ups
        order (the rule text's `weights`)."""
        W = float(sum(full)) if self.stale_normalize == "weights" else float(k)
        return dict(weights=weights, divisor=W)

    @staticmethod
    def _entry_order(plan):
        """None when weight_ups is [S_t] * c_t followed by <= 8 stale entries (the reference:
        one slow worker, index n-1); else (positions of the stale entries in weight_ups, None):
        entries are appended in worker-index order (main.py:136-178)."""
        if not plan.stale:
            return None
        fast = np.nonzero(plan.fast)[0]
        sw = np.asarray([w for (w, _) in plan.stale], np.int64)
        if len(sw) <= 8 and (len(fast) == 0 or fast.max() < sw.min()):
            return None
        pos = np.searchsorted(fast, sw) + np.arange(len(sw))
        return [int(x) for x in pos], None

    def chunks(self, lo, hi):
        """[lo, hi) in the fewest launches of <= chunk_workers workers, sizes within one of each
        other (no short tail chunk running the GEMMs at low occupancy)."""
        n = hi - lo
        if n <= 0:
            return []
        k = -(-n // self.engine.chunk_workers)
        b = [lo + (j * n) // k for j in range(k + 1)]
        return list(zip(b[:-1], b[1:]))

    def shard(self, active):
        lo = (len(active) * self.rank) // self.world
        hi = (len(active) * (self.rank + 1)) // self.world
        return lo, hi

    def epoch(self, sync_loss=True):
        # raises IndexError like rule() on an empty weight_ups, ZeroDivisionError like main.py:158
        # under --delay 0
        plan = self.sched.next_epoch()
        t = plan.t
        ks = self.rs.randint(0, self.n, size=self.n)
        if self.robust is not None:
            return self._epoch_robust(plan, ks, sync_loss)
        if self.semantics == "independent":
            return self._epoch_independent(plan, ks, sync_loss)
        active = np.nonzero(plan.computes)[0]
        lo, hi = self.shard(active)
        eng = self.engine
        G = self.G                               # 128-sample groups (units) per worker-step
        # (clipping: the slab reduction, then the clipped streaming step)
        fused = self.fused and not self.distributed and hasattr(eng, "server_step") and \
            self.clip is None
        # (a weighted or compensated rule over more arrays than the fused step takes: reduce, then
        # stream)
        keep_S = self.keep_S or (fused and
                                 (self._stale_fn is not None or self.delay_comp is not None) and
                                 len({int(src) for (_, src) in plan.stale}) > STEP_MAX_WARR)
        pushes = plan.pushed and self.semantics == "reference"
        # An epoch that pushes S_t onto the FIFO and ends with the streaming server step (world > 1,
        # or an engine without the fused step) builds S_t -- and all-reduces it -- straight in the
        # slot it pushes, a whole [S_t | losses] comm buffer: the stream then reads S_t from the slot
        # and writes no second copy (4P fewer HBM bytes at every tick).  BatchNorm runs
        # keep the shared buffer (their comm buffer also holds n x the per-call statistics).
        # (keep_S: S_t stays in comm[:P], where the caller reads it)
        in_slot = pushes and not fused and not self.nstat and not keep_S
        comm = self._slot(self.stats_off) if in_slot else self.comm
        S = comm[:self.P]
        losses = comm[self.Ppad:self.Ppad + len(active) * G]
        stats = comm[self.stats_off:self.stats_off + len(active) * self.nstat].view(
            len(active), self.nstat)
        if self.distributed:
            losses.zero_()
            stats.zero_()
        eng.begin_epoch(self.theta)
        wt = self._worker_table(t, active[lo:hi], ks)      # one async upload per epoch
        chunks = self.chunks(lo * G, hi * G)
        # several chunks: pipelined (chunk i's forward beside chunk i-1's backward, two
        # workspaces); the library joins the backward stream at end_epoch / server_step
        pipe = self.pipeline and len(chunks) > 1 and getattr(eng, "PIPELINE", False) and \
            not self.nstat
        for j, (c0, c1) in enumerate(chunks):
            if pipe:
                eng.run_chunk_async(self.theta, self.pool, wt[c0 - lo * G:c1 - lo * G], c1 - c0,
                                    self.n, self.seed, self.dropout, losses[c0:c1], j)
                continue
            kw = {"stats_out": stats[c0:c1]} if self.nstat else {}
            eng.run_chunk(self.theta, self.pool, wt[c0 - lo * G:c1 - lo * G], c1 - c0, self.n,
                          self.seed, self.dropout, losses[c0:c1], **kw)
        if not fused or keep_S:
            eng.end_epoch(S)
        self.rank_worker_steps.append(hi - lo)
        if self.distributed:
            end = self.stats_off + len(active) * self.nstat if self.nstat else \
                self.Ppad + len(active) * G
            self._all_reduce(comm[:end])
        if self.nstat:   # BatchNorm running buffers: every computing worker's call, in order
            eng.update_running(stats, len(active))
        push = snap = None
        if pushes:
            n_push = int(sum(1 for i in range(self.n) if self.delays[i] != 0 and plan.computes[i]))
            push = comm if in_slot else self._slot()
            if self.delay_comp is not None:
                snap = self._snap()
            if fused and keep_S:
                push[:self.P].copy_(S)
                if snap is not None:
                    snap[:self.P].copy_(self.theta)
            # otherwise the server step writes S_t into the slot (and theta_t into its snapshot)
            # in its own pass: the fused slab step (world = 1) or the stream after the
            # all-reduce (world > 1)
            self.stale_store[t] = [push, n_push]
            if snap is not None:
                self.stale_theta[t] = snap
        stale = []
        for (_, src) in plan.stale:
            if self.semantics == "reference":
                entry = self.stale_store[src]
                stale.append(entry[0])
            else:
                stale.append(None)
        self.step += 1
        rule = self._rule(plan, stale)
        hp = dict(lr=self.lr, betas=self.betas, eps=self.eps)
        if self._optim_arg is not None:
            hp = dict(optim=self._optim_arg)
        if snap is not None and not (fused and keep_S):
            hp["theta_out"] = snap
        if self.clip is not None:
            hp["clip"] = self.clip
        if fused and not keep_S:
            eng.server_step(push, rule, self.theta, self.m, self.v, self.step, **hp)
        elif fused:
            eng.aggregate_rule(S, rule, self.theta, self.m, self.v, self.step, **hp)
        else:
            eng.aggregate_rule(S, rule, self.theta, self.m, self.v, self.step,
                               S_out=None if in_slot else push, **hp)
        for (_, src) in plan.stale:
            if self.semantics == "reference":
                entry = self.stale_store[src]
                entry[1] -= 1
                if entry[1] == 0:
                    self.free_slots.append(entry[0])
                    if src in self.stale_theta:
                        self.free_snaps.append(self.stale_theta.pop(src))
                    del self.stale_store[src]
        self._log_norm()
        fast_pos = np.nonzero(plan.fast[active])[0]
        self.trace.append(plan)
        if sync_loss:
            lv = self._worker_losses(losses.detach().cpu().numpy())[fast_pos]
            val = float(np.mean(lv.astype(np.float32))) if len(lv) else float("nan")
            self.loss_log.append(val)
            return val
        self.loss_log.append((losses.detach().clone(), fast_pos))
        return None

    def _worker_losses(self, lv):
        """Per-worker CrossEntropyLoss(mean) from the per-group values (group sum / 128):
        sum over the worker's groups * 128 / B (agents.py:40's lossval per call)."""
        if self.G == 1 and self.batch_size == 128:
            return lv
        tot = lv.reshape(-1, self.G).astype(np.float64).sum(1)
        return (tot * 128.0 / self.batch_size).astype(np.float32)

    def _epoch_independent(self, plan, ks, sync_loss):
        """Independent-entry semantics: every weight_ups entry is a distinct
        per-worker gradient and a slow worker's FIFO holds its own gradient.  Slow workers with
        the same delay d tick together (t == 0 or t % d == 0) and pop together d epochs later, so
        their FIFO entries are kept as ONE slot per delay class holding the class's summed
        gradient: each class is one worker-batched launch, owned by rank d mod world.  The fast
        workers are sharded as usual.  Each rank adds the popped class slots it owns to its
        partial sum, so the one all-reduce combines the partial sums of all k entries; mean =
        sum / k, then the same Adam step, replicated."""
        from .schedule import DELAY_ZERO
        t = plan.t
        eng = self.engine
        active = np.nonzero(plan.computes)[0]
        slow_mask = self.delays[active] != 0
        fast, slow = active[~slow_mask], active[slow_mask]

        def dclass(i):
            d = int(self.delays[i])
            return 0 if d == DELAY_ZERO else abs(d)
        classes = {}
        for i in slow:
            classes.setdefault(dclass(i), []).append(int(i))
        own = [(d, ws) for d, ws in sorted(classes.items()) if d % self.world == self.rank]
        lo, hi = self.shard(fast)
        S = self.comm[:self.P]
        losses = self.comm[self.Ppad:self.Ppad + len(fast)]
        if self.distributed:
            losses.zero_()
        own_workers = np.asarray([i for _, ws in own for i in ws], np.int64)
        wt = self._worker_table(t, np.concatenate([own_workers, fast[lo:hi]]), ks)
        cw = self.engine.chunk_workers
        if getattr(self, "_slow_loss", None) is None or self._slow_loss.numel() < cw:
            self._slow_loss = torch.zeros(cw, device=self.device)
        off = 0
        for d, ws in own:                        # one FIFO slot per delay class (its sum)
            eng.begin_epoch(self.theta)
            n_ws = len(ws)
            k = -(-n_ws // cw)
            for j in range(k):
                c0, c1 = (j * n_ws) // k, ((j + 1) * n_ws) // k
                eng.run_chunk(self.theta, self.pool, wt[off + c0:off + c1], c1 - c0, self.n,
                              self.seed, self.dropout, self._slow_loss[:c1 - c0])
            slot = self._slot()
            eng.end_epoch(slot[:self.P])
            self.stale_store[(d, t)] = slot
            off += n_ws
        ns = off
        eng.begin_epoch(self.theta)
        for c0, c1 in self.chunks(lo, hi):
            eng.run_chunk(self.theta, self.pool, wt[ns + c0 - lo:ns + c1 - lo], c1 - c0, self.n,
                          self.seed, self.dropout, losses[c0:c1])
        eng.end_epoch(S)
        for (i, src) in plan.stale:              # popped entries, added once per class slot
            key = (dclass(int(i)), int(src))
            if key[0] % self.world == self.rank and key in self.stale_store:
                slot = self.stale_store.pop(key)
                S.add_(slot[:self.P])
                self.free_slots.append(slot)
        self.rank_worker_steps.append(hi - lo + len(own_workers))
        if self.distributed:
            self._all_reduce(self.comm[:self.Ppad + len(fast)])
        self.step += 1
        eng.aggregate_adam_sum(S, len(fast) + len(plan.stale), self.theta, self.m, self.v,
                               self.step, self.lr, self.betas, self.eps,
                               **({"optim": self._optim_arg} if self._optim_arg else {}),
                               **({"clip": self.clip} if self.clip is not None else {}))
        self._log_norm()
        self.trace.append(plan)
        if sync_loss:
            lv = losses.detach().cpu().numpy()
            val = float(np.mean(lv.astype(np.float32))) if len(lv) else float("nan")
            self.loss_log.append(val)
            return val
        self.loss_log.append((losses.detach().clone(), np.arange(len(fast))))
        return None

    def _epoch_robust(self, plan, ks, sync_loss):
        """A robust rule over bucket means (world = 1, independent entries).  The epoch's fast
        workers are split into `buckets` contiguous buckets, each one begin_epoch / chunks /
        end_epoch pass into a slot of its own (the bucket's SUM; its count = the bucket size) --
        the pattern the delay classes already follow, at no extra GEMM work.  The entries of the
        rule are the fresh buckets, then the popped delay-class slots in pop order (count = the
        popped workers sharing the slot); one fused robust step (median / trimmed mean of the
        entries' means, or Krum / Multi-Krum over them: the entry closest to its neighbours, which
        drops a popped entry that has drifted away from the fresh buckets; then the update)
        follows, clipped if configured."""
        from .engine import Robust
        from .schedule import DELAY_ZERO
        t = plan.t
        eng = self.engine
        active = np.nonzero(plan.computes)[0]
        slow_mask = self.delays[active] != 0
        fast, slow = active[~slow_mask], active[slow_mask]

        def dclass(i):
            d = int(self.delays[i])
            return 0 if d == DELAY_ZERO else abs(d)
        classes = {}
        for i in slow:
            classes.setdefault(dclass(i), []).append(int(i))
        own = sorted(classes.items())
        # Byzantine workers compute nothing: they are left out of the passes and of the losses
        is_byz = np.isin(fast, self.byz_workers)
        honest_fast = fast[~is_byz]
        hpos = np.concatenate([[0], np.cumsum(~is_byz)]).astype(np.int64)
        losses = self.comm[self.Ppad:self.Ppad + len(honest_fast)]
        own_workers = np.asarray([i for _, ws in own for i in ws], np.int64)
        wt = self._worker_table(t, np.concatenate([own_workers, honest_fast]), ks)
        cw = self.engine.chunk_workers
        if getattr(self, "_slow_loss", None) is None or self._slow_loss.numel() < cw:
            self._slow_loss = torch.zeros(cw, device=self.device)
        off = 0
        for d, ws in own:                        # one FIFO slot per delay class (its sum)
            eng.begin_epoch(self.theta)
            n_ws = len(ws)
            k = -(-n_ws // cw)
            for j in range(k):
                c0, c1 = (j * n_ws) // k, ((j + 1) * n_ws) // k
                eng.run_chunk(self.theta, self.pool, wt[off + c0:off + c1], c1 - c0, self.n,
                              self.seed, self.dropout, self._slow_loss[:c1 - c0])
            slot = self._slot()
            eng.end_epoch(slot[:self.P])
            self.stale_store[(d, t)] = slot
            off += n_ws
        ns = off
        entries, counts, byz = [], [], []
        B, nf = self.buckets, len(fast)
        for j in range(B):                       # fresh entries: one pass per non-empty bucket
            b0, b1 = (j * nf) // B, ((j + 1) * nf) // B
            if b1 == b0:
                continue
            # (the boundaries are drawn over all fast workers; the pass runs the honest ones)
            h0, h1 = int(hpos[b0]), int(hpos[b1])
            if h1 > h0:
                eng.begin_epoch(self.theta)
                for c0, c1 in self.chunks(h0, h1):
                    eng.run_chunk(self.theta, self.pool, wt[ns + c0:ns + c1], c1 - c0, self.n,
                                  self.seed, self.dropout, losses[c0:c1])
                slot = self._slot()
                eng.end_epoch(slot[:self.P])
            else:       # no honest worker: no pass, a free slot the attack writes whole
                slot = self._slot()
            entries.append(slot)
            counts.append(h1 - h0)
            byz.append((b1 - b0) - (h1 - h0))
        if self.attack is not None:
            self._attack(entries, counts, byz, len(fast))
        popped = {}
        for (i, src) in plan.stale:              # stale entries: one per (class, src) slot
            key = (dclass(int(i)), int(src))
            if key in popped:
                counts[popped[key]] += 1
            elif key in self.stale_store:
                popped[key] = len(entries)
                entries.append(self.stale_store.pop(key))
                counts.append(1)
        self.rank_worker_steps.append(len(honest_fast) + len(own_workers))
        if not entries:
            raise IndexError("empty weight_ups (reference: IndexError in rule, main.py:25)")
        if len(entries) > 64:
            raise ValueError(f"robust rule over k = {len(entries)} entries (1 .. 64): fewer "
                             "buckets or delay classes are needed")
        if self.keep_entries:
            self.last_entries = ([e[:self.P].clone() for e in entries], list(counts))
        if self.nnm is not None:
            counts = self._nnm(entries, counts)
        if self.robust[0] in KRUM_KINDS:
            # Krum / Multi-Krum: f and m against this epoch's k, as the trim is refused below
            from .engine import Krum
            _, f, m = self.robust
            check_krum(f, m, len(entries))
            self.step += 1
            krum = Krum(f, m, [e[:self.P] for e in entries], counts)
            eng.krum_step(krum, self.theta, self.m, self.v, self.step, optim=self.optim,
                          clip=self.clip)
            self.sel_log.append(krum.sel.detach().clone())      # (a device tensor: no sync)
            if self.keep_entries:           # (reads the device selection back: synchronises)
                self.last_selected = [int(j) for j in krum.sel.tolist()]
        elif self.robust[0] == BULYAN_KIND:
            # Bulyan: f against this epoch's k, as Krum's
            from .engine import Bulyan
            _, f = self.robust
            check_bulyan(f, len(entries))
            self.step += 1
            bul = Bulyan(f, [e[:self.P] for e in entries], counts)
            eng.bulyan_step(bul, self.theta, self.m, self.v, self.step, optim=self.optim,
                            clip=self.clip)
            self.sel_log.append(bul.sel.detach().clone())       # (a device tensor: no sync)
            if self.keep_entries:           # (reads the device selection back: synchronises)
                self.last_selected = [int(j) for j in bul.sel.tolist()]
        elif self.robust[0] == CCLIP_KIND:
            # centered clipping around the last epoch's aggregate (the first step: around zero,
            # the center's memory is then not read)
            from .engine import CClip
            _, tau, iters, weights = self.robust
            fresh = self.center is None
            if fresh:
                self.center = torch.empty(self.P, device=self.theta.device)
            if self.keep_entries:
                self.last_center = None if fresh else self.center.clone()
            self.step += 1
            cc = CClip(tau, iters, weights == "count", [e[:self.P] for e in entries], counts,
                       self.center, fresh=fresh)
            eng.cclip_step(cc, self.theta, self.m, self.v, self.step, optim=self.optim,
                           clip=self.clip)
            # (device tensors, cloned: no sync; the scratch is the next epoch's too)
            self.cclip_entries.append((cc.u[-1].detach().clone(), cc.w[-1].detach().clone(),
                                       cc.s[-1].detach().clone()))
            if self.keep_entries:
                self.last_cclip = cc
        elif self.robust[0] == GEOMED_KIND:
            # the geometric median (RFA): alpha = 1, or the entries' counts
            from .engine import GeoMed
            _, iters, nu, weights = self.robust
            self.step += 1
            gm = GeoMed(iters, nu, weights == "count", [e[:self.P] for e in entries], counts)
            eng.geomed_step(gm, self.theta, self.m, self.v, self.step, optim=self.optim,
                            clip=self.clip)
            # (device tensors, cloned: no sync; the scratch is the next epoch's too)
            self.geomed_entries.append((gm.obj.detach().clone(), gm.w[-1].detach().clone()))
            if self.keep_entries:
                self.last_geomed = gm
        else:
            kind, trim = self.robust
            self.step += 1
            eng.robust_step(Robust(kind, trim, [e[:self.P] for e in entries], counts),
                            self.theta, self.m, self.v, self.step, optim=self.optim,
                            clip=self.clip)
        self.free_slots.extend(entries)
        self._log_norm()
        self.trace.append(plan)
        if sync_loss:
            lv = losses.detach().cpu().numpy()
            val = float(np.mean(lv.astype(np.float32))) if len(lv) else float("nan")
            self.loss_log.append(val)
            return val
        self.loss_log.append((losses.detach().clone(), np.arange(len(honest_fast))))
        return None

    def _attack(self, entries, counts, byz, n_fast):
        """The epoch's attack on the fresh entries (bucket sums of their honest workers, `counts`;
        `byz` Byzantine workers each): one launch mixes the crafted vector into the slots in place
        and the counts become honest + Byzantine.  An epoch whose fast set holds no Byzantine
        worker (throttling) runs none; one with no honest fast worker raises the library's
        ValueError."""
        from .engine import Attack, OptAttack
        kind, strength = self.attack[0], self.attack[-1]
        present = int(sum(byz))
        if present == 0:
            self.attack_entries_log.append((kind, None, 0))
            return
        if strength is None:                    # ALIE's default: the paper's z for this epoch
            strength = alie_z(n_fast, present)
        b = None
        if self.keep_entries:
            b = torch.empty(self.P, device=self.device)
            self.last_honest = [e[:self.P].clone() if h else None
                                for e, h in zip(entries, counts)]
        if kind in OPT_ATTACK_KINDS:            # Min-Max / Min-Sum: gamma is solved on the device
            at = OptAttack(kind, self.attack[1], strength, [e[:self.P] for e in entries], counts,
                           byz)
            self.engine.attack_entries(at, b_out=b)
            self.attack_gamma_entries.append(at.gamma.detach().clone())     # (no sync)
            if self.keep_entries:
                self.last_attack_opt = tuple(x.detach().clone() for x in (
                    at.gamma, at.stats_a, at.stats_c, at.stats_q, at.dist))
        else:
            self.engine.attack_entries(Attack(kind, strength, [e[:self.P] for e in entries],
                                              counts, byz), b_out=b)
        if self.keep_entries:
            self.last_attack = (b, list(counts), list(byz))
        for j, nb in enumerate(byz):
            counts[j] += nb
        self.attack_entries_log.append((kind, float(strength), present))

    def _nnm(self, entries, counts):
        """Nearest-neighbour mixing of all the epoch's entries in place (three launches): every
        slot here is owned by this epoch and goes back to free_slots after the step, so nothing
        else reads it.  f is checked against this epoch's k, as Krum's.  Returns the counts the
        rule then reads: 1 each."""
        from .engine import NNM
        check_nnm(self.nnm, len(entries))
        mix = NNM(self.nnm, [e[:self.P] for e in entries], counts)
        self.engine.nnm_entries(mix)
        self.nnm_entries_log.append(mix.nbr.detach().clone())   # (a device tensor: no sync)
        if self.keep_entries:
            self.last_mixed = [e[:self.P].clone() for e in entries]
        return [1] * len(entries)

    def nnm_log(self):
        """Per epoch of a run with nnm (else []) the neighbour masks as cloned device tensors
        ([k] int64: bit j of word i = entry j is a neighbour of entry i).  Never synchronises."""
        return list(self.nnm_entries_log)

    def attack_log(self):
        """Per epoch of a run under attack (else []) the triple (kind, strength used, Byzantine
        workers among the epoch's fast set) as Python values; (kind, None, 0) for an epoch whose
        fast set held no Byzantine worker.  Never synchronises."""
        return list(self.attack_entries_log)

    def attack_gamma_log(self):
        """Per attacked epoch of a run under "minmax" / "minsum" (else []) the solved gamma as a
        cloned device tensor ([1] fp64).  Never synchronises."""
        return list(self.attack_gamma_entries)

    def _log_norm(self):
        """Keep this epoch's norm: a clone of the device scalar, read back only by grad_norms()."""
        if self.clip is not None:
            self.norm_log.append(self.clip.total_norm.detach().clone())

    def grad_norms(self):
        """The global 2-norm of every epoch's aggregate before clipping (clip_grad_norm runs
        only; else []), as floats.  Synchronises on the first call after new epochs."""
        self.norm_log = [float(x) for x in self.norm_log]
        return list(self.norm_log)

    def selections(self):
        """The entries Krum, Multi-Krum or Bulyan selected in every epoch (else []), as lists of ints:
        indices into the epoch's entries, the fresh buckets first, then the popped slots.
        Synchronises on the first call after new epochs."""
        self.sel_log = [x if isinstance(x, list) else [int(j) for j in x.tolist()]
                        for x in self.sel_log]
        return [list(x) for x in self.sel_log]

    def geomed_log(self):
        """Per epoch of a geometric-median run (else []) the pair (obj, w): the objective
        sum_j alpha_j ||x_j - z_r|| at every iterate z_r, r < iters, as a list of floats, and the
        final weights w^(iters) over the epoch's entries (the fresh buckets first, then the
        popped slots).  Synchronises on the first call after new epochs."""
        self.geomed_entries = [(o if isinstance(o, list) else [float(x) for x in o.tolist()],
                                w if isinstance(w, list) else [float(x) for x in w.tolist()])
                               for o, w in self.geomed_entries]
        return [(list(o), list(w)) for o, w in self.geomed_entries]

    def cclip_log(self):
        """Per epoch of a centered-clipping run (else []) the triple (u, w, n_clipped): the final
        weight of the center and the final weights of the epoch's entries (the fresh buckets
        first, then the popped slots) in g = u * center + sum_j w[j] * x_j, as a float and a list
        of floats, and the number of entries the last iteration clipped (s < 1; a dead entry, s =
        0, counts).  Synchronises on the first call after new epochs."""
        def read(e):
            if not torch.is_tensor(e[0]):
                return e
            u, w, s = e
            return (float(u), [float(x) for x in w.tolist()],
                    sum(1 for x in s.tolist() if x < 1))
        self.cclip_entries = [read(e) for e in self.cclip_entries]
        return [(u, list(w), n) for u, w, n in self.cclip_entries]

    def losses(self):
        out = []
        for e in self.loss_log:
            if isinstance(e, tuple):
                lv = self._worker_losses(e[0].cpu().numpy())[e[1]]
                out.append(float(np.mean(lv.astype(np.float32))) if len(lv) else float("nan"))
            else:
                out.append(e)
        self.loss_log = list(out)
        return out

    # ---------------------------------------------------------------------------------------------
    def evaluate(self):
        """util.print_test_accuracy (util.py:31-45) as main.py:190,196-210 uses it: the central
        model in eval mode (dropout off) over the whole test split, batches in order.  Returns
        (accuracy %, [per-class accuracy %] * 10).  The reference logs np.mean of the first as
        'Avg. Test Accuracy' and means the last class's entry as 'Class 9 Test Accuracy'
        (main.py:203 indexes the scalar util returns; here the per-class list exists)."""
        if self._test is None:
            src = self._test_src if self._test_src is not None else make_test_pool(self.seed)
            self._test = DevicePool(self.device, self.seed, src)
        pred = self.engine.evaluate(self.theta, self._test)
        labels = self._test.labels
        ok = (pred == labels)
        acc = 100.0 * int(ok.sum()) / int(labels.numel())
        per = []
        for c in range(10):
            sel = labels == c
            nc = int(sel.sum())
            per.append(100.0 * int((ok & sel).sum()) / nc if nc else float("nan"))
        return acc, per

    def model_state_dict(self):
        """The models.py module's state_dict (torch.save-compatible with the reference's
        main.py:98-100 / :192-194 load_state_dict / save); BatchNorm buffers follow their
        module's parameters, as nn.Module.state_dict orders them."""
        from collections import OrderedDict
        shapes = self.engine.SHAPES
        bufs = self.engine.buffer_state()
        out = OrderedDict()
        for (name, _), v in zip(shapes, split_views(self.theta, shapes)):
            out[name] = v.detach().cpu().clone()
            mod = name.rsplit(".", 1)[0]
            if name.endswith(".bias"):
                for bname, b in bufs:
                    if bname.rsplit(".", 1)[0] == mod:
                        out[bname] = b
        return out

    # -- checkpoint / resume ----------------------------------------------------------------------
    def checkpoint(self):
        """Everything needed to continue bit-for-bit: theta, Adam m/v/step, the epoch counter,
        the FIFO'd stale gradients still referenced, the loss log.  The schedule and the numpy
        k-draws are deterministic scans and are replayed on restore."""
        if self.semantics == "independent":
            raise NotImplementedError("checkpoint of the independent-entry semantics")
        return {
            "format": CKPT_FORMAT,
            "config": {"n": self.n, "delays": torch.from_numpy(self.delays.copy()),
                       "model": self.model,
                       "throttle": self.throttle, "seed": self.seed, "semantics": self.semantics,
                       "dropout": self.dropout, "lr": self.lr, "betas": list(self.betas),
                       "eps": self.eps, "max_throttle": self.max_throttle,
                       "batch_size": self.batch_size, **self._optim_config(),
                       **self._stale_config()},
            "epoch": len(self.trace), "step": self.step,
            "theta": self.theta.detach().cpu(),
            # the state arrays the optimizer owns (SGD: no v; without momentum no m either)
            **{k: a.detach().cpu() for k, a in (("m", self.m), ("v", self.v)) if a is not None},
            "stale": {int(src): (slot[:self.P].detach().cpu(), int(rc))
                      for src, (slot, rc) in self.stale_store.items()},
            # delay compensation: the theta snapshot of every live slot
            "stale_theta": {int(src): snap[:self.P].detach().cpu()
                            for src, snap in self.stale_theta.items()},
            "loss_log": [float(x) for x in self.losses()],
            "grad_norms": self.grad_norms(),
            "buffers": dict(getattr(self.engine, "buffer_state", list)()),
        }

    def _optim_config(self):
        o = self.optim
        return {"optimizer": o.kind, "weight_decay": o.weight_decay, "momentum": o.momentum,
                "dampening": o.dampening, "nesterov": o.nesterov, "lr_decay": o.lr_decay,
                "initial_accumulator_value": o.initial_accumulator_value}

    def _stale_config(self):
        """The discount as the checkpoint records it: its spec as a list (None: no discount) and
        the normaliser.  The weights themselves are no state: they depend only on (t, src)."""
        if callable(self.stale_weight):
            raise NotImplementedError("checkpoint of a run whose stale_weight is a callable: "
                                      "only a spec (('poly', a), ('hinge', a, b), ('const', a)) "
                                      "can be recorded and checked at restore")
        spec = None if self.stale_weight is None else \
            [self.stale_weight[0]] + [float(x) for x in self.stale_weight[1:]]
        return {"stale_weight": spec, "stale_normalize": self.stale_normalize,
                "delay_comp": self.delay_comp, "clip_grad_norm": self.clip_grad_norm,
                "robust_rule": None if self.robust is None else list(self.robust),
                "buckets": self.buckets,
                "attack": None if self.attack is None else list(self.attack),
                "nnm": self.nnm,
                "n_byz": self.n_byz, "byz_placement": self.byz_placement}

    def save_checkpoint(self, path):
        torch.save(self.checkpoint(), path)

    def restore(self, ck):
        """Resume from checkpoint() / save_checkpoint() output (a dict, or a path loaded with
        weights_only=True).  The simulation must be fresh and built with the same config."""
        if isinstance(ck, (str, bytes)) or hasattr(ck, "__fspath__"):
            ck = torch.load(ck, map_location="cpu", weights_only=True)
        fmt = ck.get("format")
        if fmt not in (CKPT_FORMAT, "flsim-checkpoint-1"):
            raise ValueError("not an flsim checkpoint")
        cfg = dict(ck["config"])
        mine = {"n": self.n, "throttle": self.throttle, "seed": self.seed,
                "semantics": self.semantics, "dropout": self.dropout, "model": self.model,
                "lr": self.lr, "betas": list(self.betas), "eps": self.eps,
                "max_throttle": self.max_throttle, "batch_size": self.batch_size,
                **self._optim_config(), **self._stale_config()}
        # a checkpoint from before the optimizer was recorded: Adam without weight decay
        for k, v in (("optimizer", "adam"), ("weight_decay", 0.0), ("momentum", 0.0),
                     ("dampening", 0.0), ("nesterov", False),
                     # ... and from before Adagrad and Yogi: neither hyper-parameter acts
                     ("lr_decay", 0.0), ("initial_accumulator_value", 0.0),
                     # ... and from before the staleness discount: none
                     ("stale_weight", None), ("stale_normalize", "weights"),
                     # ... and from before delay compensation: off
                     ("delay_comp", None),
                     # ... and from before gradient clipping: off
                     ("clip_grad_norm", None),
                     # ... and from before the robust rules: off, the default bucket count
                     ("robust_rule", None), ("buckets", 8),
                     # ... and from before the simulated Byzantine workers: none
                     ("attack", None), ("n_byz", 0), ("byz_placement", "spread"),
                     # ... and from before nearest-neighbour mixing: off
                     ("nnm", None)):
            cfg.setdefault(k, v)
        delays = cfg["delays"].numpy().astype(np.int32)
        if fmt == "flsim-checkpoint-1":
            # format 1 (round 1) had no model / optimizer / throttle-cap keys (they were the
            # defaults) and stored the slow worker of --delay 0 as 0 (now DELAY_ZERO)
            import warnings
            from .schedule import DELAY_ZERO
            for k, v in (("model", "PerformantNet1"), ("lr", 1e-3), ("betas", [0.9, 0.999]),
                         ("eps", 1e-8), ("max_throttle", 32), ("batch_size", 128)):
                if k not in cfg:
                    cfg[k] = v
                    warnings.warn(f"format-1 checkpoint: {k} not recorded, taken as {v!r}")
            delays = np.where((delays == 0) & (self.delays == DELAY_ZERO), DELAY_ZERO, delays)
        for k, v in mine.items():
            if cfg.get(k) != v:
                raise ValueError(f"checkpoint {k}={cfg.get(k)!r} differs from this run ({v!r})")
        if not np.array_equal(delays, self.delays):
            raise ValueError("checkpoint delays differ from this run")
        if self.trace:
            raise ValueError("restore() needs a fresh simulation")
        T = int(ck["epoch"])
        for _ in range(T):                    # replay the integer scan and the k-draws
            self.trace.append(self.sched.next_epoch())
            self.rs.randint(0, self.n, size=self.n)
        self.step = int(ck["step"])
        self.theta.copy_(ck["theta"].to(self.device))
        if self.m is not None:
            self.m.copy_(ck["m"].to(self.device))
        if self.v is not None:
            self.v.copy_(ck["v"].to(self.device))
        self.stale_store = {}
        for src, (vals, rc) in ck["stale"].items():
            slot = self._slot()
            slot[:self.P].copy_(vals.to(self.device))
            self.stale_store[int(src)] = [slot, int(rc)]
        self.stale_theta = {}
        if self.delay_comp is not None:
            for src, vals in ck["stale_theta"].items():
                snap = self._snap()
                snap[:self.P].copy_(vals.to(self.device))
                self.stale_theta[int(src)] = snap
        self.loss_log = list(ck["loss_log"])
        self.norm_log = [float(x) for x in ck.get("grad_norms", [])]
        if ck.get("buffers"):
            self.engine.load_buffers(ck["buffers"])

    def executed_worker_steps(self, plan):
        return int(plan.computes.sum())

    def param_views(self):
        return split_views(self.theta, self.engine.SHAPES)


__all__ = ["FLSimulation", "default_theta", "PN1_SIZES"]
