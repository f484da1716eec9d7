"""Drop-in for the reference's main.py (main.py:37-212) on MI355X.

Same flags and defaults (main.py:38-53): --n_workers --n_epochs --batch_size --learning_rate
--delay --model_file --throttle.  --optimizer {adam,adamw,sgd,adagrad,yogi} with --momentum
--dampening --nesterov --weight_decay --lr_decay --initial_accumulator_value --eps --beta1 --beta2
picks the central optimizer (main.py:106 hard-wires Adam(lr)); adagrad and yogi are FedAdagrad and
FedYogi (Reddi et al. 2021).
--stale_weight {none,poly,hinge,const} with --stale_a --stale_b --stale_normalize discounts a stale
entry by its age before the average (the alternative to --throttle).  --delay_comp LAMBDA
compensates a stale entry for the distance the model has moved since it was computed (DC-ASGD).
--clip_grad_norm MAX_NORM clips the aggregated gradient's global 2-norm before the update
(torch.nn.utils.clip_grad_norm_) and logs the norm as 'Grad Norm' per epoch.
--robust_rule {none,median,trimmed_mean} with --trim N and --buckets B replaces the mean by the
coordinate-wise median or trimmed mean over B bucket means of the fast workers and the popped
delay-class entries (needs --semantics independent).  --robust_rule {krum,multi_krum} with
--byz_f F (and --krum_m M) picks the entry closest to its k - F - 2 nearest neighbours, or averages
the M such entries (Blanchard et al. 2017), and logs the chosen entries as 'Krum Selected'.
--robust_rule bulyan with --byz_f F repeats Krum's selection until k - 2F entries are chosen and
takes, per coordinate, the mean of the k - 4F values closest to their median (El Mhamdi et al.
2018; the epoch's entry count k >= 4F + 3), and logs the chosen entries as 'Bulyan Selected'.
--robust_rule geomed with --geomed_iters R, --geomed_nu NU and --geomed_weights {uniform,count}
takes the geometric median of the entries by R smoothed Weiszfeld iterations (RFA, Pillutla et
al. 2022; no Byzantine count needed) and logs the objective at every iterate as 'GeoMed Objective'.
--robust_rule cclip with --cclip_tau T (required), --cclip_iters L and --cclip_weights {uniform,count}
clips every entry to the radius T around the previous epoch's aggregate (centered clipping,
Karimireddy et al. 2021) and logs the center's final weight, the entries' and the number of
clipped entries as 'CClip Weights'.
--attack {none,ipm,alie} with --n_byz N, --attack_strength X and --byz_placement {spread,block} turns
N of the fast workers into simulated Byzantine workers (needs --robust_rule; trimmed_mean with
--trim 0 is the undefended mean over buckets): under ipm each sends -X * mu (inner-product
manipulation, Xie et al. 2020; default X = 1), under alie mu - X * sigma ("A Little Is Enough",
Baruch et al. 2019; default X = the paper's z for the epoch's worker counts), mu and sigma being the
coordinate-wise mean and standard deviation of the honest buckets' means.  --attack_strength is not
--byz_f, which stays the count Krum tolerates.  'Attack' per epoch logs (kind, strength, Byzantine
workers present).
--attack {minmax,minsum} with --attack_dir {unit,std,sign} are the optimised attacks of Shejwalkar and
Houmansadr 2021: each Byzantine worker sends mu + X * gamma * p, p = -mu, -sigma (default) or
-sign(mu), with gamma solved on the GPU in every epoch as the largest coefficient that keeps the
crafted vector no farther from any honest bucket than the honest buckets are from each other
(minmax: the largest squared distance; minsum: the largest sum of squared distances); X defaults to
1, the paper's attack.  'Attack' then logs (kind, direction, strength, Byzantine workers present).
--nnm F (needs --robust_rule) mixes the entries before the rule (nearest-neighbour mixing, Allouah
et al. 2023): after the attack, every entry is replaced by the mean of its k - F nearest entries,
itself included, and the rule reads the mixed entries with count 1 each -- so --geomed_weights
count and --cclip_weights count then see equal weights.  F is the number of Byzantine ENTRIES
assumed, like --byz_f, and 2F must stay below every epoch's entry count.
The training loop (main.py:126-188) runs as flsim.sim.FLSimulation: host schedule,
worker-batched HIP forward/backward, fused rule()+Adam; with
`torchrun --nproc-per-node N` the computing workers are sharded over N GPUs with one RCCL
all-reduce per epoch.  'Avg. Loss' per epoch (main.py:185) goes to --log (JSONL; tensorboard is
not installed) and stdout.

Test accuracy every 100 epochs and at the end (main.py:190,196-210) runs on the device
(FLSimulation.evaluate, dropout off) and is logged as 'Avg. Test Accuracy' and 'Class 9 Test
Accuracy'.  --save_model writes saved_model_{t}.pt state_dicts every 100 epochs (main.py:192-194,
reference default off).  --checkpoint / --resume save and continue the whole simulation state.

Differences forced by the environment: without --data_dir the data is a seeded
synthetic CIFAR-shaped pool (no network for CIFAR10; --data_dir reads a local copy of the
CIFAR-10 binary distribution); RNG streams are seeded (--seed) and dropout / sampling use the
counter-based spec.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import torch  # noqa: E402


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--n_workers', type=int, default=5, help='number of FL workers')
    p.add_argument('--n_epochs', type=int, default=1000, help='number of train epochs')
    p.add_argument('--batch_size', type=int, default=128, help='samples per worker-step')
    p.add_argument('--learning_rate', type=float, default=0.001, help='learning rate')
    p.add_argument('--delay', type=int, default=100, help='delay in between slow worker')
    p.add_argument('--model_file', type=str, help='path to model to load (pretrained)')
    p.add_argument('--throttle', action='store_true', help='gradient throttling')
    # build flags
    p.add_argument('--optimizer', default='adam',
                   choices=['adam', 'adamw', 'sgd', 'adagrad', 'yogi'],
                   help="the central optimizer (main.py:106 builds Adam): torch.optim.Adam "
                        "(--weight_decay: L2), AdamW (decoupled decay), SGD, Adagrad "
                        "(FedAdagrad) or Yogi (FedYogi, flsim.optim.Yogi)")
    p.add_argument('--momentum', type=float, default=0.0, help='SGD momentum')
    p.add_argument('--dampening', type=float, default=0.0, help='SGD dampening')
    p.add_argument('--nesterov', action='store_true', help='SGD Nesterov momentum')
    p.add_argument('--weight_decay', type=float, default=0.0, help='weight decay')
    p.add_argument('--lr_decay', type=float, default=0.0, help='Adagrad learning-rate decay')
    p.add_argument('--initial_accumulator_value', type=float, default=None,
                   help="start of Adagrad's sum / Yogi's exp_avg_sq (default: 0 / 1e-6)")
    p.add_argument('--eps', type=float, default=None,
                   help="the optimizer's eps (default: the kind's, 1e-8; adagrad 1e-10, yogi 1e-3)")
    p.add_argument('--beta1', type=float, default=None,
                   help="Adam family and Yogi: beta1 (default 0.9)")
    p.add_argument('--beta2', type=float, default=None,
                   help="Adam family and Yogi: beta2 (default 0.999; yogi 0.99)")
    p.add_argument('--stale_weight', default='none', choices=['none', 'poly', 'hinge', 'const'],
                   help='discount of a stale entry of age tau before the average: poly '
                        '(1+tau)^-a, hinge 1 if tau <= b else 1/(a(tau-b)+1), const a')
    p.add_argument('--stale_a', type=float, default=0.5, help='a of --stale_weight')
    p.add_argument('--stale_b', type=float, default=0.0, help='b of --stale_weight hinge')
    p.add_argument('--stale_normalize', default='weights', choices=['weights', 'count'],
                   help='divide the weighted sum by the sum of the weights or the entry count')
    p.add_argument('--delay_comp', type=float, default=None, metavar='LAMBDA',
                   help='delay compensation (DC-ASGD): a stale entry x becomes x + x*x*LAMBDA*'
                        '(theta_now - theta_then) before the average (default: off).  An entry '
                        'is the SUM of its epoch\'s worker gradients, so x*x grows with the '
                        'square of the worker count: choose LAMBDA with that in mind')
    p.add_argument('--clip_grad_norm', type=float, default=None, metavar='MAX_NORM',
                   help='clip the aggregated gradient to this global 2-norm before the update, '
                        'as torch.nn.utils.clip_grad_norm_ (default: off; inf only logs the norm)')
    p.add_argument('--robust_rule', default='none',
                   choices=['none', 'median', 'trimmed_mean', 'krum', 'multi_krum', 'bulyan',
                            'geomed', 'cclip'],
                   help='aggregate with the coordinate-wise median or trimmed mean, with Krum / '
                        'Multi-Krum, with Bulyan, with the geometric median (RFA) or with centered '
                        'clipping, '
                        'over bucket means instead of the mean (needs --semantics independent; '
                        'default: none)')
    p.add_argument('--cclip_tau', type=float, default=None, metavar='T',
                   help="--robust_rule cclip: the clipping radius, finite and > 0, on the scale of "
                        "the gradients' norm (required: no default)")
    p.add_argument('--cclip_iters', type=int, default=1, metavar='L',
                   help='--robust_rule cclip: clipping iterations an epoch, 1 .. 32 (default 1)')
    p.add_argument('--cclip_weights', default='uniform', choices=['uniform', 'count'],
                   help="--robust_rule cclip: weigh every entry alike, or by its workers' count "
                        '(default uniform)')
    p.add_argument('--geomed_iters', type=int, default=3, metavar='R',
                   help='--robust_rule geomed: smoothed Weiszfeld iterations, 0 .. 32 (default 3)')
    p.add_argument('--geomed_nu', type=float, default=1e-6, metavar='NU',
                   help='--robust_rule geomed: the floor of a distance in the weights 1 / '
                        'max(distance, NU), finite and > 0 (default 1e-6)')
    p.add_argument('--geomed_weights', default='uniform', choices=['uniform', 'count'],
                   help="--robust_rule geomed: weigh every entry alike, or by its workers' count "
                        '(default uniform)')
    p.add_argument('--byz_f', type=int, default=None, metavar='F',
                   help="--robust_rule krum / multi_krum / bulyan: the Byzantine entries tolerated, "
                        "the epoch's entry count >= 2F + 3 (bulyan: >= 4F + 3) (required: no "
                        "default)")
    p.add_argument('--krum_m', type=int, default=1, metavar='M',
                   help='--robust_rule multi_krum: entries averaged, 1 <= M <= the entry count - F '
                        '(default 1)')
    p.add_argument('--trim', type=int, default=1, metavar='N',
                   help='--robust_rule trimmed_mean: entries dropped at each end, 2N < the '
                        "epoch's entry count (default 1)")
    p.add_argument('--buckets', type=int, default=8, metavar='B',
                   help="--robust_rule: contiguous buckets the epoch's fast workers are averaged "
                        'in before the rule (default 8)')
    p.add_argument('--attack', default='none', choices=['none', 'ipm', 'alie', 'minmax', 'minsum'],
                   help='simulated Byzantine workers: inner-product manipulation (-X * mu), "A '
                        'Little Is Enough" (mu - X * sigma), or Min-Max / Min-Sum (mu + X * gamma '
                        '* p, gamma solved per epoch) mixed into the bucket entries (needs '
                        '--robust_rule and --n_byz; default: none)')
    p.add_argument('--attack_dir', default='std', choices=['unit', 'std', 'sign'],
                   help='--attack minmax / minsum: the perturbation direction p = -mu, -sigma or '
                        '-sign(mu) (default std)')
    p.add_argument('--n_byz', type=int, default=0, metavar='N',
                   help='--attack: how many of the fast (delay-0) workers are Byzantine, fewer '
                        'than all of them (default 0)')
    p.add_argument('--attack_strength', type=float, default=None, metavar='X',
                   help="--attack: ipm's eps (default 1), alie's z (default: the paper's z for "
                        "the epoch's fast-worker and Byzantine counts) or the factor on minmax's "
                        "/ minsum's gamma (default 1); not --byz_f")
    p.add_argument('--byz_placement', default='spread', choices=['spread', 'block'],
                   help='--attack: the Byzantine workers are spread evenly over the fast workers, '
                        'or are the first N of them, filling whole buckets (default spread)')
    p.add_argument('--nnm', type=int, default=None, metavar='F',
                   help='nearest-neighbour mixing before --robust_rule: every entry becomes the '
                        'mean of its (entry count - F) nearest entries, itself included; F is the '
                        "number of Byzantine entries assumed, like --byz_f, 2F < the epoch's "
                        'entry count (default: off)')
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--semantics', default='reference', choices=['reference', 'torch1', 'independent'],
                   help='stale entry = S_{t-d} (torch>=2 aliasing), zeros (torch 1.x) or the slow '
                        "worker's own gradient with distinct per-worker entries (independent)")
    p.add_argument('--no-dropout', action='store_true')
    p.add_argument('--chunk', type=int, default=128,
                   help='workers per worker-batched launch (max 128 = 16,384 samples)')
    p.add_argument('--model', default='PerformantNet1', choices=['PerformantNet1', 'vgg11', 'vgg11_bn'],
                   help='models.py network (main.py:97 builds PerformantNet1; vgg11 = configs[4]; '
                        'vgg11_bn = models.py:106-108)')
    p.add_argument('--log', type=str, default=None,
                   help="JSONL scalar log ('Avg. Loss', 'Avg. Test Accuracy', 'Class 9 ...')")
    p.add_argument('--data_dir', type=str, default=None,
                   help='local cifar-10-batches-bin directory (default: synthetic pool)')
    p.add_argument('--eval_every', type=int, default=100, help='main.py:196 (0 = only at end)')
    p.add_argument('--save_model', action='store_true', help='main.py:192-194 saved_model_{t}.pt')
    p.add_argument('--checkpoint', type=str, default=None, help='write a resumable checkpoint')
    p.add_argument('--checkpoint_every', type=int, default=0)
    p.add_argument('--resume', type=str, default=None, help='continue from a checkpoint')
    return p.parse_args(argv)


def stale_spec(args):
    """--stale_weight / --stale_a / --stale_b as FLSimulation's stale_weight spec."""
    if args.stale_weight == 'none':
        return None
    if args.stale_weight == 'hinge':
        return ('hinge', args.stale_a, args.stale_b)
    return (args.stale_weight, args.stale_a)


def robust_spec(args):
    """--robust_rule / --trim as FLSimulation's robust_rule spec."""
    if args.robust_rule == 'none':
        return None
    if args.robust_rule in ('krum', 'multi_krum'):
        if args.byz_f is None:
            raise SystemExit(f"--robust_rule {args.robust_rule} needs --byz_f F")
        return ('krum', args.byz_f) if args.robust_rule == 'krum' else \
            ('multi_krum', args.byz_f, args.krum_m)
    if args.robust_rule == 'bulyan':
        if args.byz_f is None:
            raise SystemExit("--robust_rule bulyan needs --byz_f F")
        return ('bulyan', args.byz_f)
    if args.robust_rule == 'geomed':
        return ('geomed', args.geomed_iters, args.geomed_nu, args.geomed_weights)
    if args.robust_rule == 'cclip':
        if args.cclip_tau is None:
            raise SystemExit("--robust_rule cclip needs --cclip_tau T")
        return ('cclip', args.cclip_tau, args.cclip_iters, args.cclip_weights)
    return 'median' if args.robust_rule == 'median' else ('trimmed_mean', args.trim)


def attack_spec(args):
    """--attack / --attack_strength as FLSimulation's attack spec."""
    if args.attack == 'none':
        return None
    if args.attack in ('minmax', 'minsum'):
        return (args.attack, args.attack_dir) if args.attack_strength is None else \
            (args.attack, args.attack_dir, args.attack_strength)
    return args.attack if args.attack_strength is None else (args.attack, args.attack_strength)


def nnm_spec(args):
    """--nnm as FLSimulation's nnm (None: off)."""
    if args.nnm is None:
        return None
    if args.nnm < 0:
        raise SystemExit(f"--nnm {args.nnm}: F must be >= 0")
    if args.robust_rule == 'none':
        raise SystemExit("--nnm needs --robust_rule: the bucketed entries are what it mixes")
    return args.nnm


def optim_kwargs(args):
    """--lr_decay / --initial_accumulator_value / --eps / --beta1 / --beta2 as FLSimulation's
    arguments; a flag left out resolves to the kind's default (flsim.engine.optim_defaults)."""
    from flsim.engine import optim_defaults
    d = optim_defaults(args.optimizer)
    betas = (d["betas"][0] if args.beta1 is None else args.beta1,
             d["betas"][1] if args.beta2 is None else args.beta2)
    return dict(lr_decay=args.lr_decay, initial_accumulator_value=args.initial_accumulator_value,
                eps=args.eps, betas=betas)


def main(argv=None):
    args = parse(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device: flsim has no CPU path")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        torch.distributed.init_process_group("nccl", device_id=dev)
    rank = torch.distributed.get_rank() if world > 1 else 0
    from flsim.sim import FLSimulation, default_theta, load_model_file
    theta0 = default_theta(args.seed, args.model)
    buffers = None
    if args.model_file is not None:                       # main.py:98-100
        theta0, buffers = load_model_file(args.model_file, args.model)
    if rank == 0:
        print(dev)
    pool = test_pool = None
    if args.data_dir:
        from flsim.data import load_cifar10_bin
        pool, test_pool = load_cifar10_bin(args.data_dir)
    sim = FLSimulation(args.n_workers, delay=args.delay, throttle=args.throttle,
                       lr=args.learning_rate, seed=args.seed, semantics=args.semantics,
                       dropout=not args.no_dropout, chunk_workers=args.chunk, device=dev,
                       theta0=theta0, pool=pool, test_pool=test_pool, model=args.model,
                       batch_size=args.batch_size, optimizer=args.optimizer,
                       weight_decay=args.weight_decay, momentum=args.momentum,
                       dampening=args.dampening, nesterov=args.nesterov,
                       stale_weight=stale_spec(args), stale_normalize=args.stale_normalize,
                       delay_comp=args.delay_comp, clip_grad_norm=args.clip_grad_norm,
                       robust_rule=robust_spec(args), buckets=args.buckets,
                       attack=attack_spec(args), n_byz=args.n_byz,
                       byz_placement=args.byz_placement, nnm=nnm_spec(args),
                       **optim_kwargs(args))
    if buffers:
        sim.engine.load_buffers(buffers)
    if args.resume:
        sim.restore(args.resume)
    log = open(args.log, "a" if args.resume else "w") if (args.log and rank == 0) else None
    t0 = time.time()

    def emit(tag, value, t):
        if rank != 0:
            return
        rec = {"tag": tag, "value": value, "step": t, "wall": time.time() - t0}
        if log:
            log.write(json.dumps(rec) + "\n")
            log.flush()

    t = len(sim.trace) - 1
    first = len(sim.trace)
    for t in range(len(sim.trace), args.n_epochs):
        loss = sim.epoch()
        emit("Avg. Loss", loss, t)                                     # main.py:185
        if args.clip_grad_norm is not None:
            emit("Grad Norm", sim.grad_norms()[-1], t)
        if args.robust_rule in ('krum', 'multi_krum'):
            emit("Krum Selected", sim.selections()[-1], t)
        if args.robust_rule == 'bulyan':
            emit("Bulyan Selected", sim.selections()[-1], t)
        if args.attack != 'none':
            rec = list(sim.attack_log()[-1])
            if args.attack in ('minmax', 'minsum'):
                rec.insert(1, args.attack_dir)
            emit("Attack", rec, t)
        if rank == 0 and (t % 10 == 0 or t == args.n_epochs - 1):
            print(f"epoch {t} Avg. Loss {loss:.5f}", flush=True)
        if args.save_model and t % 100 == 0 and t > 0 and rank == 0:   # main.py:192-194
            torch.save(sim.model_state_dict(), "saved_model_{}.pt".format(t))
        if args.eval_every and t % args.eval_every == 0 and t > 0:     # main.py:196-203
            acc, per = sim.evaluate()
            emit("Avg. Test Accuracy", acc, t)
            emit("Class 9 Test Accuracy", per[-1], t)
            if rank == 0:
                print(f"Accuracy of the network on the {len(sim._test.labels)} test images: "
                      f"{int(acc)} %", flush=True)
        if args.checkpoint and args.checkpoint_every and (t + 1) % args.checkpoint_every == 0 \
                and rank == 0:
            sim.save_checkpoint(args.checkpoint)
    # (read back once, here: the epochs themselves never wait for the device)
    for i, (obj, _) in enumerate(sim.geomed_log()):
        emit("GeoMed Objective", obj, first + i)
    for i, (u, w, n_clipped) in enumerate(sim.cclip_log()):
        emit("CClip Weights", [u] + w + [n_clipped], first + i)
    acc, per = sim.evaluate()                                           # main.py:205-210
    emit("Avg. Test Accuracy", acc, t)
    emit("Class 9 Test Accuracy", per[-1], t)
    if rank == 0:
        print(f"Accuracy of the network on the {len(sim._test.labels)} test images: {int(acc)} %")
    if args.checkpoint and rank == 0:
        sim.save_checkpoint(args.checkpoint)
    if log:
        log.close()
    if rank == 0:
        print('Done training')
    if world > 1:
        torch.distributed.destroy_process_group()
    return sim


if __name__ == '__main__':
    main()
