"""Micro-benchmark of the fused server step (k_slab_step) at a tick per update kind, on
PerformantNet1's gradstate after one real 128-worker chunk: k = 513 with one stale array, the FIFO
slot written in the same pass.

  python tools/optstep_bench.py TAG adam,sgdm,adagrad,yogi
  FLSIM_LIB=<another tree's libflsim.so> python tools/optstep_bench.py parent adam,sgdm

Per kind and repeat, one JSON line: device events around 40 launches (us_events) and the library's
probe over 10 more (us_probe, the algorithmic bytes of the launch, frac_probe = bytes / time over
the 8 TB/s HBM peak).  The kinds alternate within each of three repeats.  FLSIM_LIB points the
binding at another build of the library (a parent tree's), so two trees can be alternated in one
job; an older library takes the kinds it knows (adam, sgdm).
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "fl-distributed-delay_amd")]
import torch  # noqa: E402

from flsim._lib import KernelProbe  # noqa: E402
from flsim.data import DevicePool  # noqa: E402
from flsim.engine import PN1Engine, Rule, worker_table  # noqa: E402
from oracle import oracle as O  # noqa: E402

OPT = {
    "adam": (dict(kind="adam", lr=1e-3), 2),
    "sgdm": (dict(kind="sgd", lr=0.01, momentum=0.9), 1),
    "adagrad": (dict(kind="adagrad", lr=0.01, eps=1e-10), 1),
    "yogi": (dict(kind="yogi", lr=0.01, betas=(0.9, 0.99), eps=1e-3), 2),
}


def main():
    tag, names = sys.argv[1], sys.argv[2].split(",")
    reps, iters = 3, 40
    dev = "cuda:0"
    nw = 128
    eng = PN1Engine(dev, chunk_workers=nw)
    P = eng.P
    theta0 = torch.randn(P + 64, device=dev) * 0.05
    eng.begin_epoch(theta0)
    items = [(0, i, i % 7) for i in range(nw)]
    loss = torch.zeros(nw, device=dev)
    eng.run_chunk(theta0, DevicePool(dev, 0, O.make_pool(0)), worker_table(items, dev), nw, nw, 0,
                  True, loss)
    torch.cuda.synchronize()
    stale = torch.randn(P + 64, device=dev) * 1e-3
    slot = torch.empty(P + 64, device=dev)
    rule = Rule(513, [stale], c=512)
    for rep in range(reps):
        for name in names:
            o, nstate = OPT[name]
            th = theta0.clone()
            m = torch.full((P + 64,), 1e-6, device=dev) if nstate >= 1 else None
            v = torch.full((P + 64,), 1e-6, device=dev) if nstate >= 2 else None
            for _ in range(5):
                eng.server_step(slot, rule, th, m, v, 2, optim=o)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                eng.server_step(slot, rule, th, m, v, 2, optim=o)
            b.record()
            torch.cuda.synchronize()
            us = a.elapsed_time(b) / iters * 1e3
            pr = KernelProbe()
            for _ in range(10):
                eng.server_step(slot, rule, th, m, v, 2, optim=o)
            torch.cuda.synchronize()
            rd = pr.read()
            pr.close()
            if not rd:
                raise RuntimeError("the probe recorded no launch")
            kname, (cnt, ms, byts) = max(rd.items(), key=lambda kv: kv[1][1])
            print(json.dumps(dict(tree=tag, kind=name, rep=rep, us_events=round(us, 2),
                                  kernel=kname, us_probe=round(ms / cnt * 1e3, 2),
                                  bytes=byts / cnt,
                                  frac_probe=round(byts / cnt / (ms / cnt * 1e-3) / 8e12, 4))),
                  flush=True)


if __name__ == "__main__":
    main()
