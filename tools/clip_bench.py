"""Micro-benchmark of the clipped server step (rule -> G + partial squares, finish, apply) against
the unclipped stream of the same rule, on PerformantNet1's parameter vector (GPU box), timed by the
library's live probe (flsim_probe_*: events around each launch), beside tools/cstep_bench.py.

  python tools/clip_bench.py [reps]

Launches (Adam):
  stream      tick k=513      one stale array
  stream      general k=8100  72 stale entries among 6 arrays
  epoch end   tick k=513      world 1: the fused slab step (one launch) against the slab reduction
                              + the clipped stream (reduce + three launches)
Prints per form the mean and minimum us over `reps` launches (the clipped form: the sum of its
launches, and each launch's minimum), the algorithmic HBM bytes and the GB/s they make at the
minimum; then per pair the extra time, the extra bytes (8P: G written once and read once) and the
time those bytes would take at the rate the unclipped launch reaches.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "fl-distributed-delay_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    from flsim._lib import KernelProbe
    from flsim.data import DevicePool
    from flsim.engine import Clip, PN1Engine, ProgramStager, Rule, worker_table
    from oracle import oracle as O
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    dev = "cuda:0"
    eng = PN1Engine(dev, chunk_workers=2)
    P = eng.P
    g = torch.Generator(device="cpu").manual_seed(0)
    theta = (torch.randn(P + 64, generator=g) * 0.05).to(dev)
    m = torch.zeros_like(theta)
    v = torch.zeros_like(theta)
    S = (torch.randn(P + 64, generator=g) * 1e-3).to(dev)
    arrs = [(torch.randn(P + 64, generator=g) * 1e-3).to(dev) for _ in range(6)]
    eng.begin_epoch(theta)
    # one 2-worker chunk, so the slabs hold an epoch's rows (tests/test_gpu_optim.py's chunk)
    items = [(0, 0, 1), (0, 3, 7)]
    eng.run_chunk(theta, DevicePool(dev, 0, O.make_pool(0)), worker_table(items, dev), 2, 8, 0,
                  True, torch.zeros(2, device=dev))
    rs = np.random.RandomState(0)
    pos = np.sort(rs.choice(8100, 72, replace=False))
    ev = list(zip(pos.tolist(), rs.randint(0, 6, 72).tolist()))
    stager = ProgramStager(dev)
    clip = Clip(1.0)
    S2 = torch.empty_like(S)

    def tick():
        return Rule(513, arrs[:1], c=512)

    def general():
        return Rule(8100, arrs, events=ev, stager=stager)
    probe = KernelProbe()

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        probe.read()
        per, each = [], {}
        for _ in range(reps):
            fn()
            torch.cuda.synchronize()
            rec = probe.read()
            per.append(sum(ms for (_, ms, _) in rec.values()) * 1e3)
            for k, (_, ms, _) in rec.items():
                each[k] = min(each.get(k, 1e30), ms * 1e3)
        # the probe's third figure is the launch's algorithmic HBM bytes
        nbytes = sum(b for (_, _, b) in rec.values())
        return float(np.mean(per)), float(np.min(per)), nbytes, each

    def stream(r, c):
        eng.aggregate_rule(S, r, theta, m, v, 5, clip=clip if c else None)

    def epoch_end(r, c):
        if c:
            eng.end_epoch(S2)
            eng.aggregate_rule(S2, r, theta, m, v, 5, clip=clip)
        else:
            eng.server_step(None, r, theta, m, v, 5)
    cases = [("stream    tick k=513", tick, stream),
             ("stream    general k=8100", general, stream),
             ("epoch end tick k=513", tick, epoch_end)]
    for name, make, launch in cases:
        res = {}
        for c in (False, True, False, True):            # A B A B
            rule = make()
            mean, best, nbytes, each = timed(lambda: launch(rule, c))
            form = "clipped" if c else "unclipped"
            parts = " ".join(f"{k}={t:.1f}" for k, t in sorted(each.items()))
            print(f"{name:26s} {form:9s} mean {mean:8.1f} us  min {best:8.1f} us  "
                  f"{nbytes / 1e6:8.2f} MB  {nbytes / best / 1e3:7.1f} GB/s  [{parts}]",
                  flush=True)
            res[c] = min(best, res.get(c, (1e30,))[0]), nbytes
        (tu, bu), (tc, bc) = res[False], res[True]
        print(f"{name:26s} extra {tc - tu:6.1f} us for {(bc - bu) / 1e6:.2f} MB "
              f"(8P = {8.0 * P / 1e6:.2f} MB); at the unclipped launch's {bu / tu / 1e3:.1f} GB/s "
              f"those bytes take {(bc - bu) / (bu / tu):6.1f} us", flush=True)
    probe.close()


if __name__ == "__main__":
    main()
