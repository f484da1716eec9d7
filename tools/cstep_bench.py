"""Micro-benchmark of the delay-compensated server step against the weighted one over the same
arrays, on PerformantNet1's parameter vector (GPU box), timed by the library's live probe
(flsim_probe_*: events around each launch), beside tools/wstep_bench.py.

  python tools/cstep_bench.py [reps]

Launches (Adam; every one both weighted and compensated):
  stream      tick k=513      one stale array [+ its snapshot]
  stream      general k=8100  72 stale entries among 6 arrays [+ 6 snapshots]
  fused step  tick k=513      one pop and one push: S_out written [+ the popped array's snapshot
                              read and theta_out written]
  fused step  general k=8100  as the stream's rule, no push
Prints per launch the mean and minimum us over `reps` launches, the algorithmic HBM bytes and the
GB/s they make at the minimum; then per pair the extra time, the extra bytes (4P read per distinct
compensated array, 4P written at a push) and the time those bytes would take at the rate the
weighted launch reaches.
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
    from flsim.engine import PN1Engine, ProgramStager, Rule, worker_table
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
    snaps = [theta + (torch.randn(P + 64, generator=g) * 1e-3).to(dev) for _ in range(6)]
    s_out = torch.empty_like(theta)
    t_out = torch.empty_like(theta)
    eng.begin_epoch(theta)
    # one 2-worker chunk, so the slabs hold an epoch's rows (tests/test_gpu_optim.py's chunk)
    items = [(0, 0, 1), (0, 3, 7)]
    eng.run_chunk(theta, DevicePool(dev, 0, O.make_pool(0)), worker_table(items, dev), 2, 8, 0,
                  True, torch.zeros(2, device=dev))
    rs = np.random.RandomState(0)
    pos = np.sort(rs.choice(8100, 72, replace=False))
    ev = list(zip(pos.tolist(), rs.randint(0, 6, 72).tolist()))
    stager = ProgramStager(dev)
    w6 = [(1.0 + t) ** -0.5 for t in (2, 3, 5, 8, 13, 50)]
    lam = 0.04

    def tick(comp):
        kw = dict(snapshots=snaps[:1], delay_comp=lam) if comp else {}
        return Rule(513, arrs[:1], c=512, weights=w6[:1], **kw)

    def general(comp):
        kw = dict(snapshots=snaps, delay_comp=lam) if comp else {}
        return Rule(8100, arrs, events=ev, stager=stager, weights=w6, **kw)
    probe = KernelProbe()

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        probe.read()
        per = []
        for _ in range(reps):
            fn()
            torch.cuda.synchronize()
            rec = probe.read()
            per.append(sum(ms for (_, ms, _) in rec.values()) * 1e3)
        # the probe's third figure is the launch's algorithmic HBM bytes
        nbytes = sum(b for (_, _, b) in rec.values())
        return float(np.mean(per)), float(np.min(per)), nbytes, "+".join(sorted(rec))

    # (name, make, launch(rule, comp), extra 4P arrays of the compensated form)
    cases = [
        ("stream     tick k=513", tick,
         lambda r, c: eng.aggregate_rule(S, r, theta, m, v, 5), 1),
        ("stream     general k=8100", general,
         lambda r, c: eng.aggregate_rule(S, r, theta, m, v, 5), 6),
        ("fused step tick k=513 push", tick,
         lambda r, c: eng.server_step(s_out, r, theta, m, v, 5, optim=dict(kind="adam"),
                                      **(dict(theta_out=t_out) if c else {})), 2),
        ("fused step general k=8100", general,
         lambda r, c: eng.server_step(None, r, theta, m, v, 5), 6),
    ]
    for name, make, launch, extra in cases:
        res = {}
        for comp in (False, True, False, True):         # A B A B
            rule = make(comp)
            mean, best, nbytes, kern = timed(lambda: launch(rule, comp))
            form = "compensated" if comp else "weighted"
            print(f"{name:27s} {form:11s} mean {mean:8.1f} us  min {best:8.1f} us  "
                  f"{nbytes / 1e6:8.2f} MB  {nbytes / best / 1e3:7.1f} GB/s  [{kern}]", flush=True)
            res[comp] = min(best, res.get(comp, (1e30,))[0]), nbytes
        (tw, bw), (tc, bc) = res[False], res[True]
        assert abs((bc - bw) - 4.0 * P * extra) < 1.0, (bc, bw, extra)
        print(f"{name:27s} extra {tc - tw:6.1f} us for {(bc - bw) / 1e6:.2f} MB "
              f"({extra} x 4P); at the weighted launch's {bw / tw / 1e3:.1f} GB/s those bytes "
              f"take {(bc - bw) / (bw / tw):6.1f} us", flush=True)
    probe.close()


if __name__ == "__main__":
    main()
