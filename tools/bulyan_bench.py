"""Micro-benchmark of the fused Bulyan step (k_krum_dist, k_bulyan_finish, k_bulyan_apply) on
PerformantNet1's parameter vector (GPU box), timed per kernel by the library's live probe
(flsim_probe_*: events around each launch), beside tools/krum_bench.py.

  python tools/bulyan_bench.py [reps] [k:f,k:f,...]

Per (k, f) (default 9:1, 16:3, 33:7, 64:15, 64:0), Adam: the minimum us of each of the three kernels
over `reps` launches; the apply launch's algorithmic bytes (theta * P * 4 read, plus p, m, v read and
written) as a rate and as a fraction of the tick stream's rate measured in the same job.  Yardsticks
from the same job: the existing tick stream (rule k = 513 with one stale array, Adam), Krum at the
same k (f = 1, m = 1: the shared distance launch and Krum's finish) and k_robust (median) over
theta entries, the same sorting network as the apply launch.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "fl-distributed-delay_amd")]
import torch  # noqa: E402


def main():
    from flsim._lib import KernelProbe, lib
    from flsim.engine import (Bulyan, Krum, Robust, Rule, aggregate_rule, bulyan_step, krum_step,
                              robust_step)
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    cases = [tuple(int(x) for x in c.split(":")) for c in sys.argv[2].split(",")] \
        if len(sys.argv) > 2 else [(9, 1), (16, 3), (33, 7), (64, 15), (64, 0)]
    dev = "cuda:0"
    P = int(lib().flsim_pn1_param_count())
    g = torch.Generator(device="cpu").manual_seed(0)
    theta = (torch.randn(P + 64, generator=g) * 0.05).to(dev)
    m = torch.zeros_like(theta)
    v = torch.zeros_like(theta)
    S = (torch.randn(P + 64, generator=g) * 1e-3).to(dev)
    ents = [(torch.randn(P + 64, generator=g) * 1e-3).to(dev) for _ in range(64)]
    probe = KernelProbe()

    def timed(fn):
        """name -> (minimum us, work) per kernel over `reps` launches (two warm-up calls)."""
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        probe.read()
        best = {}
        for _ in range(reps):
            fn()
            torch.cuda.synchronize()
            for name, (_, ms, work) in probe.read().items():
                us = ms * 1e3
                if name not in best or us < best[name][0]:
                    best[name] = (us, work)
        return best

    def total(best):
        return sum(u for u, _ in best.values()), sum(w for _, w in best.values())

    tick = Rule(513, ents[:1], c=512)

    def tick_rate():
        us, nbytes = total(timed(lambda: aggregate_rule(S[:P], tick, theta[:P], m[:P], v[:P], 5,
                                                        [P])))
        print(f"stream tick k=513 (yardstick)      min {us:8.1f} us  {nbytes / 1e6:8.2f} MB  "
              f"{nbytes / us / 1e6:6.2f} TB/s", flush=True)
        return nbytes / us / 1e6

    rate = tick_rate()
    for k, f in cases:
        th = k - 2 * f
        r = Robust("median", 0, [e[:P] for e in ents[:th]], [128] * th)
        us, nbytes = total(timed(lambda: robust_step(r, theta[:P], m[:P], v[:P], 5)))
        print(f"k_robust median k={th:2d}               min {us:8.1f} us  {nbytes / 1e6:8.2f} MB  "
              f"{nbytes / us / 1e6:6.2f} TB/s", flush=True)
        kr = Krum(1, 1, [e[:P] for e in ents[:k]], [128] * k)
        best = timed(lambda: krum_step(kr, theta[:P], m[:P], v[:P], 5))
        print(f"krum   k={k:2d} f=1 m=1   dist {best['krum_dist'][0]:8.1f} us  "
              f"finish {best['krum_finish'][0]:7.1f} us  apply {best['krum_apply'][0]:7.1f} us",
              flush=True)
        bu = Bulyan(f, [e[:P] for e in ents[:k]], [128] * k)
        best = timed(lambda: bulyan_step(bu, theta[:P], m[:P], v[:P], 5))
        d, fin, ap = best["bulyan_dist"], best["bulyan_finish"], best["bulyan_apply"]
        tbs = ap[1] / ap[0] / 1e6
        print(f"bulyan k={k:2d} f={f:2d} theta={th:2d} beta={th - 2 * f:2d}  dist {d[0]:8.1f} us "
              f"({d[1] / d[0] / 1e6:5.2f} TB/s)  finish {fin[0]:7.1f} us  apply {ap[0]:7.1f} us "
              f"({ap[1] / 1e6:7.2f} MB, {tbs:5.2f} TB/s, {tbs / rate:4.2f} of the tick stream)  "
              f"sum {d[0] + fin[0] + ap[0]:8.1f} us", flush=True)
    tick_rate()
    probe.close()


if __name__ == "__main__":
    main()
