"""Micro-benchmark of the fused robust step (k_robust: median / trimmed mean over k bucket sums +
the update) on PerformantNet1's parameter vector (GPU box), timed by the library's live probe
(flsim_probe_*: events around each launch), beside tools/clip_bench.py.

  python tools/robust_bench.py [reps] [k,k,...]

Per k (default 8, 16 and 64) and kind (median, trimmed mean with trim = k // 4), Adam: the mean and minimum
us over `reps` launches, the algorithmic HBM bytes ((k + 6) * 4P: every entry read once, p / m / v
read and written) and the TB/s they make at the minimum.  The yardstick is measured in the same
job: the existing tick stream (rule k = 513 with one stale array, Adam).
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "fl-distributed-delay_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    from flsim._lib import KernelProbe, lib
    from flsim.engine import Robust, Rule, aggregate_rule, robust_step
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    dev = "cuda:0"
    P = int(lib().flsim_pn1_param_count())
    g = torch.Generator(device="cpu").manual_seed(0)
    theta = (torch.randn(P + 64, generator=g) * 0.05).to(dev)
    m = torch.zeros_like(theta)
    v = torch.zeros_like(theta)
    S = (torch.randn(P + 64, generator=g) * 1e-3).to(dev)
    ents = [(torch.randn(P + 64, generator=g) * 1e-3).to(dev) for _ in range(64)]
    sizes = [P]
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
        nbytes = sum(b for (_, _, b) in rec.values())
        return float(np.mean(per)), float(np.min(per)), nbytes

    def report(name, fn):
        best = (1e30, 0.0, 0.0)
        for _ in range(2):                               # two passes, the better minimum
            mean, mn, nbytes = timed(fn)
            if mn < best[0]:
                best = (mn, mean, nbytes)
        mn, mean, nbytes = best
        print(f"{name:34s} mean {mean:8.1f} us  min {mn:8.1f} us  {nbytes / 1e6:8.2f} MB  "
              f"{nbytes / mn / 1e6:6.2f} TB/s", flush=True)

    tick = Rule(513, ents[:1], c=512)
    report("stream tick k=513 (yardstick)",
           lambda: aggregate_rule(S[:P], tick, theta[:P], m[:P], v[:P], 5, sizes))
    ks = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [8, 16, 64]
    for k in ks:
        for kind, trim in (("median", 0), ("trimmed_mean", k // 4)):
            r = Robust(kind, trim, [e[:P] for e in ents[:k]], [128] * k)
            report(f"robust {kind:12s} k={k:2d} trim={trim:2d}",
                   lambda: robust_step(r, theta[:P], m[:P], v[:P], 5))
    report("stream tick k=513 (yardstick)",
           lambda: aggregate_rule(S[:P], tick, theta[:P], m[:P], v[:P], 5, sizes))
    probe.close()


if __name__ == "__main__":
    main()
