"""Micro-benchmark of the fused Krum / Multi-Krum step (k_krum_dist, k_krum_finish, k_krum_apply)
on PerformantNet1's parameter vector (GPU box), timed per kernel by the library's live probe
(flsim_probe_*: events around each launch), beside tools/robust_bench.py.

  python tools/krum_bench.py [reps] [k,k,...]

Per k (default 4, 9, 16, 32, 64), with Krum (f = 1, or 0 at k = 4; m = 1) and Multi-Krum with
m = k - f, Adam: the minimum us of each of the three kernels over `reps` launches, the HBM floor of
the distance launch (k * P * 4 bytes at the tick stream's rate measured in the same job) and the
fp64 lane-operations it issues (k (k - 1) / 2 pairs x 2 per element).  Yardsticks from the same job:
the existing tick stream (rule k = 513 with one stale array, Adam) and k_robust (median) at each k.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "fl-distributed-delay_amd")]
import torch  # noqa: E402


def main():
    from flsim._lib import KernelProbe, lib
    from flsim.engine import Krum, Robust, Rule, aggregate_rule, krum_step, robust_step
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    ks = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [4, 9, 16, 32, 64]
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
    for k in ks:
        f = 1 if k >= 5 else 0
        r = Robust("median", 0, [e[:P] for e in ents[:k]], [128] * k)
        us, nbytes = total(timed(lambda: robust_step(r, theta[:P], m[:P], v[:P], 5)))
        print(f"k_robust median k={k:2d}               min {us:8.1f} us  {nbytes / 1e6:8.2f} MB  "
              f"{nbytes / us / 1e6:6.2f} TB/s", flush=True)
        for mm in (1, k - f):
            kr = Krum(f, mm, [e[:P] for e in ents[:k]], [128] * k)
            best = timed(lambda: krum_step(kr, theta[:P], m[:P], v[:P], 5))
            d, fin, ap = best["krum_dist"], best["krum_finish"], best["krum_apply"]
            floor = d[1] / rate / 1e6
            ops = k * (k - 1) * P                       # pairs x 2 fp64 lane-ops per element
            print(f"krum k={k:2d} f={f} m={mm:2d}  dist {d[0]:8.1f} us (HBM floor {floor:6.1f} us, "
                  f"{d[1] / d[0] / 1e6:5.2f} TB/s, {ops / d[0] / 1e6:6.2f} T fp64 lane-ops/s)  "
                  f"finish {fin[0]:7.1f} us  apply {ap[0]:7.1f} us ({ap[1] / ap[0] / 1e6:5.2f} TB/s)"
                  f"  sum {d[0] + fin[0] + ap[0]:8.1f} us", flush=True)
    tick_rate()
    probe.close()


if __name__ == "__main__":
    main()
