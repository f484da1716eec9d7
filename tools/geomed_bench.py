"""Micro-benchmark of the fused geometric-median step (k_geomed_dist, k_geomed_finish,
k_geomed_apply) on PerformantNet1's parameter vector (GPU box), timed per kernel by the library's
live probe (flsim_probe_*: events around each launch), beside tools/krum_bench.py.

  python tools/geomed_bench.py [reps] [k,k,...]

Per k (default 4, 9, 16, 32, 64), uniform weights, Adam: the minimum us of the launches of a step
over `reps` steps.  A step with iters = 3 and no dead entry runs the pair-0 distance launch, two
later distance launches and one no-op pair; the probe adds a kernel's launches up, so the three are
separated by steps with iters = 0 (pair 0 alone), 1 (pair 0 + the no-op pair) and 3:
  dist0 = T(0), noop = T(1) - T(0), later = (T(3) - T(1)) / 2         (the same for the finish).
Each distance launch against its HBM floor (k * P * 4 bytes at the tick stream's rate measured in
the same job) and against k_robust (median) at the same k, which reads the same bytes.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "fl-distributed-delay_amd")]
import torch  # noqa: E402


def main():
    from flsim._lib import KernelProbe, lib
    from flsim.engine import GeoMed, Robust, Rule, aggregate_rule, geomed_step, robust_step
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
        """name -> (minimum us of the kernel's launches in one call, work) over `reps` calls."""
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
        r = Robust("median", 0, [e[:P] for e in ents[:k]], [128] * k)
        rus, nbytes = total(timed(lambda: robust_step(r, theta[:P], m[:P], v[:P], 5)))
        print(f"k_robust median k={k:2d}               min {rus:8.1f} us  {nbytes / 1e6:8.2f} MB  "
              f"{nbytes / rus / 1e6:6.2f} TB/s", flush=True)
        T = {}
        for iters in (0, 1, 3):
            gm = GeoMed(iters, 1e-6, False, [e[:P] for e in ents[:k]], [128] * k)
            T[iters] = timed(lambda: geomed_step(gm, theta[:P], m[:P], v[:P], 5))
        d = {i: T[i]["geomed_dist"][0] for i in T}
        f = {i: T[i]["geomed_finish"][0] for i in T}
        ap = T[3]["geomed_apply"]
        nb = 4.0 * P * k
        floor = nb / rate / 1e6
        d0, dn, dl = d[0], d[1] - d[0], (d[3] - d[1]) / 2
        f0, fn_, fl = f[0], f[1] - f[0], (f[3] - f[1]) / 2
        step = d[3] + f[3] + ap[0]
        print(f"geomed k={k:2d} iters=3  dist pair0 {d0:7.1f} us ({nb / d0 / 1e6:5.2f} TB/s, "
              f"{d0 / floor:4.2f} x floor {floor:6.1f} us, {d0 / rus:4.2f} x k_robust)  "
              f"later {dl:7.1f} us ({nb / dl / 1e6:5.2f} TB/s, {dl / floor:4.2f} x floor, "
              f"{dl / rus:4.2f} x k_robust)  no-op {dn:5.1f} us  finish pair0 {f0:5.1f} later "
              f"{fl:5.1f} no-op {fn_:4.1f} us  apply {ap[0]:7.1f} us "
              f"({ap[1] / ap[0] / 1e6:5.2f} TB/s)  step {step:8.1f} us", flush=True)
    tick_rate()
    probe.close()


if __name__ == "__main__":
    main()
