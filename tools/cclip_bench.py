"""Micro-benchmark of the fused centered-clipping step (k_cclip_dist, k_cclip_finish,
k_cclip_apply) on PerformantNet1's parameter vector (GPU box), timed per kernel by the library's
live probe (flsim_probe_*: events around each launch), beside tools/geomed_bench.py.

  python tools/cclip_bench.py [reps] [k,k,...]

Per k (default 9), uniform weights, Adam, a carried and a fresh center: the minimum us of the
launches of a step over `reps` steps.  The probe adds a kernel's launches up, so the pair-0 and
the later distance launches are separated by steps with iters = 1 (pair 0 alone) and 3:
  dist0 = T(1), later = (T(3) - T(1)) / 2                             (the same for the finish).
Beside them the geometric median's launches at the same k (tools/geomed_bench.py's separation).
Information, not a bar: the acceptance of the rule does not depend on these figures.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "fl-distributed-delay_amd")]
import torch  # noqa: E402


def main():
    from flsim._lib import KernelProbe, lib
    from flsim.engine import CClip, GeoMed, cclip_step, geomed_step
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    ks = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [9]
    dev = "cuda:0"
    P = int(lib().flsim_pn1_param_count())
    g = torch.Generator(device="cpu").manual_seed(0)
    theta = (torch.randn(P + 64, generator=g) * 0.05).to(dev)
    m = torch.zeros_like(theta)
    v = torch.zeros_like(theta)
    ents = [(torch.randn(P + 64, generator=g) * 1e-3).to(dev) for _ in range(max(ks))]
    center = torch.zeros(P + 64, device=dev)
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

    for k in ks:
        e = [x[:P] for x in ents[:k]]
        # the entries' means have norm about 1e-3 * sqrt(P) / 128; half of that clips every entry
        tau = 0.5 * 1e-3 * P ** 0.5 / 128
        for fresh in (False, True):
            T = {}
            for iters in (1, 3):
                cc = CClip(tau, iters, False, e, [128] * k, center[:P], fresh=fresh)
                T[iters] = timed(lambda: cclip_step(cc, theta[:P], m[:P], v[:P], 5))
            d = {i: T[i]["cclip_dist"][0] for i in T}
            f = {i: T[i]["cclip_finish"][0] for i in T}
            ap = T[3]["cclip_apply"]
            nb = 4.0 * P * (k + (0 if fresh else 1))
            d0, dl = d[1], (d[3] - d[1]) / 2
            f0, fl = f[1], (f[3] - f[1]) / 2
            print(f"cclip k={k:2d} {'fresh  ' if fresh else 'carried'} dist pair0 {d0:7.1f} us "
                  f"({nb / d0 / 1e6:5.2f} TB/s)  later {dl:7.1f} us ({nb / dl / 1e6:5.2f} TB/s)  "
                  f"finish pair0 {f0:5.1f} later {fl:5.1f} us  apply {ap[0]:7.1f} us "
                  f"({ap[1] / ap[0] / 1e6:5.2f} TB/s)  step iters=3 {d[3] + f[3] + ap[0]:8.1f} us",
                  flush=True)
        T = {}
        for iters in (0, 1, 3):
            gm = GeoMed(iters, 1e-6, False, e, [128] * k)
            T[iters] = timed(lambda: geomed_step(gm, theta[:P], m[:P], v[:P], 5))
        d = {i: T[i]["geomed_dist"][0] for i in T}
        f = {i: T[i]["geomed_finish"][0] for i in T}
        ap = T[3]["geomed_apply"]
        nb = 4.0 * P * k
        d0, dl = d[0], (d[3] - d[1]) / 2
        print(f"geomed k={k:2d}         dist pair0 {d0:7.1f} us ({nb / d0 / 1e6:5.2f} TB/s)  "
              f"later {dl:7.1f} us ({nb / dl / 1e6:5.2f} TB/s)  finish pair0 {f[0]:5.1f} later "
              f"{(f[3] - f[1]) / 2:5.1f} us  apply {ap[0]:7.1f} us ({ap[1] / ap[0] / 1e6:5.2f} TB/s)  "
              f"step iters=3 {d[3] + f[3] + ap[0]:8.1f} us", flush=True)
    probe.close()


if __name__ == "__main__":
    main()
