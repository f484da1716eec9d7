"""Micro-benchmark of the optimised attacks' launches (flsim_attack_opt_entries: k_attack_opt_stats,
k_krum_dist + k_attack_opt_finish, k_attack's mix) on PerformantNet1's parameter vector (GPU box),
beside tools/attack_bench.py.

  python tools/attack_opt_bench.py [reps] [k,k,...]
  python tools/attack_opt_bench.py epoch ATTACK [epochs]      (the whole robust epoch, see epoch_time)

The four launches share the probe id of flsim_attack_entries (the probe's list of names is pinned
by an earlier test), so the library's probe gives their summed kernel time (the minimum over
`reps` calls); the time of each kernel comes from a `rocprofv3 --kernel-trace --stats` run of this
script (tools/gpu_job.sh's trace step shows the command line).  In the same process and at the
same k:
  k_geomed_dist pair 0   (a geometric-median step with iters = 0): reads the same k P floats once;
  k_attack ALIE          the "spread" placement (7 honest + 1 Byzantine per entry), with b_out:
                         what the mix launch is measured against.
The strength is small, so that the entries stay finite over the repeats (the mix updates them in
place).
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "fl-distributed-delay_amd")]
import torch  # noqa: E402


def main():
    from flsim._lib import KernelProbe, lib
    from flsim.engine import (Attack, GeoMed, OptAttack, attack_entries, geomed_step,
                              opt_attack_entries)
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    ks = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [4, 8, 16, 32, 64]
    dev = "cuda:0"
    P = int(lib().flsim_pn1_param_count())
    g = torch.Generator(device="cpu").manual_seed(0)
    theta = (torch.randn(P + 64, generator=g) * 0.05).to(dev)
    m = torch.zeros_like(theta)
    v = torch.zeros_like(theta)
    ents = [(torch.randn(P + 64, generator=g) * 1e-3).to(dev) for _ in range(64)]
    b_out = torch.empty(P + 64, device=dev)
    probe = KernelProbe()

    def probed(fn, name):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        probe.read()
        best = None
        for _ in range(reps):
            fn()
            torch.cuda.synchronize()
            ms = probe.read()[name][1]
            best = ms * 1e3 if best is None or ms * 1e3 < best else best
        return best

    for k in ks:
        gm = GeoMed(0, 1e-6, False, [e[:P] for e in ents[:k]], [8] * k)
        gus = probed(lambda: geomed_step(gm, theta[:P], m[:P], v[:P], 5), "geomed_dist")
        honest, byz = [7] * k, [1] * k
        al = Attack("alie", 0.01, [e[:P] for e in ents[:k]], honest, byz)
        aus = probed(lambda: attack_entries(al, b_out[:P], P), "attack_entries")
        print(f"k={k:2d} k_geomed_dist pair 0 min {gus:8.1f} us   k_attack alie spread min "
              f"{aus:8.1f} us", flush=True)
        for kind in ("minmax", "minsum"):
            for dirn in ("unit", "std", "sign"):
                at = OptAttack(kind, dirn, 0.01, [e[:P] for e in ents[:k]], honest, byz)
                us = probed(lambda: opt_attack_entries(at, b_out[:P], P), "attack_entries")
                print(f"k={k:2d} {kind:6s} {dirn:4s} four launches (kernel time summed) min "
                      f"{us:8.1f} us  {us / aus:5.2f} x alie  gamma {float(at.gamma[0]):.6g}",
                      flush=True)
    probe.close()


def epoch_time(attack, epochs):
    """The whole robust epoch of DESIGN 6p's end-to-end line (64 workers, delay 5, independent
    entries, 8 buckets, the plain bucket mean, 16 Byzantine workers in a block) under `attack`:
    `epochs` epochs after three warm-up epochs, each between two device synchronisations."""
    import statistics
    import time

    from flsim.sim import FLSimulation
    sim = FLSimulation(64, delay=5, device="cuda:0", semantics="independent",
                       robust_rule=("trimmed_mean", 0), buckets=8, attack=attack, n_byz=16,
                       byz_placement="block")
    ts = []
    for t in range(epochs + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sim.epoch()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = ts[3:]
    print(f"attack={attack} epochs={epochs} median {statistics.median(ts):.3f} ms "
          f"min {min(ts):.3f} ms max {max(ts):.3f} ms", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "epoch":
        epoch_time(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 12)
    else:
        main()
