"""Micro-benchmark of the attack launch (k_attack through flsim_attack_entries) on PerformantNet1's
parameter vector (GPU box), timed by the library's live probe (flsim_probe_*: events around each
launch), beside tools/geomed_bench.py.

  python tools/attack_bench.py [reps] [k,k,...]

Per k (default 4, 8, 16, 32, 64) and kind, two splits of the k entries, 8 workers each:
  block    the first k / 4 entries fully Byzantine (written, never read), the rest honest-only (read):
           (3 k / 4 + k / 4 + 1) * 4 P bytes with b_out;
  spread   every entry mixed (7 honest + 1 Byzantine: read and written): (2 k + 1) * 4 P bytes.
The minimum us over `reps` launches against the floor those bytes give at 6.2 TB/s (the rate
DESIGN 6o uses), and against k_geomed_dist's pair-0 launch at the same k (a step with iters = 0).
The strength is small, so that the entries stay finite over the repeats (the launch updates them in
place).
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "fl-distributed-delay_amd")]
import torch  # noqa: E402

RATE = 6.2e12


def main():
    from flsim._lib import KernelProbe, lib
    from flsim.engine import Attack, GeoMed, attack_entries, geomed_step
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
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

    def timed(fn, name):
        """(minimum us of the kernel `name` in one call, its algorithmic bytes) over `reps` calls."""
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        probe.read()
        best = None
        for _ in range(reps):
            fn()
            torch.cuda.synchronize()
            _, ms, work = probe.read()[name]
            if best is None or ms * 1e3 < best[0]:
                best = (ms * 1e3, work)
        return best

    for k in ks:
        gm = GeoMed(0, 1e-6, False, [e[:P] for e in ents[:k]], [8] * k)
        gus, _ = timed(lambda: geomed_step(gm, theta[:P], m[:P], v[:P], 5), "geomed_dist")
        print(f"k_geomed_dist pair 0 k={k:2d}           min {gus:8.1f} us", flush=True)
        nb = max(k // 4, 1)
        splits = {"block": ([0] * nb + [8] * (k - nb), [8] * nb + [0] * (k - nb)),
                  "spread": ([7] * k, [1] * k)}
        for kind in ("ipm", "alie"):
            for name, (honest, byz) in splits.items():
                at = Attack(kind, 0.01, [e[:P] for e in ents[:k]], honest, byz)
                us, nbytes = timed(lambda: attack_entries(at, b_out[:P], P), "attack_entries")
                floor = nbytes / RATE * 1e6
                print(f"k_attack {kind:4s} {name:6s} k={k:2d}  min {us:8.1f} us  "
                      f"{nbytes / 1e6:8.2f} MB  {nbytes / us / 1e6:5.2f} TB/s  floor {floor:6.1f} us  "
                      f"{us / floor:4.2f} x floor  {us / gus:4.2f} x k_geomed_dist", flush=True)
    probe.close()


if __name__ == "__main__":
    main()
