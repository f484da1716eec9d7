"""Micro-benchmark of nearest-neighbour mixing (Krum's k_krum_dist, k_nnm_finish and k_nnm_mix
through flsim_nnm_entries) on PerformantNet1's parameter vector (GPU box), beside
tools/attack_bench.py.

  python tools/nnm_bench.py [reps] [k,k,...]
  rocprofv3 --kernel-trace --stats -d DIR -o nnm -- python tools/nnm_bench.py 20 9

Per k (default 9 and 64; f = (k - 1) // 2) the three launches are timed by the library's live probe
(events around each launch; the minimum and the median us over `reps` calls after two warm-up
calls), and the mix launch's algorithmic bytes, 2 k P * 4 (every entry read once and written once),
are put over its time.  The entries are restored from a pristine copy before every call (the mixing
is in place), by a torch copy outside the timed launches.  Under rocprofv3 the same calls give the
kernel trace; one k a run keeps k_nnm_finish's rows apart, the other two kernels carry KPAD in
their names.
"""
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "fl-distributed-delay_amd")]
import torch  # noqa: E402


def main():
    from flsim._lib import KernelProbe, lib
    from flsim.engine import NNM, nnm_entries
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    ks = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [9, 64]
    dev = "cuda:0"
    P = int(lib().flsim_pn1_param_count())
    g = torch.Generator(device="cpu").manual_seed(0)
    kmax = max(ks)
    Ppad = (P + 63) // 64 * 64             # (every row 16-byte aligned)
    pristine = torch.stack([torch.randn(Ppad, generator=g) * (1e-3 * (1 + 0.25 * j)) * 8
                            for j in range(kmax)]).to(dev)
    work = torch.empty_like(pristine)
    probe = KernelProbe()
    names = ("nnm_dist", "nnm_finish", "nnm_mix")
    for k in ks:
        f = (k - 1) // 2
        mix = NNM(f, [work[j][:P] for j in range(k)], [8] * k)
        times = {n: [] for n in names}
        nbytes = 0.0
        for r in range(reps + 2):
            work[:k].copy_(pristine[:k])
            torch.cuda.synchronize()
            probe.read()
            nnm_entries(mix, P)
            torch.cuda.synchronize()
            got = probe.read()
            if r >= 2:
                for n in names:
                    times[n].append(got[n][1] * 1e3)
                nbytes = got["nnm_mix"][2]
        assert nbytes == 8.0 * P * k
        nbr = mix.neighbours()
        assert all(len(row) == k - f and i in row for i, row in enumerate(nbr))
        for n in names:
            print(f"k={k:2d} f={f:2d} {n:10s} min {min(times[n]):8.1f} us  "
                  f"median {statistics.median(times[n]):8.1f} us", flush=True)
        us = min(times["nnm_mix"])
        print(f"k={k:2d} f={f:2d} nnm_mix    {nbytes / 1e6:8.2f} MB  {nbytes / us / 1e6:5.2f} TB/s "
              f"(2 k P * 4 bytes over the minimum)", flush=True)
    probe.close()


if __name__ == "__main__":
    main()
