"""Micro-benchmark of the staleness-weighted server step against the plain one on
PerformantNet1's parameter vector (GPU box): the fused slab step (k_slab_step / k_slab_step_seq)
and the streaming step (k_agg_stream_reg / k_agg_stream) with the same rule, unweighted and
weighted, timed by the library's live probe (flsim_probe_*: events around each launch).

  python tools/wstep_bench.py [reps]

Rules: the tick rule k = 513 with one stale array; a configs[3]-style general-order program
(k = 8100, 72 stale entries among 6 arrays, as tools/step_bench.py's seq mode).  Prints one line
per (kernel, rule, form): mean and minimum us over `reps` launches.  On a tree from before the
weighted rule only the plain forms run.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "fl-distributed-delay_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    from flsim._lib import KernelProbe
    from flsim.engine import PN1Engine, ProgramStager, Rule
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
    from flsim.data import DevicePool
    from flsim.engine import worker_table
    from oracle import oracle as O
    items = [(0, 0, 1), (0, 3, 7)]
    eng.run_chunk(theta, DevicePool(dev, 0, O.make_pool(0)), worker_table(items, dev), 2, 8, 0,
                  True, torch.zeros(2, device=dev))
    rs = np.random.RandomState(0)
    pos = np.sort(rs.choice(8100, 72, replace=False))
    ev = list(zip(pos.tolist(), rs.randint(0, 6, 72).tolist()))
    stager = ProgramStager(dev)
    w6 = [(1.0 + t) ** -0.5 for t in (2, 3, 5, 8, 13, 50)]
    rules = {"tick k=513": (lambda **kw: Rule(513, arrs[:1], c=512, **kw), w6[:1]),
             "general k=8100": (lambda **kw: Rule(8100, arrs, events=ev, stager=stager, **kw),
                                w6)}
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
        return float(np.mean(per)), float(np.min(per)), "+".join(sorted(rec))

    for name, (make, ws) in rules.items():
        forms = [("plain", make())]
        try:
            forms.append(("weighted", make(weights=ws)))
        except TypeError:
            pass
        for form, rule in forms:
            for what, fn in (("fused step", lambda: eng.server_step(None, rule, theta, m, v, 5)),
                             ("stream", lambda: eng.aggregate_rule(S, rule, theta, m, v, 5))):
                mean, best, kern = timed(fn)
                print(f"{what:10s} {name:15s} {form:8s} mean {mean:8.1f} us  min {best:8.1f} us"
                      f"  [{kern}]", flush=True)
    probe.close()


if __name__ == "__main__":
    main()
