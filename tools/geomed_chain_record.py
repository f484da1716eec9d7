"""The whole-chain difference of the fused geometric-median step (recorded, not gated): g of the
device against flsim.robust.geomed_flat run from scratch on the CPU, over the cases of
tests/test_gpu_geomed.py::test_stepwise_against_the_text.  The distances differ in their last bits
(summation order), the weights inherit that, so g can differ in its last bit; the tests pin every
stage at the device's own inputs instead (tests/_geomed.py).

  python tools/geomed_chain_record.py          # prints one line per k and a total
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "fl-distributed-delay_amd"), os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    import _geomed as G
    from flsim._lib import lib
    from flsim.engine import GeoMed, geomed_step
    dev = "cuda:0"
    tot_words = tot_diff = 0
    tot_ulp = 0
    for k in G.KS:
        E = int(lib().flsim_geomed_tile_elems(k))
        words = diff = 0
        ulp = 0
        for P in (1, 255, 256, 257, E - 1, E, E + 1, 3 * E + 5):
            ent, cnt = G.inputs(k, P)
            dent = [torch.from_numpy(e).to(dev) for e in ent]
            for iters in (0, 1, 3):
                for weighted in (False, True):
                    g = torch.empty(P, device=dev)
                    gm = GeoMed(iters, G.NU, weighted, dent, cnt)
                    geomed_step(gm, None, None, None, 1, P=P, optim=False, g_out=g)
                    got = g.cpu().numpy()
                    ref = G.text(ent, cnt, iters, G.NU, weighted)[0]
                    u = G.ulp_distance(got, ref)
                    words += P
                    diff += int((u != 0).sum())
                    ulp = max(ulp, int(u.max()))
        print(f"k={k:2d}  words {words:7d}  differing {diff:5d} ({100.0 * diff / words:6.3f} %)  "
              f"max ulp distance {ulp}", flush=True)
        tot_words += words
        tot_diff += diff
        tot_ulp = max(tot_ulp, ulp)
    print(f"all    words {tot_words:7d}  differing {tot_diff:5d} "
          f"({100.0 * tot_diff / tot_words:6.3f} %)  max ulp distance {tot_ulp}")


if __name__ == "__main__":
    main()
