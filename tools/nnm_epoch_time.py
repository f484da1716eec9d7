"""The whole robust epoch with and without nearest-neighbour mixing (GPU box):

  python tools/nnm_epoch_time.py TREE F|none [epochs]

TREE is a built checkout of this repository (".", or a parent commit's tree to compare against: it
is put first on sys.path); FLSimulation(64 workers, delay 5, independent entries, the trimmed mean
with trim 1 over 8 buckets, ALIE by 16 Byzantine workers) runs `epochs` epochs after three warm-up
epochs, each between two device synchronisations; the median, minimum and maximum ms are printed.
"none" leaves the nnm argument out altogether, so a tree from before it runs too.
"""
import os
import statistics
import sys
import time

tree = os.path.abspath(sys.argv[1])
sys.path[:0] = [tree, os.path.join(tree, "fl-distributed-delay_amd")]
import torch  # noqa: E402
from flsim.sim import FLSimulation  # noqa: E402

nnm = None if sys.argv[2] == "none" else int(sys.argv[2])
epochs = int(sys.argv[3]) if len(sys.argv) > 3 else 12
kw = {} if nnm is None else dict(nnm=nnm)
sim = FLSimulation(64, delay=5, device="cuda:0", semantics="independent",
                   robust_rule=("trimmed_mean", 1), buckets=8, attack="alie", n_byz=16, **kw)
ts = []
for t in range(epochs + 3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sim.epoch()
    torch.cuda.synchronize()
    ts.append((time.perf_counter() - t0) * 1e3)
ts = ts[3:]
print(f"tree={sys.argv[1]} nnm={nnm} epochs={epochs} median {statistics.median(ts):.3f} ms "
      f"min {min(ts):.3f} ms max {max(ts):.3f} ms", flush=True)
