# Periodic range queries, friends-of-friends and pair counts next to the open calls, on the 10^6
# uniform particles of perf_fof.py (the unit box), with the period equal to the data's extent,
# L = (1, 1, 1).  Cases: range_counts_sph at every particle's own 32nd-neighbour distance (counts,
# and counts with one channel of gather sums), fof_labels_sph at b = 0.2 mean separations, and
# pair_counts_sph at 16 logarithmic edges from 0.04 to 4 mean separations.
# Stateless calls: two warm-ups of each case, then rounds that alternate open and periodic; printed
# as median [min .. max] of the walk alone (grace_trace_last_kernel_ms) and of the whole call (device
# events: keys, sort and packet scan included).
#   perf_periodic_queries.py                      open and periodic, this checkout
#   perf_periodic_queries.py --open-only --package <other checkout>/grace-devel_amd
#                                                 the open calls of another build (the parent commit's),
#                                                 run in turns with the first form for the comparison
import argparse
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--package", default=None, help="a grace-devel_amd directory to import grace_hip from")
ap.add_argument("--open-only", action="store_true")
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, args.package or os.path.join(ROOT, 'grace-devel_amd'))
import numpy as np
import torch
import grace_hip as gh

dev = torch.device('cuda:0')
PERIOD = (1.0, 1.0, 1.0)


def spread(v):
    v = sorted(v)
    return "%.3f [%.3f .. %.3f]" % (v[len(v) // 2], v[0], v[-1])


def once(f):
    a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
    a.record(); f(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b), gh.last_kernel_ms()


def uniform(n, seed):
    s = np.random.default_rng(seed).random((n, 4), dtype=np.float32)
    s[:, 3] = 0.01
    return s


n = 1_000_000
sep = (1.0 / n) ** (1.0 / 3.0)
s = torch.from_numpy(uniform(n, 22)).to(dev)
t = gh.Tree(n, 32, device=dev); gh.build_tree(s, t, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
gh.set_cache_auto(False)
gh.enable_kernel_timing(True)
h = gh.smoothing_lengths_sph(s, t, 32, 1.0)
w1 = torch.ones(n, dtype=torch.float32, device=dev)
cnt = torch.empty(n, dtype=torch.int32, device=dev)
o1 = torch.empty(n, dtype=torch.float32, device=dev)
labels = torch.empty(n, dtype=torch.int32, device=dev)
b = 0.2 * sep
edges = np.exp(np.linspace(np.log(0.04 * sep), np.log(4.0 * sep), 16)).astype(np.float32)


def cases(period):
    kw = {} if period is None else {"period": period}
    return [
        ("range_counts_sph COUNT", lambda: gh.range_counts_sph(s, h, s, t, counts=cnt, **kw),
         lambda: int(cnt.sum(dtype=torch.int64))),
        ("range_counts_sph COUNT+SUMS C = 1", lambda: gh.range_counts_sph(s, h, s, t, weights=w1, counts=cnt, out=o1, **kw),
         lambda: int(cnt.sum(dtype=torch.int64))),
        ("fof_labels_sph b = 0.2 sep", lambda: gh.fof_labels_sph(s, t, b, labels=labels, **kw),
         lambda: int(torch.unique(labels).numel())),
        ("pair_counts_sph 16 edges to 4 sep", lambda: gh.pair_counts_sph(s, edges, s, t, **kw),
         lambda: int(gh.pair_counts_sph(s, edges, s, t, **kw).cpu().numpy().astype(np.int64).sum())),
    ]


versions = [("open", cases(None))] + ([] if args.open_only else [("periodic", cases(PERIOD))])
times = {(v, c[0]): ([], []) for v, cs in versions for c in cs}
for v, cs in versions:
    for name, call, _ in cs:
        call(); call()
torch.cuda.synchronize()
for _ in range(args.reps):
    for k in range(len(versions[0][1])):
        for v, cs in versions:                                      # the versions of a case in turns
            ms, kms = once(cs[k][1])
            times[(v, cs[k][0])][0].append(ms); times[(v, cs[k][0])][1].append(kms)
gh.trace_status()
for k in range(len(versions[0][1])):
    for v, cs in versions:
        name, call, result = cs[k]
        call(); torch.cuda.synchronize()
        ms, kms = times[(v, name)]
        print("%-34s %-8s walk %s ms, call %s ms, result %d" % (name, v, spread(kms), spread(ms), result()))
print("%d uniform particles, mean separation %.3e, period %s, median 32nd-neighbour distance %.3e"
      % (n, sep, PERIOD, float(h.median())))
gh.enable_kernel_timing(False)
