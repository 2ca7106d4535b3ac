# Periodic nearest neighbours, smoothing lengths and interpolation next to the open calls, on the 10^6
# uniform particles of perf_periodic_queries.py (the unit box), with the period equal to the data's
# extent, L = (1, 1, 1).  The spheres carry H = their open 32nd-neighbour distance (the tree is built
# with it; the order does not change).  Cases: smoothing_lengths_sph at k = 32, nearest_neighbours_sph
# at k = 32 for 10^6 random points of the box, and interpolate_grid_sph on a 256^3 mesh over the box
# with one channel and the counts.
# Stateless calls: two warm-ups of each case, then rounds that alternate open and periodic; printed
# as median [min .. max] of the walk alone (grace_trace_last_kernel_ms) and of the whole call (device
# events: keys, sort and packet scan included).  Then, outside the timing, the measurement hooks:
# candidate tests per point and insertion steps per packet (neighbours), survivor tests per point
# (interpolation).
#   perf_periodic_points.py [--k K]               open and periodic, this checkout (K: another list size)
#   perf_periodic_points.py --open-only --package <other checkout>/grace-devel_amd
#                                                 the open calls of another build (the parent commit's),
#                                                 run in turns with the first form for the comparison
import argparse
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--package", default=None, help="a grace-devel_amd directory to import grace_hip from")
ap.add_argument("--open-only", action="store_true")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--mesh", type=int, default=256)
ap.add_argument("--k", type=int, default=32, help="neighbours per point (the kernels are built for 8, 16, 32, 64)")
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


n, k, m = 1_000_000, args.k, args.mesh
s = torch.from_numpy(uniform(n, 22)).to(dev)
t = gh.Tree(n, 32, device=dev); gh.build_tree(s, t, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
s[:, 3] = gh.smoothing_lengths_sph(s, t, 32, 1.0)                 # the open lengths, in every run
t = gh.Tree(n, 32, device=dev); gh.build_tree(s, t, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
gh.set_cache_auto(False)
gh.enable_kernel_timing(True)
pts = torch.from_numpy(np.random.default_rng(23).random((n, 3), dtype=np.float32)).to(dev)
h = torch.empty(n, dtype=torch.float32, device=dev)
idx = torch.empty((n, k), dtype=torch.int32, device=dev)
d2 = torch.empty((n, k), dtype=torch.float32, device=dev)
w1 = torch.ones(n, dtype=torch.float32, device=dev)
mesh = torch.empty((m, m, m), dtype=torch.float32, device=dev)
cnt = torch.empty((m, m, m), dtype=torch.int32, device=dev)
o, dx = (0.0, 0.0, 0.0), 1.0 / m


def cases(period):
    kw = {} if period is None else {"period": period}
    return [
        ("smoothing_lengths_sph k = %d" % k, n, "nbr", lambda: gh.smoothing_lengths_sph(s, t, k, 1.0, out=h, **kw),
         lambda: float(h.sum(dtype=torch.float64))),
        ("nearest_neighbours_sph 10^6 pts k = %d" % k, n, "nbr",
         lambda: gh.nearest_neighbours_sph(pts, s, t, k, indices=idx, d2=d2, **kw),
         lambda: float(d2[:, k - 1].sqrt().sum(dtype=torch.float64))),
        ("interpolate_grid_sph %d^3 C = 1" % m, m ** 3, "interp",
         lambda: gh.interpolate_grid_sph(o, (dx, 0, 0), (0, dx, 0), (0, 0, dx), (m, m, m), s, t, w1, out=mesh, counts=cnt, **kw),
         lambda: float(cnt.sum(dtype=torch.int64))),
    ]


versions = [("open", cases(None))] + ([] if args.open_only else [("periodic", cases(PERIOD))])
times = {(v, c[0]): ([], []) for v, cs in versions for c in cs}
for v, cs in versions:
    for c in cs:
        c[3](); c[3]()
torch.cuda.synchronize()
for _ in range(args.reps):
    for i in range(len(versions[0][1])):
        for v, cs in versions:                                      # the versions of a case in turns
            ms, kms = once(cs[i][3])
            times[(v, cs[i][0])][0].append(ms); times[(v, cs[i][0])][1].append(kms)
gh.trace_status()
for i in range(len(versions[0][1])):
    for v, cs in versions:
        name, points, family, call, result = cs[i]
        call(); torch.cuda.synchronize()
        ms, kms = times[(v, name)]
        print("%-38s %-8s walk %s ms, call %s ms, result %.6e" % (name, v, spread(kms), spread(ms), result()))
gh.enable_kernel_timing(False)
# the hooks: work per point, periodic against open
for i in range(len(versions[0][1])):
    for v, cs in versions:
        name, points, family, call, _ = cs[i]
        if family == "nbr":
            gh.neighbours_enable_stats(True); call(); tests, packets, steps = gh.neighbours_last_stats(); gh.neighbours_enable_stats(False)
            print("%-38s %-8s candidate tests / point %.1f, insertion steps / packet %.1f, packets %d"
                  % (name, v, tests / points, steps / packets, packets))
        else:
            gh.interpolate_enable_stats(True); call(); tests = gh.interpolate_last_stats(); gh.interpolate_enable_stats(False)
            print("%-38s %-8s survivor tests / point %.1f" % (name, v, tests / points))
print("%d uniform particles, period %s, median H %.3e (the open 32nd-neighbour distance), mesh %d^3"
      % (n, PERIOD, float(s[:, 3].median()), m))
