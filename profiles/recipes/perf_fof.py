# Friends-of-friends groups (fof_labels_sph / fof_groups_sph) on 10^6 clustered particles (the tests'
# clustered generator) and on 10^6 uniform ones, at b = 0.2 mean separations = 0.2 (V / n)^(1/3), next
# to the yardstick: range_counts_sph(points = spheres, radius = b) on the same particles, which does
# every pair test from both sides and nothing else.
# Stateless calls: two warm-ups, then 7 repeats; printed as median [min .. max].  Per case: call ms
# (device events around the call: keys, sort and packet scan included) and kernel ms
# (grace_trace_last_kernel_ms: the link and flatten kernels, or the range walk, alone).  The
# catalogue (groups + members, min_members = 32) is timed by the host clock around a synchronised
# call: it reads the group count back.
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'grace-devel_amd'))
import numpy as np
import torch
import grace_hip as gh

dev = torch.device('cuda:0')
REPS = 7


def spread(v):
    v = sorted(v)
    return "%.3f [%.3f .. %.3f]" % (v[len(v) // 2], v[0], v[-1])


def timeit(f):
    f(); f(); torch.cuda.synchronize(); ts, ks = [], []
    for _ in range(REPS):
        a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b)); ks.append(gh.last_kernel_ms())
    return spread(ts), spread(ks)


def host_timeit(f):
    f(); f(); torch.cuda.synchronize(); ts = []
    for _ in range(REPS):
        t0 = time.perf_counter(); f(); torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return spread(ts)


def clustered(n, seed):
    rng = np.random.default_rng(seed)
    centres = np.array([[0.3, 0.3, 0.3], [0.7, 0.6, 0.4], [0.5, 0.5, 0.8]])
    k = rng.integers(0, 3, n)
    s = np.empty((n, 4), np.float32)
    s[:, :3] = np.clip(centres[k] + rng.normal(0.0, 0.02, (n, 3)) * rng.random((n, 1)) ** 3, 0.001, 0.999)
    s[:, 3] = (0.004 + 0.02 * rng.random(n)).astype(np.float32)
    return s


def uniform(n, seed):
    s = np.random.default_rng(seed).random((n, 4), dtype=np.float32)
    s[:, 3] = 0.01
    return s


n = 1_000_000
b = 0.2 * (1.0 / n) ** (1.0 / 3.0)
gh.set_cache_auto(False)
gh.enable_kernel_timing(True)
for name, scene in (("clustered", clustered(n, 21)), ("uniform", uniform(n, 22))):
    s = torch.from_numpy(scene).to(dev)
    t = gh.Tree(n, 32, device=dev); gh.build_tree(s, t, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    ms, kms = timeit(lambda: gh.fof_labels_sph(s, t, b, labels=labels))
    print("%s fof_labels_sph: %s ms call, %s ms link + flatten" % (name, ms, kms))
    ms, kms = timeit(lambda: gh.range_counts_sph(s, b, s, t, counts=cnt))
    print("%s range_counts_sph: %s ms call, %s ms walk" % (name, ms, kms))
    print("%s fof_groups_sph (min_members 32, with members): %s ms" % (name, host_timeit(lambda: gh.fof_groups_sph(labels, 32))))
    gh.trace_status()
    group_of, sizes, offsets, members = gh.fof_groups_sph(labels, 32)
    print("%s: %d particles, b = %.3e, %.1f pairs in range per particle, %d groups in all, %d of 32 or more "
          "(largest %d) holding %d particles" % (name, n, b, float(cnt.sum(dtype=torch.int64)) / n - 1.0,
                                                 int(torch.unique(labels).numel()), len(sizes),
                                                 int(sizes.max()) if len(sizes) else 0, len(members)))
gh.enable_kernel_timing(False)
