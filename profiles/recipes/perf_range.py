# Range queries (range_counts_sph / range_neighbours_sph) on 10^6 clustered particles (the tests'
# clustered generator), querying every particle at r = its own 32nd-neighbour distance
# (smoothing_lengths_sph(k = 32, eta = 1)), next to nearest_neighbours_sph(k = 32) on the same points.
# Stateless calls: a warm-up, then the median of 5.  Per case: call ms (device events around the
# call: keys, sort and packet scan included) and walk ms (grace_trace_last_kernel_ms: the walks of
# the call alone).
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'grace-devel_amd'))
import ctypes as C
import numpy as np
import torch
import grace_hip as gh

dev = torch.device('cuda:0')


def timeit(f, reps=5):
    f(); torch.cuda.synchronize(); ts, ks = [], []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b)); ks.append(gh.last_kernel_ms())
    return sorted(ts)[len(ts) // 2], sorted(ks)[len(ks) // 2]


def clustered(n, seed):
    rng = np.random.default_rng(seed)
    centres = np.array([[0.3, 0.3, 0.3], [0.7, 0.6, 0.4], [0.5, 0.5, 0.8]])
    k = rng.integers(0, 3, n)
    s = np.empty((n, 4), np.float32)
    s[:, :3] = np.clip(centres[k] + rng.normal(0.0, 0.02, (n, 3)) * rng.random((n, 1)) ** 3, 0.001, 0.999)
    s[:, 3] = (0.004 + 0.02 * rng.random(n)).astype(np.float32)
    return s


n = 1_000_000
s = torch.from_numpy(clustered(n, 21)).to(dev)
t = gh.Tree(n, 32, device=dev); gh.build_tree(s, t, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
gh.set_cache_auto(False)
gh.enable_kernel_timing(True)
h = gh.smoothing_lengths_sph(s, t, 32, 1.0)
w1 = torch.ones(n, dtype=torch.float32, device=dev)
w4 = torch.ones((n, 4), dtype=torch.float32, device=dev)
cnt = torch.empty(n, dtype=torch.int32, device=dev)
o1 = torch.empty(n, dtype=torch.float32, device=dev)
o4 = torch.empty((n, 4), dtype=torch.float32, device=dev)
offsets = torch.zeros(n + 1, dtype=torch.int32, device=dev)
gh.range_counts_sph(s, h, s, t, counts=offsets[:n])
total = gh.exclusive_scan(offsets, offsets)
idx = torch.empty(total, dtype=torch.int32, device=dev)
d2 = torch.empty(total, dtype=torch.float32, device=dev)
ki = torch.empty((n, 32), dtype=torch.int32, device=dev)
kd = torch.empty((n, 32), dtype=torch.float32, device=dev)


def fill():
    gh._check(gh._lib.grace_range_neighbours_f4(gh._ptr(s), C.c_size_t(n), C.c_int(4), gh._ptr(h), C.c_float(0.0),
                                                *gh._interp_scene(s, t), gh._ptr(offsets), gh._ptr(idx), gh._ptr(d2),
                                                gh._stream()))


cases = [
    ("COUNT", lambda: gh.range_counts_sph(s, h, s, t, counts=cnt)),
    ("COUNT+SUMS C = 1", lambda: gh.range_counts_sph(s, h, s, t, weights=w1, counts=cnt, out=o1)),
    ("COUNT+SUMS C = 4", lambda: gh.range_counts_sph(s, h, s, t, weights=w4, counts=cnt, out=o4)),
    ("FILL (%d list entries)" % total, fill),
    ("nearest_neighbours_sph k = 32", lambda: gh.nearest_neighbours_sph(s, s, t, 32, indices=ki, d2=kd)),
]
for name, call in cases:
    ms, kms = timeit(call)
    print("%s: %.3f ms call, %.3f ms walk" % (name, ms, kms))
gh.trace_status()
print("%d points, %.1f entries per row, longest row %d" % (n, total / n, int(cnt.max())))
gh.enable_kernel_timing(False)
