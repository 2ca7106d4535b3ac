# Nearest neighbours and smoothing lengths (smoothing_lengths_sph / nearest_neighbours_sph) on
# bench.py's scene (10^7 particles, uniform in the unit cube): smoothing lengths at k = 32 and
# k = 64, and the 32 nearest neighbours of 10^6 random points (key, sort and packet scan included).
# Stateless calls: a warm-up, then the median of 5.  Per case: call ms (device events around the
# call), walk ms (grace_trace_last_kernel_ms: the neighbour kernel alone), candidate tests per
# point (active lanes x survivors of the culling rounds, over points), insertion steps per packet
# (survivors on which at least one lane inserted) and lane fill (points over 64 x packets).
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'grace-devel_amd'))
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


n = 10_000_000
g = torch.Generator(device=dev); g.manual_seed(42)
s = torch.empty((n, 4), dtype=torch.float32, device=dev)
s[:, :3] = torch.rand((n, 3), generator=g, device=dev); s[:, 3] = float((3 * 48 / (4 * math.pi * n)) ** (1 / 3))
lo, hi = gh.min_max_vec4(s); lo[3] = hi[3] = 0
t = gh.Tree(n, 32, device=dev); gh.build_tree(s, t, lo[:3], hi[:3])
gh.set_cache_auto(False)
gh.enable_kernel_timing(True)

pts = torch.rand((1_000_000, 3), generator=g, device=dev)
h = torch.empty(n, dtype=torch.float32, device=dev)
idx = torch.empty((len(pts), 32), dtype=torch.int32, device=dev)
d2 = torch.empty((len(pts), 32), dtype=torch.float32, device=dev)
cases = [
    ("smoothing lengths k = 32", n, lambda: gh.smoothing_lengths_sph(s, t, 32, 1.0, out=h)),
    ("smoothing lengths k = 64", n, lambda: gh.smoothing_lengths_sph(s, t, 64, 1.0, out=h)),
    ("10^6 random points k = 32", len(pts), lambda: gh.nearest_neighbours_sph(pts, s, t, 32, indices=idx, d2=d2)),
]
for name, m, call in cases:
    ms, kms = timeit(call)
    gh.neighbours_enable_stats(True); call(); tests, packets, steps = gh.neighbours_last_stats(); gh.neighbours_enable_stats(False)
    # tests / point = survivors a lane ranks; steps / packet = survivors on which some lane of the wave
    # ran the K-slot insertion
    print("%s: %.3f ms call, %.3f ms walk, %d points, %.1f candidate tests/point, %.1f insertion steps/packet, "
          "lane fill %.3f" % (name, ms, kms, m, tests / m, steps / max(packets, 1), m / (64.0 * max(packets, 1))))
gh.trace_status()
gh.enable_kernel_timing(False)
