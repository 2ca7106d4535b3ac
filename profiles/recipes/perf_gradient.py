# SPH gradients at points (interpolate_gradient_sph / interpolate_gradient_grid_sph) on bench.py's scene
# (10^7 particles, ~48 neighbours per point, cubic kernel): the gradient of 1, 3 and 4 channels with
# 1 and with 2 gradient channels per walk (interpolate_gradient_channels_per_walk), and the 4-channel
# field call (interpolate_sph / interpolate_grid_sph) on the same points in the same job, at 10^6 random
# points (sort included in the call time) and on a 1024^2 axis-aligned slice.  Stateless calls: a
# warm-up, then the median of 5.  Per case: call ms (device events around the call) and walk ms
# (grace_trace_last_kernel_ms: the sum of the call's walks).
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
w4 = torch.rand((n, 4), generator=g, device=dev)
gh.set_cache_auto(False)
gh.enable_kernel_timing(True)

points = torch.rand((1_000_000, 3), generator=g, device=dev)
slice_ = ((0.0005, 0.0005, 0.5), (1 / 1024, 0, 0), (0, 1 / 1024, 0), (0, 0, 1), (1024, 1024, 1))
print("gradient channels per walk by default: %d" % gh.interpolate_gradient_channels_per_walk(0))
for name, grid in (("10^6 random points", None), ("slice 1024^2 axis-aligned", slice_)):
    m = len(points) if grid is None else grid[4][0] * grid[4][1] * grid[4][2]
    shape = (m,) if grid is None else (grid[4][2], grid[4][1], grid[4][0])
    out = torch.empty(shape + (4,), dtype=torch.float32, device=dev)
    if grid is None:
        field = lambda: gh.interpolate_sph(points, s, t, w4, out=out)
    else:
        field = lambda: gh.interpolate_grid_sph(*grid, s, t, w4, out=out)
    ms, kms = timeit(field)
    print("%s: field, 4 channels: %.3f ms call, %.3f ms walk" % (name, ms, kms))
    base = kms
    for n_ch in (1, 3, 4):
        w = w4[:, :n_ch].contiguous()
        grad = torch.empty(shape + (n_ch, 3), dtype=torch.float32, device=dev)
        for per_walk in (1, 2):
            gh.interpolate_gradient_channels_per_walk(per_walk)
            for with_value in (False, True):
                value = torch.empty(shape + (n_ch,), dtype=torch.float32, device=dev) if with_value else None
                if grid is None:
                    call = lambda: gh.interpolate_gradient_sph(points, s, t, w, grad=grad, value=value)
                else:
                    call = lambda: gh.interpolate_gradient_grid_sph(*grid, s, t, w, grad=grad, value=value)
                ms, kms = timeit(call)
                print("%s: gradient, %d channels, %d per walk%s: %.3f ms call, %.3f ms walk (%.2f x the field walk)"
                      % (name, n_ch, per_walk, ", with value" if with_value else "", ms, kms, kms / base))
gh.interpolate_gradient_channels_per_walk(0)
gh.trace_status()
gh.enable_kernel_timing(False)
