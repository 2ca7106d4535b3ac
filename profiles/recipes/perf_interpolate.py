# SPH interpolation at points (interpolate_grid_sph / interpolate_sph) on bench.py's scene (10^7
# particles, ~48 neighbours per point, cubic kernel, one channel w = 1): a 1024^2 axis-aligned
# slice, a 1024^2 oblique slice, a 256^3 grid and 10^6 random points (sort included).  Stateless
# calls: a warm-up, then the median of 5.  Per case: call ms (device events around the call),
# walk ms (grace_trace_last_kernel_ms: the interpolation kernel alone), terms/s (sum of counts /
# walk time), lane fill (terms / survivor tests); and the same job's trace_cumulative_sph hits/s
# on 1024^2 orthographic rays for comparison.
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
w = torch.ones(n, dtype=torch.float32, device=dev)
gh.set_cache_auto(False)
gh.enable_kernel_timing(True)

rays, _ = gh.orthogonal_rays_z(1024, lo, hi, device=dev)
col = torch.empty(len(rays), dtype=torch.float32, device=dev)
cnt = torch.empty(len(rays), dtype=torch.int32, device=dev)
gh.trace_hitcounts_sph(rays, s, t, cnt)
hits = int(cnt.long().sum())
ms, kms = timeit(lambda: gh.trace_cumulative_sph(rays, s, t, col))
print("trace_cumulative_sph 1024^2 z-rays: %.3f ms call, %.3f ms kernel, %d hits, %.3g hits/s"
      % (ms, kms, hits, hits / (kms * 1e-3)))

th = 0.4
cases = [
    ("slice 1024^2 axis-aligned", "grid", ((0.0005, 0.0005, 0.5), (1 / 1024, 0, 0), (0, 1 / 1024, 0), (0, 0, 1), (1024, 1024, 1))),
    ("slice 1024^2 oblique", "grid", ((0.05, 0.05, 0.2), (0.9 * math.cos(th) / 1024, 0, 0.9 * math.sin(th) / 1024),
                                      (0, 0.9 / 1024, 0), (0, 0, 1), (1024, 1024, 1))),
    ("grid 256^3", "grid", ((0.5 / 256,) * 3, (1 / 256, 0, 0), (0, 1 / 256, 0), (0, 0, 1 / 256), (256, 256, 256))),
    ("10^6 random points", "points", torch.rand((1_000_000, 3), generator=g, device=dev)),
]
for name, kind, spec in cases:
    if kind == "grid":
        o, u, v, ww, dims = spec
        m = dims[0] * dims[1] * dims[2]
        out = torch.empty(m, dtype=torch.float32, device=dev).view(dims[2], dims[1], dims[0])
        c = torch.empty_like(out, dtype=torch.int32)
        call = lambda: gh.interpolate_grid_sph(o, u, v, ww, dims, s, t, w, out=out, counts=c)
    else:
        m = len(spec)
        out = torch.empty(m, dtype=torch.float32, device=dev)
        c = torch.empty(m, dtype=torch.int32, device=dev)
        call = lambda: gh.interpolate_sph(spec, s, t, w, out=out, counts=c)
    ms, kms = timeit(call)
    gh.interpolate_enable_stats(True); call(); tests = gh.interpolate_last_stats(); gh.interpolate_enable_stats(False)
    terms = int(c.long().sum())
    print("%s: %.3f ms call, %.3f ms walk, %d points, %.1f terms/point, %.3g terms/s, lane fill %.3f"
          % (name, ms, kms, m, terms / m, terms / (kms * 1e-3), terms / max(tests, 1)))
gh.trace_status()
gh.enable_kernel_timing(False)
