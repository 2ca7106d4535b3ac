# Weighted column densities (trace_cumulative_weighted_sph) against the unweighted trace and the
# per-hit composition (trace_sph + multiply_by_weights + segmented sum) on BASELINE config 2
# (10^6 spheres, 10^5 isotropic rays) and bench.py's scene (10^7 particles, 1024^2 orthographic
# rays, where the per-hit path's int offsets overflow).  Stateless calls, median of 5.
import sys, os, math
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'grace-devel_amd'))
import torch, grace_hip as gh
dev = torch.device('cuda:0')


def timeit(f, reps=5):
    f(); torch.cuda.synchronize(); ts = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def scene(name, s, lo, hi, rays, composition):
    n, R = len(s), len(rays)
    t = gh.Tree(n, 32, device=dev); gh.build_tree(s, t, lo, hi)
    c = torch.empty(R, dtype=torch.float32, device=dev)
    w = {C: torch.rand((n, C), device=dev) + 0.5 for C in (1, 2, 4)}
    gh.set_cache_auto(False)      # every call derives its records
    line = "%s: unweighted %.3f ms" % (name, timeit(lambda: gh.trace_cumulative_sph(rays, s, t, c)))
    for C in (1, 2, 4):
        out = torch.empty((R, C) if C > 1 else (R,), dtype=torch.float32, device=dev)
        wc = w[C] if C > 1 else w[C][:, 0].contiguous()
        line += ", C=%d %.3f ms" % (C, timeit(lambda: gh.trace_cumulative_weighted_sph(rays, s, t, wc, out)))
    if composition:
        # per hit: trace_sph, then w[idx] * integral and a per-ray sum (one channel)
        w1 = w[1][:, 0].contiguous()
        def comp():
            off, idx, integ, _ = gh.trace_sph(rays, s, t)
            vals = w1[idx.long()] * integ
            seg = torch.repeat_interleave(torch.arange(R, device=dev), torch.diff(
                torch.cat([off.long(), torch.tensor([len(idx)], device=dev)])))
            return torch.zeros(R, device=dev).index_add_(0, seg, vals)
        line += ", composition (trace_sph + weights + segmented sum) %.3f ms" % timeit(comp)
    gh.set_cache_auto(True)
    gh.trace_status()
    print(line)
    gh.trace_release(); gh.trace_release_rays()


g = torch.Generator(device=dev); g.manual_seed(3)
s = torch.rand((1_000_000, 4), generator=g, device=dev); s[:, 3] *= 0.1
scene("config 2", s, (0, 0, 0), (1, 1, 1), gh.uniform_random_rays(100_000, (0.5, 0.5, 0.5), 2.0, seed=1234, device=dev),
      True)
del s
n = 10_000_000
g.manual_seed(42)
s4 = torch.empty((n, 4), dtype=torch.float32, device=dev)
s4[:, :3] = torch.rand((n, 3), generator=g, device=dev); s4[:, 3] = float((3 * 48 / (4 * math.pi * n)) ** (1 / 3))
lo, hi = gh.min_max_vec4(s4); lo[3] = hi[3] = 0
r4, _ = gh.orthogonal_rays_z(1024, lo, hi, device=dev)
scene("bench scene", s4, lo[:3], hi[:3], r4, False)
