# Mixed-precision column densities (trace_cumulative_sph<float4, double>) against the float4/float
# and double4/double paths on the same scenes: config 2 (10^6 spheres, 10^5 isotropic rays) and
# bench.py's scene (10^7 particles, 1024^2 orthographic rays).  Stateless calls, median of 5.
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


def scene(name, sd, lo, hi, rays):
    n, R = len(sd), len(rays)
    sf = sd.float().contiguous()
    tf = gh.Tree(n, 32, device=dev); gh.build_tree(sf, tf, lo, hi)        # sorts sf
    td = gh.Tree(n, 32, device=dev); gh.build_tree_d4(sd, td, lo, hi)     # sorts sd
    c32 = torch.empty(R, dtype=torch.float32, device=dev)
    c64 = torch.empty(R, dtype=torch.float64, device=dev)
    cd = torch.empty(R, dtype=torch.float64, device=dev)
    hc = torch.empty(R, dtype=torch.int32, device=dev)
    gh.set_cache_auto(False)      # every call derives its records (the mixed and double paths always do)
    t32 = timeit(lambda: gh.trace_cumulative_sph(rays, sf, tf, c32))
    tmx = timeit(lambda: gh.trace_cumulative_sph(rays, sf, tf, c64))
    td4 = timeit(lambda: gh.trace_cumulative_d4(rays, sd, td, cd))
    thm = timeit(lambda: gh.trace_hitcounts_f4_f64(rays, sf, tf, hc))
    thd = timeit(lambda: gh.trace_hitcounts_d4(rays, sd, td, hc))
    gh.set_cache_auto(True)
    t32c = timeit(lambda: gh.trace_cumulative_sph(rays, sf, tf, c32))     # float, scene cached
    gh.trace_status()
    print("%s: column densities float4/float %.3f ms (cached %.3f), float4/double %.3f ms, "
          "double4/double %.3f ms; hit counts float4/double %.3f ms, double4 %.3f ms"
          % (name, t32, t32c, tmx, td4, thm, thd))
    gh.trace_release(); gh.trace_release_rays()


g = torch.Generator(device=dev); g.manual_seed(3)
s = torch.rand((1_000_000, 4), generator=g, device=dev, dtype=torch.float64); s[:, 3] *= 0.1
scene("config 2", s, (0, 0, 0), (1, 1, 1), gh.uniform_random_rays(100_000, (0.5, 0.5, 0.5), 2.0, seed=1234, device=dev))
del s
n = 10_000_000
g.manual_seed(42)
s4 = torch.empty((n, 4), dtype=torch.float32, device=dev)
s4[:, :3] = torch.rand((n, 3), generator=g, device=dev); s4[:, 3] = float((3 * 48 / (4 * math.pi * n)) ** (1 / 3))
lo, hi = gh.min_max_vec4(s4); lo[3] = hi[3] = 0
r4, _ = gh.orthogonal_rays_z(1024, lo, hi, device=dev)
sd = s4.double().contiguous(); del s4
scene("bench scene", sd, lo[:3], hi[:3], r4)
