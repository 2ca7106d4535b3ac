# Column densities with the default cubic spline against Wendland C2 (grace_hip.set_sph_kernel), in
# one process, on BASELINE config 2 (10^6 spheres, 10^5 isotropic rays) and bench.py's scene
# (10^7 particles, 1024^2 orthographic rays).  The kernel only changes the table the traversal copies
# into LDS, so the times should agree within noise.  Stateless calls, median of 5, fast and exact
# integrals; the two kernels alternate so that drift hits both.
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


def scene(name, s, lo, hi, rays):
    t = gh.Tree(len(s), 32, device=dev); gh.build_tree(s, t, lo, hi)
    c = torch.empty(len(rays), dtype=torch.float32, device=dev)
    gh.set_cache_auto(False)      # every call derives its records
    for exact in (False, True):
        gh.set_exact_integrals(exact)
        ms = {"cubic": [], "wendland_c2": []}
        for _ in range(2):
            for k in ms:
                gh.set_sph_kernel(k)
                ms[k].append(timeit(lambda: gh.trace_cumulative_sph(rays, s, t, c)))
        print("%s, %s integrals: cubic %s ms, wendland_c2 %s ms" % (
            name, "exact" if exact else "fast",
            " / ".join("%.3f" % v for v in ms["cubic"]), " / ".join("%.3f" % v for v in ms["wendland_c2"])))
    gh.set_exact_integrals(False)
    gh.set_sph_kernel("cubic")
    gh.set_cache_auto(True)
    gh.trace_status()
    gh.trace_release(); gh.trace_release_rays()


g = torch.Generator(device=dev); g.manual_seed(3)
s = torch.rand((1_000_000, 4), generator=g, device=dev); s[:, 3] *= 0.1
scene("config 2", s, (0, 0, 0), (1, 1, 1), gh.uniform_random_rays(100_000, (0.5, 0.5, 0.5), 2.0, seed=1234, device=dev))
del s
n = 10_000_000
g.manual_seed(42)
s4 = torch.empty((n, 4), dtype=torch.float32, device=dev)
s4[:, :3] = torch.rand((n, 3), generator=g, device=dev); s4[:, 3] = float((3 * 48 / (4 * math.pi * n)) ** (1 / 3))
lo, hi = gh.min_max_vec4(s4); lo[3] = hi[3] = 0
r4, _ = gh.orthogonal_rays_z(1024, lo, hi, device=dev)
scene("bench scene", s4, lo[:3], hi[:3], r4)
