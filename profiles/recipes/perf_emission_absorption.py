# Emission-absorption integrals (trace_emission_absorption_sph):
#   python perf_emission_absorption.py cfg3    BASELINE config 3's scene (one source, HEALPix rays
#       through a 128^3 snapshot): the fused call against the four-call chain doing the same job
#       (trace_sph, sort_by_distance, weighted_exclusive_segmented_scan, a torch reduction), C = 1
#       and C = 4, median of 5 after warm-up.
#   python perf_emission_absorption.py bench   bench.py's scene (10^7 particles, 1024^2 orthographic
#       rays; no chain to compare with): total time, phases and batches for three budgets.
# The phases and the rays per tier come from the stats hook (ordered_enable_stats), which
# synchronises: totals are timed with the hook off.
import sys, os, math
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'grace-devel_amd'))
import torch, numpy as np, grace_hip as gh
dev = torch.device('cuda:0')
which = sys.argv[1] if len(sys.argv) > 1 else "cfg3"


def timeit(f, reps=5):
    f(); torch.cuda.synchronize(); ts = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def coefficients(s, C):
    g = torch.Generator(device=dev); g.manual_seed(7)
    e = torch.rand((len(s), C), generator=g, device=dev) + 0.25
    k = 1e-3 * s[:, 3] ** 2 * (0.5 + torch.rand(len(s), generator=g, device=dev))
    return (e if C > 1 else e[:, 0].contiguous()), k.contiguous()


def stats_line(f):
    gh.ordered_enable_stats(True); f(); st = gh.ordered_last_stats(); gh.ordered_enable_stats(False)
    return ("batches %d, hits %d, rays wave/block/global %d/%d/%d, count %.3f ms, per-hit walks %.3f ms, "
            "fused kernels %.3f ms, frame %.0f MiB" % (
                st["batches"], st["total_hits"], st["rays_wave"], st["rays_block"], st["rays_global"],
                st["ms_count"], st["ms_trace"], st["ms_composite"], st["frame_bytes"] / 2 ** 20))


if which == "cfg3":
    n_side = 128; n = n_side ** 3
    g = torch.Generator(device=dev); g.manual_seed(42)
    grid = torch.stack(torch.meshgrid(*[torch.arange(n_side, device=dev)] * 3, indexing="ij"), -1).reshape(-1, 3).float()
    pos = (grid + torch.rand((n, 3), generator=g, device=dev)) / n_side
    h = (3 * 48 / (4 * math.pi * n)) ** (1 / 3)
    s = torch.cat([pos, torch.full((n, 1), h, device=dev)], 1).contiguous()
    lo, hi = gh.min_max_vec4(s)
    tree = gh.Tree(n, 32, device=dev); gh.build_tree(s, tree, lo[:3], hi[:3])
    centre = (lo[:3] + hi[:3]) / 2; length = float(np.linalg.norm(hi[:3] - lo[:3]))
    rays = gh.healpix_rays(64, centre, length, device=dev)
    R = len(rays)
    for C in (1, 4):
        e, k = coefficients(s, C)
        out = torch.empty((R, C) if C > 1 else (R,), device=dev); tau = torch.empty(R, device=dev)
        fused = lambda: gh.trace_emission_absorption_sph(rays, s, tree, e, k, out=out, tau=tau)
        e2 = e.reshape(n, C)

        def chain():
            # the caller's assembly: per-hit trace, per-ray sort, tau in front of every hit by the
            # weighted segmented scan, then the formula and a per-ray sum in torch (fp32 scan)
            off, idx, integ, dist = gh.trace_sph(rays, s, tree)
            gh.sort_by_distance(dist, off, idx, integ)
            tau_k = torch.empty_like(integ)
            gh.weighted_exclusive_segmented_scan(integ, k, idx, off, tau_k)
            a = (k[idx.long()] * integ).double()
            f = integ.double() * torch.where(a > 0, -torch.expm1(-a) / a, torch.ones_like(a)) * torch.exp(-tau_k.double())
            seg = torch.repeat_interleave(torch.arange(R, device=dev), torch.diff(
                torch.cat([off.long(), torch.tensor([len(idx)], device=dev)])))
            return torch.zeros((R, C), dtype=torch.float64, device=dev).index_add_(
                0, seg, e2[idx.long()].double() * f[:, None]).float()
        t_f, t_c = timeit(fused), timeit(chain)
        rel = float(((chain().reshape(out.shape) - out).abs() / out.abs().clamp_min(1e-30)).max())
        print("config 3, C=%d: fused %.3f ms, four-call chain %.3f ms, ratio %.2f (max rel. difference %.1e; "
              "the chain scans tau in fp32 and breaks ties by traversal order)" % (C, t_f, t_c, t_c / t_f, rel))
    print("config 3:", stats_line(fused))
else:
    n = 10_000_000
    g = torch.Generator(device=dev); g.manual_seed(42)
    s = torch.empty((n, 4), dtype=torch.float32, device=dev)
    s[:, :3] = torch.rand((n, 3), generator=g, device=dev); s[:, 3] = float((3 * 48 / (4 * math.pi * n)) ** (1 / 3))
    lo, hi = gh.min_max_vec4(s); lo[3] = hi[3] = 0
    tree = gh.Tree(n, 32, device=dev); gh.build_tree(s, tree, lo[:3], hi[:3])
    rays, _ = gh.orthogonal_rays_z(1024, lo, hi, device=dev)
    e, k = coefficients(s, 1)
    out = torch.empty(len(rays), device=dev); tau = torch.empty(len(rays), device=dev)
    fused = lambda: gh.trace_emission_absorption_sph(rays, s, tree, e, k, out=out, tau=tau)
    for budget in (256 << 20, 1 << 30, 4 << 30):
        gh.set_ordered_budget(budget)
        print("bench scene, budget %d MiB: total %.1f ms; %s" % (budget >> 20, timeit(fused, 3), stats_line(fused)))
    gh.set_ordered_budget(0)
gh.trace_status()
