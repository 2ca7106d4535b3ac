# Absorption deposits (trace_absorption_deposit_sph):
#   python perf_absorption_deposit.py cfg3 [label]   BASELINE config 3's scene (one source, HEALPix
#       rays through a 128^3 snapshot): the fused call against the chain a caller would otherwise
#       write (trace_sph, sort_by_distance, weighted_exclusive_segmented_scan per channel, the
#       formula and index_add_ in torch), C = 1 and C = 4, median of 5 after warm-up.
#   python perf_absorption_deposit.py bench [label]  bench.py's scene (10^7 particles, 1024^2
#       orthographic rays; no chain to compare with): total time, phases and batches for three
#       budgets at C = 1 and C = 4, beside trace_emission_absorption_sph (C = 1) from the same job.
# The phases and the rays per tier come from the stats hook (ordered_enable_stats), which
# synchronises: totals are timed with the hook off.  `label` is printed in front of every line:
# it names the build when the library is a timing-only one (-DGRACE_DEPOSIT_TIMING_NO_ADD: the
# fused kernel without its atomic add, wrong results, to price the atomics).
import sys, os, math
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'grace-devel_amd'))
import torch, numpy as np, grace_hip as gh
dev = torch.device('cuda:0')
which = sys.argv[1] if len(sys.argv) > 1 else "cfg3"
label = (sys.argv[2] + ": ") if len(sys.argv) > 2 else ""


def timeit(f, reps=5):
    f(); torch.cuda.synchronize(); ts = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def coefficients(s, n_rays, C):
    g = torch.Generator(device=dev); g.manual_seed(7)
    L = torch.rand((n_rays, C), generator=g, device=dev) + 0.25
    k = 1e-3 * s[:, 3:4] ** 2 * (0.5 + torch.rand((len(s), C), generator=g, device=dev))
    return L.contiguous(), k.contiguous()


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
        L, k = coefficients(s, R, C)
        dep = torch.empty((n, C), dtype=torch.float64, device=dev); tr = torch.empty((R, C), device=dev)
        fused = lambda: gh.trace_absorption_deposit_sph(rays, s, tree, L, k, deposit=dep, transmitted=tr)
        kc = [k[:, c].contiguous() for c in range(C)]

        def chain():
            # the caller's assembly: per-hit trace, per-ray sort, tau in front of every hit by the
            # weighted segmented scan (fp32, once per channel), then the formula and a scatter-add
            # onto the spheres in torch (fp64 index_add_: atomics, not reproducible)
            off, idx, integ, dist = gh.trace_sph(rays, s, tree)
            gh.sort_by_distance(dist, off, idx, integ)
            i64 = idx.long()
            seg = torch.repeat_interleave(torch.arange(R, device=dev), torch.diff(
                torch.cat([off.long(), torch.tensor([len(idx)], device=dev)])))
            out = torch.zeros((n, C), dtype=torch.float64, device=dev)
            for c in range(C):
                tau_k = torch.empty_like(integ)
                gh.weighted_exclusive_segmented_scan(integ, kc[c], idx, off, tau_k)
                a = (kc[c][i64] * integ).double()
                out[:, c].index_add_(0, i64, L[seg, c].double() * torch.exp(-tau_k.double()) * -torch.expm1(-a))
            return out
        t_f, t_c = timeit(fused), timeit(chain)
        ref = chain()
        rel = float(((ref - dep).abs().max(0).values / ref.abs().max(0).values).max())
        print(label + "config 3, C=%d: fused %.3f ms, chain %.3f ms, ratio %.2f (max difference / max deposit %.1e; "
              "the chain scans tau in fp32 and breaks ties by traversal order)" % (C, t_f, t_c, t_c / t_f, rel))
        print(label + "config 3, C=%d: %s" % (C, stats_line(fused)))
else:
    n = 10_000_000
    g = torch.Generator(device=dev); g.manual_seed(42)
    s = torch.empty((n, 4), dtype=torch.float32, device=dev)
    s[:, :3] = torch.rand((n, 3), generator=g, device=dev); s[:, 3] = float((3 * 48 / (4 * math.pi * n)) ** (1 / 3))
    lo, hi = gh.min_max_vec4(s); lo[3] = hi[3] = 0
    tree = gh.Tree(n, 32, device=dev); gh.build_tree(s, tree, lo[:3], hi[:3])
    rays, _ = gh.orthogonal_rays_z(1024, lo, hi, device=dev)
    R = len(rays)
    e = torch.rand(n, device=dev) + 0.25
    out = torch.empty(R, device=dev); tau = torch.empty(R, device=dev)
    for budget in (256 << 20, 1 << 30, 4 << 30):
        gh.set_ordered_budget(budget)
        for C in (1, 4):
            L, k = coefficients(s, R, C)
            dep = torch.empty((n, C), dtype=torch.float64, device=dev); tr = torch.empty((R, C), device=dev)
            fused = lambda: gh.trace_absorption_deposit_sph(rays, s, tree, L, k, deposit=dep, transmitted=tr)
            print(label + "bench scene, budget %d MiB, deposit C=%d: total %.1f ms; %s" % (
                budget >> 20, C, timeit(fused, 3), stats_line(fused)))
            if C == 1:
                k1 = k[:, 0].contiguous()
                ea = lambda: gh.trace_emission_absorption_sph(rays, s, tree, e, k1, out=out, tau=tau)
                print(label + "bench scene, budget %d MiB, emission-absorption C=1: total %.1f ms; %s" % (
                    budget >> 20, timeit(ea, 3), stats_line(ea)))
    gh.set_ordered_budget(0)
gh.trace_status()
