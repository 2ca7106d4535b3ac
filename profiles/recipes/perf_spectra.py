# Sightline spectra (trace_spectra_sph):
#   python perf_spectra.py            runs the two steps below one after the other, each in a child
#       process of its own under a time limit; the first step that fails (or runs out of time)
#       ends the script with its status, and nothing more is started.
#   python perf_spectra.py cfg3       BASELINE config 3's scene (one observer, 49152 HEALPix rays
#       through a 128^3 snapshot)
#   python perf_spectra.py bench      bench.py's scene (10^7 particles) with 4096 of its 1024^2
#       orthographic rays (every 256th)
# Each step, for n_bins 256 and 2048 and C 1 and 4, on a periodic grid over one Hubble length of
# the ray (velocities of +-5 % of it, Doppler widths log-uniform between 1/1000 and 1/100 of it, so
# windows of 3 to 31 bins at 256 bins and 25 to 246 at 2048): the fused call's time (median of 5,
# stats hook off), its phases from the stats hook (ordered_enable_stats, which synchronises), and
# the chain a caller would otherwise write: trace_sph, sort_by_distance, then per channel the same
# terms in torch (every hit repeated over its window, erf at both edges of every bin, fp64) and an
# index_add_ onto the [ray, channel, bin] array (atomics: not reproducible), in slices of at most
# 2^27 terms so that the temporaries stay bounded.  The chain is timed once after one warm-up run.
import sys, os, math, subprocess
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEPS = (("cfg3", 550), ("bench", 550))

if len(sys.argv) < 2:
    for step, limit in STEPS:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), step], timeout=limit).returncode
        except subprocess.TimeoutExpired:
            print("step %s ran out of its %d s" % (step, limit)); sys.exit(124)
        if rc != 0:
            print("step %s failed with status %d" % (step, rc)); sys.exit(rc if rc > 0 else 1)
    sys.exit(0)

sys.path.insert(0, os.path.join(ROOT, 'grace-devel_amd'))
import torch, numpy as np, grace_hip as gh
dev = torch.device('cuda:0')
which = sys.argv[1]
TERMS = 1 << 27


def timeit(f, reps=5):
    f(); torch.cuda.synchronize(); ts = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def stats_line(f):
    gh.ordered_enable_stats(True); f(); st = gh.ordered_last_stats(); gh.ordered_enable_stats(False)
    return ("batches %d, hits %d, rays wave/block/global %d/%d/%d, count %.3f ms, per-hit walks %.3f ms, "
            "fused kernels %.3f ms" % (st["batches"], st["total_hits"], st["rays_wave"], st["rays_block"],
                                       st["rays_global"], st["ms_count"], st["ms_trace"], st["ms_composite"]))


def fields(n, C, span):
    g = torch.Generator(device=dev); g.manual_seed(7)
    amount = torch.rand((n, C), generator=g, device=dev) + 0.25
    width = span / 1000.0 * 10.0 ** torch.rand((n, C), generator=g, device=dev)
    vel = (torch.rand((n, 3), generator=g, device=dev) - 0.5) * 0.1 * span
    return amount.contiguous(), width.contiguous(), vel.contiguous()


def chain(rays, s, tree, amount, width, vel, v0, dv, n_bins, hubble):
    R, C = len(rays), amount.shape[1]
    off, idx, integ, dist = gh.trace_sph(rays, s, tree)
    gh.sort_by_distance(dist, off, idx, integ)
    i64 = idx.long()
    counts = torch.diff(torch.cat([off.long(), torch.tensor([len(idx)], device=dev)]))
    seg = torch.repeat_interleave(torch.arange(R, device=dev), counts)
    v = hubble * dist.double() + (vel[i64].double() * rays[seg, :3].double()).sum(1)
    out = torch.zeros(R * C * n_bins, dtype=torch.float64, device=dev)
    for c in range(C):
        N = amount[i64, c].double() * integ.double() / dv
        b = width[i64, c].double()
        lo = torch.floor((v - 6 * b - v0) / dv); hi = torch.floor((v + 6 * b - v0) / dv)
        ln = (hi - lo).long() + 1
        cum = torch.cumsum(ln, 0)
        h0, done = 0, 0
        while h0 < len(ln):
            h1 = int(torch.searchsorted(cum, torch.tensor(done + TERMS, device=dev), right=True))
            h1 = min(max(h1, h0 + 1), len(ln))
            sl = slice(h0, h1)
            rep = torch.repeat_interleave(torch.arange(h0, h1, device=dev), ln[sl])
            u = lo[rep] + (torch.arange(len(rep), device=dev) - (cum[rep] - ln[rep] - done)).double()
            P = 0.5 * (torch.erf(((v0 + (u + 1) * dv) - v[rep]) / b[rep]) - torch.erf(((v0 + u * dv) - v[rep]) / b[rep]))
            out.index_add_(0, (seg[rep] * C + c) * n_bins + torch.remainder(u, n_bins).long(), N[rep] * P)
            done = int(cum[h1 - 1]); h0 = h1
    return out.reshape(R, C, n_bins)


def measure(name, rays, s, tree, hubble, span):
    R = len(rays)
    for n_bins in (256, 2048):
        for C in (1, 4):
            amount, width, vel = fields(len(s), C, span)
            v0, dv = -0.1 * span, 1.2 * span / n_bins
            tau = torch.empty((R, C, n_bins), device=dev); col = torch.empty((R, C), device=dev)
            fused = lambda: gh.trace_spectra_sph(rays, s, tree, amount, width, vel, v0, dv, n_bins, periodic=True,
                                                 hubble=hubble, tau=tau, column=col)
            t_f = timeit(fused)
            t_c = timeit(lambda: chain(rays, s, tree, amount, width, vel, v0, dv, n_bins, hubble), 1)
            ref = chain(rays, s, tree, amount, width, vel, v0, dv, n_bins, hubble)
            rel = float((ref - tau.double()).abs().max() / ref.abs().max())
            cons = float(((dv * tau.double().sum(2) - col.double()).abs() / col.double().clamp_min(1e-300)).max())
            del ref
            print("%s, n_bins=%d, C=%d: fused %.3f ms, chain %.3f ms, ratio %.2f (max difference / max tau %.1e; "
                  "conservation %.1e of the column)" % (name, n_bins, C, t_f, t_c, t_c / t_f, rel, cons))
            print("%s, n_bins=%d, C=%d: %s" % (name, n_bins, C, stats_line(fused)))
            sys.stdout.flush()


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
    measure("config 3", rays, s, tree, 100.0, 100.0 * length)
elif which == "bench":
    n = 10_000_000
    g = torch.Generator(device=dev); g.manual_seed(42)
    s = torch.empty((n, 4), dtype=torch.float32, device=dev)
    s[:, :3] = torch.rand((n, 3), generator=g, device=dev); s[:, 3] = float((3 * 48 / (4 * math.pi * n)) ** (1 / 3))
    lo, hi = gh.min_max_vec4(s); lo[3] = hi[3] = 0
    tree = gh.Tree(n, 32, device=dev); gh.build_tree(s, tree, lo[:3], hi[:3])
    rays, _ = gh.orthogonal_rays_z(1024, lo, hi, device=dev)
    rays = rays[::256].contiguous()
    measure("bench scene, 4096 rays", rays, s, tree, 100.0, 100.0 * float(rays[0, 6]))
else:
    sys.exit("unknown step %r" % which)
gh.trace_status()
