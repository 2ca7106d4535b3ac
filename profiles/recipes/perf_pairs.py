# Pair counts in separation bins (pair_counts_sph: totals only; radial_profiles_sph: per-point counts)
# on 10^6 particles queried from themselves, next to what the library offered for the same answer
# before: one range_counts_sph call per edge.  Two scenes: the tests' clustered generator (three
# cusps: at the last edge a particle sees most of its cusp) and "halos" (half a uniform background,
# half in 200 Gaussian blobs of sigma 0.01).  Edges: logarithmic from 0.04 to 4 mean interparticle
# spacings (V / n)^(1/3); 16 edges (the 16-bin tier), 17 (one past it: the 64-bin tier on almost the
# same work) and 8 (the 8-bin tier).
# Stateless calls: one warm-up of each, then REPS rounds that alternate the three versions; printed as
# median [min .. max].  Per version: call ms (device events around the call or the 16 calls: keys, sort
# and packet scan included) and kernel ms (grace_trace_last_kernel_ms: the walk alone, summed over the
# calls of the baseline).
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'grace-devel_amd'))
import numpy as np
import torch
import grace_hip as gh

dev = torch.device('cuda:0')


def spread(v):
    v = sorted(v)
    return "%.3f [%.3f .. %.3f]" % (v[len(v) // 2], v[0], v[-1])


def median(v):
    return sorted(v)[len(v) // 2]


def clustered(n, seed):
    rng = np.random.default_rng(seed)
    centres = np.array([[0.3, 0.3, 0.3], [0.7, 0.6, 0.4], [0.5, 0.5, 0.8]])
    k = rng.integers(0, 3, n)
    s = np.empty((n, 4), np.float32)
    s[:, :3] = np.clip(centres[k] + rng.normal(0.0, 0.02, (n, 3)) * rng.random((n, 1)) ** 3, 0.001, 0.999)
    s[:, 3] = (0.004 + 0.02 * rng.random(n)).astype(np.float32)
    return s


def halos(n, seed):
    rng = np.random.default_rng(seed)
    s = np.empty((n, 4), np.float32)
    s[:, :3] = rng.random((n, 3))
    c = rng.random((200, 3)) * 0.9 + 0.05
    m = n // 2
    s[:m, :3] = np.clip(c[rng.integers(0, 200, m)] + rng.normal(0.0, 0.01, (m, 3)), 0.001, 0.999)
    s[:, 3] = 0.01
    return s[rng.permutation(n)]


def once(f):
    """(call ms, kernel ms) of one f(), which returns its kernel ms."""
    a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
    a.record(); k = f(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b), k


n = 1_000_000
spacing = (1.0 / n) ** (1.0 / 3.0)
gh.enable_kernel_timing(True)
for name, scene, reps in (("halos", halos(n, 22), 5), ("clustered", clustered(n, 21), 3)):
    s = torch.from_numpy(scene).to(dev)
    t = gh.Tree(n, 32, device=dev); gh.build_tree(s, t, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    for n_edges in (16, 17, 8):
        e = np.exp(np.linspace(np.log(0.04 * spacing), np.log(4.0 * spacing), n_edges)).astype(np.float32)

        def fused():
            gh.pair_counts_sph(s, e, s, t)
            torch.cuda.synchronize()
            return gh.last_kernel_ms()

        def profiles():
            gh.radial_profiles_sph(s, e, s, t)
            torch.cuda.synchronize()
            return gh.last_kernel_ms()

        def per_edge():
            ms = 0.0
            for ek in e:
                gh.range_counts_sph(s, float(ek), s, t, counts=cnt)
                torch.cuda.synchronize()
                ms += gh.last_kernel_ms()
            return ms

        versions = (("pair_counts_sph", fused), ("range_counts_sph x %d" % n_edges, per_edge),
                    ("radial_profiles_sph", profiles))
        times = {v: ([], []) for v, _ in versions}
        for v, f in versions:
            f()
        for _ in range(reps):
            for v, f in versions:
                c, k = once(f)
                times[v][0].append(c); times[v][1].append(k)
        gh.trace_status()
        totals = gh.pair_counts_sph(s, e, s, t, check=True).cpu().numpy()
        gh.range_counts_sph(s, float(e[-1]), s, t, counts=cnt, check=True)
        assert int(totals.sum()) == int(cnt.sum(dtype=torch.int64))
        print("%s, %d edges up to %.3e: %.4g ordered pairs in range (%.1f per particle)"
              % (name, n_edges, e[-1], float(totals.sum()), float(totals.sum()) / n))
        for v, _ in versions:
            print("  %-22s %s ms call, %s ms walk" % (v, spread(times[v][0]), spread(times[v][1])))
        base = times[versions[1][0]]
        for v in (versions[0][0], versions[2][0]):
            print("  per-edge calls / %s: %.2f x (call), %.2f x (walk)"
                  % (v, median(base[0]) / median(times[v][0]), median(base[1]) / median(times[v][1])))
        sys.stdout.flush()
gh.enable_kernel_timing(False)
