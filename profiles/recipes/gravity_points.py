# Tree gravity (gravity_moments_sph, gravity_sph): accuracy on the CPU and speed on the GPU.
#
#   python profiles/recipes/gravity_points.py accuracy
# No GPU.  The contract's NumPy restatement (tests/gravity_cases.py) on the CPU oracle's ALBVH against an fp64
# direct sum: 4000 particles of the tests' random and clustered generators, unit masses, max_per_leaf 8,
# eps 0, the potential and acceleration at 1000 of the centres.  Per theta: the median and the maximum of
# |a - a_ref| / |a_ref| and of |phi - phi_ref| / |phi_ref|, and the mean node and particle terms per point.
#
#   python profiles/recipes/gravity_points.py speed
# 10^6 particles of the clustered generator, max_per_leaf 32, potentials at all centres (eps 1e-4).  One
# warm-up of each call, then REPS rounds; device events around the call (keys, sort and packet scan
# included) and grace_trace_last_kernel_ms (the walk alone), printed as median [min .. max].  The
# moments pass on its own, the walk at theta 0.5 and 0.7 with its terms per point and per second, and
# range_counts_sph on the same scene at the radius whose pair count is closest to the walk's term
# count at theta 0.5: the pairs it tests per second are what this tree's traversal does when the
# pair term is one compare.
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ('grace-devel_amd', 'oracle', 'tests'):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np

REPS = 5


def spread(v):
    v = sorted(v)
    return "%.3f [%.3f .. %.3f]" % (v[len(v) // 2], v[0], v[-1])


def accuracy():
    import gravity_cases as G
    n, mpl, m_pts = 4000, 8, 1000
    print("accuracy: %d particles, unit masses, max_per_leaf %d, eps 0, %d centres; restatement vs fp64 direct sum"
          % (n, mpl, m_pts))
    print("%-10s %5s  %10s %10s  %10s %10s  %8s %8s" % ("scene", "theta", "a median", "a max", "phi median",
                                                        "phi max", "nodes", "parts"))
    for name, gen in (("random", G.random_scene), ("clustered", G.clustered_scene)):
        s, nodes, leaves, root = G.cpu_tree(gen(n, 5), mpl)
        masses = np.ones(n, np.float32)
        rec = G.moments(nodes, leaves, root, s, masses)
        pts = s[np.random.default_rng(1).choice(n, m_pts, replace=False), :3]
        ref = G.fp64_direct(pts, s, masses, 0.0)
        for theta in (0.0, 0.3, 0.5, 0.7, 1.0):
            out, cnt = G.walk(nodes, leaves, root, s, masses, rec, pts, theta, 0.0)
            ea = np.linalg.norm(out[:, :3] - ref[:, :3], axis=1) / np.linalg.norm(ref[:, :3], axis=1)
            ep = np.abs(out[:, 3] - ref[:, 3]) / np.abs(ref[:, 3])
            print("%-10s %5.1f  %10.2e %10.2e  %10.2e %10.2e  %8.1f %8.1f"
                  % (name, theta, np.median(ea), ea.max(), np.median(ep), ep.max(), cnt[:, 0].mean(), cnt[:, 1].mean()))


def speed():
    import torch
    import grace_hip as gh
    import gravity_cases as G
    dev = torch.device('cuda:0')
    n = 1_000_000
    s = torch.from_numpy(G.clustered_scene(n, 21)).to(dev)
    t = gh.Tree(n, 32, device=dev)
    gh.build_tree(s, t, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    masses = torch.ones(n, dtype=torch.float32, device=dev)
    moments = torch.empty((t.n_nodes, 12), dtype=torch.float32, device=dev)
    out = torch.empty((n, 4), dtype=torch.float64, device=dev)
    cnt = torch.empty((n, 2), dtype=torch.int32, device=dev)
    rc = torch.empty(n, dtype=torch.int32, device=dev)
    gh.enable_kernel_timing(True)

    def timed(f, kernel=True):
        f(); torch.cuda.synchronize()
        call, walk = [], []
        for _ in range(REPS):
            a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
            a.record(); f(); b.record(); torch.cuda.synchronize()
            call.append(a.elapsed_time(b))
            if kernel:
                walk.append(gh.last_kernel_ms())
        return call, walk

    call, _ = timed(lambda: gh.gravity_moments_sph(s, masses, t, moments), kernel=False)
    print("clustered, %d particles, max_per_leaf 32, %d nodes" % (n, t.n_nodes))
    print("  gravity_moments_sph          %s ms call" % spread(call))
    terms_05 = None
    for theta in (0.5, 0.7):
        call, walk = timed(lambda: gh.gravity_sph(s, s, masses, t, moments, theta=theta, eps=1e-4, out=out, counts=cnt))
        gh.trace_status()
        tot = cnt.sum(dim=0, dtype=torch.int64).cpu().numpy()
        terms = float(tot.sum())
        terms_05 = terms if terms_05 is None else terms_05
        w = sorted(walk)[len(walk) // 2]
        print("  gravity_sph theta %.1f        %s ms call, %s ms walk; %.1f node + %.1f particle terms per point, "
              "%.3e terms/s (walk)" % (theta, spread(call), spread(walk), tot[0] / n, tot[1] / n, terms / (w * 1e-3)))
    # the yardstick: the range query whose pair count is closest to the walk's term count at theta 0.5
    best = None
    for r in (0.0005, 0.001, 0.002, 0.004, 0.008):
        gh.range_counts_sph(s, r, s, t, counts=rc, check=True)
        pairs = float(rc.sum(dtype=torch.int64).item())
        if best is None or abs(np.log(pairs / terms_05)) < abs(np.log(best[1] / terms_05)):
            best = (r, pairs)
    r, pairs = best
    call, walk = timed(lambda: gh.range_counts_sph(s, r, s, t, counts=rc))
    w = sorted(walk)[len(walk) // 2]
    print("  range_counts_sph r %.4f    %s ms call, %s ms walk; %.1f pairs in range per point, %.3e pairs/s (walk)"
          % (r, spread(call), spread(walk), pairs / n, pairs / (w * 1e-3)))
    gh.enable_kernel_timing(False)


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "accuracy":
        accuracy()
    elif len(sys.argv) == 2 and sys.argv[1] == "speed":
        speed()
    else:
        sys.exit("usage: gravity_points.py accuracy | speed")
