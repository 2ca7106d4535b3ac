# Gravity within groups (gravity_group_moments_sph, gravity_groups_sph): speed on the GPU.
#
#   python profiles/recipes/gravity_groups.py
# The scene of gravity_points.py: 10^6 particles of the clustered generator, max_per_leaf 32, unit masses,
# potentials at all centres (eps 1e-4), theta 0.5.  One warm-up of each call, then REPS rounds; device events
# around the call (keys, sort and packet scan included) and grace_trace_last_kernel_ms (the walk alone), printed
# as median [min .. max].  In one run:
#   1. gravity_sph, the open walk, to set beside the figure of profiles/gravity_points_mi355x.txt;
#   2. gravity_groups_sph with the label 0 on every particle and point: the same terms, so the ratio to 1. is
#      the cost of the label tests and of staging the labels;
#   3. a catalogue call: labels = group_of of fof_groups_sph(min_members 32) over fof_labels_sph at the linking
#      length B, the points are all particles with their own labels; ms per call, terms per point and per second;
#   4. the per-group recipe of INTEGRATION.md (gather, a tree of the group's own, moments, walk) over the
#      PER_GROUP largest groups of the same catalogue, wall time with a synchronisation per group as the recipe
#      has it (it reads the result), and an extrapolation to all groups: the measured time of those groups plus,
#      for every further group, the median time of the ten smallest measured ones;
#   5. gravity_group_moments_sph beside gravity_moments_sph.
# The clustered scene is three haloes, so its catalogue is three large groups and a small one: 3. and 4. measure
# the walk inside large groups, not the host loop over a catalogue of 10^4 groups that the call replaces.
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ('grace-devel_amd', 'oracle', 'tests'):
    sys.path.insert(0, os.path.join(ROOT, p))

REPS = 5
B = 0.002                 # 0.2 of the mean separation of 10^6 particles in the unit box
MIN_MEMBERS = 32
PER_GROUP = 100
THETA, EPS = 0.5, 1e-4


def spread(v):
    v = sorted(v)
    return "%.3f [%.3f .. %.3f]" % (v[len(v) // 2], v[0], v[-1])


def median(v):
    return sorted(v)[len(v) // 2]


def run(title, scene, open_walk):
    import torch
    import grace_hip as gh
    dev = torch.device('cuda:0')
    n = len(scene)
    s = torch.from_numpy(scene).to(dev)
    t = gh.Tree(n, 32, device=dev)
    gh.build_tree(s, t, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    masses = torch.ones(n, dtype=torch.float32, device=dev)
    moments = torch.empty((t.n_nodes, 12), dtype=torch.float32, device=dev)
    gmoments = torch.empty((t.n_nodes, 12), dtype=torch.float32, device=dev)
    ranges = torch.empty((t.n_nodes, 2), dtype=torch.int32, device=dev)
    out = torch.empty((n, 4), dtype=torch.float64, device=dev)
    cnt = torch.empty((n, 2), dtype=torch.int32, device=dev)
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

    def terms_line(name, call, walk):
        gh.trace_status()
        tot = cnt.sum(dim=0, dtype=torch.int64).cpu().numpy()
        print("  %-34s %s ms call, %s ms walk; %.1f node + %.1f particle terms per point, %.3e terms/s (walk)"
              % (name, spread(call), spread(walk), tot[0] / n, tot[1] / n, float(tot.sum()) / (median(walk) * 1e-3)))
        return tot

    print("%s, %d particles, max_per_leaf 32, %d nodes, theta %.1f, eps %g" % (title, n, t.n_nodes, THETA, EPS))
    if open_walk:
        open_and_one_label(gh, s, t, masses, moments, gmoments, ranges, out, cnt, timed, terms_line)
    catalogue(gh, s, t, masses, gmoments, ranges, out, cnt, timed, terms_line)
    gh.enable_kernel_timing(False)


def open_and_one_label(gh, s, t, masses, moments, gmoments, ranges, out, cnt, timed, terms_line):
    import torch
    n, dev = len(s), s.device
    # 5. the moments
    zeros = torch.zeros(n, dtype=torch.int32, device=dev)
    call_m, _ = timed(lambda: gh.gravity_moments_sph(s, masses, t, moments), kernel=False)
    call_g, _ = timed(lambda: gh.gravity_group_moments_sph(s, masses, zeros, t, gmoments, ranges), kernel=False)
    print("  %-34s %s ms call" % ("gravity_moments_sph", spread(call_m)))
    print("  %-34s %s ms call (ratio of medians %.2f)" % ("gravity_group_moments_sph, one label", spread(call_g),
                                                          median(call_g) / median(call_m)))
    assert torch.equal(moments.view(torch.int32), gmoments.view(torch.int32))
    # 1. the open walk
    call_o, walk_o = timed(lambda: gh.gravity_sph(s, s, masses, t, moments, theta=THETA, eps=EPS, out=out, counts=cnt))
    tot_o = terms_line("gravity_sph", call_o, walk_o)
    ref = out.clone()
    # 2. one label everywhere
    call_1, walk_1 = timed(lambda: gh.gravity_groups_sph(s, zeros, s, masses, zeros, t, gmoments, ranges, theta=THETA,
                                                         eps=EPS, out=out, counts=cnt))
    tot_1 = terms_line("gravity_groups_sph, one label", call_1, walk_1)
    assert torch.equal(out.view(torch.int64), ref.view(torch.int64)) and (tot_1 == tot_o).all()
    print("  %-34s call %.3f, walk %.3f (ratios of medians)" % ("  one label / open", median(call_1) / median(call_o),
                                                                median(walk_1) / median(walk_o)))


def catalogue(gh, s, t, masses, gmoments, ranges, out, cnt, timed, terms_line):
    import torch
    n, dev = len(s), s.device
    # 3. the catalogue
    labels = gh.fof_labels_sph(s, t, B, check=True)
    group_of, sizes, offsets, members = gh.fof_groups_sph(labels, MIN_MEMBERS)
    ng = len(sizes)
    in_groups = int((group_of >= 0).sum().item())
    top = torch.sort(sizes, descending=True).values[:5].tolist()
    print("  catalogue: fof_labels_sph b %.4f, %d groups of >= %d members holding %d particles; largest %s"
          % (B, ng, MIN_MEMBERS, in_groups, top))
    call_gm, _ = timed(lambda: gh.gravity_group_moments_sph(s, masses, group_of, t, gmoments, ranges), kernel=False)
    print("  %-34s %s ms call" % ("gravity_group_moments_sph, catalogue", spread(call_gm)))
    call_c, walk_c = timed(lambda: gh.gravity_groups_sph(s, group_of, s, masses, group_of, t, gmoments, ranges,
                                                         theta=THETA, eps=EPS, out=out, counts=cnt))
    terms_line("gravity_groups_sph, catalogue", call_c, walk_c)
    pure = int((ranges[:, 0] == ranges[:, 1]).sum().item())
    empty = int((ranges[:, 1] < 0).sum().item())
    print("    nodes: %d of one label, %d without a label, %d mixed" % (pure, empty, t.n_nodes - pure - empty))
    phi_cat = out[:, 3].clone()
    # 4. the per-group recipe over the largest groups
    order = torch.argsort(sizes, descending=True)[:PER_GROUP].tolist()
    lo, hi = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)

    def one_group(g):
        idx = members[offsets[g]:offsets[g + 1]].long()
        gs = s[idx].clone()
        gtree, gperm = gh.build_tree(gs, gh.Tree(len(gs), 8, device=dev), lo, hi, want_perm=True)
        gm = masses[idx][gperm.long()].contiguous()
        mom = gh.gravity_moments_sph(gs, gm, gtree)
        o, _ = gh.gravity_sph(gs[:, :3].contiguous(), gs, gm, gtree, mom, theta=THETA, eps=EPS)
        return idx[gperm.long()], float(o[:, 3].min().item())      # (the recipe reads its result: one sync per group)

    one_group(order[-1]); torch.cuda.synchronize()                  # warm-up
    per = []
    for g in order:
        t0 = time.perf_counter()
        one_group(g)
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) * 1e3)
    small = median(per[-10:])
    total = sum(per)
    print("  per-group recipe, %d largest groups (sizes %d .. %d): %.1f ms in all, measured; the ten smallest %.3f ms each"
          % (len(order), int(sizes[order[0]]), int(sizes[order[-1]]), total, small))
    print("    extrapolated to all %d groups: %.1f ms (measured %.1f + %d x %.3f); the catalogue call with its moments: %.1f ms"
          % (ng, total + max(ng - len(order), 0) * small, total, max(ng - len(order), 0), small,
             median(call_c) + median(call_gm)))
    # the same physics: the most bound member of the largest group, by both routes (theta > 0: two trees, two sums)
    idx, phi_min = one_group(order[0])
    print("    largest group: min phi %.6e by its own tree, %.6e by the catalogue call" % (phi_min, float(phi_cat[idx].min().item())))


if __name__ == "__main__":
    import gravity_cases as G
    run("clustered", G.clustered_scene(1_000_000, 21), True)
