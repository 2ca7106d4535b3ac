# python profiles/recipes/perf_plan.py [particles] [side]: the calls around a packet plan on the
# bench workload (bench.py's particles, side^2 orthographic rays), each timed on its own with the
# device idle before and after: the cold call, the first repeated call (cache fill), the call that
# records the plan, the steady state, a call where only the rays repeat (another scene) and one
# where only the scene repeats (another ray batch); then the plan's size.  Works with a library
# from before the plan (the plan lines then say "n/a"), so two libraries can be compared.
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "grace-devel_amd")); sys.path.insert(0, ROOT)
import torch
import grace_hip as gh
from bench import make_particles

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
side = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
dev = torch.device("cuda:0")
has_plan = hasattr(gh._lib, "grace_trace_last_plan_used")


def scene(seed):
    s = make_particles(n, dev, seed)
    lo, hi = gh.min_max_vec4(s); lo[3] = hi[3] = 0.0
    tree = gh.Tree(n, 32, device=dev)
    gh.build_tree(s, tree, lo[:3], hi[:3])
    return s, tree, lo, hi


s1, t1, lo, hi = scene(42)
s2, t2, _, _ = scene(43)      # another scene of the same size
rays1, _ = gh.orthogonal_rays_z(side, lo, hi, device=dev)
rays2 = rays1.clone(); rays2[:, 3] += 0.25 * float(hi[0] - lo[0]) / side
out = torch.empty(len(rays1), dtype=torch.float32, device=dev)


def call(rays, s, t):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gh.trace_cumulative_sph(rays, s, t, out)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    return ms, (gh.last_plan_used() if has_plan else "n/a")


def report(name, ms_used):
    print("%-44s %8.3f ms   plan used: %s" % (name, ms_used[0], ms_used[1]), flush=True)


call(rays1, s1, t1); gh.trace_release(); gh.trace_release_rays()      # workspace grown, nothing cached
for rep in range(3):
    report("cold call (first sight)", call(rays1, s1, t1))
    report("first repeated call (caches filled)", call(rays1, s1, t1))
    report("second repeated call (plan recorded)", call(rays1, s1, t1))
    for _ in range(3):
        report("steady state", call(rays1, s1, t1))
    if has_plan:
        print("plan: %.1f MB" % (gh.plan_bytes() / 1e6), flush=True)
    report("only the rays repeat (other scene)", call(rays1, s2, t2))
    report("only the rays repeat (first scene again)", call(rays1, s1, t1))
    report("only the scene repeats (other rays)", call(rays2, s1, t1))
    report("only the scene repeats (first rays again)", call(rays1, s1, t1))
    gh.trace_release(); gh.trace_release_rays()
