# python profiles/recipes/perf_subtiles.py: the planned kernel with the plan's sub-tile layout forced
# on (set_plan_subtiles(1)) against forced off (0), perf_planned_split.py's method -- 30 calls per
# setting after 5 warm ones, grace_trace_last_kernel_ms, median; two repeats:
#   1. bench.py's frame and its shards, 16384 ... 1024 packets: the sweep behind PLAN_SUB_MIN_PACKETS
#   2. bench-shape scenes with h scaled by 1 ... 4 (4096 or 2048 packets), with the recorder's
#      steps / survivors: the sweep behind PLAN_SUB_MAX_RATIO (csrc/trace_state.hpp)
# Also prints plan_bytes() of both layouts and checks that both give the same bits.
import sys, os, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "grace-devel_amd")); sys.path.insert(0, ROOT)
import numpy as np
import torch
import grace_hip as gh
from bench import make_particles
dev = torch.device("cuda:0")
n = 10_000_000
s0 = make_particles(n, dev)
gh.enable_kernel_timing(True)
gh.set_plan_budget(12 << 30)


def median_ms(call, reps=30):
    for _ in range(5): call()
    v = []
    for _ in range(reps):
        call(); v.append(gh.last_kernel_ms())
    return statistics.median(v)


def on_against_off(rays, s, tree, label):
    out = torch.empty(len(rays), dtype=torch.float32, device=dev)
    call = lambda: gh.trace_cumulative_sph(rays, s, tree, out)
    row, bits = [], {}
    for rep in range(2):
        for mode in (0, 1):
            gh.set_plan_subtiles(mode)
            row.append("sub=%d %.4f" % (mode, median_ms(call)))
            bits[mode] = out.cpu().numpy().view(np.uint32).copy()
            if rep == 0:
                used, steps, slots = gh.plan_subtiles()
                surv = gh.plan_stats().survivors
                row.append("[sub-tiles %d, %d survivors, steps / survivors %.4f, real words %.4f, %d bytes]"
                           % (used, surv, steps / max(surv, 1), slots / max(4 * steps, 1), gh.plan_bytes()))
    print("%s: %s  same bits: %s" % (label, "  ".join(row), np.array_equal(bits[0], bits[1])), flush=True)


for scale in (1.0, 1.5, 2.0, 3.0, 4.0):
    s = s0.clone()
    s[:, 3] *= scale
    lo, hi = gh.min_max_vec4(s); lo[3] = hi[3] = 0.0
    tree = gh.Tree(n, 32, device=dev)
    gh.build_tree(s, tree, lo[:3], hi[:3])
    rays, _ = gh.orthogonal_rays_z(1024, lo, hi, device=dev)
    if scale == 1.0:
        for packets in (16384, 8192, 4096, 2048, 1024):
            on_against_off(rays[: packets * 64].contiguous(), s, tree, "%d packets" % packets)
    else:
        packets = 4096 if scale <= 2.0 else 2048
        on_against_off(rays[: packets * 64].contiguous(), s, tree, "h x %.1f, %d packets" % (scale, packets))
    gh.set_plan_subtiles(0)
    del tree
