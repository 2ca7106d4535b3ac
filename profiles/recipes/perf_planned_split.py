# python profiles/recipes/perf_planned_split.py [fast|exact|w4|w4exact]: the planned kernel's time
# per packet split on bench.py's frame and its shards -- 16384 ... 1024 packets; K = automatic
# (planned_split, csrc/trace_state.hpp), 1, 2, 4, 8 through set_packet_split; 30 calls per setting
# after 5 warm ones, grace_trace_last_kernel_ms, median; two repeats.  The sweep behind
# planned_split's thresholds.  fast (default): the unweighted fast integral, bench.py's;
# exact: the exact integral; w4 / w4exact: four weighted channels.  Run it under with_lib.py to
# compare two libraries.
import sys, os, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "grace-devel_amd")); sys.path.insert(0, ROOT)
import torch
import grace_hip as gh
from bench import make_particles
mode = sys.argv[1] if len(sys.argv) > 1 else "fast"
assert mode in ("fast", "exact", "w4", "w4exact")
dev = torch.device("cuda:0")
n = 10_000_000
s = make_particles(n, dev)
lo, hi = gh.min_max_vec4(s); lo[3] = hi[3] = 0.0
tree = gh.Tree(n, 32, device=dev)
gh.build_tree(s, tree, lo[:3], hi[:3])
rays, _ = gh.orthogonal_rays_z(1024, lo, hi, device=dev)
gh.enable_kernel_timing(True)
gh.set_exact_integrals(mode.endswith("exact"))
w = torch.rand((n, 4), dtype=torch.float32, device=dev) if mode.startswith("w4") else None
for packets in (16384, 12288, 8192, 6144, 4096, 3072, 2048, 1024):
    sh = rays[: packets * 64].contiguous()
    out = torch.empty((len(sh), 4) if w is not None else len(sh), dtype=torch.float32, device=dev)
    if w is not None:
        call = lambda: gh.trace_cumulative_weighted_sph(sh, s, tree, w, out=out)
    else:
        call = lambda: gh.trace_cumulative_sph(sh, s, tree, out)
    row = []
    for rep in range(2):
        for K in (-1, 1, 2, 4, 8):
            gh.set_packet_split(K)
            for _ in range(5): call()
            v = []
            for _ in range(30):
                call(); v.append(gh.last_kernel_ms())
            row.append("K=%d %.4f" % (K, statistics.median(v)))
    gh.set_packet_split(-1); call()
    print("%s, %d packets, plan used %d: %s" % (mode, packets, gh.last_plan_used(), "  ".join(row)), flush=True)
