# python profiles/recipes/perf_dense_rounds.py: the planned kernel on bench.py's frame and its
# shards -- what the plan's recorder tallied (entries, survivors and dense rounds per packet;
# a library without grace_trace_plan_stats prints none) and the kernel time per packet split
# K = automatic, 1, 2, 4, 8 (30 calls per setting after 5 warm ones, grace_trace_last_kernel_ms,
# median; two repeats).  Run it under with_lib.py to compare two libraries.
import sys, os, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "grace-devel_amd")); sys.path.insert(0, ROOT)
import torch
import grace_hip as gh
from bench import make_particles
dev = torch.device("cuda:0")
n = 10_000_000
s = make_particles(n, dev)
lo, hi = gh.min_max_vec4(s); lo[3] = hi[3] = 0.0
tree = gh.Tree(n, 32, device=dev)
gh.build_tree(s, tree, lo[:3], hi[:3])
rays, _ = gh.orthogonal_rays_z(1024, lo, hi, device=dev)
gh.enable_kernel_timing(True)
for d in (1, 2, 4, 8):
    sh = rays[: len(rays) // d].contiguous()
    out = torch.empty(len(sh), dtype=torch.float32, device=dev)
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
    packets = len(sh) // 64
    line = "1/%d shard (%d packets) plan used %d: %s" % (d, packets, gh.last_plan_used(), "  ".join(row))
    try:
        st = gh.plan_stats()
    except AttributeError:      # a library from before grace_trace_plan_stats
        st = None
    if st is not None:
        line += "\n    per packet: entries %.1f survivors %.1f rounds %.1f (full %.1f, closed by capacity %.1f, by flags %.1f), largest round %d" % (
            st.entries / packets, st.survivors / packets, st.rounds / packets, st.full_rounds / packets,
            st.closed_by_capacity / packets, st.closed_by_flags / packets, st.largest_round)
    print(line, flush=True)
