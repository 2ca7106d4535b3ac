# python profiles/recipes/plan_image_hash.py: hashes of column-density images over frames, shards
# and packet splits K = automatic, 1, 2, 4, 8, fast and exact integrals, each traced four times
# in a row (from the third call on a library with packet plans runs from the plan) -- the first
# and the last call's image must hash alike, and two libraries' outputs must be the same text.
import sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "grace-devel_amd")); sys.path.insert(0, ROOT)
import torch, hashlib
import grace_hip as gh
from bench import make_particles
dev = torch.device("cuda:0")
n = 2_000_000
s = make_particles(n, dev)
lo, hi = gh.min_max_vec4(s); lo[3] = hi[3] = 0.0
tree = gh.Tree(n, 32, device=dev)
gh.build_tree(s, tree, lo[:3], hi[:3])
for exact in (False, True):
    gh.set_exact_integrals(exact)
    for side in (512, 200):
        rays, _ = gh.orthogonal_rays_z(side, lo, hi, device=dev)
        for nr in (len(rays), len(rays) // 8 // 64 * 64):     # (ray counts are multiples of 32)
            r = rays[:nr].contiguous()
            out = torch.empty(nr, dtype=torch.float32, device=dev)
            for split in (-1, 1, 2, 4, 8):
                gh.set_packet_split(split)
                hs = []
                for rep in range(4):
                    gh.trace_cumulative_sph(r, s, tree, out)
                    hs.append(hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16])
                assert hs[0] == hs[-1], hs
                print("exact %d side %d rays %d split %d: cum %s" % (exact, side, nr, split, hs[-1]), flush=True)
            gh.set_packet_split(-1)
