# The periodic column-density trace next to the open one, on bench.py's scene: 10^7 particles uniform
# in the unit box (its make_particles), 1024^2 rays that span one period of the box L = (1, 1, 1) at
# the origin, looking down -z from the top face (project_sph(period=...)'s rays).
# Cases, each as median [min .. max] of device-event times over --reps rounds after two warm-ups:
#   periodic_scene                 images (count, scan, fill), keys, two sorts, deltas, ALBVH
#   build_tree                     the open scene's build, for comparison
#   periodic_ray_segments          count, scan (a host read of the total), fill
#   fold                           grace_periodic_fold_f32 alone
#   trace_cumulative_sph           the open trace: the same rays over the spheres without images
#   trace on segments x images     the open trace inside the periodic call
#   trace_cumulative_periodic_sph  the whole call
#   perf_periodic_trace.py [--n N] [--side S] [--reps R]
#   perf_periodic_trace.py --open-only --package <other checkout>/grace-devel_amd
#                                  the open build and trace of another build (the parent commit's)
import argparse
import ctypes as C
import math
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--package", default=None, help="a grace-devel_amd directory to import grace_hip from")
ap.add_argument("--open-only", action="store_true")
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--side", type=int, default=1024)
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, args.package or os.path.join(ROOT, 'grace-devel_amd'))
import numpy as np
import torch
import grace_hip as gh

dev = torch.device('cuda:0')
LO, PERIOD = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


def spread(v):
    v = sorted(v)
    return "%.3f [%.3f .. %.3f] ms" % (v[len(v) // 2], v[0], v[-1])


def timed(f, reps=args.reps, warm=2):
    out = []
    for i in range(warm + reps):
        a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record(); torch.cuda.synchronize()
        if i >= warm:
            out.append(a.elapsed_time(b))
    return spread(out)


def make_particles(n, seed=42):                                   # bench.py's
    g = torch.Generator(device=dev); g.manual_seed(seed)
    s = torch.empty((n, 4), dtype=torch.float32, device=dev)
    s[:, :3] = torch.rand((n, 3), generator=g, device=dev, dtype=torch.float32)
    s[:, 3] = float((3.0 * 48.0 / (4.0 * math.pi * n)) ** (1.0 / 3.0))
    return s


caller = make_particles(args.n)
side = args.side
rays = gh.orthographic_projection_rays(side, side, (0.5, 0.5, 1.0), (0.5, 0.5, 0.0), (0.0, 1.0, 0.0), 1.0, 1.0,
                                       device=dev)
print("scene: %d particles, h = %.5f; %d rays spanning one period" % (args.n, float(caller[0, 3]), len(rays)))

# ---- open -----------------------------------------------------------------------------------------
spheres = caller.clone()
tree = gh.Tree(args.n, 32, device=dev)


def build_open():
    global tree
    spheres.copy_(caller)
    tree = gh.Tree(args.n, 32, device=dev)
    gh.build_tree(spheres, tree)


print("build_tree (open scene, incl. the copy):", timed(build_open, reps=3, warm=1))
out = torch.empty(len(rays), dtype=torch.float32, device=dev)
print("trace_cumulative_sph (open, no images):", timed(lambda: gh.trace_cumulative_sph(rays, spheres, tree, out)))
gh.trace_status()
open_sum = float(out.double().sum())
if args.open_only:
    sys.exit(0)

# ---- periodic -------------------------------------------------------------------------------------
scene = [None]


def build_periodic():
    scene[0] = None
    scene[0] = gh.periodic_scene(caller, LO, PERIOD)


print("periodic_scene:", timed(build_periodic, reps=3, warm=1))
sc = scene[0]
print("images: %d (%.4f per particle)" % (len(sc.spheres), len(sc.spheres) / args.n))
seg = [None]


def segments():
    seg[0] = gh.periodic_ray_segments(rays, LO, PERIOD)


print("periodic_ray_segments:", timed(segments))
segs, offsets = seg[0]
print("segments: %d (%.4f per ray)" % (len(segs), len(segs) / len(rays)))
per_segment = torch.empty(len(segs), dtype=torch.float32, device=dev)
args_seg = gh._trace_args(segs, sc.spheres, sc.tree)
print("trace on segments x images:", timed(lambda: gh._check(
    gh._lib.grace_trace_cumulative_f4(*args_seg, gh._ptr(per_segment), gh._stream()))))
print("fold:", timed(lambda: gh._check(gh._lib.grace_periodic_fold_f32(
    gh._ptr(per_segment), gh._ptr(offsets), C.c_size_t(len(rays)), C.c_int(1), gh._ptr(out), gh._stream()))))
print("trace_cumulative_periodic_sph (whole call):", timed(lambda: gh.trace_cumulative_periodic_sph(rays, sc, out)))
gh.trace_status()
print("sum of the map: open %.6e, periodic %.6e (ratio %.5f)" % (open_sum, float(out.double().sum()),
                                                                  float(out.double().sum()) / open_sum))
