# The depth-ordered traces in a periodic box (trace_*_periodic_sph) and what they leave of the open ones:
#   python perf_periodic_ordered.py open <root>   one repetition of the three OPEN calls with the library
#       under <root>/grace-devel_amd (a checkout of the parent commit, or this tree): the stats hook's
#       ms_count / ms_trace / ms_composite of each.  Run it alternately on both roots, each run a process
#       of its own, to compare the parent's open calls with this tree's (the GROUPED = false instantiations).
#   python perf_periodic_ordered.py periodic      this tree only: (a) the periodic call in a box so large
#       that no ray is cut and no sphere imaged against the open call on the same data -- the grouped
#       sequence's own overhead; (b) a unit box crossed by rays of 2.3 periods (3 segments each) against
#       the open call on the same rays (which loses what lies beyond the faces: fewer hits).  Medians of 5
#       with device events, stats hook off, and one stats line each.
# Scene: 10^6 spheres uniform in the unit cube, H = 0.01 .. 0.02, a 128 x 128 grid of rays along +z
# (about 700 hits a ray, 1.1e7 in all); three emission channels, two luminosity channels, one spectrum
# channel on 256 periodic bins.
import os
import sys

mode = sys.argv[1]
ROOT = os.path.abspath(sys.argv[2]) if mode == "open" else \
    os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "grace-devel_amd"))
import numpy as np
import torch
import grace_hip as gh

dev = torch.device("cuda:0")
N, SIDE = 1000000, 128


def scene():
    g = torch.Generator(device=dev); g.manual_seed(3)
    s = torch.rand((N, 4), generator=g, device=dev)
    s[:, 3] = 0.01 + 0.01 * s[:, 3]
    return s.contiguous()


def rays(z0, length):
    i, j = torch.meshgrid(torch.arange(SIDE, device=dev), torch.arange(SIDE, device=dev), indexing="ij")
    r = torch.zeros((SIDE * SIDE, 7), device=dev)
    r[:, 2] = 1.0
    r[:, 3] = (i.reshape(-1) + 0.5) / SIDE
    r[:, 4] = (j.reshape(-1) + 0.5) / SIDE
    r[:, 5] = z0
    r[:, 6] = length
    return r.contiguous()


def fields(n):
    g = torch.Generator(device=dev); g.manual_seed(7)
    u = lambda *shape: torch.rand(shape, generator=g, device=dev)
    return dict(emission=u(n, 3), absorption=1e-6 * (0.5 + u(n)), luminosity=1.0 + u(SIDE * SIDE, 2),
                absorption2=1e-6 * (0.5 + u(n, 2)), amount=0.25 + u(n, 1), width=1.0 + 9.0 * u(n, 1),
                velocity=100.0 * (u(n, 3) - 0.5))


GRID = dict(v0=-500.0, dv=1000.0 / 256, n_bins=256, periodic=True, hubble=100.0)


def stats(f):
    gh.ordered_enable_stats(True); f(); st = gh.ordered_last_stats(); gh.ordered_enable_stats(False)
    return st


def timeit(f, reps=5):
    f(); torch.cuda.synchronize(); ts = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
        a.record(); f(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2], min(ts), max(ts)


def open_calls(r, s, tree, F):
    return (("emission_absorption", lambda: gh.trace_emission_absorption_sph(r, s, tree, F["emission"], F["absorption"])),
            ("absorption_deposit", lambda: gh.trace_absorption_deposit_sph(r, s, tree, F["luminosity"], F["absorption2"])),
            ("spectra", lambda: gh.trace_spectra_sph(r, s, tree, F["amount"], F["width"], F["velocity"], **GRID)))


def periodic_calls(r, sc, F):
    return (("emission_absorption", lambda: gh.trace_emission_absorption_periodic_sph(r, sc, F["emission"], F["absorption"])),
            ("absorption_deposit", lambda: gh.trace_absorption_deposit_periodic_sph(r, sc, F["luminosity"], F["absorption2"])),
            ("spectra", lambda: gh.trace_spectra_periodic_sph(r, sc, F["amount"], F["width"], F["velocity"], **GRID)))


if mode == "open":
    s = scene()
    tree = gh.Tree(N, 32, device=dev)
    gh.build_tree(s, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    r = rays(0.0, 1.0)
    F = fields(N)
    for name, f in open_calls(r, s, tree, F):
        f(); torch.cuda.synchronize()                     # warm-up
        st = stats(f)
        print("open %-20s root %s hits %d count %.3f trace %.3f composite %.3f" % (
            name, sys.argv[2], st["total_hits"], st["ms_count"], st["ms_trace"], st["ms_composite"]), flush=True)
else:
    caller = scene()
    F = fields(N)
    for what, lo, period, z0, length in (("huge box (nothing cut, nothing imaged)", (-100.0,) * 3, (1000.0,) * 3, 0.0, 1.0),
                                         ("unit box, 2.3 periods (3 segments a ray)", (0.0,) * 3, (1.0,) * 3, 0.35, 2.3)):
        sc = gh.periodic_scene(caller, lo, period)
        r = rays(z0, length)
        src = sc.source.long()
        Ft = {k: (v if k == "luminosity" else v[src].contiguous()) for k, v in F.items()}      # tree order for the open calls
        print("%s: %d images of %d spheres" % (what, len(sc.spheres), N), flush=True)
        for (name, fo), (_, fp) in zip(open_calls(r, sc.spheres, sc.tree, Ft), periodic_calls(r, sc, F)):
            to, tp = timeit(fo), timeit(fp)
            so, sp = stats(fo), stats(fp)
            print("  %-20s open %.3f ms (min %.3f max %.3f; hits %d, count %.3f trace %.3f composite %.3f)" % (
                name, *to, so["total_hits"], so["ms_count"], so["ms_trace"], so["ms_composite"]), flush=True)
            print("  %-20s periodic %.3f ms (min %.3f max %.3f; hits %d, count %.3f trace %.3f composite %.3f; "
                  "the segments alone %.3f ms)" % (
                      "", *tp, sp["total_hits"], sp["ms_count"], sp["ms_trace"], sp["ms_composite"],
                      timeit(lambda: gh.periodic_ray_segments(r, sc.lo, sc.period, want_t0=(name == "spectra")))[0]),
                  flush=True)
    gh.trace_status()
