# python profiles/recipes/subtile_model.py [h_scale]: CPU model of the packet plan's survivor streams
# on bench.py's scene shape -- 10^7 uniform particles in Morton order, h from the 48-neighbour
# rule (times h_scale), 40 random 8 x 8-pixel packets of the 1024^2 orthographic frame, classes of
# 1024 consecutive particles (GRANULE_SHIFT = 10).  Prints the survivors per packet, the fraction
# of (survivor, ray) pairs that are hits, and the steps a list keeps if each 4 x 4 quadrant, or
# each 8 x 4 half, walks only the survivors that can reach it (sum over classes of the longest
# stream / sum of the list lengths).  The model behind the sub-tile layout (PLAN_FORMAT_SUBTILE,
# csrc/trace_state.hpp); the recorder's own figures come from grace_trace_plan_subtiles.
import math
import sys
import numpy as np

h_scale = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
rng = np.random.default_rng(42)
n = 10_000_000
P = rng.random((n, 3), dtype=np.float32)
h = h_scale * (3 * 48 / (4 * math.pi * n)) ** (1 / 3)


def spread(v):
    v = v.astype(np.uint64) & 0x3ff
    v = (v | (v << 16)) & 0x030000FF
    v = (v | (v << 8)) & 0x0300F00F
    v = (v | (v << 4)) & 0x030C30C3
    v = (v | (v << 2)) & 0x09249249
    return v


q = np.minimum((P * 1024).astype(np.int64), 1023)
key = (spread(q[:, 0]) << 2) | (spread(q[:, 1]) << 1) | spread(q[:, 2])
P = P[np.argsort(key, kind="stable")]
pix = 1.0 / 1024


def dist2_rect(x, y, x0, x1, y0, y1):
    dx = x - np.clip(x, x0, x1)
    dy = y - np.clip(y, y0, y1)
    return dx * dx + dy * dy


survivors = quadrant_steps = half_x_steps = half_y_steps = hits = 0
tiles = rng.integers(8, 120, size=(40, 2))
for tx, ty in tiles:
    x0, y0 = (tx * 8 + 0.5) * pix, (ty * 8 + 0.5) * pix
    near = (np.abs(P[:, 0] - (x0 + 3.5 * pix)) < 3.5 * pix + h) & (np.abs(P[:, 1] - (y0 + 3.5 * pix)) < 3.5 * pix + h)
    idx = np.nonzero(near)[0]
    x, y = P[idx, 0], P[idx, 1]
    keep = dist2_rect(x, y, x0, x0 + 7 * pix, y0, y0 + 7 * pix) < h * h
    idx, x, y = idx[keep], x[keep], y[keep]
    cls = (idx >> 10) & 7
    ox, oy = x0 + pix * np.arange(8), y0 + pix * np.arange(8)
    hits += ((x[:, None, None] - ox[None, :, None]) ** 2 + (y[:, None, None] - oy[None, None, :]) ** 2 < h * h).sum()
    quad = np.zeros((len(idx), 4), bool)
    for qi in range(2):
        for qj in range(2):
            quad[:, qi * 2 + qj] = dist2_rect(x, y, x0 + 4 * qi * pix, x0 + (4 * qi + 3) * pix,
                                              y0 + 4 * qj * pix, y0 + (4 * qj + 3) * pix) < h * h
    lower_x, upper_x = quad[:, 0] | quad[:, 1], quad[:, 2] | quad[:, 3]
    lower_y, upper_y = quad[:, 0] | quad[:, 2], quad[:, 1] | quad[:, 3]
    for c in range(8):
        mc = cls == c
        survivors += mc.sum()
        quadrant_steps += quad[mc].sum(axis=0).max()
        half_x_steps += max(lower_x[mc].sum(), upper_x[mc].sum())
        half_y_steps += max(lower_y[mc].sum(), upper_y[mc].sum())
print("h = %.2f pixels: %.0f survivors per packet, fill %.3f" % (h / pix, survivors / len(tiles), hits / (survivors * 64)))
print("steps kept: 4 x 4 quadrants %.3f, halves split in x %.3f, in y %.3f"
      % (quadrant_steps / survivors, half_x_steps / survivors, half_y_steps / survivors))
