"""Gadget-2 (format 1) snapshot I/O for the SPH fields GRACE uses: gas positions and
smoothing lengths, positions and masses of any particle type (read_gadget_particles), and the
velocities and gas fields a sightline spectrum needs (read_gadget_fields), and the header's
fields (read_gadget_header: the particle counts, the masses, the time, the redshift and the box
size a periodic query needs).
Block layout as read by the reference's tests/helper/read_gadget.cuh: header of 256 B
(npart[6] int32, mass[6] float64, time and redshift float64, ..., BoxSize float64 at byte 128,
..., padding) and POS, VEL, ID, [MASS], U, RHO, HSML blocks,
every block framed by 4-byte markers.  Host-side file I/O only (numpy)."""
import numpy as np


def write_gadget(fname, pos, hsml, masses_in_header=True, vel=None, u=None, box_size=0.0):
    """Writes a gas-only snapshot: pos [N,3] float32, hsml [N] float32; vel [N,3] and u [N]
    float32 fill the VEL and U blocks (zeros when None); box_size is the header's BoxSize (0: the
    zero bytes of a header without one)."""
    pos = np.ascontiguousarray(pos, np.float32); hsml = np.ascontiguousarray(hsml, np.float32)
    n = len(pos)
    vel = np.zeros((n, 3), np.float32) if vel is None else np.ascontiguousarray(vel, np.float32)
    u = np.zeros(n, np.float32) if u is None else np.ascontiguousarray(u, np.float32)
    if vel.shape != (n, 3) or u.shape != (n,):
        raise ValueError("vel must have shape [N, 3] and u shape [N]")
    npart = np.array([n, 0, 0, 0, 0, 0], np.int32)
    mass = np.array([1.0 if masses_in_header else 0.0, 0, 0, 0, 0, 0], np.float64)

    def block(f, payload):
        nbytes = np.array([len(payload)], np.int32).tobytes()
        f.write(nbytes); f.write(payload); f.write(nbytes)

    with open(fname, "wb") as f:
        header = npart.tobytes() + mass.tobytes()
        header = header + bytes(128 - len(header)) + np.array([box_size], np.float64).tobytes()
        block(f, header + bytes(256 - len(header)))
        block(f, pos.tobytes())                                   # POS
        block(f, vel.tobytes())                                   # VEL
        block(f, np.arange(n, dtype=np.int32).tobytes())          # ID
        if not masses_in_header:
            block(f, np.ones(n, np.float32).tobytes())            # MASS (only if header mass == 0)
        block(f, u.tobytes())                                     # U
        block(f, np.ones(n, np.float32).tobytes())                # RHO
        block(f, hsml.tobytes())                                  # HSML


def read_gadget_header(fname):
    """Returns the header's fields as a dict: "npart" (6 ints) and "mass" (6 floats), "time" and
    "redshift" (the float64 at bytes 72 and 80), "flag_sfr" and "flag_feedback" (int32 at 88 and
    92), "npart_total" (6 ints at 96), "flag_cooling" and "num_files" (int32 at 120 and 124) and
    "box_size", "omega0", "omega_lambda" and "hubble_param" (float64 at 128, 136, 144 and 152).
    box_size is the period of a periodic snapshot, in the units of the positions."""
    with open(fname, "rb") as f:
        raw = f.read(4 + 256)
    if len(raw) < 260 or int(np.frombuffer(raw[:4], np.int32)[0]) != 256:
        raise RuntimeError("Gadget file %s does not start with a 256-byte header block" % fname)
    h = np.frombuffer(raw[4:], np.uint8)
    f64 = lambda at: float(h[at:at + 8].view(np.float64)[0])
    i32 = lambda at: int(h[at:at + 4].view(np.int32)[0])
    return {"npart": [int(x) for x in h[:24].view(np.int32)],
            "mass": [float(x) for x in h[24:72].view(np.float64)],
            "time": f64(72), "redshift": f64(80), "flag_sfr": i32(88), "flag_feedback": i32(92),
            "npart_total": [int(x) for x in h[96:120].view(np.uint32)],
            "flag_cooling": i32(120), "num_files": i32(124),
            "box_size": f64(128), "omega0": f64(136), "omega_lambda": f64(144), "hubble_param": f64(152)}


def read_gadget(fname):
    """Returns spheres [N_gas, 4] float32 = (x, y, z, hsml) -- read_gadget.cuh:69-159."""
    with open(fname, "rb") as f:
        raw = np.frombuffer(f.read(), np.uint8)
    pos = 0

    def take_block():
        nonlocal pos
        nbytes = int(raw[pos:pos + 4].view(np.int32)[0])
        data = raw[pos + 4: pos + 4 + nbytes]
        pos += 8 + nbytes
        return data

    header = take_block()
    npart = header[:24].view(np.int32)
    mass = header[24:72].view(np.float64)
    n_gas = int(npart[0])
    if n_gas == 0:
        raise RuntimeError("Gadget file %s has no gas particles!" % fname)
    n_withmass = int(sum(int(npart[i]) for i in range(6) if mass[i] == 0))
    p = take_block().view(np.float32).reshape(-1, 3)[:n_gas]
    take_block()                 # VEL
    take_block()                 # ID
    if n_withmass > 0:
        take_block()             # MASS
    take_block()                 # U
    take_block()                 # RHO
    h = take_block().view(np.float32)[:n_gas]
    out = np.empty((n_gas, 4), np.float32)
    out[:, :3] = p
    out[:, 3] = h
    return out


def read_gadget_particles(fname, ptype):
    """Returns (positions [N, 3], masses [N]), both float32, of the particles of type ptype (0..5) --
    any type, with or without HSML.  POS holds every type in type order; a type's masses come from
    the header, or from the MASS block when its header mass is 0 (the block holds those types only,
    in type order)."""
    if not 0 <= int(ptype) <= 5:
        raise ValueError("ptype must be 0..5")
    ptype = int(ptype)
    with open(fname, "rb") as f:
        raw = np.frombuffer(f.read(), np.uint8)
    pos = 0

    def take_block():
        nonlocal pos
        nbytes = int(raw[pos:pos + 4].view(np.int32)[0])
        data = raw[pos + 4: pos + 4 + nbytes]
        pos += 8 + nbytes
        return data

    header = take_block()
    npart = [int(x) for x in header[:24].view(np.int32)]
    mass = header[24:72].view(np.float64)
    first = sum(npart[:ptype])
    n = npart[ptype]
    if n == 0:
        return np.empty((0, 3), np.float32), np.empty(0, np.float32)
    p = take_block().view(np.float32).reshape(-1, 3)[first:first + n].copy()
    if mass[ptype] != 0:
        return p, np.full(n, mass[ptype], np.float32)
    take_block()                 # VEL
    take_block()                 # ID
    m_first = sum(npart[t] for t in range(ptype) if mass[t] == 0)
    m = take_block().view(np.float32)[m_first:m_first + n].copy()
    return p, m


def read_gadget_fields(fname, ptype):
    """Returns a dict of float32 arrays for the particles of type ptype (0..5): "pos" [N, 3] and
    "vel" [N, 3], and for gas (ptype 0) also "u", "rho" and "hsml" [N] -- the blocks read_gadget
    skips.  POS and VEL hold every type in type order; U, RHO and HSML hold the gas only."""
    if not 0 <= int(ptype) <= 5:
        raise ValueError("ptype must be 0..5")
    ptype = int(ptype)
    with open(fname, "rb") as f:
        raw = np.frombuffer(f.read(), np.uint8)
    pos = 0

    def take_block():
        nonlocal pos
        nbytes = int(raw[pos:pos + 4].view(np.int32)[0])
        data = raw[pos + 4: pos + 4 + nbytes]
        pos += 8 + nbytes
        return data

    header = take_block()
    npart = [int(x) for x in header[:24].view(np.int32)]
    mass = header[24:72].view(np.float64)
    first, n = sum(npart[:ptype]), npart[ptype]
    out = {"pos": take_block().view(np.float32).reshape(-1, 3)[first:first + n].copy(),
           "vel": take_block().view(np.float32).reshape(-1, 3)[first:first + n].copy()}
    if ptype == 0:
        take_block()             # ID
        if any(npart[t] > 0 and mass[t] == 0 for t in range(6)):
            take_block()         # MASS
        for name in ("u", "rho", "hsml"):
            out[name] = take_block().view(np.float32)[:n].copy()
    return out
