// grace/detail/periodic_box.h -- the period of a periodic box, the trailing argument of the periodic
// overloads of range_counts_sph, range_neighbours_sph, fof_labels_sph, pair_counts_sph,
// radial_profiles_sph, nearest_neighbours_sph, smoothing_lengths_sph, interpolate_sph and
// interpolate_grid_sph (an extension the reference lacks).  A period of 0 leaves that axis open; a
// negative or non-finite one is refused by the library.  No origin is needed: the separation
// d = p - x is wrapped once into [-L/2, L/2] per component, whatever the coordinates
// (grace_hip.h, "Periodic boxes", states the arithmetic).
#pragma once

namespace grace {

struct PeriodicBox {
    float lx, ly, lz;
};

// A periodic box with its origin, for the periodic traces (grace/detail/periodic_trace.h): unlike the
// point queries, which wrap a separation, a trace has to know where the faces are.  The box is
// [ox, ox + lx] x [oy, oy + ly] x [oz, oz + lz]; a period of 0 leaves that axis open.
struct PeriodicDomain {
    float ox, oy, oz;
    PeriodicBox period;
};

} // namespace grace
