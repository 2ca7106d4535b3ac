// The set-up of one packet (one wave = up to 64 rays), shared by trace_kernel (trace_kernel.hpp) and
// the packet plan's plan_record_kernel (trace_planned.hip): the packet's rays, its axis, its beam,
// the per-lane and wave-uniform constants of the axis path, and the origin lattice.  (The pencil
// set-up, which only trace_kernel needs, stays in its body.)
#pragma once

#include "trace_state.hpp"

namespace {

using namespace grace_hip;

__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off));
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// A lane's ray of the packet that starts at slot first_ray of the batch's ray order.
struct PacketRay {
    bool valid;       // the lane holds a ray of its own
    int index;        // the ray's index in the caller's arrays
    float dx, dy, dz, ox, oy, oz, len;
};

__device__ __forceinline__ PacketRay load_packet_ray(const TraceArgs& a, const int first_ray, const int lane)
{
    PacketRay r;
    const int slot_index = first_ray + lane;
    r.valid = lane < a.width && slot_index < a.n_rays;
    // Idle and tail lanes re-trace the packet's last ray so that they do not widen the packet.
    const int slot_clamped = r.valid ? slot_index : min(first_ray + a.width, a.n_rays) - 1;
    r.index = a.perm ? int(a.perm[slot_clamped]) : slot_clamped;
    const float* rp = a.rays + 7 * size_t(r.index);
    r.dx = rp[0]; r.dy = rp[1]; r.dz = rp[2];
    r.ox = rp[3]; r.oy = rp[4]; r.oz = rp[5];
    r.len = rp[6];
    return r;
}

// Axis-aligned packet (every direction = +-e_axis)?  The axis, or -1.  (wave-uniform; tail lanes
// replicate a valid ray)
__device__ __forceinline__ int packet_axis(const float dx, const float dy, const float dz)
{
    const unsigned long long all = ~0ull;
    const bool zx = dx == 0.f, zy = dy == 0.f, zz = dz == 0.f;
    int axis = -1;
    if (__builtin_amdgcn_ballot_w64(zy && zz && fabsf(dx) == 1.f) == all) axis = 0;
    else if (__builtin_amdgcn_ballot_w64(zx && zz && fabsf(dy) == 1.f) == all) axis = 1;
    else if (__builtin_amdgcn_ballot_w64(zx && zy && fabsf(dz) == 1.f) == all) axis = 2;
    return axis;
}

// Permuted per-lane constants of the axis path: along-axis origin / direction, then the two
// perpendicular origins in component order.
struct AxisRay {
    float oa, da, o1, o2;
    // (s_a - o_a) * d_a with d_a = +-1 is the correctly rounded +-(s_a - o_a): one FMA
    // s_a * d_a + (-o_a * d_a) gives the same bits (both products are exact).
    float noda;
};

__device__ __forceinline__ AxisRay axis_ray(const int axis, const PacketRay& r)
{
    // (the selections are made on values: a selection between the struct's members would be one
    // between addresses, and keep the whole ray in memory)
    const float dx = r.dx, dy = r.dy, dz = r.dz, ox = r.ox, oy = r.oy, oz = r.oz;
    const float oa = axis == 0 ? ox : axis == 1 ? oy : oz;
    const float da = axis == 0 ? dx : axis == 1 ? dy : dz;
    const float o1 = axis == 0 ? oy : ox;
    const float o2 = axis == 2 ? oy : oz;
    return AxisRay{ oa, da, o1, o2, -(oa * da) };
}

// Wave-uniform, for the range-check-free sweep of an axis-aligned packet: the packet's extremes of
// -o_a d_a and of the ray length, the rays' sense along the axis (+-1, the first lane's if they
// differ) and whether all rays share it.  (Results through references to the caller's own
// variables: returned in a struct, the flag cost the class-split kernels three inverted branches.)
__device__ __forceinline__ void axis_extremes(const AxisRay& x, const float len, float& noda_lo, float& noda_hi,
                                              float& len_lo, float& da0, bool& same_sense)
{
    noda_lo = wave_min(x.noda); noda_hi = wave_max(x.noda); len_lo = wave_min(len);
    const unsigned long long fwd = __builtin_amdgcn_ballot_w64(x.da > 0.f);
    same_sense = fwd == 0ull || fwd == ~0ull;
    da0 = fwd ? 1.f : -1.f;
}

// Bounding boxes of the packet's origins and directions (wave-uniform, SGPRs).
struct Beam {
    float olo[3], ohi[3], dlo[3], dhi[3];
};

__device__ __forceinline__ Beam packet_beam(const PacketRay& r)
{
    Beam beam;
    beam.olo[0] = wave_min(r.ox); beam.ohi[0] = wave_max(r.ox);
    beam.olo[1] = wave_min(r.oy); beam.ohi[1] = wave_max(r.oy);
    beam.olo[2] = wave_min(r.oz); beam.ohi[2] = wave_max(r.oz);
    beam.dlo[0] = wave_min(r.dx); beam.dhi[0] = wave_max(r.dx);
    beam.dlo[1] = wave_min(r.dy); beam.dhi[1] = wave_max(r.dy);
    beam.dlo[2] = wave_min(r.dz); beam.dhi[2] = wave_max(r.dz);
    return beam;
}

// Axis-aligned packets, fast integral: a sphere hit by SOME ray of the packet lies within
// h + D of every other ray (D = diagonal of the origins' box), i.e. at a table position below
// 50 (1 + D / h).  For h >= D / 3 that stays below 200 < LUTF_N: such survivors need no clamp.
// Returns the r^2 from which on that holds, from the extents e1, e2 of the origins' rectangle.
__device__ __forceinline__ float fat_radius2(const float e1, const float e2)
{
    return (e1 * e1 + e2 * e2) * (1.0f / 9.0f) * 1.0001f;
}

__device__ __forceinline__ float fat_radius2(const int axis, const Beam& beam)
{
    const float ex = beam.ohi[0] - beam.olo[0], ey = beam.ohi[1] - beam.olo[1], ez = beam.ohi[2] - beam.olo[2];
    return fat_radius2(axis == 0 ? ey : ex, axis == 2 ? ey : ez);
}

// Origin lattice of an axis-aligned packet.  The beam cull bounds b^2 at the point of the
// origin RECTANGLE nearest to the sphere; a sphere smaller than the ray spacing can lie
// inside the rectangle and still between the rays -- in the dense cores of clustered SPH
// data most do (h << pixel), and every one of them used to cost all 64 lanes a test (10^7
// particles, 90 % of them in 50 clumps: 180 863 surviving candidates in the heaviest packet
// against 2273 in the median one, whose wave outlived the launch 30x).  If the packet's
// origins take at most 8 distinct values in each perpendicular co-ordinate (pixel grids do:
// 8 x 8 tiles), the tables of those values give the exact minimum of the rays' own b^2
// expression over the lattice {x_i} x {y_j} -- a superset of the rays --: |s - x| rounds
// monotonically in the true difference, so the nearest table value minimises the rounded |q|
// in each co-ordinate, and b^2 is monotone in both.  No margin, same bits as the ray's test.
// Fills this wave's two tables lat[threadIdx.x >> 6][0 / 1][8] (lane 0 writes; the workgroup's whole
// array is passed and the wave's row is taken here, as the kernel's own text did) from the lanes'
// perpendicular origins.  Hands back ok -- the origins form a lattice -- and cell2, the squared
// diagonal of its mean cell: the caller's r^2 below which a sphere can fall between the rays is
// ok ? cell2 : 0 (0 = no lattice; spheres wider than the cell diagonal meet a ray wherever they lie
// inside the lattice).
template <int WAVES>
__device__ __forceinline__ void build_origin_lattice(const float o1, const float o2, const int lane,
                                                     float (&lat)[WAVES][2][8], bool& ok, float& cell2)
{
    // The distinct values of each co-ordinate, in any order (the nearest one is found by a
    // plain minimum): take the first lane not yet accounted for, strike every lane that
    // holds its value, eight times at most.  NaN origins strike nobody: no lattice.
    ok = true;
    cell2 = 0.f;
#pragma unroll
    for (int dim = 0; dim < 2; ++dim) {
        const float o = dim ? o2 : o1;
        unsigned long long todo = ~0ull;
        int n_val = 0;
        float v = 0.f, v_lo = INFINITY, v_hi = -INFINITY;
#pragma unroll 1
        for (int k = 0; k < 8 && todo != 0ull; ++k) {
            v = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, o),
                                                                    __builtin_ctzll(todo)));
            v_lo = fminf(v_lo, v); v_hi = fmaxf(v_hi, v);
            todo &= ~__builtin_amdgcn_ballot_w64(o == v);
            if (lane == 0) lat[threadIdx.x >> 6][dim][k] = v;
            ++n_val;
        }
        ok = ok && todo == 0ull;
        if (lane == 0)
            for (int k = n_val; k < 8; ++k) lat[threadIdx.x >> 6][dim][k] = v;   // padding repeats
        // mean spacing (a gate only: it decides which spheres are worth the lattice test)
        const float gap = n_val > 1 ? (v_hi - v_lo) / float(n_val - 1) : 0.f;
        cell2 += gap * gap;
    }
}

} // namespace
