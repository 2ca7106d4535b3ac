// Velocity-space absorption spectra along rays (grace_trace_spectra_f4; the contract is in
// grace_hip.h).  gfx950 only.
//
// The third consumer of ordered_core.hpp: the host sequence, the tiers and the load + sort are its.
// The other two reduce over a ray's hits; this one scatters every hit over a window of velocity
// bins.  What is here:
//   spectra_kernel<T, CAP, TIER, BINS>   one workgroup per ray, channels outermost.  Per channel the
//       ray's n_bins fp64 bins live in LDS (BINS * 8 bytes: 2 KiB for grids of up to SPEC_BINS_SMALL
//       bins, 8 KiB up to SPEC_BINS_MID, 32 KiB otherwise; the grid picks the instantiation).  The
//       hits are taken in depth order in chunks of SPEC_CHUNK:
//         prepare   lane l of the first wave gathers hit k's amount, width and velocity and stores
//                   the hit's record -- v_k, 1 / b_kc, N_kc and its window of unwrapped bins -- in LDS;
//         scatter   every wave owns a contiguous range of bins and walks the chunk's records in
//                   order (wave-uniform LDS broadcasts).  A window that reaches the wave's range is
//                   taken 63 bins at a time: lane l evaluates erf at edge s + l, takes edge s + l + 1
//                   from its neighbour, and does a plain read-add-write on bin s + l.
//       A bin belongs to one wave, and a wave executes its LDS operations in program order, so per
//       bin the terms are added hit by hit in depth order and within a hit in ascending unwrapped
//       bin: the contract's order, with no atomics, whatever the tier, the batch or the other rays.
//       In periodic mode a window is walked one period image after the other (ascending), so within
//       one step no two lanes meet on a bin.  Work is hits x window bins, not hits x n_bins.
//   v_k is recomputed per channel in `prepare` (three cached loads and six fp64 operations per hit
//   against at least 64 erf evaluations): keeping it would cost 48 KiB of LDS in the block tier.

#include "ordered_core.hpp"

#include <cmath>

namespace grace_hip {
namespace {

constexpr int SPEC_MAX_CHANNELS = 16, SPEC_MAX_BINS = 4096, SPEC_BINS_SMALL = 256, SPEC_BINS_MID = 1024;
constexpr int SPEC_CHUNK = 64;          // hits prepared at a time: one per lane of the first wave
constexpr int SPEC_STEP = 63;           // bins per step: 64 edges
constexpr double SPEC_REACH = 6.0;      // the window: v_k -+ 6 b_kc

struct SpecArgs : OrdBatch {
    const char* rays;           // the call's rays (28 bytes each: direction, origin, length)
    const float* amount;        // [n_spheres * C]
    const float* width;         // [n_spheres * C]
    const float* velocity;      // [n_spheres * 3]
    int channels, n_bins, periodic;
    double v0, dv, inv_dv, hubble;
    float* tau;                 // [n_rays * C * n_bins]
    float* column;              // [n_rays * C], or null
};

// GROUPED: the ray's hits are those of all its segments, ordered segment first, and X holds the
// caller's particle of every hit (ordered_core.hpp); a.rays are the SEGMENTS.  The direction is the
// ray's first segment's (every segment has the ray's, bit for bit), and hit k's distance from the
// ray's origin is seg_t0[its segment] + its distance within the segment, in fp64.
template <int T, int CAP, int TIER, int BINS, bool GROUPED>
__global__ __launch_bounds__(T) void spectra_kernel(const SpecArgs a)
{
    constexpr int WAVES = T / 64;
    __shared__ uint32_t s_d[CAP ? CAP : 1];
    __shared__ int s_x[CAP ? CAP : 1];
    __shared__ uint32_t s_i[CAP ? CAP : 1];
    __shared__ double s_bins[BINS];
    __shared__ double s_v[SPEC_CHUNK], s_ib[SPEC_CHUNK], s_N[SPEC_CHUNK];
    __shared__ long long s_ub[SPEC_CHUNK];      // unwrapped bin of t == 0: a multiple of n_bins
    __shared__ int s_t[SPEC_CHUNK], s_len[SPEC_CHUNK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t *D, *I;
    int* X;
    int n;
    size_t r;
    OrdSpan span;
    if (!ordered_load_sort<T, CAP, TIER, GROUPED>(a, s_d, s_x, s_i, D, X, I, n, r, span)) return;

    const int C = a.channels, nb = a.n_bins;
    double dx = 0.0, dy = 0.0, dz = 0.0;
    if (!GROUPED || span.g0 < span.g1) {        // (a ray without segments has no hits either)
        const float* ray = reinterpret_cast<const float*>(a.rays + (GROUPED ? size_t(span.g0) : r) * 28);
        dx = static_cast<double>(ray[0]); dy = static_cast<double>(ray[1]); dz = static_cast<double>(ray[2]);
    }
    const double v0 = a.v0, dv = a.dv;
    const int per = (nb + WAVES - 1) / WAVES;                       // the wave's bins: [j0, j1)
    const int j0 = wave * per < nb ? wave * per : nb, j1 = j0 + per < nb ? j0 + per : nb;

    for (int j = tid; j < nb; j += T) s_bins[j] = 0.0;
    for (int c = 0; c < C; ++c) {
        double col = 0.0;
        for (int base = 0; base < n; base += SPEC_CHUNK) {
            const int cn = n - base < SPEC_CHUNK ? n - base : SPEC_CHUNK;
            __syncthreads();                    // the previous chunk's records (and the zeroed bins) are done with
            if (tid < cn) {
                const int k = base + tid, x = X[k];
                const double Ik = static_cast<double>(__uint_as_float(I[k]));
                double d = static_cast<double>(dist_from_key(D[k]));
                if constexpr (GROUPED) d = a.seg_t0[ordered_segment_of(a, span, k)] + d;
                const float* vel = a.velocity + size_t(x) * 3;
                const double v = a.hubble * d + ((static_cast<double>(vel[0]) * dx + static_cast<double>(vel[1]) * dy)
                                                 + static_cast<double>(vel[2]) * dz);
                const double b = static_cast<double>(a.width[size_t(x) * C + c]);
                long long ub = 0;
                int t = 0, len = 0;
                if (b > 0.0 && b < __builtin_huge_val() && fabs(v) < __builtin_huge_val()) {
                    double lo = floor(((v - SPEC_REACH * b) - v0) / dv), hi = floor(((v + SPEC_REACH * b) - v0) / dv);
                    if (a.periodic) {
                        const double mid = floor((v - v0) / dv);
                        if (fabs(mid) < 0x1p52) {
                            lo = fmax(lo, mid - nb); hi = fmin(hi, mid + nb);
                            const long long u_lo = static_cast<long long>(lo);
                            long long m = u_lo % nb;
                            if (m < 0) m += nb;
                            t = static_cast<int>(m); ub = u_lo - m;
                            len = static_cast<int>(hi - lo) + 1;
                        }
                    } else {
                        lo = fmax(lo, 0.0); hi = fmin(hi, static_cast<double>(nb - 1));
                        if (hi >= lo) { t = static_cast<int>(lo); len = static_cast<int>(hi - lo) + 1; }
                    }
                }
                s_v[tid] = v; s_ib[tid] = len ? 1.0 / b : 0.0;
                s_N[tid] = static_cast<double>(a.amount[size_t(x) * C + c]) * Ik;
                s_ub[tid] = ub; s_t[tid] = t; s_len[tid] = len;
            }
            __syncthreads();
            for (int kk = 0; kk < cn; ++kk) {
                const double N = s_N[kk];
                col += N;
                const int len = s_len[kk];
                if (len == 0) continue;
                const int t_lo = s_t[kk], t_hi = t_lo + len - 1;
                if (t_hi < j0) continue;                                    // (t_lo < n_bins: no image below j0)
                if (t_hi < nb && t_lo >= j1) continue;
                const double v = s_v[kk], ib = s_ib[kk];
                const long long ub = s_ub[kk];
                for (int q = 0; q <= t_hi; q += nb) {                       // period images, ascending
                    const int lo = t_lo > q + j0 ? t_lo : q + j0, hi = t_hi < q + j1 - 1 ? t_hi : q + j1 - 1;
                    for (int s = lo; s <= hi; s += SPEC_STEP) {
                        const int t = s + lane;
                        const double e = v0 + static_cast<double>(ub + t) * dv;
                        const double E = erf((e - v) * ib);
                        const double up = __shfl_down(E, 1);
                        if (lane < SPEC_STEP && t <= hi) s_bins[t - q] += N * (0.5 * (up - E));
                    }
                }
            }
        }
        __syncthreads();
        float* out = a.tau + (r * C + c) * size_t(nb);
        for (int j = tid; j < nb; j += T) {
            out[j] = static_cast<float>(a.inv_dv * s_bins[j]);
            s_bins[j] = 0.0;
        }
        if (tid == 0 && a.column) a.column[r * C + c] = static_cast<float>(col);
    }
}

template <int BINS, bool GROUPED>
grace_status spectra_launch(const SpecArgs& a, const int nb, const bool any_block, const bool any_global,
                            const hipStream_t stream)
{
    spectra_kernel<64, ORD_WAVE_MAX, 0, BINS, GROUPED><<<nb, 64, 0, stream>>>(a);
    GRACE_CHECK_LAUNCH();
    if (any_block) {
        spectra_kernel<256, ORD_BLOCK_MAX, 1, BINS, GROUPED><<<nb, 256, 0, stream>>>(a);
        GRACE_CHECK_LAUNCH();
    }
    if (any_global) {
        spectra_kernel<256, 0, 2, BINS, GROUPED><<<nb, 256, 0, stream>>>(a);
        GRACE_CHECK_LAUNCH();
    }
    return GRACE_OK;
}

template <bool GROUPED>
grace_status spectra_launch_bins(const SpecArgs& a, const int nb, const bool any_block, const bool any_global,
                                 const hipStream_t stream)
{
    return a.n_bins <= SPEC_BINS_SMALL ? spectra_launch<SPEC_BINS_SMALL, GROUPED>(a, nb, any_block, any_global, stream)
         : a.n_bins <= SPEC_BINS_MID ? spectra_launch<SPEC_BINS_MID, GROUPED>(a, nb, any_block, any_global, stream)
                                     : spectra_launch<SPEC_MAX_BINS, GROUPED>(a, nb, any_block, any_global, stream);
}

// The open call (grouped == null) and the periodic one: d_rays are then the segments, the
// per-particle arrays are indexed by source, the outputs by ray.
grace_status spectra(const void* d_rays, size_t n_rays, const float* d_spheres, size_t n_spheres,
                     const int* d_nodes, size_t n_nodes, const int* d_leaves, const int* d_root,
                     const float* d_amount, const float* d_width, const float* d_velocity,
                     int n_channels, const grace_spectrum_grid* grid, float* d_tau, float* d_column,
                     grace_stream stream_, const OrdGroups* grouped)
{
    GRACE_REQUIRE(n_channels >= 1 && n_channels <= SPEC_MAX_CHANNELS, "trace_spectra: channels must be 1..16");
    GRACE_REQUIRE(grid, "trace_spectra: null grid");
    GRACE_REQUIRE(grid->n_bins >= 1 && grid->n_bins <= SPEC_MAX_BINS, "trace_spectra: n_bins must be 1..4096");
    GRACE_REQUIRE(grid->dv > 0.0 && std::isfinite(grid->dv), "trace_spectra: dv must be positive and finite");
    GRACE_REQUIRE(std::isfinite(grid->v0) && std::isfinite(grid->hubble), "trace_spectra: v0 and hubble must be finite");
    GRACE_REQUIRE(d_amount && d_width && d_velocity, "trace_spectra: null amount, width or velocity");
    GRACE_REQUIRE(d_tau, "trace_spectra: null output");
    GRACE_REQUIRE(n_spheres < (size_t(1) << 31), "trace_spectra: bad primitive count");
    if (n_rays == 0) return GRACE_OK;
    GRACE_REQUIRE(d_rays && d_spheres && d_nodes && d_leaves && d_root, "trace_spectra: null pointer");
    GRACE_REQUIRE(n_rays < (size_t(1) << 31), "trace_spectra: bad ray count");
    GRACE_REQUIRE(n_nodes >= 1 && n_nodes < (size_t(1) << 30), "trace_spectra: bad node count");
    GRACE_REQUIRE(n_spheres > 0, "trace_spectra: bad primitive count");
    const hipStream_t stream = as_stream(stream_);

    SpecArgs a;
    a.rays = static_cast<const char*>(d_rays);
    a.amount = d_amount; a.width = d_width; a.velocity = d_velocity;
    a.channels = n_channels; a.n_bins = grid->n_bins; a.periodic = grid->periodic != 0;
    a.v0 = grid->v0; a.dv = grid->dv; a.inv_dv = 1.0 / grid->dv; a.hubble = grid->hubble;
    a.tau = d_tau; a.column = d_column;
    FrameGuard frame;
    GRACE_TRY(ordered_run(
        frame, d_rays, n_rays, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root, 0, stream,
        [](char*) -> grace_status { return GRACE_OK; },
        [&](const OrdBatch& batch, const int nb, const bool any_block, const bool any_global) -> grace_status {
            static_cast<OrdBatch&>(a) = batch;
            return grouped ? spectra_launch_bins<true>(a, nb, any_block, any_global, stream)
                           : spectra_launch_bins<false>(a, nb, any_block, any_global, stream);
        },
        grouped));
    return GRACE_OK;
}

} // namespace
} // namespace grace_hip

using namespace grace_hip;

extern "C" {

grace_status grace_trace_spectra_f4(const void* d_rays, size_t n_rays, const float* d_spheres, size_t n_spheres,
                                    const int* d_nodes, size_t n_nodes, const int* d_leaves, const int* d_root,
                                    const float* d_amount, const float* d_width, const float* d_velocity,
                                    int n_channels, const grace_spectrum_grid* grid, float* d_tau, float* d_column,
                                    grace_stream stream_)
{
    return spectra(d_rays, n_rays, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root, d_amount, d_width,
                   d_velocity, n_channels, grid, d_tau, d_column, stream_, nullptr);
}

grace_status grace_trace_spectra_periodic_f4(const void* d_segments, size_t n_segments, const float* d_images,
                                             size_t n_images, const int* d_nodes, size_t n_nodes,
                                             const int* d_leaves, const int* d_root, const int* d_segment_offsets,
                                             size_t n_rays, const int* d_source, size_t n_sources,
                                             const double* d_segment_t0, const float* d_amount, const float* d_width,
                                             const float* d_velocity, int n_channels,
                                             const grace_spectrum_grid* grid, float* d_tau, float* d_column,
                                             grace_stream stream_)
{
    if (n_rays == 0) return GRACE_OK;
    GRACE_REQUIRE(d_segment_t0, "trace_spectra_periodic: null segment starts");
    OrdGroups g;
    GRACE_TRY(ordered_groups(g, d_segments, n_segments, d_segment_offsets, n_rays, d_source, n_sources, d_segment_t0));
    return spectra(d_segments, n_segments, d_images, n_images, d_nodes, n_nodes, d_leaves, d_root, d_amount, d_width,
                   d_velocity, n_channels, grid, d_tau, d_column, stream_, &g);
}

} // extern "C"
