// Absorbed radiation deposited on the particles, per ray and channel
// (grace_trace_absorption_deposit_f4; the contract is in grace_hip.h).  gfx950 only.
//
// The transpose of ordered.hip's integral: ray r carries L[r, c]; its hits, ordered by (distance,
// sphere index), absorb dep_kc = L exp(-tau_kc) (1 - exp(-a_kc)) each, and what every sphere
// absorbs is summed over all rays.  The host sequence, the tiers and the load + sort are
// ordered_core.hpp's.  What is here:
//   deposit_scale_kernel / deposit_quantum_kernel   M_c = max_r |L[r, c]| by integer atomicMax on
//       the bits (order-free for non-negative floats), then q_c = 2^(e_c + b - 62).
//   deposit_composite_kernel<T, CAP, TIER>   one workgroup per ray.  Per group of four channels
//       the fp64 exclusive scan of a_kc (tau_k = carry + waves before + exclusive wave scan, the
//       carry running over groups of blockDim hits: every addition's place is a function of k and
//       n alone), then dep_kc / q_c rounded half-even to a 64-bit integer and ONE no-return integer
//       atomic add at acc[i_k * C + c] (channel-minor: a hit's four channels are one 32-byte
//       segment).  Integer addition is associative, so the accumulators -- hence the deposits -- do
//       not depend on the order in which rays, batches or workgroups arrive.
//   deposit_finish_kernel   deposit = (double)acc * q_c.
// The accumulators live in the call's frame in front of the per-batch region, so they survive
// the batches.  A timing-only build with -DGRACE_DEPOSIT_TIMING_NO_ADD keeps the whole
// instruction stream but the atomic add (its results are wrong; it exists to price the atomics).

#include "ordered_core.hpp"

namespace grace_hip {
namespace {

constexpr int DEP_MAX_CHANNELS = 64;

struct DepArgs : OrdBatch {
    const float* luminosity;    // [n_rays * C]
    const float* absorption;    // [n_spheres * C]
    int channels;
    const double* quantum;      // [C]
    long long* acc;             // [n_spheres * C]
    float* transmitted;         // [n_rays * C], or null
};

__global__ __launch_bounds__(256) void deposit_scale_kernel(const float* __restrict__ lum, const size_t n_rays,
                                                            const int C, uint32_t* __restrict__ max_bits)
{
    __shared__ uint32_t s_max[DEP_MAX_CHANNELS];
    const int tid = threadIdx.x;
    if (tid < DEP_MAX_CHANNELS) s_max[tid] = 0;
    __syncthreads();
    for (size_t r = size_t(blockIdx.x) * 256 + tid; r < n_rays; r += size_t(gridDim.x) * 256)
        for (int c = 0; c < C; ++c) {
            const uint32_t v = __float_as_uint(lum[r * C + c]) & 0x7fffffffu;
            if (v > s_max[c]) atomicMax(&s_max[c], v);      // (the plain read only spares atomics: max is monotone)
        }
    __syncthreads();
    if (tid < C && s_max[tid]) atomicMax(&max_bits[tid], s_max[tid]);
}

// q_c = 2^(e_c + b - 62) with 2^(e_c - 1) <= M_c < 2^(e_c); 0 for M_c == 0 (and for a non-finite M_c,
// outside the contract: the channel then deposits nothing).
__global__ void deposit_quantum_kernel(const uint32_t* __restrict__ max_bits, const int C, const int b,
                                       double* __restrict__ quantum, double* __restrict__ quantum_out)
{
    const int c = threadIdx.x;
    if (c >= C) return;
    const float m = __uint_as_float(max_bits[c]);
    double q = 0.0;
    if (m > 0.0f && m < __builtin_huge_valf()) {
        int e = 0;
        (void)frexp(static_cast<double>(m), &e);
        q = ldexp(1.0, e + b - 62);
    }
    quantum[c] = q;
    if (quantum_out) quantum_out[c] = q;
}

// dep / q rounded half-even as a 64-bit integer; clamped to [-2^62, 2^62] with NaN -> 0 before the
// cast (outside the contract's domain the value is unspecified, the cast must stay defined).
__device__ __forceinline__ long long deposit_units(const double dep, const double inv_q)
{
    double s = rint(dep * inv_q);       // q is a power of two: the scaling is exact
    if (!(s == s)) s = 0.0;
    s = fmin(fmax(s, -0x1p62), 0x1p62);
    return static_cast<long long>(s);
}

// TIER 0 / 1: arrays of CAP hits in LDS; TIER 2: in place in global memory.  GROUPED: the ray's hits
// are those of all its segments, ordered segment first, and X holds the caller's particle of every
// hit (ordered_core.hpp): absorption and acc are indexed by it, luminosity and transmitted by the ray.
template <int T, int CAP, int TIER, bool GROUPED>
__global__ __launch_bounds__(T) void deposit_composite_kernel(const DepArgs a)
{
    constexpr int WAVES = T / 64;
    __shared__ uint32_t s_d[CAP ? CAP : 1];
    __shared__ int s_x[CAP ? CAP : 1];
    __shared__ uint32_t s_i[CAP ? CAP : 1];
    __shared__ double s_wave[WAVES][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t *D, *I;
    int* X;
    int n;
    size_t r;
    OrdSpan span;
    if (!ordered_load_sort<T, CAP, TIER, GROUPED>(a, s_d, s_x, s_i, D, X, I, n, r, span)) return;

    const int C = a.channels;
    for (int c0 = 0; c0 < C; c0 += 4) {
        const int nc = C - c0 < 4 ? C - c0 : 4;
        double L[4], inv_q[4], carry[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            L[j] = inv_q[j] = carry[j] = 0.0;
            if (j < nc) {
                L[j] = static_cast<double>(a.luminosity[r * C + c0 + j]);
                const double q = a.quantum[c0 + j];
                inv_q[j] = q != 0.0 ? 1.0 / q : 0.0;
            }
        }
        for (int base = 0; base < n; base += T) {
            const int k = base + tid;
            int x = 0;
            double ak[4] = { 0.0, 0.0, 0.0, 0.0 };
            if (k < n) {
                x = X[k];
                const double Ik = static_cast<double>(__uint_as_float(I[k]));
                const float* ab = a.absorption + size_t(x) * C + c0;
#pragma unroll
                for (int j = 0; j < 4; ++j) if (j < nc) ak[j] = static_cast<double>(ab[j]) * Ik;
            }
            double before[4], total[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                before[j] = total[j] = 0.0;
                if (j < nc) {
                    double inc = ak[j];
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const double v = __shfl_up(inc, o);
                        if (lane >= o) inc += v;
                    }
                    double exc = __shfl_up(inc, 1);
                    if (lane == 0) exc = 0.0;
                    before[j] = exc;
                    total[j] = __shfl(inc, 63);
                }
            }
            if (WAVES > 1) {
                if (lane == 63)
#pragma unroll
                    for (int j = 0; j < 4; ++j) s_wave[wave][j] = total[j];
                __syncthreads();
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (j < nc) {
                        double run = 0.0, mine = 0.0;
#pragma unroll
                        for (int w = 0; w < WAVES; ++w) { if (w == wave) mine = run; run += s_wave[w][j]; }
                        before[j] = mine + before[j];
                        total[j] = run;
                    }
                }
                __syncthreads();
            }
            if (k < n) {
                long long* acc = a.acc + size_t(x) * C + c0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (j < nc) {
                        const double dep = L[j] * exp(-(carry[j] + before[j])) * -expm1(-ak[j]);
                        const long long u = deposit_units(dep, inv_q[j]);
#ifndef GRACE_DEPOSIT_TIMING_NO_ADD
                        if (u != 0)
                            (void)__hip_atomic_fetch_add(acc + j, u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
                        if (u == INT64_MIN) acc[j] = u;      // never true (clamped): keeps the arithmetic alive
#endif
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) carry[j] += total[j];
        }
        if (tid == 0 && a.transmitted)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nc) a.transmitted[r * C + c0 + j] = static_cast<float>(L[j] * exp(-carry[j]));
    }
}

__global__ __launch_bounds__(256) void deposit_finish_kernel(const long long* __restrict__ acc,
                                                             const double* __restrict__ quantum, const size_t n,
                                                             const int C, double* __restrict__ deposit)
{
    for (size_t i = size_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += size_t(gridDim.x) * 256)
        deposit[i] = static_cast<double>(acc[i]) * quantum[i % C];
}

template <bool GROUPED>
grace_status deposit_launch(const DepArgs& a, const int nb, const bool any_block, const bool any_global,
                            const hipStream_t stream)
{
    deposit_composite_kernel<64, ORD_WAVE_MAX, 0, GROUPED><<<nb, 64, 0, stream>>>(a);
    GRACE_CHECK_LAUNCH();
    if (any_block) {
        deposit_composite_kernel<256, ORD_BLOCK_MAX, 1, GROUPED><<<nb, 256, 0, stream>>>(a);
        GRACE_CHECK_LAUNCH();
    }
    if (any_global) {
        deposit_composite_kernel<256, 0, 2, GROUPED><<<nb, 256, 0, stream>>>(a);
        GRACE_CHECK_LAUNCH();
    }
    return GRACE_OK;
}

// The open call (grouped == null: the traced rays are the rays, the particles the spheres) and the
// periodic one (the traced rays are the n_traced segments of n_rays rays, the spheres the images of
// n_particles caller particles).  n_rays sets the quantum, n_particles sizes the deposit.
grace_status absorption_deposit(const void* d_traced, size_t n_traced, const float* d_spheres, size_t n_spheres,
                                const int* d_nodes, size_t n_nodes, const int* d_leaves, const int* d_root,
                                size_t n_rays, size_t n_particles, const float* d_luminosity,
                                const float* d_absorption, int n_channels, double* d_deposit, float* d_transmitted,
                                double* d_quantum, grace_stream stream_, const OrdGroups* grouped)
{
    GRACE_REQUIRE(n_channels >= 1 && n_channels <= DEP_MAX_CHANNELS, "trace_absorption_deposit: channels must be 1..64");
    GRACE_REQUIRE(d_deposit, "trace_absorption_deposit: null output");
    GRACE_REQUIRE(n_spheres < (size_t(1) << 31) && n_particles < (size_t(1) << 31),
                  "trace_absorption_deposit: bad primitive count");
    const hipStream_t stream = as_stream(stream_);
    const size_t C = size_t(n_channels), n_acc = n_particles * C;
    if (n_rays == 0) {      // nothing is absorbed: unlike the per-ray outputs, the deposit is defined
        if (n_acc) GRACE_TRY_HIP(hipMemsetAsync(d_deposit, 0, n_acc * sizeof(double), stream));
        if (d_quantum) GRACE_TRY_HIP(hipMemsetAsync(d_quantum, 0, C * sizeof(double), stream));
        return GRACE_OK;
    }
    GRACE_REQUIRE(d_luminosity && d_absorption, "trace_absorption_deposit: null luminosity or absorption");
    GRACE_REQUIRE(d_traced && d_spheres && d_nodes && d_leaves && d_root, "trace_absorption_deposit: null pointer");
    GRACE_REQUIRE(n_rays < (size_t(1) << 31) && n_traced < (size_t(1) << 31), "trace_absorption_deposit: bad ray count");
    GRACE_REQUIRE(n_nodes >= 1 && n_nodes < (size_t(1) << 30), "trace_absorption_deposit: bad node count");
    GRACE_REQUIRE(n_spheres > 0, "trace_absorption_deposit: bad primitive count");
    int b = 0;                                          // ceil(log2(n_rays))
    while ((size_t(1) << b) < n_rays) ++b;

    // the front of the frame: accumulators, then the channels' maxima and quanta
    const size_t off_max = Workspace::aligned(n_acc * sizeof(long long)),
                 off_q = off_max + Workspace::aligned(DEP_MAX_CHANNELS * sizeof(uint32_t)),
                 front_bytes = off_q + Workspace::aligned(DEP_MAX_CHANNELS * sizeof(double));
    DepArgs a;
    a.luminosity = d_luminosity; a.absorption = d_absorption; a.channels = n_channels;
    a.transmitted = d_transmitted;
    FrameGuard frame;
    GRACE_TRY(ordered_run(
        frame, d_traced, n_traced, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root, front_bytes, stream,
        [&](char* front) -> grace_status {
            a.acc = reinterpret_cast<long long*>(front);
            uint32_t* max_bits = reinterpret_cast<uint32_t*>(front + off_max);
            double* quantum = reinterpret_cast<double*>(front + off_q);
            a.quantum = quantum;
            GRACE_TRY_HIP(hipMemsetAsync(front, 0, off_q, stream));     // accumulators and maxima
            deposit_scale_kernel<<<stream_grid(n_rays, 256), 256, 0, stream>>>(d_luminosity, n_rays, n_channels, max_bits);
            GRACE_CHECK_LAUNCH();
            deposit_quantum_kernel<<<1, DEP_MAX_CHANNELS, 0, stream>>>(max_bits, n_channels, b, quantum, d_quantum);
            GRACE_CHECK_LAUNCH();
            return GRACE_OK;
        },
        [&](const OrdBatch& batch, const int nb, const bool any_block, const bool any_global) -> grace_status {
            static_cast<OrdBatch&>(a) = batch;
            return grouped ? deposit_launch<true>(a, nb, any_block, any_global, stream)
                           : deposit_launch<false>(a, nb, any_block, any_global, stream);
        },
        grouped));
    deposit_finish_kernel<<<stream_grid(n_acc, 256), 256, 0, stream>>>(a.acc, a.quantum, n_acc, n_channels, d_deposit);
    GRACE_CHECK_LAUNCH();
    return GRACE_OK;
}

} // namespace
} // namespace grace_hip

using namespace grace_hip;

extern "C" {

grace_status grace_trace_absorption_deposit_f4(const void* d_rays, size_t n_rays, const float* d_spheres,
                                               size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                               const int* d_leaves, const int* d_root,
                                               const float* d_luminosity, const float* d_absorption,
                                               int n_channels, double* d_deposit, float* d_transmitted,
                                               double* d_quantum, grace_stream stream_)
{
    return absorption_deposit(d_rays, n_rays, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root, n_rays,
                              n_spheres, d_luminosity, d_absorption, n_channels, d_deposit, d_transmitted, d_quantum,
                              stream_, nullptr);
}

grace_status grace_trace_absorption_deposit_periodic_f4(const void* d_segments, size_t n_segments,
                                                        const float* d_images, size_t n_images, const int* d_nodes,
                                                        size_t n_nodes, const int* d_leaves, const int* d_root,
                                                        const int* d_segment_offsets, size_t n_rays,
                                                        const int* d_source, size_t n_sources,
                                                        const float* d_luminosity, const float* d_absorption,
                                                        int n_channels, double* d_deposit, float* d_transmitted,
                                                        double* d_quantum, grace_stream stream_)
{
    OrdGroups g = {};
    if (n_rays != 0)
        GRACE_TRY(ordered_groups(g, d_segments, n_segments, d_segment_offsets, n_rays, d_source, n_sources, nullptr));
    return absorption_deposit(d_segments, n_segments, d_images, n_images, d_nodes, n_nodes, d_leaves, d_root, n_rays,
                              n_sources, d_luminosity, d_absorption, n_channels, d_deposit, d_transmitted, d_quantum,
                              stream_, &g);
}

} // extern "C"
