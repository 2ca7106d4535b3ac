// Pair counts in separation bins and radial profiles (grace_pair_counts_f4): every sphere centre
// within the outermost edge of each query point, binned by separation as it is found -- totals over
// all points (the DD(r) of a two-point correlation function), per-point histograms and per-point
// sums of weights per bin (counts and mass in shells).  An extension the reference lacks; the
// distance, the bins and the sums' order are stated exactly in include/grace_hip.h.
//
// The walk -- packets, order, stack, cluster sweep and the widening argument that makes pruning
// exact -- is range_walk.hpp's, at the radius e_last, so R2 == E2_last and hit() sees exactly the
// pairs that have a bin, with their d2 in a register.  This file holds what a lane does with it.
//
// Bin.  The bin of d2 is the number of k < n_edges - 1 with E2_k < d2: the smallest k with
// d2 <= E2_k, and n_edges - 1 at most because d2 <= E2_last got it here.  The table travels in the
// kernel arguments, entries from n_edges - 1 on +inf, so no value of d2 yields a bin past the last.
// Up to 16 bins the count is taken directly, one compare against a scalar operand and one
// add-with-carry per edge, no memory and no dependent chain; the 64-bin tier searches a copy of
// the table in LDS, six dependent reads (lanes at different entries are in different banks, lanes
// at one entry are a broadcast).
//
// Histograms.  Per lane, in LDS, laid out [bin][lane]: whatever bins the lanes are in, lane l
// touches bank l (mod the bank count), so increments never conflict, and nothing is indexed
// dynamically in registers.  Counts are LDS integer adds without return; a sums cell is read,
// added to and written back, in the walk's order, which is ascending j.  The LDS is sized by the
// tier BT of bin capacity (8, 16, 64) and the channels NW: BT rows of counts and min(BT NW, 64)
// rows of sums (n_edges NW <= 64 is required) of 256 bytes per wave.  DESIGN.md section 4 lists the
// bytes per block and the waves per CU of each.
//
// Outputs.  finish() writes the lane's rows.  For the totals the wave, reconverged after the walk,
// sums each bin over its 64 lanes -- lane k takes bin k and reads the columns rotated by k, so the
// lanes stay in different banks -- and issues one 64-bit atomicAdd per non-empty bin per packet:
// integer adds commute, so the totals are exact and independent of order.
#include "range_walk.hpp"

#include <cmath>
#include <limits>

using namespace grace_hip;

namespace {

constexpr int PC_MAX_EDGES = 64;
constexpr int PC_MAX_CHANNELS = 4;
constexpr int PC_MAX_CELLS = 64;      // n_edges * n_channels
constexpr int PC_LINEAR_MAX = 16;     // tiers up to here count edges below d2; above: search in LDS

struct PairArgs : WalkArgs {
    float e2[PC_MAX_EDGES];           // E2_k for k < n_edges - 1, +inf from there on
    int n_edges;
    const float* weights;             // sphere j's channel c at weights[j NW + c]
    unsigned long long* totals;       // or null
    int* counts;                      // or null
    float* sums;                      // or null (NW == 0)
};

constexpr int sums_rows(const int bt, const int nw) { return bt * nw < PC_MAX_CELLS ? bt * nw : PC_MAX_CELLS; }

// range_walk.hpp's Visitor.  BT: the tier of bin capacity, NW: the channels of the sums (0: none).
// s_cnt, s_sum: the lane's column of the wave's [bin][lane] and [bin NW + c][lane] arrays; s_w: the
// weights of the wave's 64 survivor records; s_e2: the block's copy of the table (BT > 16).
template <int BT, int NW>
struct PairVisitor {
    static constexpr int NS = NW > 0 ? NW : 1;
    const PairArgs& a;
    uint32_t* s_cnt;
    float* s_sum;
    float (*s_w)[NS];
    const float* s_e2;

    __device__ __forceinline__ PairVisitor(const PairArgs& args, uint32_t* cnt, float* sum, float (*weights)[NS],
                                           const float* table)
        : a(args), s_cnt(cnt), s_sum(sum), s_w(weights), s_e2(table) {}

    __device__ __forceinline__ int find_bin(const float d2) const
    {
        int bin = 0;
        if constexpr (BT <= PC_LINEAR_MAX) {
#pragma unroll
            for (int k = 0; k < BT - 1; ++k) bin += a.e2[k] < d2 ? 1 : 0;
        } else {
#pragma unroll
            for (int step = BT / 2; step >= 1; step >>= 1) bin += s_e2[bin + step - 1] < d2 ? step : 0;
        }
        return bin;                                          // <= n_edges - 1: the entries from there on are +inf
    }

    // every lane's column starts at 0 (off lanes and lanes beyond the packet keep it: no hit)
    __device__ __forceinline__ void begin(const bool, const bool, const uint32_t, const float)
    {
        for (int k = 0; k < a.n_edges; ++k) s_cnt[k * 64] = 0u;
        if constexpr (NW > 0) {
            for (int i = 0; i < a.n_edges * NW; ++i) s_sum[i * 64] = 0.0f;
        }
    }
    __device__ __forceinline__ bool clip(int&, int&) const { return true; }
    __device__ __forceinline__ void stage(const int pos, const int j)
    {
        if constexpr (NW > 0) {
#pragma unroll
            for (int c = 0; c < NW; ++c) s_w[pos][c] = a.weights[size_t(j) * NW + c];
        }
    }
    __device__ __forceinline__ void hit(const int pos, const float4&, const float d2)
    {
        const int bin = find_bin(d2);
        __hip_atomic_fetch_add(s_cnt + bin * 64, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        if constexpr (NW > 0) {
#pragma unroll
            for (int c = 0; c < NW; ++c) {
                float* cell = s_sum + (bin * NW + c) * 64;
                *cell = *cell + s_w[pos][c];
            }
        }
    }
    __device__ __forceinline__ void finish(const uint32_t src)
    {
        if (a.counts) {
            int* row = a.counts + size_t(src) * a.n_edges;
            for (int k = 0; k < a.n_edges; ++k) row[k] = int(s_cnt[k * 64]);
        }
        if constexpr (NW > 0) {
            float* row = a.sums + size_t(src) * a.n_edges * NW;
            for (int i = 0; i < a.n_edges * NW; ++i) row[i] = s_sum[i * 64];
        }
    }
};

template <int BT, int NW, typename Args>
__global__ __launch_bounds__(PW_BLOCK) void pair_kernel(const Args a)
{
    constexpr int NS = NW > 0 ? NW : 1;
    constexpr int SR = sums_rows(BT, NW);
    __shared__ float4 s_rec[PW_WAVES][64];
    __shared__ float s_w[PW_WAVES][NW > 0 ? 64 : 1][NS];
    __shared__ uint32_t s_cnt[PW_WAVES][BT][64];
    __shared__ float s_sum[PW_WAVES][SR > 0 ? SR : 1][SR > 0 ? 64 : 1];
    __shared__ float s_e2[BT > PC_LINEAR_MAX ? BT : 1];
    if constexpr (BT > PC_LINEAR_MAX) {
        if (threadIdx.x < BT) s_e2[threadIdx.x] = a.e2[threadIdx.x];
        __syncthreads();
    }
    const PacketWave w = packet_wave();
    const int lane = w.lane, wv = w.wv, packet = w.packet;
    if (packet >= int(*a.n_starts)) return;
    PairVisitor<BT, NW> v(a, &s_cnt[wv][0][lane], &s_sum[wv][0][SR > 0 ? lane : 0], s_w[wv], s_e2);
    walk(a, packet, lane, s_rec[wv], v);
    if (!a.totals) return;
    // all 64 lanes again: bin `lane` over the wave's columns
    wave_sync();
    if (lane < a.n_edges) {
        const uint32_t* bin_row = s_cnt[wv][lane];
        unsigned long long t = 0ull;
#pragma unroll 8
        for (int i = 0; i < 64; ++i) t += bin_row[(i + lane) & 63];
        if (t) atomicAdd(a.totals + lane, t);
    }
}

template <int BT, typename Args>
void launch_tier(const Args& a, int nw, int blocks, hipStream_t stream)
{
    switch (nw) {
    case 0: pair_kernel<BT, 0><<<blocks, PW_BLOCK, 0, stream>>>(a); break;
    case 1: pair_kernel<BT, 1><<<blocks, PW_BLOCK, 0, stream>>>(a); break;
    case 2: pair_kernel<BT, 2><<<blocks, PW_BLOCK, 0, stream>>>(a); break;
    case 3: pair_kernel<BT, 3><<<blocks, PW_BLOCK, 0, stream>>>(a); break;
    default: pair_kernel<BT, 4><<<blocks, PW_BLOCK, 0, stream>>>(a); break;
    }
}

template <typename Args>
grace_status launch_pairs(const Args& a, int nw, size_t waves, hipStream_t stream)
{
    const int blocks = ceil_div(waves, PW_WAVES);
    if (a.n_edges <= 8) launch_tier<8>(a, nw, blocks, stream);
    else if (a.n_edges <= 16) launch_tier<16>(a, nw, blocks, stream);
    else launch_tier<64>(a, nw, blocks, stream);
    GRACE_CHECK_LAUNCH();
    return GRACE_OK;
}

// grace_pair_counts_f4 and its periodic form (Periodic<PairArgs>: the same visitor over the walk's
// periodic variant): `a` is zero.  h_period3: the periodic form's period, checked together with the
// last edge once the edges are known to be good.
template <typename Args>
grace_status pair_counts(Args a, const float* d_points, size_t n_points, int elems_per_point,
                         const float* h_edges, int n_edges, const float* d_spheres, size_t n_spheres,
                         const int* d_nodes, size_t n_nodes, const int* d_leaves, const int* d_root,
                         const float* d_weights, int n_channels, unsigned long long* d_totals, int* d_counts,
                         float* d_sums, const float* h_period3, grace_stream stream)
{
    GRACE_REQUIRE(elems_per_point >= 3 && elems_per_point <= 16, "pair_counts: elements per point must be 3..16");
    GRACE_REQUIRE(n_points < (size_t(1) << 31), "pair_counts: too many points");
    GRACE_REQUIRE(n_edges >= 1 && n_edges <= PC_MAX_EDGES, "pair_counts: the number of edges must be 1..64");
    GRACE_REQUIRE(h_edges, "pair_counts: null edges");
    for (int k = 0; k < n_edges; ++k)
        GRACE_REQUIRE(std::isfinite(h_edges[k]) && h_edges[k] >= 0.0f && (k == 0 || h_edges[k] > h_edges[k - 1]),
                      "pair_counts: the edges must be finite, not negative and strictly ascending");
    if constexpr (is_periodic<Args>::value) GRACE_TRY(walk_period(a.per, h_period3, h_edges + n_edges - 1));
    if (d_sums) {
        GRACE_REQUIRE(n_channels >= 1 && n_channels <= PC_MAX_CHANNELS, "pair_counts: channels must be 1..4");
        GRACE_REQUIRE(n_edges * n_channels <= PC_MAX_CELLS, "pair_counts: edges times channels must not exceed 64");
        GRACE_REQUIRE(d_weights, "pair_counts: sums need weights");
    }
    const hipStream_t stream_ = as_stream(stream);
    if (n_points == 0) {                  // (before the output checks: a caller's empty arrays may be null)
        if (d_totals) GRACE_TRY_HIP(hipMemsetAsync(d_totals, 0, size_t(n_edges) * sizeof(unsigned long long), stream_));
        return GRACE_OK;
    }
    GRACE_REQUIRE(d_totals || d_counts || d_sums, "pair_counts: no output");
    GRACE_REQUIRE(d_points, "pair_counts: null points");
    GRACE_TRY(walk_scene(a, nullptr, h_edges[n_edges - 1], d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root));
    TraceState* ts = nullptr;
    GRACE_TRY(trace_state(&ts));
    for (int k = 0; k < PC_MAX_EDGES; ++k)
        a.e2[k] = k < n_edges - 1 ? h_edges[k] * h_edges[k] : std::numeric_limits<float>::infinity();
    a.n_edges = n_edges;
    a.weights = d_weights;
    a.totals = d_totals;
    a.counts = d_counts;
    a.sums = d_sums;
    if (d_totals) GRACE_TRY_HIP(hipMemsetAsync(d_totals, 0, size_t(n_edges) * sizeof(unsigned long long), stream_));
    return packet_run(a, *ts, d_points, n_points, elems_per_point, stream_,
                      [&](const Args& w, size_t waves) -> grace_status {
        return launch_pairs(w, d_sums ? n_channels : 0, waves, stream_);
    });
}


} // namespace

extern "C" {

grace_status grace_pair_counts_f4(const float* d_points, size_t n_points, int elems_per_point,
                                  const float* h_edges, int n_edges,
                                  const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                  size_t n_nodes, const int* d_leaves, const int* d_root,
                                  const float* d_weights, int n_channels,
                                  unsigned long long* d_totals, int* d_counts, float* d_sums,
                                  grace_stream stream)
{
    return pair_counts(PairArgs(), d_points, n_points, elems_per_point, h_edges, n_edges, d_spheres, n_spheres,
                       d_nodes, n_nodes, d_leaves, d_root, d_weights, n_channels, d_totals, d_counts, d_sums, nullptr, stream);
}

grace_status grace_pair_counts_periodic_f4(const float* d_points, size_t n_points, int elems_per_point,
                                           const float* h_edges, int n_edges,
                                           const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                           size_t n_nodes, const int* d_leaves, const int* d_root,
                                           const float* d_weights, int n_channels,
                                           unsigned long long* d_totals, int* d_counts, float* d_sums,
                                           const float* h_period3, grace_stream stream)
{
    return pair_counts(Periodic<PairArgs>(), d_points, n_points, elems_per_point, h_edges, n_edges, d_spheres, n_spheres,
                       d_nodes, n_nodes, d_leaves, d_root, d_weights, n_channels, d_totals, d_counts, d_sums, h_period3, stream);
}

} // extern "C"
