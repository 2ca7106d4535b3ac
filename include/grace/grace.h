// grace.h -- host-only C++ mirror of the grace:: header API for the BVH-build + SPH
// ray-traversal hot path, forwarding to the C ABI of libgrace_hip.so (include/grace_hip.h).
//
// Same names, template signatures, argument meaning and error behaviour as the reference headers
// it replaces (paths relative to the reference root):
//   include/grace/ray.h, types.h                     -> grace::Ray, uinteger32/64, Octants, RaySortType
//   include/grace/cuda/nodes.h                       -> grace::Tree
//   include/grace/cuda/build_sph.cuh                 -> morton_keys*_sph, *_deltas_sph, ALBVH_sph
//   include/grace/cuda/trace_sph.cuh                 -> trace_hitcounts_sph, trace_cumulative_sph,
//                                                       trace_sph, trace_with_sentinels_sph
//   include/grace/cuda/scan.cuh                      -> [weighted_]exclusive_segmented_scan
//   include/grace/cuda/sort.cuh                      -> sort_by_distance
//   include/grace/cuda/gen_rays.cuh                  -> uniform_random_rays ... pinhole_camera_rays
//   tests/helper/tree.cuh, tests/helper/rays.cuh     -> build_tree, orthogonal_rays_z
//   (no reference symbol; named by the task)         -> project_sph
// and this library's extensions: weighted, emission-absorption, deposit and spectra traces,
// SphKernel, PreparedTrace (with trace_sph.cuh), interpolate_sph / interpolate_grid_sph,
// nearest_neighbours_sph / smoothing_lengths_sph, range_counts_sph / range_neighbours_sph,
// fof_labels_sph / fof_groups_sph, pair_counts_sph / radial_profiles_sph,
// gravity_moments_sph / gravity_sph, gravity_group_moments_sph / gravity_groups_sph.
//
// The functions themselves are defined once, in grace/detail/{build_sph,trace_sph,scan,sort,
// gen_rays,interpolate_sph,neighbours_sph,range_sph,fof_sph,pairs_sph,gravity_sph}.h, for this mirror and for the drop-in grace/cuda/*.cuh
// set alike (grace/detail/front_end.h).  What is this header's own: the vector types, the
// container, Tree, the error policy and the three helpers at its end.
//
// The reference's boundary type is thrust::device_vector; this mirror is HIP-free (plain
// g++ compiles it), so it ships grace::device_vector<T>, a minimal owning device array with
// the subset of the thrust interface the reference's call sites use (size, resize, data, assign,
// assignment from / copy to std::vector).  Errors: a bad argument throws
// std::invalid_argument exactly where the reference does; a GPU API failure prints the
// message and exit()s like GRACE_CUDA_CHECK (include/grace/error.h:40-56).
#pragma once

#ifdef GRACE_DROPIN_HEADERS_INCLUDED
#error "grace/grace.h (HIP-free mirror) and the grace/cuda/*.cuh drop-in headers define the same names: include one set only"
#endif
#define GRACE_HIP_FREE_MIRROR_INCLUDED 1

#include <cstdio>
#include <cstdlib>
#include <array>
#include <cstring>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "grace_hip.h"
#include "grace/generic/morton.h"   // host-callable grace::morton_key, detail::space_by_two_* (generic/morton.h:14-55)
#include "grace/ray.h"   // grace::Ray (include/grace/ray.h:5-10)

namespace grace {

typedef uint32_t uinteger32; // include/grace/types.h:29-32
typedef uint64_t uinteger64;

struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
struct int3 { int x, y, z; };
struct int4 { int x, y, z, w; };
struct double3 { double x, y, z; };
struct double4 { double x, y, z, w; };

// include/grace/types.h:36-51
enum Octants { PPP = 7, PPM = 6, PMP = 5, PMM = 4, MPP = 3, MPM = 2, MMP = 1, MMM = 0 };
enum RaySortType { NoSort, DirectionSort, EndPointSort };

inline float3 make_float3(float x, float y, float z) { float3 v = { x, y, z }; return v; }
inline float4 make_float4(float x, float y, float z, float w) { float4 v = { x, y, z, w }; return v; }

namespace detail {

inline void check(grace_status s)
{
    if (s == GRACE_OK) return;
    if (s == GRACE_INVALID_ARGUMENT) throw std::invalid_argument(grace_last_error());
    // include/grace/error.h:40-56: print and exit with the error code.
    std::fprintf(stderr, "**** GRACE HIP Error ****\n%s\n", grace_last_error());
    std::exit(int(s));
}

// More per-hit slots than the int ray offsets address.
inline void too_many_hits(bool with_sentinels)
{
    throw std::invalid_argument(with_sentinels
        ? "trace_with_sentinels_sph: more than INT_MAX output slots; trace fewer rays per call."
        : "trace_sph: more than INT_MAX hits; trace fewer rays per call.");
}

} // namespace detail

// The status policy the shared API bodies apply (grace/detail/front_end.h).
#define GRACE_STATUS_CHECK(status) { grace::detail::check(status); }

// Minimal stand-in for thrust::device_vector<T> (device memory owned through the C ABI).
template <typename T>
class device_vector {
public:
    device_vector() : ptr_(nullptr), size_(0), capacity_(0) {}
    explicit device_vector(size_t n) : ptr_(nullptr), size_(0), capacity_(0)
    {
        resize(n);
        if (n) detail::check(grace_memset(ptr_, 0, n * sizeof(T), nullptr)); // value-init
    }
    device_vector(const std::vector<T>& h) : ptr_(nullptr), size_(0), capacity_(0) { *this = h; }
    device_vector(const device_vector& o) : ptr_(nullptr), size_(0), capacity_(0)
    {
        resize(o.size_);
        detail::check(grace_memcpy_dtod(ptr_, o.ptr_, size_ * sizeof(T), nullptr));
    }
    ~device_vector() { grace_device_free(ptr_); }

    device_vector& operator=(const std::vector<T>& h)
    {
        resize(h.size());
        detail::check(grace_memcpy_htod(ptr_, h.data(), h.size() * sizeof(T), nullptr));
        return *this;
    }
    device_vector& operator=(const device_vector& o)
    {
        if (this != &o) {
            resize(o.size_);
            detail::check(grace_memcpy_dtod(ptr_, o.ptr_, size_ * sizeof(T), nullptr));
        }
        return *this;
    }

    // Keeps the old contents (thrust semantics); new elements are unspecified.
    void resize(size_t n)
    {
        if (n > capacity_) {
            void* p = nullptr;
            detail::check(grace_device_malloc(&p, n * sizeof(T)));
            if (size_) detail::check(grace_memcpy_dtod(p, ptr_, size_ * sizeof(T), nullptr));
            detail::check(grace_stream_synchronize(nullptr));
            grace_device_free(ptr_);
            ptr_ = static_cast<T*>(p);
            capacity_ = n;
        }
        size_ = n;
    }
    void assign(size_t n, const T& value) { *this = std::vector<T>(n, value); }
    size_t size() const { return size_; }
    T* data() { return ptr_; }
    const T* data() const { return ptr_; }

    std::vector<T> to_host() const
    {
        std::vector<T> h(size_);
        detail::check(grace_memcpy_dtoh(h.data(), ptr_, size_ * sizeof(T), nullptr));
        return h;
    }
    T at_host(size_t i) const
    {
        T v;
        detail::check(grace_memcpy_dtoh(&v, ptr_ + i, sizeof(T), nullptr));
        return v;
    }

private:
    T* ptr_;
    size_t size_, capacity_;
};

// include/grace/cuda/nodes.h:14-58.  nodes holds 4 int4 per node, leaves one int4 per leaf;
// both are allocated for N leaves and shrunk by the build (albvh.cuh:842-845).
class Tree {
public:
    device_vector<int4> nodes;
    device_vector<int4> leaves;
    int* root_index_ptr;
    int max_per_leaf;

    Tree(size_t N_leaves, int max_per_leaf_ = 1)
        : nodes(4 * (N_leaves - 1)), leaves(N_leaves), root_index_ptr(nullptr),
          max_per_leaf(max_per_leaf_)
    {
        void* p = nullptr;
        detail::check(grace_device_malloc(&p, sizeof(int)));
        root_index_ptr = static_cast<int*>(p);
    }
    ~Tree() { grace_device_free(root_index_ptr); }

private:
    Tree(const Tree&);
    Tree& operator=(const Tree&);
};

// The container and raw pointers the shared API bodies are written against.
namespace detail {
template <typename T> using dvec = device_vector<T>;
template <typename T> inline T* raw(device_vector<T>& v) { return v.data(); }
template <typename T> inline const T* raw(const device_vector<T>& v) { return v.data(); }
} // namespace detail

} // namespace grace

#include "grace/detail/build_sph.h"
#include "grace/detail/trace_sph.h"
#include "grace/detail/scan.h"
#include "grace/detail/sort.h"
#include "grace/detail/gen_rays.h"
#include "grace/detail/interpolate_sph.h"
#include "grace/detail/neighbours_sph.h"
#include "grace/detail/range_sph.h"
#include "grace/detail/fof_sph.h"
#include "grace/detail/pairs_sph.h"
#include "grace/detail/gravity_sph.h"
#include "grace/detail/periodic_trace.h"

namespace grace {

// util/extrema.cuh min_vec4 / max_vec4 as used by tests/project_gadget/project_gadget.cu:66-68
inline void min_max_vec4(const device_vector<float4>& d_v, float4* mins, float4* maxs)
{
    detail::check(grace_minmax_f4(&d_v.data()->x, d_v.size(), &mins->x, &maxs->x, nullptr));
}

} // namespace grace

// ---- test helpers the task names as API (global namespace in the reference) -------------

// tests/helper/tree.cuh:30-43
inline void build_tree(grace::device_vector<grace::float4>& spheres, const grace::float4 low,
                       const grace::float4 high, grace::Tree& tree)
{
    grace::device_vector<float> deltas;
    deltas.resize(spheres.size() + 1);
    grace::morton_keys30_sort_sph(spheres, grace::make_float3(low.x, low.y, low.z),
                                  grace::make_float3(high.x, high.y, high.z));
    grace::euclidean_deltas_sph(spheres, deltas);
    grace::ALBVH_sph(spheres, deltas, tree);
}

// tests/helper/tree.cuh:15-25
inline void build_tree(grace::device_vector<grace::float4>& spheres, grace::Tree& tree)
{
    grace::device_vector<float> deltas;
    deltas.resize(spheres.size() + 1);
    grace::morton_keys30_sort_sph(spheres);
    grace::euclidean_deltas_sph(spheres, deltas);
    grace::ALBVH_sph(spheres, deltas, tree);
}

// tests/helper/rays.cuh:55-79
inline void orthogonal_rays_z(const size_t N_side, const grace::float4 mins,
                              const grace::float4 maxs, grace::device_vector<grace::Ray>& d_rays,
                              float* area = NULL)
{
    d_rays.resize(N_side * N_side);
    grace::detail::check(grace_rays_orthogonal_z(int(N_side), &mins.x, &maxs.x, d_rays.data(), area,
                                                 nullptr));
}

// The projection of tests/project_gadget/project_gadget.cu:58-81 as one call: bounds with
// w = 0, build_tree (sorts d_spheres), orthogonal_rays_z, trace_cumulative_sph.
inline void project_sph(grace::device_vector<grace::float4>& d_spheres, const size_t N_side,
                        const int max_per_leaf, grace::device_vector<float>& d_image)
{
    grace::float4 mins, maxs;
    grace::min_max_vec4(d_spheres, &mins, &maxs);
    mins.w = maxs.w = 0;
    grace::Tree tree(d_spheres.size(), max_per_leaf);
    build_tree(d_spheres, mins, maxs, tree);
    grace::device_vector<grace::Ray> rays;
    orthogonal_rays_z(N_side, mins, maxs, rays);
    d_image.resize(rays.size());
    grace::trace_cumulative_sph(rays, d_spheres, tree, d_image);
}
