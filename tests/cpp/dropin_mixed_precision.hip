// Drop-in check of the mixed-precision SPH traces (Real4 = float4, Real = double): a caller
// written against the reference's include paths and thrust::device_vector types instantiates
// trace_cumulative_sph<float4, double>, trace_sph<float4, int, double> and
// trace_with_sentinels_sph<float4, int, double>, then sorts the per-hit outputs by distance and
// takes the exclusive segmented scan of the integrals -- the chain of
// tests/project_gadget/project_gadget.cu with double outputs.
//   dropin_mixed_precision <spheres.f32> <rays.f32> <max_per_leaf> <out_dir>
// spheres: n x 4 float32 inside the unit box (sorted here, by build_tree over [0, 1]^3); rays:
// m x 7 float32 (grace::Ray), m a multiple of 32.  Every output is written raw to out_dir so
// that the test can compare it bit for bit with the ctypes path.
#include "grace/cuda/nodes.h"
#include "grace/cuda/scan.cuh"
#include "grace/cuda/sort.cuh"
#include "grace/cuda/trace_sph.cuh"
#include "grace/ray.h"
#include "helper/tree.cuh"

#include <thrust/device_vector.h>
#include <thrust/host_vector.h>

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

template <typename T>
static bool read_all(const std::string& path, std::vector<T>& out)
{
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out.resize(size_t(bytes) / sizeof(T));
    const bool ok = std::fread(out.data(), sizeof(T), out.size(), f) == out.size();
    std::fclose(f);
    return ok;
}

template <typename T>
static bool write_all(const std::string& path, const thrust::device_vector<T>& d)
{
    thrust::host_vector<T> h = d;
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(thrust::raw_pointer_cast(h.data()), sizeof(T), h.size(), f) == h.size();
    std::fclose(f);
    return ok;
}

int main(int argc, char* argv[])
{
    if (argc < 5) { std::cerr << "usage: spheres.f32 rays.f32 max_per_leaf out_dir\n"; return 2; }
    std::vector<float4> h_spheres;
    std::vector<grace::Ray> h_rays;
    if (!read_all(argv[1], h_spheres) || !read_all(argv[2], h_rays)) { std::cerr << "cannot read inputs\n"; return 2; }
    const int max_per_leaf = int(std::strtol(argv[3], NULL, 10));
    const std::string out = argv[4];

    thrust::device_vector<float4> d_spheres(h_spheres.begin(), h_spheres.end());
    thrust::device_vector<grace::Ray> d_rays(h_rays.begin(), h_rays.end());
    grace::Tree d_tree(d_spheres.size(), max_per_leaf);
    build_tree(d_spheres, make_float3(0.f, 0.f, 0.f), make_float3(1.f, 1.f, 1.f), d_tree);

    thrust::device_vector<double> d_cumulated(d_rays.size());
    grace::trace_cumulative_sph(d_rays, d_spheres, d_tree, d_cumulated);

    thrust::device_vector<int> d_offsets(d_rays.size());
    thrust::device_vector<int> d_indices;
    thrust::device_vector<double> d_integrals, d_distances;
    grace::trace_sph(d_rays, d_spheres, d_tree, d_offsets, d_indices, d_integrals, d_distances);
    bool ok = write_all(out + "/cum.f64", d_cumulated) && write_all(out + "/off.i32", d_offsets)
        && write_all(out + "/idx.i32", d_indices) && write_all(out + "/w.f64", d_integrals)
        && write_all(out + "/d.f64", d_distances);

    grace::sort_by_distance(d_distances, d_offsets, d_indices, d_integrals);
    thrust::device_vector<double> d_scanned(d_integrals.size());
    grace::exclusive_segmented_scan(d_offsets, d_integrals, d_scanned);
    ok = ok && write_all(out + "/sorted_idx.i32", d_indices) && write_all(out + "/sorted_w.f64", d_integrals)
        && write_all(out + "/sorted_d.f64", d_distances) && write_all(out + "/scan.f64", d_scanned);

    thrust::device_vector<int> s_offsets(d_rays.size());
    thrust::device_vector<int> s_indices;
    thrust::device_vector<double> s_integrals, s_distances;
    grace::trace_with_sentinels_sph(d_rays, d_spheres, d_tree, s_offsets, s_indices, -1,
                                    s_integrals, -2.0, s_distances, -3.0);
    ok = ok && write_all(out + "/s_off.i32", s_offsets) && write_all(out + "/s_idx.i32", s_indices)
        && write_all(out + "/s_w.f64", s_integrals) && write_all(out + "/s_d.f64", s_distances);
    if (!ok) { std::cerr << "cannot write outputs\n"; return 3; }
    std::cout << "rays " << d_rays.size() << ", hits " << d_indices.size() << std::endl;
    return EXIT_SUCCESS;
}
