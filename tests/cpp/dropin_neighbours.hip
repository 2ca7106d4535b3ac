// Drop-in check of nearest neighbours and smoothing lengths (an extension the reference lacks): a
// caller written against the reference's include paths and thrust::device_vector types builds the
// tree, then calls grace::nearest_neighbours_sph and grace::smoothing_lengths_sph.
//   dropin_neighbours <spheres.f32> <points.f32> <k> <eta> <out_dir>
// spheres: n x 4 float32 inside the unit box, already in tree order (sorting them again keeps their
// order); points: m x 4 float32.  Outputs are written raw to out_dir/{indices.i32, d2.f32, h.f32}
// for a bit-for-bit comparison with the ctypes path.
#include "grace/cuda/neighbours_sph.cuh"
#include "grace/cuda/nodes.h"
#include "helper/tree.cuh"

#include <thrust/device_vector.h>
#include <thrust/host_vector.h>

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <stdexcept>
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
    if (argc < 6) { std::cerr << "usage: spheres.f32 points.f32 k eta out_dir\n"; return 2; }
    std::vector<float4> h_spheres, h_points;
    if (!read_all(argv[1], h_spheres) || !read_all(argv[2], h_points)) {
        std::cerr << "cannot read inputs\n";
        return 2;
    }
    const int k = int(std::strtol(argv[3], NULL, 10));
    const float eta = std::strtof(argv[4], NULL);
    const std::string out = argv[5];

    thrust::device_vector<float4> d_spheres(h_spheres.begin(), h_spheres.end());
    thrust::device_vector<float4> d_points(h_points.begin(), h_points.end());
    grace::Tree d_tree(d_spheres.size(), 32);
    build_tree(d_spheres, make_float3(0.f, 0.f, 0.f), make_float3(1.f, 1.f, 1.f), d_tree);

    thrust::device_vector<int> d_indices(d_points.size() * k);
    thrust::device_vector<float> d_d2(d_points.size() * k), d_h(d_spheres.size());
    grace::nearest_neighbours_sph(d_points, d_spheres, d_tree, k, d_indices, d_d2);
    grace::smoothing_lengths_sph(d_spheres, d_tree, k, eta, d_h);

    // a size mismatch is std::invalid_argument
    bool threw = false;
    try {
        thrust::device_vector<float> short_h(d_spheres.size() - 1);
        grace::smoothing_lengths_sph(d_spheres, d_tree, k, eta, short_h);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    if (!threw) { std::cerr << "no std::invalid_argument for a short output\n"; return 1; }

    if (!write_all(out + "/indices.i32", d_indices) || !write_all(out + "/d2.f32", d_d2)
        || !write_all(out + "/h.f32", d_h))
        return 1;
    std::cout << "dropin_neighbours ok: " << d_points.size() << " points, k = " << k << "\n";
    return 0;
}
