// Drop-in check of SPH interpolation at points (an extension the reference lacks): a caller written
// against the reference's include paths and thrust::device_vector types builds the tree, then calls
// grace::interpolate_sph (with and without counts) and grace::interpolate_grid_sph.
//   dropin_interpolate <spheres.f32> <points.f32> <weights.f32> <n_channels> <out_dir>
// spheres: n x 4 float32 inside the unit box, already in tree order (sorting them again keeps their
// order); points: m x 4 float32; weights: n x n_channels float32.  Outputs are written raw to
// out_dir/{points.f32, counts.i32, grid.f32} (grid: 16 x 32 x 3 lattice over the unit box) for a
// bit-for-bit comparison with the ctypes path.
#include "grace/cuda/interpolate_sph.cuh"
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
    if (argc < 6) { std::cerr << "usage: spheres.f32 points.f32 weights.f32 n_channels out_dir\n"; return 2; }
    std::vector<float4> h_spheres, h_points;
    std::vector<float> h_weights;
    if (!read_all(argv[1], h_spheres) || !read_all(argv[2], h_points) || !read_all(argv[3], h_weights)) {
        std::cerr << "cannot read inputs\n";
        return 2;
    }
    const int n_channels = int(std::strtol(argv[4], NULL, 10));
    const std::string out = argv[5];

    thrust::device_vector<float4> d_spheres(h_spheres.begin(), h_spheres.end());
    thrust::device_vector<float4> d_points(h_points.begin(), h_points.end());
    thrust::device_vector<float> d_weights(h_weights.begin(), h_weights.end());
    grace::Tree d_tree(d_spheres.size(), 32);
    build_tree(d_spheres, make_float3(0.f, 0.f, 0.f), make_float3(1.f, 1.f, 1.f), d_tree);

    thrust::device_vector<float> d_out(d_points.size() * n_channels), d_out2(d_points.size() * n_channels);
    thrust::device_vector<int> d_counts(d_points.size());
    grace::interpolate_sph(d_points, d_spheres, d_tree, d_weights, n_channels, d_out, d_counts);
    grace::interpolate_sph(d_points, d_spheres, d_tree, d_weights, n_channels, d_out2);
    if (!(thrust::host_vector<float>(d_out) == thrust::host_vector<float>(d_out2))) {
        std::cerr << "the counts overload changed the field\n";
        return 1;
    }

    const int nx = 16, ny = 32, nz = 3;   // (steps exact in binary)
    thrust::device_vector<float> d_grid(size_t(nx) * ny * nz * n_channels);
    grace::interpolate_grid_sph(make_float3(0.f, 0.f, 0.25f), make_float3(1.f / nx, 0.f, 0.f),
                                make_float3(0.f, 1.f / ny, 0.f), make_float3(0.f, 0.f, 0.25f),
                                make_int3(nx, ny, nz), d_spheres, d_tree, d_weights, n_channels, d_grid);

    // a size mismatch is std::invalid_argument
    bool threw = false;
    try {
        thrust::device_vector<float> short_out(d_points.size() * n_channels - 1);
        grace::interpolate_sph(d_points, d_spheres, d_tree, d_weights, n_channels, short_out);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    if (!threw) { std::cerr << "no std::invalid_argument for a short output\n"; return 1; }

    if (!write_all(out + "/points.f32", d_out) || !write_all(out + "/counts.i32", d_counts)
        || !write_all(out + "/grid.f32", d_grid))
        return 1;
    std::cout << "dropin_interpolate ok: " << d_points.size() << " points, " << n_channels << " channels\n";
    return 0;
}
