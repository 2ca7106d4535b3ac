// Drop-in check of the range queries (an extension the reference lacks): a caller written against
// the reference's include paths and thrust::device_vector types builds the tree, then calls
// grace::range_counts_sph (with per-point radii and gather sums, and with one radius) and
// grace::range_neighbours_sph.
//   dropin_range <spheres.f32> <points.f32> <radii.f32> <weights.f32> <n_channels> <radius>
// spheres: n x 4 float32 inside the unit box, already in tree order (sorting them again keeps their
// order); points: m x 4 float32; radii: m float32; weights: n x n_channels float32.  Prints one
// digest line per output, "<name> <entries> <digest>", for a comparison with the ctypes path: the
// digest of 32-bit words v[i] is the sum of v[i] (2 i + 1) modulo 2^64.
#include "grace/cuda/range_sph.cuh"
#include "grace/cuda/nodes.h"
#include "helper/tree.cuh"

#include <thrust/device_vector.h>
#include <thrust/host_vector.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
static void print_digest(const char* name, const thrust::device_vector<T>& d)
{
    static_assert(sizeof(T) == 4, "32-bit words");
    thrust::host_vector<T> h = d;
    uint64_t sum = 0;
    for (size_t i = 0; i < h.size(); ++i) {
        uint32_t w;
        std::memcpy(&w, &h[i], 4);
        sum += uint64_t(w) * (2 * uint64_t(i) + 1);
    }
    std::printf("%s %zu %llu\n", name, h.size(), (unsigned long long)sum);
}

int main(int argc, char* argv[])
{
    if (argc < 7) { std::cerr << "usage: spheres.f32 points.f32 radii.f32 weights.f32 n_channels radius\n"; return 2; }
    std::vector<float4> h_spheres, h_points;
    std::vector<float> h_radii, h_weights;
    if (!read_all(argv[1], h_spheres) || !read_all(argv[2], h_points) || !read_all(argv[3], h_radii)
        || !read_all(argv[4], h_weights)) {
        std::cerr << "cannot read inputs\n";
        return 2;
    }
    const int n_channels = int(std::strtol(argv[5], NULL, 10));
    const float radius = std::strtof(argv[6], NULL);

    thrust::device_vector<float4> d_spheres(h_spheres.begin(), h_spheres.end());
    thrust::device_vector<float4> d_points(h_points.begin(), h_points.end());
    thrust::device_vector<float> d_radii(h_radii.begin(), h_radii.end());
    thrust::device_vector<float> d_weights(h_weights.begin(), h_weights.end());
    grace::Tree d_tree(d_spheres.size(), 32);
    build_tree(d_spheres, make_float3(0.f, 0.f, 0.f), make_float3(1.f, 1.f, 1.f), d_tree);

    thrust::device_vector<int> d_counts(d_points.size()), d_counts_one(d_points.size());
    thrust::device_vector<float> d_sums(d_points.size() * n_channels);
    grace::range_counts_sph(d_points, d_radii, d_spheres, d_tree, d_weights, n_channels, d_counts, d_sums);
    grace::range_counts_sph(d_points, radius, d_spheres, d_tree, d_counts_one);

    thrust::device_vector<int> d_offsets, d_indices;
    thrust::device_vector<float> d_d2;
    grace::range_neighbours_sph(d_points, d_radii, d_spheres, d_tree, d_offsets, d_indices, d_d2);

    // a size mismatch is std::invalid_argument
    bool threw = false;
    try {
        thrust::device_vector<float> short_radii(d_points.size() - 1);
        grace::range_counts_sph(d_points, short_radii, d_spheres, d_tree, d_counts);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    if (!threw) { std::cerr << "no std::invalid_argument for short radii\n"; return 1; }

    print_digest("counts", d_counts);
    print_digest("sums", d_sums);
    print_digest("counts_one", d_counts_one);
    print_digest("offsets", d_offsets);
    print_digest("indices", d_indices);
    print_digest("d2", d_d2);
    return 0;
}
