// Drop-in check of the periodic nearest neighbours, smoothing lengths and interpolation (an extension
// the reference lacks): a caller builds the tree, then calls the grace::PeriodicBox overloads of
// grace::nearest_neighbours_sph, grace::smoothing_lengths_sph, grace::interpolate_sph (with and
// without counts) and grace::interpolate_grid_sph.  It compiles against either header set: the
// reference's include paths with thrust::device_vector (the default), or, with -DDROPIN_MIRROR, the
// HIP-free mirror grace/grace.h with grace::device_vector.
//   dropin_periodic_points <spheres.f32> <points.f32> <weights.f32> <n_channels> <k> <eta> <n_grid>
//                          <Lx> <Ly> <Lz>
// spheres: n x 4 float32 inside the unit box, already in tree order (sorting them again keeps their
// order); points: m x 4 float32; weights: n x n_channels float32; the grid is n_grid^3 points at
// spacing 1 / n_grid from the origin.  Prints one digest line per output, "<name> <words> <digest>",
// for a comparison with the ctypes path: the digest of 32-bit words v[i] is the sum of
// v[i] (2 i + 1) modulo 2^64.
#ifdef DROPIN_MIRROR
#include "grace/grace.h"
template <typename T> using dvec = grace::device_vector<T>;
typedef grace::float4 point4;
using grace::make_float3;
template <typename T> static std::vector<T> to_host(const dvec<T>& d) { return d.to_host(); }
static void build_unit_tree(dvec<point4>& s, grace::Tree& tree)
{
    build_tree(s, grace::make_float4(0.f, 0.f, 0.f, 0.f), grace::make_float4(1.f, 1.f, 1.f, 0.f), tree);
}
#else
#include "grace/cuda/interpolate_sph.cuh"
#include "grace/cuda/neighbours_sph.cuh"
#include "grace/cuda/nodes.h"
#include "helper/tree.cuh"

#include <thrust/device_vector.h>
#include <thrust/host_vector.h>
template <typename T> using dvec = thrust::device_vector<T>;
typedef float4 point4;
template <typename T> static std::vector<T> to_host(const dvec<T>& d)
{
    thrust::host_vector<T> h = d;
    return std::vector<T>(h.begin(), h.end());
}
static void build_unit_tree(dvec<point4>& s, grace::Tree& tree)
{
    build_tree(s, make_float3(0.f, 0.f, 0.f), make_float3(1.f, 1.f, 1.f), tree);
}
#endif

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
static void print_digest(const char* name, const dvec<T>& d)
{
    static_assert(sizeof(T) % 4 == 0, "32-bit words");
    const std::vector<T> h = to_host(d);
    const size_t words = h.size() * (sizeof(T) / 4);
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(h.data());
    uint64_t sum = 0;
    for (size_t i = 0; i < words; ++i) {
        uint32_t w;
        std::memcpy(&w, bytes + 4 * i, 4);
        sum += uint64_t(w) * (2 * uint64_t(i) + 1);
    }
    std::printf("%s %zu %llu\n", name, words, (unsigned long long)sum);
}

int main(int argc, char* argv[])
{
    if (argc < 11) {
        std::cerr << "usage: spheres.f32 points.f32 weights.f32 n_channels k eta n_grid Lx Ly Lz\n";
        return 2;
    }
    std::vector<point4> h_spheres, h_points;
    std::vector<float> h_weights;
    if (!read_all(argv[1], h_spheres) || !read_all(argv[2], h_points) || !read_all(argv[3], h_weights)) {
        std::cerr << "cannot read inputs\n";
        return 2;
    }
    const int n_channels = int(std::strtol(argv[4], NULL, 10));
    const int k = int(std::strtol(argv[5], NULL, 10));
    const float eta = std::strtof(argv[6], NULL);
    const int n_grid = int(std::strtol(argv[7], NULL, 10));
    const grace::PeriodicBox box = { std::strtof(argv[8], NULL), std::strtof(argv[9], NULL),
                                     std::strtof(argv[10], NULL) };

    dvec<point4> d_spheres(h_spheres);
    dvec<point4> d_points(h_points);
    dvec<float> d_weights(h_weights);
    grace::Tree d_tree(d_spheres.size(), 32);
    build_unit_tree(d_spheres, d_tree);

    dvec<int> d_indices(d_points.size() * k);
    dvec<float> d_d2(d_points.size() * k), d_h(d_spheres.size());
    grace::nearest_neighbours_sph(d_points, d_spheres, d_tree, k, d_indices, d_d2, box);
    grace::smoothing_lengths_sph(d_spheres, d_tree, k, eta, d_h, box);

    dvec<float> d_out(d_points.size() * n_channels), d_out_only(d_points.size() * n_channels);
    dvec<int> d_counts(d_points.size());
    grace::interpolate_sph(d_points, d_spheres, d_tree, d_weights, n_channels, d_out, d_counts, box);
    grace::interpolate_sph(d_points, d_spheres, d_tree, d_weights, n_channels, d_out_only, box);

    const float dx = 1.0f / float(n_grid);
    dvec<float> d_grid(size_t(n_grid) * n_grid * n_grid * n_channels);
    grace::interpolate_grid_sph(make_float3(0.f, 0.f, 0.f), make_float3(dx, 0.f, 0.f), make_float3(0.f, dx, 0.f),
                                make_float3(0.f, 0.f, dx), n_grid, n_grid, n_grid, d_spheres, d_tree, d_weights,
                                n_channels, d_grid, box);

    // a bad period is refused (std::invalid_argument) by both families
    int threw = 0;
    const grace::PeriodicBox bad = { 1.0f, -1.0f, 1.0f };
    try {
        grace::smoothing_lengths_sph(d_spheres, d_tree, k, eta, d_h, bad);
    } catch (const std::invalid_argument&) {
        ++threw;
    }
    try {
        grace::interpolate_sph(d_points, d_spheres, d_tree, d_weights, n_channels, d_out_only, bad);
    } catch (const std::invalid_argument&) {
        ++threw;
    }
    if (threw != 2) { std::cerr << "no std::invalid_argument for a bad period\n"; return 1; }

    print_digest("indices", d_indices);
    print_digest("d2", d_d2);
    print_digest("h", d_h);
    print_digest("out", d_out);
    print_digest("out_only", d_out_only);
    print_digest("counts", d_counts);
    print_digest("grid", d_grid);
    return 0;
}
