// Drop-in check of the periodic point queries (an extension the reference lacks): a caller written
// against the reference's include paths and thrust::device_vector types builds the tree, then calls
// the grace::PeriodicBox overloads of grace::range_counts_sph (per-point radii with gather sums, and
// one radius), grace::range_neighbours_sph, grace::fof_labels_sph, grace::pair_counts_sph and
// grace::radial_profiles_sph.
//   dropin_periodic <spheres.f32> <points.f32> <radii.f32> <weights.f32> <n_channels> <radius>
//                   <linking_length> <edges.f32> <Lx> <Ly> <Lz>
// spheres: n x 4 float32 inside the unit box, already in tree order (sorting them again keeps their
// order); points: m x 4 float32; radii: m float32; weights: n x n_channels float32; edges: float32,
// ascending.  Prints one digest line per output, "<name> <words> <digest>", for a comparison with
// the ctypes path: the digest of 32-bit words v[i] is the sum of v[i] (2 i + 1) modulo 2^64.
#include "grace/cuda/fof_sph.cuh"
#include "grace/cuda/pairs_sph.cuh"
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
    static_assert(sizeof(T) % 4 == 0, "32-bit words");
    thrust::host_vector<T> h = d;
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
    if (argc < 12) {
        std::cerr << "usage: spheres.f32 points.f32 radii.f32 weights.f32 n_channels radius linking_length edges.f32 "
                     "Lx Ly Lz\n";
        return 2;
    }
    std::vector<float4> h_spheres, h_points;
    std::vector<float> h_radii, h_weights, edges;
    if (!read_all(argv[1], h_spheres) || !read_all(argv[2], h_points) || !read_all(argv[3], h_radii)
        || !read_all(argv[4], h_weights) || !read_all(argv[8], edges)) {
        std::cerr << "cannot read inputs\n";
        return 2;
    }
    const int n_channels = int(std::strtol(argv[5], NULL, 10));
    const float radius = std::strtof(argv[6], NULL);
    const float linking_length = std::strtof(argv[7], NULL);
    const grace::PeriodicBox box = { std::strtof(argv[9], NULL), std::strtof(argv[10], NULL),
                                     std::strtof(argv[11], NULL) };

    thrust::device_vector<float4> d_spheres(h_spheres.begin(), h_spheres.end());
    thrust::device_vector<float4> d_points(h_points.begin(), h_points.end());
    thrust::device_vector<float> d_radii(h_radii.begin(), h_radii.end());
    thrust::device_vector<float> d_weights(h_weights.begin(), h_weights.end());
    grace::Tree d_tree(d_spheres.size(), 32);
    build_tree(d_spheres, make_float3(0.f, 0.f, 0.f), make_float3(1.f, 1.f, 1.f), d_tree);

    thrust::device_vector<int> d_counts(d_points.size()), d_counts_one(d_points.size());
    thrust::device_vector<float> d_sums(d_points.size() * n_channels);
    grace::range_counts_sph(d_points, d_radii, d_spheres, d_tree, d_weights, n_channels, d_counts, d_sums, box);
    grace::range_counts_sph(d_points, radius, d_spheres, d_tree, d_counts_one, box);

    thrust::device_vector<int> d_offsets, d_indices;
    thrust::device_vector<float> d_d2;
    grace::range_neighbours_sph(d_points, d_radii, d_spheres, d_tree, d_offsets, d_indices, d_d2, box);

    thrust::device_vector<int> d_labels;
    grace::fof_labels_sph(d_spheres, d_tree, linking_length, d_labels, box);

    thrust::device_vector<unsigned long long> d_totals;
    grace::pair_counts_sph(d_points, edges, d_spheres, d_tree, d_totals, box);
    thrust::device_vector<int> d_shells_only, d_shells;
    thrust::device_vector<float> d_shell_sums;
    grace::radial_profiles_sph(d_points, edges, d_spheres, d_tree, d_shells_only, box);
    grace::radial_profiles_sph(d_points, edges, d_spheres, d_tree, d_shells, d_weights, n_channels, d_shell_sums, box);

    // a radius above half a period, and a negative period, are refused (std::invalid_argument)
    int threw = 0;
    try {
        grace::range_counts_sph(d_points, 0.75f, d_spheres, d_tree, d_counts_one, box);
    } catch (const std::invalid_argument&) {
        ++threw;
    }
    try {
        const grace::PeriodicBox bad = { 1.0f, -1.0f, 1.0f };
        grace::fof_labels_sph(d_spheres, d_tree, linking_length, d_labels, bad);
    } catch (const std::invalid_argument&) {
        ++threw;
    }
    if (threw != 2) { std::cerr << "no std::invalid_argument for a radius above half a period or a bad period\n"; return 1; }

    print_digest("counts", d_counts);
    print_digest("sums", d_sums);
    print_digest("counts_one", d_counts_one);
    print_digest("offsets", d_offsets);
    print_digest("indices", d_indices);
    print_digest("d2", d_d2);
    print_digest("labels", d_labels);
    print_digest("totals", d_totals);
    print_digest("shells_only", d_shells_only);
    print_digest("shells", d_shells);
    print_digest("shell_sums", d_shell_sums);
    return 0;
}
