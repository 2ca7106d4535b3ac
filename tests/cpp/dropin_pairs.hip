// Drop-in check of the pair counts and radial profiles (an extension the reference lacks): a caller
// written against the reference's include paths and thrust::device_vector types builds the tree,
// then calls grace::pair_counts_sph and grace::radial_profiles_sph (counts alone, and counts with
// sums of weights).
//   dropin_pairs <spheres.f32> <points.f32> <weights.f32> <n_channels> <edges.f32>
// spheres: n x 4 float32 inside the unit box, already in tree order (sorting them again keeps their
// order); points: m x 4 float32; weights: n x n_channels float32; edges: float32, ascending.  Prints
// one digest line per output, "<name> <words> <digest>", for a comparison with the ctypes path: the
// digest of the output's 32-bit words v[i] (a 64-bit total is two of them, low word first) is the
// sum of v[i] (2 i + 1) modulo 2^64.
#include "grace/cuda/pairs_sph.cuh"
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
    if (argc < 6) { std::cerr << "usage: spheres.f32 points.f32 weights.f32 n_channels edges.f32\n"; return 2; }
    std::vector<float4> h_spheres, h_points;
    std::vector<float> h_weights, edges;
    if (!read_all(argv[1], h_spheres) || !read_all(argv[2], h_points) || !read_all(argv[3], h_weights)
        || !read_all(argv[5], edges)) {
        std::cerr << "cannot read inputs\n";
        return 2;
    }
    const int n_channels = int(std::strtol(argv[4], NULL, 10));

    thrust::device_vector<float4> d_spheres(h_spheres.begin(), h_spheres.end());
    thrust::device_vector<float4> d_points(h_points.begin(), h_points.end());
    thrust::device_vector<float> d_weights(h_weights.begin(), h_weights.end());
    grace::Tree d_tree(d_spheres.size(), 32);
    build_tree(d_spheres, make_float3(0.f, 0.f, 0.f), make_float3(1.f, 1.f, 1.f), d_tree);

    thrust::device_vector<unsigned long long> d_totals;
    grace::pair_counts_sph(d_points, edges, d_spheres, d_tree, d_totals);

    thrust::device_vector<int> d_counts_only, d_counts;
    thrust::device_vector<float> d_sums;
    grace::radial_profiles_sph(d_points, edges, d_spheres, d_tree, d_counts_only);
    grace::radial_profiles_sph(d_points, edges, d_spheres, d_tree, d_counts, d_weights, n_channels, d_sums);

    // edges that do not ascend, and weights of the wrong size, are std::invalid_argument
    int threw = 0;
    try {
        std::vector<float> bad(edges.rbegin(), edges.rend());
        bad.push_back(bad.back());
        thrust::device_vector<unsigned long long> d_none;
        grace::pair_counts_sph(d_points, bad, d_spheres, d_tree, d_none);
    } catch (const std::invalid_argument&) {
        ++threw;
    }
    try {
        thrust::device_vector<float> short_weights(d_weights.size() - 1);
        grace::radial_profiles_sph(d_points, edges, d_spheres, d_tree, d_counts, short_weights, n_channels, d_sums);
    } catch (const std::invalid_argument&) {
        ++threw;
    }
    if (threw != 2) { std::cerr << "no std::invalid_argument for bad edges or short weights\n"; return 1; }

    print_digest("totals", d_totals);
    print_digest("counts_only", d_counts_only);
    print_digest("counts", d_counts);
    print_digest("sums", d_sums);
    return 0;
}
