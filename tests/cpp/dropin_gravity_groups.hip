// Drop-in check of the gravity within groups (an extension the reference lacks): a caller written
// against the reference's include paths and thrust::device_vector types builds the tree, then calls
// grace::gravity_group_moments_sph and grace::gravity_groups_sph (the outputs alone, and with the term
// counts).
//   dropin_gravity_groups <spheres.f32> <points.f32> <masses.f32> <labels.i32> <point_labels.i32> <theta> <eps>
// spheres: n x 4 float32 inside the unit box, already in tree order (sorting them again keeps their
// order); points: m x 4 float32; masses: n float32; labels: n int32 in the spheres' order;
// point_labels: m int32.  Prints one digest line per output,
// "<name> <words> <digest>", for a comparison with the ctypes path: the digest of the output's 32-bit
// words v[i] (a double is two of them, low word first) is the sum of v[i] (2 i + 1) modulo 2^64.
#include "grace/cuda/gravity_sph.cuh"
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
    if (argc < 8) {
        std::cerr << "usage: spheres.f32 points.f32 masses.f32 labels.i32 point_labels.i32 theta eps\n";
        return 2;
    }
    std::vector<float4> h_spheres, h_points;
    std::vector<float> h_masses;
    std::vector<int> h_labels, h_point_labels;
    if (!read_all(argv[1], h_spheres) || !read_all(argv[2], h_points) || !read_all(argv[3], h_masses)
        || !read_all(argv[4], h_labels) || !read_all(argv[5], h_point_labels)) {
        std::cerr << "cannot read inputs\n";
        return 2;
    }
    const float theta = std::strtof(argv[6], NULL), eps = std::strtof(argv[7], NULL);

    thrust::device_vector<float4> d_spheres(h_spheres.begin(), h_spheres.end());
    thrust::device_vector<float4> d_points(h_points.begin(), h_points.end());
    thrust::device_vector<float> d_masses(h_masses.begin(), h_masses.end());
    thrust::device_vector<int> d_labels(h_labels.begin(), h_labels.end());
    thrust::device_vector<int> d_point_labels(h_point_labels.begin(), h_point_labels.end());
    grace::Tree d_tree(d_spheres.size(), 32);
    build_tree(d_spheres, make_float3(0.f, 0.f, 0.f), make_float3(1.f, 1.f, 1.f), d_tree);

    thrust::device_vector<float> d_moments;
    thrust::device_vector<int> d_ranges;
    grace::gravity_group_moments_sph(d_spheres, d_masses, d_labels, d_tree, d_moments, d_ranges);

    thrust::device_vector<double> d_out_only, d_out;
    thrust::device_vector<int> d_counts;
    grace::gravity_groups_sph(d_points, d_point_labels, d_spheres, d_masses, d_labels, d_tree, d_moments, d_ranges,
                              theta, eps, d_out_only);
    grace::gravity_groups_sph(d_points, d_point_labels, d_spheres, d_masses, d_labels, d_tree, d_moments, d_ranges,
                              theta, eps, d_out, d_counts);

    // labels, point labels or label ranges of the wrong size, and a negative theta, are std::invalid_argument
    int threw = 0;
    try {
        thrust::device_vector<int> short_labels(d_labels.size() - 1);
        grace::gravity_group_moments_sph(d_spheres, d_masses, short_labels, d_tree, d_moments, d_ranges);
    } catch (const std::invalid_argument&) {
        ++threw;
    }
    try {
        thrust::device_vector<int> short_point_labels(d_point_labels.size() - 1);
        grace::gravity_groups_sph(d_points, short_point_labels, d_spheres, d_masses, d_labels, d_tree, d_moments,
                                  d_ranges, theta, eps, d_out);
    } catch (const std::invalid_argument&) {
        ++threw;
    }
    try {
        thrust::device_vector<int> short_ranges(d_ranges.size() - 2);
        grace::gravity_groups_sph(d_points, d_point_labels, d_spheres, d_masses, d_labels, d_tree, d_moments,
                                  short_ranges, theta, eps, d_out);
    } catch (const std::invalid_argument&) {
        ++threw;
    }
    try {
        grace::gravity_groups_sph(d_points, d_point_labels, d_spheres, d_masses, d_labels, d_tree, d_moments, d_ranges,
                                  -1.0f, eps, d_out);
    } catch (const std::invalid_argument&) {
        ++threw;
    }
    if (threw != 4) {
        std::cerr << "no std::invalid_argument for short labels, point labels or label ranges, or a negative theta\n";
        return 1;
    }

    print_digest("moments", d_moments);
    print_digest("label_ranges", d_ranges);
    print_digest("out_only", d_out_only);
    print_digest("out", d_out);
    print_digest("counts", d_counts);
    return 0;
}
