// Drop-in check of the periodic traces (an extension the reference lacks): a caller makes a
// grace::PeriodicScene of its spheres (grace::periodic_scene_sph) and calls the scene overloads of
// grace::trace_hitcounts_sph, grace::trace_cumulative_sph and grace::trace_cumulative_weighted_sph.
// It compiles against either header set: the reference's include paths with thrust::device_vector
// (the default), or, with -DDROPIN_MIRROR, the HIP-free mirror grace/grace.h with grace::device_vector.
//   dropin_periodic_trace <spheres.f32> <rays.f32> <weights.f32> <n_channels> <ox> <oy> <oz> <Lx> <Ly> <Lz>
// spheres: n x 4 float32 inside the box, in any order; rays: m x 7 float32, any m; weights:
// n x n_channels float32 in the order of the spheres.  Prints one digest line per output,
// "<name> <words> <digest>", for a comparison with the ctypes path: the digest of 32-bit words v[i] is
// the sum of v[i] (2 i + 1) modulo 2^64.
#ifdef DROPIN_MIRROR
#include "grace/grace.h"
template <typename T> using dvec = grace::device_vector<T>;
typedef grace::float4 point4;
template <typename T> static std::vector<T> to_host(const dvec<T>& d) { return d.to_host(); }
#else
#include "grace/cuda/periodic_trace.cuh"

#include <thrust/device_vector.h>
#include <thrust/host_vector.h>
template <typename T> using dvec = thrust::device_vector<T>;
typedef float4 point4;
template <typename T> static std::vector<T> to_host(const dvec<T>& d)
{
    thrust::host_vector<T> h = d;
    return std::vector<T>(h.begin(), h.end());
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
        std::cerr << "usage: spheres.f32 rays.f32 weights.f32 n_channels ox oy oz Lx Ly Lz\n";
        return 2;
    }
    std::vector<point4> h_spheres;
    std::vector<grace::Ray> h_rays;
    std::vector<float> h_weights;
    if (!read_all(argv[1], h_spheres) || !read_all(argv[2], h_rays) || !read_all(argv[3], h_weights)) {
        std::cerr << "cannot read inputs\n";
        return 2;
    }
    const int n_channels = int(std::strtol(argv[4], NULL, 10));
    const grace::PeriodicDomain domain = { std::strtof(argv[5], NULL), std::strtof(argv[6], NULL),
                                           std::strtof(argv[7], NULL),
                                           { std::strtof(argv[8], NULL), std::strtof(argv[9], NULL),
                                             std::strtof(argv[10], NULL) } };

    dvec<point4> d_spheres(h_spheres);
    dvec<grace::Ray> d_rays(h_rays);
    dvec<float> d_weights(h_weights);

    grace::PeriodicScene scene;
    grace::periodic_scene_sph(d_spheres, domain, 32, scene);

    dvec<int> d_counts(d_rays.size());
    dvec<float> d_cumulated(d_rays.size()), d_weighted(d_rays.size() * n_channels);
    grace::trace_hitcounts_sph(d_rays, scene, d_counts);
    grace::trace_cumulative_sph(d_rays, scene, d_cumulated);
    grace::trace_cumulative_weighted_sph(d_rays, scene, d_weights, n_channels, d_weighted);

    // a bad period and a sphere outside the box are refused (std::invalid_argument)
    int threw = 0;
    grace::PeriodicDomain bad = domain;
    bad.period.ly = -1.0f;
    grace::PeriodicScene other;
    try {
        grace::periodic_scene_sph(d_spheres, bad, 32, other);
    } catch (const std::invalid_argument&) {
        ++threw;
    }
    bad = domain;
    bad.ox = domain.ox + 0.5f * domain.period.lx;       // half the spheres are now outside
    try {
        grace::periodic_scene_sph(d_spheres, bad, 32, other);
    } catch (const std::invalid_argument&) {
        ++threw;
    }
    if (threw != 2) { std::cerr << "no std::invalid_argument for a bad box\n"; return 1; }

    print_digest("images", scene.spheres);
    print_digest("source", scene.source);
    print_digest("counts", d_counts);
    print_digest("cumulated", d_cumulated);
    print_digest("weighted", d_weighted);
    return 0;
}
