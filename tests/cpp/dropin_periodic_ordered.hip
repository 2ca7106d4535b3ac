// Drop-in check of the depth-ordered traces in a periodic box (an extension the reference lacks): a
// caller makes a grace::PeriodicScene of its spheres and calls the scene overloads of
// grace::trace_emission_absorption_sph, grace::trace_absorption_deposit_sph and grace::trace_spectra_sph.
// It compiles against either header set: the reference's include paths with thrust::device_vector
// (the default), or, with -DDROPIN_MIRROR, the HIP-free mirror grace/grace.h with grace::device_vector.
//   dropin_periodic_ordered <spheres.f32> <rays.f32> <fields.f32> <luminosity.f32> <ox> <oy> <oz> <Lx> <Ly> <Lz>
// spheres: n x 4 float32 inside the box, in any order; rays: m x 7 float32, any m; fields: n x 10
// float32 per sphere, in the order of the spheres -- emission (2 channels), absorption, absorption per
// channel (2), amount, width, velocity (3); luminosity: m x 2 float32.  The velocity grid is fixed
// below.  Prints one digest line per output, "<name> <words> <digest>", for a comparison with the
// ctypes path: the digest of 32-bit words v[i] is the sum of v[i] (2 i + 1) modulo 2^64.
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

// columns [first, first + count) of the n x 10 fields
static std::vector<float> columns(const std::vector<float>& fields, const size_t n, const int first, const int count)
{
    std::vector<float> out(n * count);
    for (size_t i = 0; i < n; ++i)
        for (int c = 0; c < count; ++c) out[i * count + c] = fields[i * 10 + first + c];
    return out;
}

int main(int argc, char* argv[])
{
    if (argc < 11) {
        std::cerr << "usage: spheres.f32 rays.f32 fields.f32 luminosity.f32 ox oy oz Lx Ly Lz\n";
        return 2;
    }
    std::vector<point4> h_spheres;
    std::vector<grace::Ray> h_rays;
    std::vector<float> h_fields, h_luminosity;
    if (!read_all(argv[1], h_spheres) || !read_all(argv[2], h_rays) || !read_all(argv[3], h_fields)
        || !read_all(argv[4], h_luminosity) || h_fields.size() != h_spheres.size() * 10
        || h_luminosity.size() != h_rays.size() * 2) {
        std::cerr << "cannot read inputs\n";
        return 2;
    }
    const grace::PeriodicDomain domain = { std::strtof(argv[5], NULL), std::strtof(argv[6], NULL),
                                           std::strtof(argv[7], NULL),
                                           { std::strtof(argv[8], NULL), std::strtof(argv[9], NULL),
                                             std::strtof(argv[10], NULL) } };
    const size_t n = h_spheres.size(), m = h_rays.size();

    dvec<point4> d_spheres(h_spheres);
    dvec<grace::Ray> d_rays(h_rays);
    dvec<float> d_emission(columns(h_fields, n, 0, 2)), d_absorption(columns(h_fields, n, 2, 1)),
        d_absorption2(columns(h_fields, n, 3, 2)), d_amount(columns(h_fields, n, 5, 1)),
        d_width(columns(h_fields, n, 6, 1)), d_velocity(columns(h_fields, n, 7, 3)), d_luminosity(h_luminosity);

    grace::PeriodicScene scene;
    grace::periodic_scene_sph(d_spheres, domain, 32, scene);

    dvec<float> d_out(m * 2), d_tau(m), d_transmitted(m * 2);
    dvec<double> d_deposit(n * 2), d_quantum(2);
    grace::trace_emission_absorption_sph(d_rays, scene, d_emission, 2, d_absorption, d_out, &d_tau);
    grace::trace_absorption_deposit_sph(d_rays, scene, d_luminosity, 2, d_absorption2, d_deposit, &d_transmitted,
                                        &d_quantum);
    grace::SpectrumGrid grid;
    grid.v0 = -200.0; grid.dv = 10.0; grid.n_bins = 64; grid.periodic = 1; grid.hubble = 50.0;
    dvec<float> d_spectra(m * 64), d_column(m);
    grace::trace_spectra_sph(d_rays, scene, d_amount, d_width, d_velocity, 1, grid, d_spectra, &d_column);

    // per-particle arrays sized for the images instead of the caller's spheres are refused
    int threw = 0;
    dvec<float> d_wrong(scene.spheres.size() + 1);
    try {
        grace::trace_emission_absorption_sph(d_rays, scene, d_emission, 2, d_wrong, d_out);
    } catch (const std::invalid_argument&) {
        ++threw;
    }
    if (threw != 1) { std::cerr << "no std::invalid_argument for a wrong-length array\n"; return 1; }

    print_digest("emission_absorption", d_out);
    print_digest("tau", d_tau);
    print_digest("deposit", d_deposit);
    print_digest("transmitted", d_transmitted);
    print_digest("quantum", d_quantum);
    print_digest("spectra", d_spectra);
    print_digest("column", d_column);
    return 0;
}
