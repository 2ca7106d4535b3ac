// Drop-in check of the sightline spectra (an extension the reference lacks): a caller written against
// the reference's include paths and thrust::device_vector types builds the tree, casts HEALPix rays
// from one observer through the scene and calls grace::trace_spectra_sph with n_channels amounts and
// Doppler widths per sphere and one velocity per sphere, all in tree order, on a periodic grid.
//   dropin_spectra <spheres.f32> <nside> <amount.f32> <width.f32> <velocity.f32> <n_channels>
//                  <n_bins> <v0> <dv> <hubble>
// spheres: n x 4 float32 inside the unit box, already in tree order (sorting them again keeps their
// order: their Morton keys are ascending); the observer sits at (0.45, 0.55, 0.5), rays of length 1;
// amount (>= 0) and width: n x n_channels float32; velocity: n x 3 float32.  Checks conservation on
// the device's output -- dv sum_j tau[r, c, j] against column[r, c], which in periodic mode differ
// by the outputs' fp32 roundings only: both sides are sums of non-negative terms, so by at most
// 2^-24 of the column each, and 4 x 2^-24 is allowed -- and prints an FNV-1a checksum of tau's and of
// column's bits for a bit-for-bit comparison with the ctypes path.
#include "grace/cuda/nodes.h"
#include "grace/cuda/trace_sph.cuh"
#include "grace/ray.h"
#include "grace_hip.h"
#include "helper/tree.cuh"

#include <thrust/device_vector.h>
#include <thrust/equal.h>
#include <thrust/host_vector.h>

#include <cmath>
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

static unsigned long long fnv1a(const thrust::host_vector<float>& v)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < v.size(); ++i) {
        unsigned int u; const float x = v[i]; std::memcpy(&u, &x, 4);
        for (int b = 0; b < 4; ++b) { h ^= (u >> (8 * b)) & 0xffu; h *= 1099511628211ull; }
    }
    return h;
}

int main(int argc, char* argv[])
{
    if (argc < 11) {
        std::cerr << "usage: spheres.f32 nside amount.f32 width.f32 velocity.f32 n_channels n_bins v0 dv hubble\n";
        return 2;
    }
    std::vector<float4> h_spheres;
    std::vector<float> h_amount, h_width, h_velocity;
    if (!read_all(argv[1], h_spheres) || !read_all(argv[3], h_amount) || !read_all(argv[4], h_width)
        || !read_all(argv[5], h_velocity)) {
        std::cerr << "cannot read inputs\n";
        return 2;
    }
    const int nside = int(std::strtol(argv[2], NULL, 10));
    const int n_channels = int(std::strtol(argv[6], NULL, 10));
    grace::SpectrumGrid grid;
    grid.n_bins = int(std::strtol(argv[7], NULL, 10));
    grid.v0 = std::strtod(argv[8], NULL);
    grid.dv = std::strtod(argv[9], NULL);
    grid.hubble = std::strtod(argv[10], NULL);
    grid.periodic = 1;

    thrust::device_vector<float4> d_spheres(h_spheres.begin(), h_spheres.end());
    thrust::device_vector<float> d_amount(h_amount.begin(), h_amount.end());
    thrust::device_vector<float> d_width(h_width.begin(), h_width.end());
    thrust::device_vector<float> d_velocity(h_velocity.begin(), h_velocity.end());
    grace::Tree d_tree(d_spheres.size(), 32);
    build_tree(d_spheres, make_float3(0.f, 0.f, 0.f), make_float3(1.f, 1.f, 1.f), d_tree);

    thrust::device_vector<grace::Ray> d_rays(size_t(12) * nside * nside);
    if (grace_rays_healpix(nside, 0.45f, 0.55f, 0.5f, 1.0f, thrust::raw_pointer_cast(d_rays.data()), NULL) != GRACE_OK) {
        std::cerr << "grace_rays_healpix: " << grace_last_error() << "\n";
        return 1;
    }

    const size_t per_ray = size_t(n_channels) * size_t(grid.n_bins);
    thrust::device_vector<float> d_tau(d_rays.size() * per_ray), d_column(d_rays.size() * n_channels);
    grace::trace_spectra_sph(d_rays, d_spheres, d_tree, d_amount, d_width, d_velocity, n_channels, grid, d_tau,
                             &d_column);
    // without the optional output: the same spectra
    thrust::device_vector<float> d_again(d_tau.size());
    grace::trace_spectra_sph(d_rays, d_spheres, d_tree, d_amount, d_width, d_velocity, n_channels, grid, d_again);
    if (!thrust::equal(d_tau.begin(), d_tau.end(), d_again.begin())) {
        std::cerr << "the spectra depend on the optional output\n";
        return 1;
    }

    // a size mismatch is std::invalid_argument
    bool threw = false;
    try {
        thrust::device_vector<float> short_out(d_tau.size() - 1);
        grace::trace_spectra_sph(d_rays, d_spheres, d_tree, d_amount, d_width, d_velocity, n_channels, grid, short_out);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    if (!threw) { std::cerr << "no std::invalid_argument for a short output\n"; return 1; }
    threw = false;
    try {
        grace::trace_spectra_sph(d_rays, d_spheres, d_tree, d_amount, d_width, d_velocity, 17, grid, d_tau);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    if (!threw) { std::cerr << "no std::invalid_argument for 17 channels\n"; return 1; }

    thrust::host_vector<float> h_tau = d_tau, h_column = d_column;
    double worst = 0.0;
    size_t lit = 0;
    for (size_t rc = 0; rc < h_column.size(); ++rc) {
        double sum = 0.0;
        for (int j = 0; j < grid.n_bins; ++j) sum += double(h_tau[rc * grid.n_bins + j]);
        const double col = double(h_column[rc]), err = std::fabs(grid.dv * sum - col);
        if (col > 0.0) { ++lit; if (err / col > worst) worst = err / col; }
        if (err > 4.0 * std::ldexp(col, -24)) {
            std::cerr << "ray * channel " << rc << ": dv sum tau = " << grid.dv * sum << ", column = " << col << "\n";
            return 1;
        }
    }
    if (lit == 0) { std::cerr << "no ray hit anything\n"; return 1; }
    std::printf("tau %016llx\ncolumn %016llx\n", fnv1a(h_tau), fnv1a(h_column));
    std::printf("dropin_spectra ok: %zu rays, %d channels, %d bins; conservation within %.3g of the column\n",
                d_rays.size(), n_channels, grid.n_bins, worst);
    return 0;
}
