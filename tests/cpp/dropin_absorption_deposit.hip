// Drop-in check of the absorption-deposit trace (an extension the reference lacks): a caller written
// against the reference's include paths and thrust::device_vector types builds the tree, casts
// HEALPix rays from one source through the scene (the reference's RayVectorGeneration shape) and
// calls grace::trace_absorption_deposit_sph with n_channels luminosities per ray and absorption
// coefficients per sphere in tree order -- one photon-conserving sweep.
//   dropin_absorption_deposit <spheres.f32> <nside> <luminosity.f32> <n_channels> <absorption.f32>
// spheres: n x 4 float32 inside the unit box, already in tree order (sorting them again keeps their
// order: their Morton keys are ascending); the source sits at (0.45, 0.55, 0.5), rays of length 1;
// luminosity: 12 nside^2 x n_channels float32; absorption: n x n_channels float32.  Prints the bits
// of every output, one hexadecimal word per line ("q", "d" and "t" lines: quantum, deposit,
// transmitted, each in array order), for a bit-for-bit comparison with the ctypes path.
#include "grace/cuda/nodes.h"
#include "grace/cuda/trace_sph.cuh"
#include "grace/ray.h"
#include "grace_hip.h"
#include "helper/tree.cuh"

#include <thrust/device_vector.h>
#include <thrust/equal.h>
#include <thrust/host_vector.h>

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

int main(int argc, char* argv[])
{
    if (argc < 6) { std::cerr << "usage: spheres.f32 nside luminosity.f32 n_channels absorption.f32\n"; return 2; }
    std::vector<float4> h_spheres;
    std::vector<float> h_luminosity, h_absorption;
    if (!read_all(argv[1], h_spheres) || !read_all(argv[3], h_luminosity) || !read_all(argv[5], h_absorption)) {
        std::cerr << "cannot read inputs\n";
        return 2;
    }
    const int nside = int(std::strtol(argv[2], NULL, 10));
    const int n_channels = int(std::strtol(argv[4], NULL, 10));

    thrust::device_vector<float4> d_spheres(h_spheres.begin(), h_spheres.end());
    thrust::device_vector<float> d_luminosity(h_luminosity.begin(), h_luminosity.end());
    thrust::device_vector<float> d_absorption(h_absorption.begin(), h_absorption.end());
    grace::Tree d_tree(d_spheres.size(), 32);
    build_tree(d_spheres, make_float3(0.f, 0.f, 0.f), make_float3(1.f, 1.f, 1.f), d_tree);

    thrust::device_vector<grace::Ray> d_rays(size_t(12) * nside * nside);
    if (grace_rays_healpix(nside, 0.45f, 0.55f, 0.5f, 1.0f, thrust::raw_pointer_cast(d_rays.data()), NULL) != GRACE_OK) {
        std::cerr << "grace_rays_healpix: " << grace_last_error() << "\n";
        return 1;
    }

    thrust::device_vector<double> d_deposit(d_spheres.size() * n_channels), d_quantum(n_channels);
    thrust::device_vector<float> d_transmitted(d_rays.size() * n_channels);
    grace::trace_absorption_deposit_sph(d_rays, d_spheres, d_tree, d_luminosity, n_channels, d_absorption,
                                        d_deposit, &d_transmitted, &d_quantum);
    // without the optional outputs: the same deposit
    thrust::device_vector<double> d_again(d_spheres.size() * n_channels);
    grace::trace_absorption_deposit_sph(d_rays, d_spheres, d_tree, d_luminosity, n_channels, d_absorption, d_again);
    if (!thrust::equal(d_deposit.begin(), d_deposit.end(), d_again.begin())) {
        std::cerr << "the deposit depends on the optional outputs\n";
        return 1;
    }

    // a size mismatch is std::invalid_argument
    bool threw = false;
    try {
        thrust::device_vector<double> short_out(d_spheres.size() * n_channels - 1);
        grace::trace_absorption_deposit_sph(d_rays, d_spheres, d_tree, d_luminosity, n_channels, d_absorption,
                                            short_out);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    if (!threw) { std::cerr << "no std::invalid_argument for a short output\n"; return 1; }
    threw = false;
    try {
        grace::trace_absorption_deposit_sph(d_rays, d_spheres, d_tree, d_luminosity, 65, d_absorption, d_deposit);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    if (!threw) { std::cerr << "no std::invalid_argument for 65 channels\n"; return 1; }

    thrust::host_vector<double> hq = d_quantum, hd = d_deposit;
    thrust::host_vector<float> ht = d_transmitted;
    for (size_t i = 0; i < hq.size(); ++i) {
        unsigned long long u; const double v = hq[i]; std::memcpy(&u, &v, 8);
        std::printf("q %016llx\n", u);
    }
    for (size_t i = 0; i < hd.size(); ++i) {
        unsigned long long u; const double v = hd[i]; std::memcpy(&u, &v, 8);
        std::printf("d %016llx\n", u);
    }
    for (size_t i = 0; i < ht.size(); ++i) {
        unsigned int u; const float v = ht[i]; std::memcpy(&u, &v, 4);
        std::printf("t %08x\n", u);
    }
    std::printf("dropin_absorption_deposit ok: %zu rays, %d channels\n", d_rays.size(), n_channels);
    return 0;
}
