// Drop-in check of the depth-ordered emission-absorption trace (an extension the reference lacks):
// a caller written against the reference's include paths and thrust::device_vector types builds
// the tree, then calls grace::trace_emission_absorption_sph with n_channels emission coefficients
// and one absorption coefficient per sphere in tree order.
//   dropin_emission_absorption <spheres.f32> <rays.f32> <emission.f32> <n_channels> <absorption.f32> <out_dir>
// spheres: n x 4 float32 inside the unit box, already in tree order (sorting them again keeps their
// order: their Morton keys are ascending); rays: m x 7 float32, m a multiple of 32; emission:
// n x n_channels float32; absorption: n float32.  The outputs are written raw to out_dir/ea.f32
// and out_dir/tau.f32 for a bit-for-bit comparison with the ctypes path.
#include "grace/cuda/nodes.h"
#include "grace/cuda/trace_sph.cuh"
#include "grace/ray.h"
#include "helper/tree.cuh"

#include <thrust/device_vector.h>
#include <thrust/equal.h>
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

int main(int argc, char* argv[])
{
    if (argc < 7) { std::cerr << "usage: spheres.f32 rays.f32 emission.f32 n_channels absorption.f32 out_dir\n"; return 2; }
    std::vector<float4> h_spheres;
    std::vector<grace::Ray> h_rays;
    std::vector<float> h_emission, h_absorption;
    if (!read_all(argv[1], h_spheres) || !read_all(argv[2], h_rays) || !read_all(argv[3], h_emission)
        || !read_all(argv[5], h_absorption)) {
        std::cerr << "cannot read inputs\n";
        return 2;
    }
    const int n_channels = int(std::strtol(argv[4], NULL, 10));
    const std::string out = argv[6];

    thrust::device_vector<float4> d_spheres(h_spheres.begin(), h_spheres.end());
    thrust::device_vector<grace::Ray> d_rays(h_rays.begin(), h_rays.end());
    thrust::device_vector<float> d_emission(h_emission.begin(), h_emission.end());
    thrust::device_vector<float> d_absorption(h_absorption.begin(), h_absorption.end());
    grace::Tree d_tree(d_spheres.size(), 32);
    build_tree(d_spheres, make_float3(0.f, 0.f, 0.f), make_float3(1.f, 1.f, 1.f), d_tree);

    thrust::device_vector<float> d_out(d_rays.size() * n_channels), d_tau(d_rays.size());
    grace::trace_emission_absorption_sph(d_rays, d_spheres, d_tree, d_emission, n_channels, d_absorption, d_out,
                                         &d_tau);
    // without the optical depths: the same image
    thrust::device_vector<float> d_again(d_rays.size() * n_channels);
    grace::trace_emission_absorption_sph(d_rays, d_spheres, d_tree, d_emission, n_channels, d_absorption, d_again);
    if (!thrust::equal(d_out.begin(), d_out.end(), d_again.begin())) { std::cerr << "the image depends on d_tau\n"; return 1; }

    // a size mismatch is std::invalid_argument
    bool threw = false;
    try {
        thrust::device_vector<float> short_out(d_rays.size() * n_channels - 1);
        grace::trace_emission_absorption_sph(d_rays, d_spheres, d_tree, d_emission, n_channels, d_absorption,
                                             short_out);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    if (!threw) { std::cerr << "no std::invalid_argument for a short output\n"; return 1; }

    threw = false;
    try {
        grace::trace_emission_absorption_sph(d_rays, d_spheres, d_tree, d_emission, 65, d_absorption, d_out);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    if (!threw) { std::cerr << "no std::invalid_argument for 65 channels\n"; return 1; }

    thrust::host_vector<float> h = d_out, ht = d_tau;
    std::FILE* f = std::fopen((out + "/ea.f32").c_str(), "wb");
    if (!f || std::fwrite(thrust::raw_pointer_cast(h.data()), sizeof(float), h.size(), f) != h.size()) return 1;
    std::fclose(f);
    f = std::fopen((out + "/tau.f32").c_str(), "wb");
    if (!f || std::fwrite(thrust::raw_pointer_cast(ht.data()), sizeof(float), ht.size(), f) != ht.size()) return 1;
    std::fclose(f);
    std::cout << "dropin_emission_absorption ok: " << d_rays.size() << " rays, " << n_channels << " channels\n";
    return 0;
}
