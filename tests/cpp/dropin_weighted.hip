// Drop-in check of the weighted, multi-channel column-density trace (an extension the reference
// lacks): a caller written against the reference's include paths and thrust::device_vector types
// builds the tree, then calls grace::trace_cumulative_weighted_sph with n_channels weights per
// sphere in tree order.
//   dropin_weighted <spheres.f32> <rays.f32> <weights.f32> <n_channels> <out_dir>
// spheres: n x 4 float32 inside the unit box, already in tree order (sorting them again keeps their
// order: their Morton keys are ascending); rays: m x 7 float32, m a multiple of 32; weights:
// n x n_channels float32.  The output is written raw to out_dir/wcum.f32 for a bit-for-bit
// comparison with the ctypes path.
#include "grace/cuda/nodes.h"
#include "grace/cuda/trace_sph.cuh"
#include "grace/ray.h"
#include "helper/tree.cuh"

#include <thrust/device_vector.h>
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
    if (argc < 6) { std::cerr << "usage: spheres.f32 rays.f32 weights.f32 n_channels out_dir\n"; return 2; }
    std::vector<float4> h_spheres;
    std::vector<grace::Ray> h_rays;
    std::vector<float> h_weights;
    if (!read_all(argv[1], h_spheres) || !read_all(argv[2], h_rays) || !read_all(argv[3], h_weights)) {
        std::cerr << "cannot read inputs\n";
        return 2;
    }
    const int n_channels = int(std::strtol(argv[4], NULL, 10));
    const std::string out = argv[5];

    thrust::device_vector<float4> d_spheres(h_spheres.begin(), h_spheres.end());
    thrust::device_vector<grace::Ray> d_rays(h_rays.begin(), h_rays.end());
    thrust::device_vector<float> d_weights(h_weights.begin(), h_weights.end());
    grace::Tree d_tree(d_spheres.size(), 32);
    build_tree(d_spheres, make_float3(0.f, 0.f, 0.f), make_float3(1.f, 1.f, 1.f), d_tree);

    thrust::device_vector<float> d_out(d_rays.size() * n_channels);
    grace::trace_cumulative_weighted_sph(d_rays, d_spheres, d_tree, d_weights, n_channels, d_out);

    // a size mismatch is std::invalid_argument
    bool threw = false;
    try {
        thrust::device_vector<float> short_out(d_rays.size() * n_channels - 1);
        grace::trace_cumulative_weighted_sph(d_rays, d_spheres, d_tree, d_weights, n_channels, short_out);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    if (!threw) { std::cerr << "no std::invalid_argument for a short output\n"; return 1; }

    thrust::host_vector<float> h = d_out;
    std::FILE* f = std::fopen((out + "/wcum.f32").c_str(), "wb");
    if (!f || std::fwrite(thrust::raw_pointer_cast(h.data()), sizeof(float), h.size(), f) != h.size()) return 1;
    std::fclose(f);
    std::cout << "dropin_weighted ok: " << d_rays.size() << " rays, " << n_channels << " channels\n";
    return 0;
}
