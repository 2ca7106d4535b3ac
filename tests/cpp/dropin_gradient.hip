// Drop-in check of the SPH gradients at points (an extension the reference lacks): a caller builds the
// tree, then calls grace::interpolate_gradient_sph (with and without value and counts),
// grace::interpolate_gradient_grid_sph and grace::divergence_curl_sph, open and with a
// grace::PeriodicBox.  It compiles against either header set: the reference's include paths with
// thrust::device_vector (the default), or, with -DDROPIN_MIRROR, the HIP-free mirror grace/grace.h with
// grace::device_vector.
//   dropin_gradient <spheres.f32> <points.f32> <weights.f32> <n_channels> <n_grid> <Lx> <Ly> <Lz>
// spheres: n x 4 float32 inside the unit box, already in tree order (sorting them again keeps their
// order); points: m x 4 float32; weights: n x n_channels float32, n_channels >= 3 (the first three are
// the vector field of the divergence and curl); the grid is n_grid^3 points at spacing 1 / n_grid from
// the origin.  Prints one digest line per output, "<name> <words> <digest>", for a comparison with the
// ctypes path: the digest of 32-bit words v[i] is the sum of v[i] (2 i + 1) modulo 2^64.
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
    if (argc < 9) {
        std::cerr << "usage: spheres.f32 points.f32 weights.f32 n_channels n_grid Lx Ly Lz\n";
        return 2;
    }
    std::vector<point4> h_spheres, h_points;
    std::vector<float> h_weights;
    if (!read_all(argv[1], h_spheres) || !read_all(argv[2], h_points) || !read_all(argv[3], h_weights)) {
        std::cerr << "cannot read inputs\n";
        return 2;
    }
    const int n_channels = int(std::strtol(argv[4], NULL, 10));
    const int n_grid = int(std::strtol(argv[5], NULL, 10));
    const grace::PeriodicBox box = { std::strtof(argv[6], NULL), std::strtof(argv[7], NULL),
                                     std::strtof(argv[8], NULL) };
    if (n_channels < 3) { std::cerr << "n_channels must be at least 3\n"; return 2; }

    dvec<point4> d_spheres(h_spheres);
    dvec<point4> d_points(h_points);
    dvec<float> d_weights(h_weights);
    grace::Tree d_tree(d_spheres.size(), 32);
    build_unit_tree(d_spheres, d_tree);
    const size_t m = d_points.size();

    dvec<float> d_grad(m * n_channels * 3), d_grad_only(m * n_channels * 3), d_value(m * n_channels);
    dvec<int> d_counts(m);
    grace::interpolate_gradient_sph(d_points, d_spheres, d_tree, d_weights, n_channels, d_grad, &d_value, &d_counts);
    grace::interpolate_gradient_sph(d_points, d_spheres, d_tree, d_weights, n_channels, d_grad_only);
    if (to_host(d_grad) != to_host(d_grad_only)) { std::cerr << "the optional outputs changed the gradient\n"; return 1; }
    dvec<float> d_field(m * n_channels);
    grace::interpolate_sph(d_points, d_spheres, d_tree, d_weights, n_channels, d_field);
    if (to_host(d_field) != to_host(d_value)) { std::cerr << "value differs from interpolate_sph\n"; return 1; }

    dvec<float> d_pgrad(m * n_channels * 3), d_pvalue(m * n_channels);
    dvec<int> d_pcounts(m);
    grace::interpolate_gradient_sph(d_points, d_spheres, d_tree, d_weights, n_channels, d_pgrad, &d_pvalue, &d_pcounts,
                                    box);

    const float dx = 1.0f / float(n_grid);
    const size_t n3 = size_t(n_grid) * n_grid * n_grid;
    dvec<float> d_grid(n3 * n_channels * 3), d_grid_value(n3 * n_channels), d_pgrid(n3 * n_channels * 3);
    grace::interpolate_gradient_grid_sph(make_float3(0.f, 0.f, 0.f), make_float3(dx, 0.f, 0.f),
                                         make_float3(0.f, dx, 0.f), make_float3(0.f, 0.f, dx), n_grid, n_grid, n_grid,
                                         d_spheres, d_tree, d_weights, n_channels, d_grid, &d_grid_value);
    grace::interpolate_gradient_grid_sph(make_float3(0.f, 0.f, 0.f), make_float3(dx, 0.f, 0.f),
                                         make_float3(0.f, dx, 0.f), make_float3(0.f, 0.f, dx), n_grid, n_grid, n_grid,
                                         d_spheres, d_tree, d_weights, n_channels, d_pgrid, (dvec<float>*)NULL, box);

    // the first three channels as a vector field
    std::vector<float> h_vec(h_spheres.size() * 3);
    for (size_t i = 0; i < h_spheres.size(); ++i)
        for (int c = 0; c < 3; ++c) h_vec[i * 3 + c] = h_weights[i * n_channels + c];
    dvec<float> d_vec(h_vec), d_div(m), d_curl(m * 3), d_pdiv(m), d_pcurl(m * 3);
    grace::divergence_curl_sph(d_points, d_spheres, d_tree, d_vec, d_div, d_curl);
    grace::divergence_curl_sph(d_points, d_spheres, d_tree, d_vec, d_pdiv, d_pcurl, box);

    // a size mismatch is std::invalid_argument
    bool threw = false;
    try {
        dvec<float> short_grad(m * n_channels * 3 - 1);
        grace::interpolate_gradient_sph(d_points, d_spheres, d_tree, d_weights, n_channels, short_grad);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    if (!threw) { std::cerr << "no std::invalid_argument for a short gradient\n"; return 1; }

    print_digest("grad", d_grad);
    print_digest("value", d_value);
    print_digest("counts", d_counts);
    print_digest("periodic_grad", d_pgrad);
    print_digest("periodic_value", d_pvalue);
    print_digest("periodic_counts", d_pcounts);
    print_digest("grid_grad", d_grid);
    print_digest("grid_value", d_grid_value);
    print_digest("periodic_grid_grad", d_pgrid);
    print_digest("div", d_div);
    print_digest("curl", d_curl);
    print_digest("periodic_div", d_pdiv);
    print_digest("periodic_curl", d_pcurl);
    return 0;
}
