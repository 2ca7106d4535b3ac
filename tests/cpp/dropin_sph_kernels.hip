// Drop-in check of the selectable SPH kernel (an extension the reference lacks): a caller written
// against the reference's include paths builds the tree, selects grace::SphKernel::wendland_c2 and
// calls the reference-signature grace::trace_cumulative_sph.
//   dropin_sph_kernels <spheres.f32> <rays.f32> <out_dir>
// spheres: n x 4 float32 inside the unit box, already in tree order; rays: m x 7 float32, m a
// multiple of 32.  The column densities are written raw to out_dir/wc2.f32 for a bit-for-bit
// comparison with the ctypes path; the program leaves the default (cubic) kernel selected.
#include "grace/cuda/nodes.h"
#include "grace/cuda/trace_sph.cuh"
#include "grace/ray.h"
#include "helper/tree.cuh"

#include <thrust/device_vector.h>
#include <thrust/host_vector.h>

#include <cmath>
#include <cstdio>
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
    if (argc < 4) { std::cerr << "usage: spheres.f32 rays.f32 out_dir\n"; return 2; }
    std::vector<float4> h_spheres;
    std::vector<grace::Ray> h_rays;
    if (!read_all(argv[1], h_spheres) || !read_all(argv[2], h_rays)) {
        std::cerr << "cannot read inputs\n";
        return 2;
    }
    const std::string out = argv[3];

    // the built-in table: F(0) of Wendland C2 is 7 / pi
    const std::array<double, grace::N_table> c2 = grace::sph_kernel_table(grace::SphKernel::wendland_c2);
    if (std::fabs(c2[0] - 7.0 / M_PI) > 1e-13 || c2[grace::N_table - 1] != 0.0) {
        std::cerr << "unexpected Wendland C2 table\n";
        return 1;
    }

    thrust::device_vector<float4> d_spheres(h_spheres.begin(), h_spheres.end());
    thrust::device_vector<grace::Ray> d_rays(h_rays.begin(), h_rays.end());
    grace::Tree d_tree(d_spheres.size(), 32);
    build_tree(d_spheres, make_float3(0.f, 0.f, 0.f), make_float3(1.f, 1.f, 1.f), d_tree);

    thrust::device_vector<float> d_cubic(d_rays.size()), d_wc2(d_rays.size()), d_user(d_rays.size());
    grace::trace_cumulative_sph(d_rays, d_spheres, d_tree, d_cubic);
    grace::set_sph_kernel(grace::SphKernel::wendland_c2);
    grace::trace_cumulative_sph(d_rays, d_spheres, d_tree, d_wc2);

    // the same table given as a caller's table: the same bits
    grace::set_sph_kernel_table(std::vector<double>(c2.begin(), c2.end()));
    grace::trace_cumulative_sph(d_rays, d_spheres, d_tree, d_user);

    // refused tables throw std::invalid_argument and leave the caller's table active
    int refused = 0;
    std::vector<double> bad(c2.begin(), c2.end());
    bad.pop_back();
    try { grace::set_sph_kernel_table(bad); } catch (const std::invalid_argument&) { ++refused; }
    bad = std::vector<double>(c2.begin(), c2.end());
    bad[grace::N_table - 1] = 1e-3;
    try { grace::set_sph_kernel_table(bad); } catch (const std::invalid_argument&) { ++refused; }
    if (refused != 2) { std::cerr << "invalid tables were not refused\n"; return 1; }
    int kind = 0;
    GRACE_STATUS_CHECK(grace_trace_get_sph_kernel(&kind, NULL));
    if (kind != GRACE_SPH_KERNEL_CUSTOM) { std::cerr << "a refused table changed the kernel\n"; return 1; }
    grace::set_sph_kernel(grace::SphKernel::cubic);

    thrust::host_vector<float> h_cubic = d_cubic, h_wc2 = d_wc2, h_user = d_user;
    size_t differ = 0;
    for (size_t i = 0; i < h_wc2.size(); ++i) {
        if (h_user[i] != h_wc2[i]) { std::cerr << "custom table differs at ray " << i << "\n"; return 1; }
        differ += h_cubic[i] != h_wc2[i];
    }
    if (differ == 0) { std::cerr << "Wendland C2 gave the cubic spline's column densities\n"; return 1; }

    std::FILE* f = std::fopen((out + "/wc2.f32").c_str(), "wb");
    if (!f || std::fwrite(thrust::raw_pointer_cast(h_wc2.data()), sizeof(float), h_wc2.size(), f) != h_wc2.size())
        return 1;
    std::fclose(f);
    std::cout << "dropin_sph_kernels ok: " << d_rays.size() << " rays, " << differ << " differ from cubic\n";
    return 0;
}
