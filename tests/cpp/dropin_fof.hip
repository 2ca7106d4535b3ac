// Drop-in check of the friends-of-friends groups (an extension the reference lacks): a caller
// written against the reference's include paths and thrust::device_vector types builds the tree,
// then calls grace::fof_labels_sph and grace::fof_groups_sph.
//   dropin_fof <spheres.f32> <linking_length> <min_members>
// spheres: n x 4 float32 inside the unit box, already in tree order (sorting them again keeps their
// order).  Prints one digest line per output, "<name> <entries> <digest>", for a comparison with the
// ctypes path: the digest of 32-bit words v[i] is the sum of v[i] (2 i + 1) modulo 2^64.
#include "grace/cuda/fof_sph.cuh"
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
    static_assert(sizeof(T) == 4, "32-bit words");
    thrust::host_vector<T> h = d;
    uint64_t sum = 0;
    for (size_t i = 0; i < h.size(); ++i) {
        uint32_t w;
        std::memcpy(&w, &h[i], 4);
        sum += uint64_t(w) * (2 * uint64_t(i) + 1);
    }
    std::printf("%s %zu %llu\n", name, h.size(), (unsigned long long)sum);
}

int main(int argc, char* argv[])
{
    if (argc < 4) { std::cerr << "usage: spheres.f32 linking_length min_members\n"; return 2; }
    std::vector<float4> h_spheres;
    if (!read_all(argv[1], h_spheres)) {
        std::cerr << "cannot read inputs\n";
        return 2;
    }
    const float linking_length = std::strtof(argv[2], NULL);
    const int min_members = int(std::strtol(argv[3], NULL, 10));

    thrust::device_vector<float4> d_spheres(h_spheres.begin(), h_spheres.end());
    grace::Tree d_tree(d_spheres.size(), 32);
    build_tree(d_spheres, make_float3(0.f, 0.f, 0.f), make_float3(1.f, 1.f, 1.f), d_tree);

    thrust::device_vector<int> d_labels, d_group_of, d_sizes, d_offsets, d_members;
    grace::fof_labels_sph(d_spheres, d_tree, linking_length, d_labels);
    grace::fof_groups_sph(d_labels, min_members, d_group_of, d_sizes, d_offsets, d_members);

    // a bad linking length is std::invalid_argument
    bool threw = false;
    try {
        grace::fof_labels_sph(d_spheres, d_tree, -1.0f, d_labels);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    if (!threw) { std::cerr << "no std::invalid_argument for a negative linking length\n"; return 1; }

    print_digest("labels", d_labels);
    print_digest("sizes", d_sizes);
    print_digest("group_of", d_group_of);
    print_digest("offsets", d_offsets);
    print_digest("members", d_members);
    return 0;
}
