// grace/detail/raw.h -- helpers shared by the drop-in headers: the container and the raw device
// pointers the shared API bodies are written against (grace/detail/front_end.h), and compile-time
// tags for the (Real4, key, delta) types the C ABI covers.
#pragma once

#include "grace/detail/front_end.h"
#include "grace/error.h"
#include "grace/types.h"

#include <thrust/device_vector.h>

namespace grace {
namespace detail {

template <typename T> using dvec = thrust::device_vector<T>;

template <typename T>
inline T* raw(thrust::device_vector<T>& v) { return thrust::raw_pointer_cast(v.data()); }
template <typename T>
inline const T* raw(const thrust::device_vector<T>& v) { return thrust::raw_pointer_cast(v.data()); }

// Raw device pointer behind an iterator: a plain pointer, or a Thrust device iterator /
// device_ptr over contiguous storage.
template <typename T>
inline T* raw_of(T* p) { return p; }
template <typename Iter>
inline auto raw_of(Iter it) -> decltype(thrust::raw_pointer_cast(&*it)) { return thrust::raw_pointer_cast(&*it); }

template <typename T> struct always_false { static const bool value = false; };

template <typename Real4> struct is_float4 { static const bool value = false; };
template <> struct is_float4<float4> { static const bool value = true; };
template <typename Real4> struct is_double4 { static const bool value = false; };
template <> struct is_double4<double4> { static const bool value = true; };

} // namespace detail
} // namespace grace
