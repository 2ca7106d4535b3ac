// Micro-benchmarks behind the quad-wise survivor reads of the planned column-density kernel
// (run on the GPU box; 8 workgroups of 4 waves per CU = 8 waves per SIMD on every CU):
//  a. issue rate of independent v_sub_f32 / v_mul_f32 / v_fmac_f32, plain against the same
//     instructions with a quad_perm DPP modifier on src0
//  b. LDS-array cycles of the survivor record read: the wave-uniform ds_read_b128 against a per-lane
//     ds_read_b32 at base + 16 k + 4 (lane & 3)
//  c. the test-free survivor loop itself (run_lean4<FAT>, trace_kernel.hpp) in both forms over a
//     staged tile and a 256-entry table; the two forms' sums are compared bit for bit
// hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize quad_read_ubench.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define DPP_TAIL(k) " quad_perm:[" #k "," #k "," #k "," #k "] row_mask:0xf bank_mask:0xf bound_ctrl:1"

// OP 0: a = s - a, 1: a = s * a, 2: a += s * t.  DPP: s (src0) read through quad_perm.
// s is written once, far ahead of the loop: no VALU-write -> DPP-read wait states are owed.
template <int OP, bool DPP>
__global__ __launch_bounds__(256) void valu_kernel(float* out, int iters)
{
    const int lane = threadIdx.x & 63;
    float a[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = 1.0f + 0.01f * float(lane + k);
    const float s = OP == 1 ? 1.0000001f + 1e-9f * float(lane) : 1e-3f * float(lane + 1);
    const float t = 1e-6f;
    (void)t;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (OP == 0 && !DPP) asm volatile("v_sub_f32 %0, %1, %0" : "+v"(a[k]) : "v"(s));
                if (OP == 0 && DPP) asm volatile("v_sub_f32_dpp %0, %1, %0" DPP_TAIL(0) : "+v"(a[k]) : "v"(s));
                if (OP == 1 && !DPP) asm volatile("v_mul_f32 %0, %1, %0" : "+v"(a[k]) : "v"(s));
                if (OP == 1 && DPP) asm volatile("v_mul_f32_dpp %0, %1, %0" DPP_TAIL(2) : "+v"(a[k]) : "v"(s));
                if (OP == 2 && !DPP) asm volatile("v_fmac_f32 %0, %1, %2" : "+v"(a[k]) : "v"(s), "v"(t));
                if (OP == 2 && DPP) asm volatile("v_fmac_f32_dpp %0, %1, %2" DPP_TAIL(3) : "+v"(a[k]) : "v"(s), "v"(t));
            }
        }
    }
    float r = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) r += a[k];
    out[blockIdx.x * 256 + threadIdx.x] = r;
}

// QUAD false: one wave-uniform ds_read_b128 per record; true: lane l reads dword l & 3 of it.
// Four reads in flight, then one wait; the values are kept live without vector instructions.
template <bool QUAD>
__global__ __launch_bounds__(256) void lds_kernel(float* out, int iters)
{
    __shared__ __align__(16) float4 tile[4][132];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < 4 * 132 * 4; i += 256) (&tile[0][0].x)[i] = float(i & 7);
    __syncthreads();
    const unsigned base = unsigned(reinterpret_cast<size_t>(&tile[wv][0])) + (QUAD ? 4u * unsigned(lane & 3) : 0u);
    for (int i = 0; i < iters; ++i) {
        const unsigned addr = base + unsigned(i & 63) * 16u;
        if (QUAD) {
            float p0, p1, p2, p3;
            asm volatile("ds_read_b32 %0, %1" : "=v"(p0) : "v"(addr));
            asm volatile("ds_read_b32 %0, %1 offset:16" : "=v"(p1) : "v"(addr));
            asm volatile("ds_read_b32 %0, %1 offset:32" : "=v"(p2) : "v"(addr));
            asm volatile("ds_read_b32 %0, %1 offset:48" : "=v"(p3) : "v"(addr));
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            asm volatile("" :: "v"(p0), "v"(p1), "v"(p2), "v"(p3));
        } else {
            f32x4 p0, p1, p2, p3;
            asm volatile("ds_read_b128 %0, %1" : "=v"(p0) : "v"(addr));
            asm volatile("ds_read_b128 %0, %1 offset:16" : "=v"(p1) : "v"(addr));
            asm volatile("ds_read_b128 %0, %1 offset:32" : "=v"(p2) : "v"(addr));
            asm volatile("ds_read_b128 %0, %1 offset:48" : "=v"(p3) : "v"(addr));
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            asm volatile("" :: "v"(p0), "v"(p1), "v"(p2), "v"(p3));
        }
    }
    out[blockIdx.x * 256 + threadIdx.x] = float(lane);
}

template <int K>
__device__ __forceinline__ float quad(const float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), K * 0x55, 0xf, 0xf, true));
}

// The survivor loop of run_lean4<FAT>: `rounds` rounds of `n` survivors over the wave's tile,
// two reads ahead through three rotating register sets.
template <bool QUAD>
__global__ __launch_bounds__(256, 8) void loop_kernel(float* out, int rounds, int n)
{
    __shared__ __align__(16) float4 tile[4][132];
    __shared__ float2 s_lutf[256];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // records {s1, s2, 50 / h, 1 / h^2} around the packet's 8 x 8 origins, h ~ 10 pixels
    for (int i = threadIdx.x; i < 4 * 132; i += 256) {
        const int j = i % 132;
        tile[i / 132][j] = make_float4(3.5f + 0.37f * float(j % 29) - 5.f, 3.5f + 0.53f * float(j % 23) - 6.f,
                                       50.f / (10.f + 0.1f * float(j % 7)), 0.01f - 1e-5f * float(j % 11));
    }
    {
        const float x = float(threadIdx.x) / 50.f, y0 = threadIdx.x < 50 ? (1.f - x) * (1.f - x) : 0.f;
        const float x1 = float(threadIdx.x + 1) / 50.f, y1 = threadIdx.x + 1 < 50 ? (1.f - x1) * (1.f - x1) : 0.f;
        const float dy = y1 - y0;
        s_lutf[threadIdx.x] = threadIdx.x < 50 ? make_float2(y0 - float(threadIdx.x) * dy, dy) : make_float2(0.f, 0.f);
    }
    __syncthreads();
    const float o1 = float(lane & 7), o2 = float(lane >> 3);
    float sum = 0.f;
    const float4* const tile4 = &tile[wv][0];
    for (int r = 0; r < rounds; ++r) {
        int left = n;
        if constexpr (QUAD) {
            const float* t1 = &tile4[r & 1].x + (lane & 3);
            float c0, c1, c2;
            auto proc = [&](const float c) {
                const float q1 = quad<0>(c) - o1, q2 = quad<1>(c) - o2;
                const float b = quad<2>(c) * __builtin_amdgcn_sqrtf(__builtin_fmaf(q1, q1, q2 * q2));
                const float2 y = s_lutf[static_cast<int>(b)];
                const float t = __builtin_fmaf(y.y, b, y.x);
                asm("v_fmac_f32_dpp %0, %1, %2" DPP_TAIL(3) : "+v"(sum) : "v"(c), "v"(t));
            };
            c0 = t1[0]; __builtin_amdgcn_sched_barrier(0);
            c1 = t1[4]; __builtin_amdgcn_sched_barrier(0);
            for (;;) {
                c2 = t1[8]; __builtin_amdgcn_sched_barrier(0);
                proc(c0);
                if (--left == 0) break;
                c0 = t1[12]; __builtin_amdgcn_sched_barrier(0);
                proc(c1);
                if (--left == 0) break;
                c1 = t1[16]; __builtin_amdgcn_sched_barrier(0);
                proc(c2);
                if (--left == 0) break;
                t1 += 12;
            }
        } else {
            const float4* t4 = tile4 + (r & 1);
            float4 c0, c1, c2;
            auto proc = [&](const float4 c) {
                const float q1 = c.x - o1, q2 = c.y - o2;
                const float b = __builtin_amdgcn_sqrtf(__builtin_fmaf(q1, q1, q2 * q2)) * c.z;
                const float2 y = s_lutf[static_cast<int>(b)];
                sum = __builtin_fmaf(__builtin_fmaf(y.y, b, y.x), c.w, sum);
            };
            c0 = t4[0]; __builtin_amdgcn_sched_barrier(0);
            c1 = t4[1]; __builtin_amdgcn_sched_barrier(0);
            for (;;) {
                c2 = t4[2]; __builtin_amdgcn_sched_barrier(0);
                proc(c0);
                if (--left == 0) break;
                c0 = t4[3]; __builtin_amdgcn_sched_barrier(0);
                proc(c1);
                if (--left == 0) break;
                c1 = t4[4]; __builtin_amdgcn_sched_barrier(0);
                proc(c2);
                if (--left == 0) break;
                t4 += 3;
            }
        }
    }
    out[blockIdx.x * 256 + threadIdx.x] = sum;
}

// Best of three timed launches after a warm one, ms; negative if any HIP call failed (main stops).
template <typename F>
static float time_ms(F launch)
{
    hipEvent_t e0, e1;
    bool ok = hipEventCreate(&e0) == hipSuccess;
    ok = hipEventCreate(&e1) == hipSuccess && ok;
    launch();
    ok = hipDeviceSynchronize() == hipSuccess && ok;
    float best = 1e30f;
    for (int rep = 0; rep < 3 && ok; ++rep) {
        ok = hipEventRecord(e0) == hipSuccess && ok;
        launch();
        ok = hipEventRecord(e1) == hipSuccess && ok;
        ok = hipEventSynchronize(e1) == hipSuccess && ok;
        float ms = 0.f;
        ok = hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ok;
        best = ms < best ? ms : best;
    }
    ok = hipGetLastError() == hipSuccess && ok;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return ok ? best : -1.f;
}
#define TIMED(t) do { if ((t) < 0.f) { printf("HIP error while timing, line %d\n", __LINE__); return 1; } } while (0)

int main()
{
    float* out;
    const int blocks = 256 * 8;
    const size_t n_out = size_t(blocks) * 256;
    CK(hipMalloc(&out, n_out * sizeof(float)));
    // a.
    const int iters = 2000;
    const double per_simd = 8.0 * iters * 64;   // wave-instructions per SIMD: 8 waves x iters x 64
    const char* names[3] = { "v_sub_f32", "v_mul_f32", "v_fmac_f32" };
    float tp[3], td[3];
    tp[0] = time_ms([&] { valu_kernel<0, false><<<blocks, 256>>>(out, iters); });
    td[0] = time_ms([&] { valu_kernel<0, true><<<blocks, 256>>>(out, iters); });
    tp[1] = time_ms([&] { valu_kernel<1, false><<<blocks, 256>>>(out, iters); });
    td[1] = time_ms([&] { valu_kernel<1, true><<<blocks, 256>>>(out, iters); });
    tp[2] = time_ms([&] { valu_kernel<2, false><<<blocks, 256>>>(out, iters); });
    td[2] = time_ms([&] { valu_kernel<2, true><<<blocks, 256>>>(out, iters); });
    for (int k = 0; k < 3; ++k) { TIMED(tp[k]); TIMED(td[k]); }
    for (int k = 0; k < 3; ++k)
        printf("a. %-10s plain %.3f ms (%.2f ns per wave-instruction per SIMD) | quad_perm dpp %.3f ms (%.2f ns) | dpp / plain %.3f\n",
               names[k], tp[k], tp[k] * 1e6 / per_simd, td[k], td[k] * 1e6 / per_simd, td[k] / tp[k]);
    // b.
    const int li = 16000;
    const double per_cu = 32.0 * li * 4;        // reads per CU: 32 waves x iters x 4
    const float l128 = time_ms([&] { lds_kernel<false><<<blocks, 256>>>(out, li); });
    const float l32 = time_ms([&] { lds_kernel<true><<<blocks, 256>>>(out, li); });
    TIMED(l128); TIMED(l32);
    printf("b. record read, ns per wave-read per CU (cycles at 2.4 GHz): uniform ds_read_b128 %.3f (%.2f) | quad ds_read_b32 %.3f (%.2f) | ratio %.3f\n",
           l128 * 1e6 / per_cu, l128 * 1e6 / per_cu * 2.4, l32 * 1e6 / per_cu, l32 * 1e6 / per_cu * 2.4, l32 / l128);
    // c.
    const int rounds = 400, n = 49;
    std::vector<float> ha(n_out), hb(n_out);
    const float c128 = time_ms([&] { loop_kernel<false><<<blocks, 256>>>(out, rounds, n); });
    CK(hipMemcpy(ha.data(), out, n_out * sizeof(float), hipMemcpyDeviceToHost));
    const float c32 = time_ms([&] { loop_kernel<true><<<blocks, 256>>>(out, rounds, n); });
    CK(hipMemcpy(hb.data(), out, n_out * sizeof(float), hipMemcpyDeviceToHost));
    TIMED(c128); TIMED(c32);
    const double surv_per_simd = 8.0 * rounds * n;
    printf("c. survivor loop, %d rounds of %d: b128 form %.3f ms (%.2f ns per survivor per SIMD) | quad form %.3f ms (%.2f ns) | quad / b128 %.3f | sums %s (first %.9g)\n",
           rounds, n, c128, c128 * 1e6 / surv_per_simd, c32, c32 * 1e6 / surv_per_simd, c32 / c128,
           memcmp(ha.data(), hb.data(), n_out * sizeof(float)) == 0 ? "bit-identical" : "DIFFER", double(ha[0]));
    CK(hipGetLastError());
    return 0;
}
