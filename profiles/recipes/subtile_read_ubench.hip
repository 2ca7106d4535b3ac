// Micro-benchmark behind the per-quadrant survivor streams of the planned column-density kernel
// (same pattern as quad_read_ubench.hip; 8 workgroups of 4 waves per CU = 8 waves per SIMD on every CU):
//  b. LDS-array cycles of the survivor record read: the wave-uniform ds_read_b128 at base + 16 k against
//     the sub-tile read, lane l at base + 64 k + 16 (l >> 4): every 16-lane group of the instruction
//     sees two adjacent 16-byte records
//  c. the test-free survivor loop (run_lean4<FAT>, trace_kernel.hpp) over the same number of steps in
//     both forms: uniform tile pointer and stride of one record against per-lane pointer and stride of four
// hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize subtile_read_ubench.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TILE = 132;          // records per wave in the kernel's tile
constexpr int STEPS = TILE / 4;    // sub-tile steps that fit it

// SUB false: one wave-uniform ds_read_b128 per record; true: quadrant q = lane >> 4 reads record 4 k + q.
// Four reads in flight, then one wait; the values are kept live without vector instructions.
template <bool SUB>
__global__ __launch_bounds__(256) void lds_kernel(float* out, int iters)
{
    __shared__ __align__(16) float4 tile[4][TILE];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < 4 * TILE * 4; i += 256) (&tile[0][0].x)[i] = float(i & 7);
    __syncthreads();
    const unsigned base = unsigned(reinterpret_cast<size_t>(&tile[wv][0])) + (SUB ? 16u * unsigned(lane >> 4) : 0u);
    for (int i = 0; i < iters; ++i) {
        // SUB: steps 0 .. 27 + 3 < STEPS; uniform: records 0 .. 63 + 3 < TILE
        const unsigned addr = base + (SUB ? unsigned(i % 28) * 64u : unsigned(i & 63) * 16u);
        f32x4 p0, p1, p2, p3;
        if (SUB) {
            asm volatile("ds_read_b128 %0, %1" : "=v"(p0) : "v"(addr));
            asm volatile("ds_read_b128 %0, %1 offset:64" : "=v"(p1) : "v"(addr));
            asm volatile("ds_read_b128 %0, %1 offset:128" : "=v"(p2) : "v"(addr));
            asm volatile("ds_read_b128 %0, %1 offset:192" : "=v"(p3) : "v"(addr));
        } else {
            asm volatile("ds_read_b128 %0, %1" : "=v"(p0) : "v"(addr));
            asm volatile("ds_read_b128 %0, %1 offset:16" : "=v"(p1) : "v"(addr));
            asm volatile("ds_read_b128 %0, %1 offset:32" : "=v"(p2) : "v"(addr));
            asm volatile("ds_read_b128 %0, %1 offset:48" : "=v"(p3) : "v"(addr));
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        asm volatile("" :: "v"(p0), "v"(p1), "v"(p2), "v"(p3));
    }
    out[blockIdx.x * 256 + threadIdx.x] = float(lane);
}

// The survivor loop of run_lean4<FAT>: `rounds` rounds of `n` steps over the wave's tile,
// two reads ahead through three rotating register sets.  n <= STEPS - 2 when SUB.
template <bool SUB>
__global__ __launch_bounds__(256, 8) void loop_kernel(float* out, int rounds, int n)
{
    __shared__ __align__(16) float4 tile[4][TILE];
    __shared__ float2 s_lutf[256];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // records {s1, s2, 50 / h, 1 / h^2} around the packet's 8 x 8 origins, h ~ 10 pixels
    for (int i = threadIdx.x; i < 4 * TILE; i += 256) {
        const int j = i % TILE;
        tile[i / TILE][j] = make_float4(3.5f + 0.37f * float(j % 29) - 5.f, 3.5f + 0.53f * float(j % 23) - 6.f,
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
    constexpr int S = SUB ? 4 : 1;
    const float4* const tile4 = &tile[wv][0] + (SUB ? lane >> 4 : 0);
    for (int r = 0; r < rounds; ++r) {
        int left = n;
        const float4* t4 = tile4 + S * (r & 1);
        float4 c0, c1, c2;
        auto proc = [&](const float4 c) {
            const float q1 = c.x - o1, q2 = c.y - o2;
            const float b = __builtin_amdgcn_sqrtf(__builtin_fmaf(q1, q1, q2 * q2)) * c.z;
            const float2 y = s_lutf[static_cast<int>(b)];
            sum = __builtin_fmaf(__builtin_fmaf(y.y, b, y.x), c.w, sum);
        };
        c0 = t4[0]; __builtin_amdgcn_sched_barrier(0);
        c1 = t4[S]; __builtin_amdgcn_sched_barrier(0);
        for (;;) {
            c2 = t4[2 * S]; __builtin_amdgcn_sched_barrier(0);
            proc(c0);
            if (--left == 0) break;
            c0 = t4[3 * S]; __builtin_amdgcn_sched_barrier(0);
            proc(c1);
            if (--left == 0) break;
            c1 = t4[4 * S]; __builtin_amdgcn_sched_barrier(0);
            proc(c2);
            if (--left == 0) break;
            t4 += 3 * S;
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
    // b.
    const int li = 16000;
    const double per_cu = 32.0 * li * 4;        // reads per CU: 32 waves x iters x 4
    const float lu = time_ms([&] { lds_kernel<false><<<blocks, 256>>>(out, li); });
    const float ls = time_ms([&] { lds_kernel<true><<<blocks, 256>>>(out, li); });
    TIMED(lu); TIMED(ls);
    printf("b. record read, ns per wave-read per CU (cycles at 2.4 GHz): uniform ds_read_b128 %.3f (%.2f) | sub-tile ds_read_b128 %.3f (%.2f) | ratio %.3f\n",
           lu * 1e6 / per_cu, lu * 1e6 / per_cu * 2.4, ls * 1e6 / per_cu, ls * 1e6 / per_cu * 2.4, ls / lu);
    // c.
    const int rounds = 400, n = 30;
    const float cu = time_ms([&] { loop_kernel<false><<<blocks, 256>>>(out, rounds, n); });
    const float cs = time_ms([&] { loop_kernel<true><<<blocks, 256>>>(out, rounds, n); });
    TIMED(cu); TIMED(cs);
    const double steps_per_simd = 8.0 * rounds * n;
    printf("c. survivor loop, %d rounds of %d steps: uniform form %.3f ms (%.2f ns per step per SIMD) | sub-tile form %.3f ms (%.2f ns) | sub-tile / uniform %.3f\n",
           rounds, n, cu, cu * 1e6 / steps_per_simd, cs, cs * 1e6 / steps_per_simd, cs / cu);
    CK(hipGetLastError());
    CK(hipFree(out));
    return 0;
}
