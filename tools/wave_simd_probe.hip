// Where do the four waves of a Gram workgroup run?  gram_item (k_gram.hip) gives wave w the quadrant (w >> 1, w & 1) of the
// tile; on an edge tile the quadrants carry unequal work, and the four workgroups resident on a CU are usually edge tiles of the
// same shape (the planner puts like items side by side).  Whether the light quadrants of all four then share a SIMD depends on how
// the hardware maps a workgroup's wave index to a SIMD -- which this probe records.
//
// One bounded kernel with the Gram kernel's footprint (256 threads, 32 KB of LDS, amdgpu_num_vgpr(52) and enough live
// accumulators to allocate what gram_kernel<float> allocates: four workgroups a CU), a few microseconds of dependent MFMAs per
// workgroup (the length varies with the block index, so that the slots of a CU refill one at a time as in the real launch), no
// spinning, no waiting on anything.  Lane 0 of every wave stores, with ordinary vector stores, the hardware-id register, the XCC
// id, its block index, its wave index and the wall clock at its start and end; tools/wave_simd_probe.py reads the table.
//   hipcc --offload-arch=gfx950 -O3 -shared -fPIC -o libwavesimd.so tools/wave_simd_probe.hip
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int REC = 8;                      // dwords per wave record

__global__ __launch_bounds__(256, 4) __attribute__((amdgpu_num_vgpr(52))) void wave_simd_kernel(uint32_t* __restrict__ rec, float* __restrict__ sink,
                                                                                                int iters, float seed)
{
    __shared__ __attribute__((aligned(16))) float lds[32768 / 4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint32_t hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    const unsigned long long t0 = wall_clock64();
    for (int e = tid; e < 32768 / 4; e += 256) lds[e] = seed * (float)(e & 7);
    __syncthreads();
    // dependent work: six accumulators (96 registers) fed round robin, 64 cycles of the SIMD's matrix pipe per MFMA
    f32x16 acc[6];
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[a][r] = (float)a;
    const int n = iters * (1 + (int)((blockIdx.x * 2654435761u) >> 30));       // 1 .. 4 x iters
    for (int i = 0; i < n; i++) {
        const float x = lds[(lane + 64 * i) & (32768 / 4 - 1)], y = lds[(lane * 3 + i) & (32768 / 4 - 1)];
#pragma unroll
        for (int a = 0; a < 6; a++) acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(x, y, acc[a], 0, 0, 0);
    }
    float s = 0.f;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int r = 0; r < 16; r++) s += acc[a][r];
    if (s == 12345.678f) sink[tid] = s;                                         // (keeps the accumulators alive; never true in practice)
    const unsigned long long t1 = wall_clock64();
    if (lane == 0) {
        uint32_t* o = rec + ((size_t)blockIdx.x * 4 + wave) * REC;              // grid x 4 waves x REC dwords: the table's size
        o[0] = hw; o[1] = xcc; o[2] = blockIdx.x; o[3] = (uint32_t)wave;
        o[4] = (uint32_t)t0; o[5] = (uint32_t)(t0 >> 32); o[6] = (uint32_t)t1; o[7] = (uint32_t)(t1 >> 32);
    }
}

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return -1; } } while (0)

// runs the kernel on `n_wg` workgroups and copies the n_wg x 4 x 8 dwords of records to `out`; returns the workgroups per CU
// the occupancy calculator reports for the kernel (4 expected), or -1
extern "C" int wave_simd_probe(int n_wg, int iters, uint32_t* out)
{
    if (n_wg <= 0 || n_wg > (1 << 20) || iters <= 0 || iters > 4096 || !out) return -1;
    const size_t bytes = (size_t)n_wg * 4 * REC * sizeof(uint32_t);
    uint32_t* d_rec = nullptr;
    float* d_sink = nullptr;
    CHK(hipMalloc(&d_rec, bytes));
    CHK(hipMalloc(&d_sink, 256 * sizeof(float)));
    CHK(hipMemset(d_rec, 0xff, bytes));
    int per_cu = 0;
    CHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, wave_simd_kernel, 256, 0));
    hipLaunchKernelGGL(wave_simd_kernel, dim3(n_wg), dim3(256), 0, 0, d_rec, d_sink, iters, 1.0f);
    CHK(hipGetLastError());
    CHK(hipDeviceSynchronize());
    CHK(hipMemcpy(out, d_rec, bytes, hipMemcpyDeviceToHost));
    CHK(hipFree(d_rec));
    CHK(hipFree(d_sink));
    return per_cu;
}
