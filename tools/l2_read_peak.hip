// What does the vector memory path of a CU deliver into registers / LDS when the data sits in L2?
// (The 16-bit conv and weight-gradient kernels stage 350-700 MB per launch through it and never
// exceed ~11 TB/s chip-wide = ~45 GB/s per CU)
//   hipcc --offload-arch=gfx950 -O3 -o /tmp/l2_peak tools/l2_read_peak.hip && /tmp/l2_peak
// Every workgroup re-reads its own `region` bytes (16 B per lane, rows of `row_bytes`) `iters`
// times: region * workgroups per XCD < 4 MB keeps it in the XCD's L2 after the first pass.
//   mode 0: global_load_dwordx4 into registers, 8 loads in flight per lane
//   mode 1: buffer_load_dwordx4 ... lds (LDS-DMA), 8 in flight, vmcnt(0) + barrier per batch
//   mode 2: like 1, then the tile is read back from LDS (ds_read_b128) as an MFMA loop would
//
//   /tmp/l2_peak pieces: does HALF a 128-B line cost a whole one between L2 and the CU?  The same
//   useful bytes (512 rows of 1 or 2 KB per workgroup, registers, 8 loads in flight per lane) read
//     as pieces: one load instruction = 16 rows x 64 B per wave (four lanes per piece, one piece per
//                row); the other half of every line follows one step later, after the workgroup has
//                read 32 KB more -- how conv1d_wino_kernel reads a U stored [4][n][K];
//     contiguously: one load instruction = 1 KB per wave, one step = one 32 KB block.
//   The workgroups of an XCD share one region (as the workgroups of a conv share U), each starting
//   at its own step, so the region stays in that XCD's L2 at any number of workgroups per CU.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdint>
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

template <int MODE>
__global__ __launch_bounds__(256) void reader(const unsigned char* __restrict__ src, size_t region,
                                              int iters, unsigned* out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x, wave = tid >> 6;
  const unsigned char* base = src + (size_t)blockIdx.x * region;
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(base), 0, (int)region, 0x00020000);
  const int batches = (int)(region / (256 * 16 * 8));      // 32 KB per batch of 8 loads per lane
  u32x4 acc = {0, 0, 0, 0};
  for (int it = 0; it < iters; ++it)
    for (int b = 0; b < batches; ++b) {
      const uint32_t off0 = (uint32_t)b * (256 * 16 * 8) + (uint32_t)tid * 16;
      if (MODE == 0) {
        u32x4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
          v[k] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(off0 + k * 4096), 0, 0);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc ^= v[k];
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(
              rs, (__attribute__((address_space(3))) void*)(lds + k * 4096 + wave * 1024), 16,
              (int)(off0 + k * 4096), 0, 0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (MODE == 2) {
#pragma unroll
          for (int k = 0; k < 8; ++k) acc ^= *reinterpret_cast<const u32x4*>(lds + k * 4096 + tid * 16);
          __syncthreads();
        }
      }
    }
  if (MODE == 1) acc ^= *reinterpret_cast<const u32x4*>(lds + tid * 16);
  if ((acc[0] ^ acc[1] ^ acc[2] ^ acc[3]) == 0x12345678u) out[tid] = acc[0];
}

constexpr int kPieceRows = 512;      // 8 row groups of 64 rows = the 8 loads a lane keeps in flight
template <bool PIECES>
__global__ __launch_bounds__(256) void piece_reader(const unsigned char* __restrict__ src,
                                                    int row_bytes, int passes, unsigned* out) {
  const int tid = threadIdx.x;
  const uint32_t region = (uint32_t)kPieceRows * row_bytes;
  const unsigned char* base = src + (size_t)(blockIdx.x % 8) * region;     // block b runs on XCD b % 8
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(base), 0, (int)region, 0x00020000);
  const int steps = row_bytes / 64;                                        // 32 KB useful per step
  int step = (int)((blockIdx.x / 8) * 7 % steps);
  // pieces: row (tid / 4) + 64 k, bytes [64 step, 64 step + 64) of it; contiguous: block `step`
  const uint32_t lane_off = PIECES ? (uint32_t)(tid >> 2) * row_bytes + (tid & 3) * 16 : (uint32_t)tid * 16;
  const uint32_t k_stride = PIECES ? 64u * row_bytes : 4096u, s_stride = PIECES ? 64u : 32768u;
  u32x4 acc = {0, 0, 0, 0};
  for (int i = 0; i < passes * steps; ++i) {
    const uint32_t so = (uint32_t)step * s_stride;
    u32x4 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k)
      v[k] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(lane_off + k * k_stride), (int)so, 0);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc ^= v[k];
    step = step + 1 == steps ? 0 : step + 1;
  }
  if ((acc[0] ^ acc[1] ^ acc[2] ^ acc[3]) == 0x12345678u) out[tid] = acc[0];
}

template <typename F>
double time_ms(F f) {
  hipEvent_t a, b;
  hipEventCreate(&a); hipEventCreate(&b);
  f();
  hipDeviceSynchronize();
  hipEventRecord(a);
  f();
  hipEventRecord(b);
  hipEventSynchronize(b);
  float ms;
  hipEventElapsedTime(&ms, a, b);
  return ms;
}

int main(int argc, char** argv) {
  hipDeviceProp_t pr;
  hipGetDeviceProperties(&pr, 0);
  const int cus = pr.multiProcessorCount;
  unsigned char* src;
  unsigned* out;
  const size_t total = (size_t)1 << 30;
  hipMalloc(&src, total);
  hipMemset(src, 1, total);
  hipMalloc(&out, 4096);
  if (argc > 1 && argv[1][0] == 'p') {
    printf("%s, %d CUs.  USEFUL GB/s per CU (TB/s chip-wide), 512 rows per workgroup, L2-resident\n",
           pr.gcnArchName, cus);
    for (int row_bytes : {1024, 2048})
      for (int wpc : {1, 2, 4, 5}) {
        const int blocks = cus * wpc;
        const size_t region = (size_t)kPieceRows * row_bytes;
        const int passes = (int)(((size_t)48 << 20) / region);   // 48 MB per workgroup
        const double bytes = (double)blocks * region * passes;
        double t[2][2];
        for (int rep = 0; rep < 2; ++rep) {                      // alternating, both shown
          t[rep][0] = time_ms([&] { hipLaunchKernelGGL(piece_reader<true>, dim3(blocks), dim3(256), 0, 0, src, row_bytes, passes, out); });
          t[rep][1] = time_ms([&] { hipLaunchKernelGGL(piece_reader<false>, dim3(blocks), dim3(256), 0, 0, src, row_bytes, passes, out); });
        }
        printf("rows of %4d B, %d workgroups/CU:  64-B pieces %5.1f / %5.1f (%4.1f)   contiguous %5.1f / %5.1f (%4.1f)   "
               "x%.2f\n", row_bytes, wpc, bytes / t[0][0] / 1e6 / cus, bytes / t[1][0] / 1e6 / cus,
               bytes / t[1][0] / 1e9, bytes / t[0][1] / 1e6 / cus, bytes / t[1][1] / 1e6 / cus,
               bytes / t[1][1] / 1e9, t[1][0] / t[1][1]);
      }
    return 0;
  }
  printf("%s, %d CUs.  TB/s delivered chip-wide (GB/s per CU)\n", pr.gcnArchName, cus);
  for (size_t region : {(size_t)32 << 10, (size_t)256 << 10}) {
    for (int wpc : {1, 2, 4, 5}) {
      const int blocks = cus * wpc;
      if ((size_t)blocks * region > total) continue;
      const int iters = (int)(((size_t)48 << 20) / region);      // 48 MB per workgroup
      const double bytes = (double)blocks * region * iters;
      double t[3];
      t[0] = time_ms([&] { hipLaunchKernelGGL(reader<0>, dim3(blocks), dim3(256), 0, 0, src, region, iters, out); });
      t[1] = time_ms([&] { hipLaunchKernelGGL(reader<1>, dim3(blocks), dim3(256), 32768, 0, src, region, iters, out); });
      t[2] = time_ms([&] { hipLaunchKernelGGL(reader<2>, dim3(blocks), dim3(256), 32768, 0, src, region, iters, out); });
      printf("region %4zu KB/workgroup (%6.1f MB total), %d workgroups/CU:  registers %5.1f (%4.0f)   LDS-DMA %5.1f (%4.0f)   "
             "LDS-DMA + ds_read %5.1f (%4.0f)\n",
             region >> 10, blocks * region / 1048576.0, wpc, bytes / t[0] / 1e9, bytes / t[0] / 1e6 / cus,
             bytes / t[1] / 1e9, bytes / t[1] / 1e6 / cus, bytes / t[2] / 1e9, bytes / t[2] / 1e6 / cus);
    }
  }
  return 0;
}
