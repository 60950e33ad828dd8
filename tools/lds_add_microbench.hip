// lds_add_microbench.hip -- what an LDS add without return costs on gfx950, next to a plain LDS store (GPU box):
//
//   hipcc --offload-arch=gfx950 -O3 tools/lds_add_microbench.hip -o build/lds_add_microbench && build/lds_add_microbench
//
// One workgroup of eight waves per CU (k_delta_direct's shape), every wave issues ITERS x 8 LDS instructions on 64
// consecutive dwords of its own (no bank conflict, no two lanes on one address), eight distinct rows per wave.  Printed:
// ns per wave instruction as one CU's LDS sees them (time x CUs' share / instructions of the CU's eight waves).
// The question behind it (profiles/NOTES_r07.md): can k_delta_direct's loop sum its one-hot input rows with LDS adds
// in the MFMAs' shadow?  No: see the figures there.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr int WAVES = 8, ROWS = 8;

// OP 0: ds_add_f32, 1: ds_add_u32, 2: ds_write_b32
template <int OP> __global__ __launch_bounds__(64 * WAVES) void k_lds(float *out, int iters, float value) {
  __shared__ float rows[WAVES * ROWS * 64];
  for (int i = threadIdx.x; i < WAVES * ROWS * 64; i += 64 * WAVES) rows[i] = 0.0f;
  __syncthreads();
  /* this lane's dword of its wave's row 0; row r is 256 bytes further (the instruction's immediate offset) */
  const unsigned addr = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float *)rows + (threadIdx.x >> 6) * ROWS * 256 + (threadIdx.x & 63) * 4;
  for (int i = 0; i < iters; i++) {
    if constexpr (OP == 0)
      asm volatile("ds_add_f32 %0, %1\n\tds_add_f32 %0, %1 offset:256\n\tds_add_f32 %0, %1 offset:512\n\tds_add_f32 %0, %1 offset:768\n\t"
                   "ds_add_f32 %0, %1 offset:1024\n\tds_add_f32 %0, %1 offset:1280\n\tds_add_f32 %0, %1 offset:1536\n\tds_add_f32 %0, %1 offset:1792"
                   : : "v"(addr), "v"(value) : "memory");
    else if constexpr (OP == 1)
      asm volatile("ds_add_u32 %0, %1\n\tds_add_u32 %0, %1 offset:256\n\tds_add_u32 %0, %1 offset:512\n\tds_add_u32 %0, %1 offset:768\n\t"
                   "ds_add_u32 %0, %1 offset:1024\n\tds_add_u32 %0, %1 offset:1280\n\tds_add_u32 %0, %1 offset:1536\n\tds_add_u32 %0, %1 offset:1792"
                   : : "v"(addr), "v"(value) : "memory");
    else
      asm volatile("ds_write_b32 %0, %1\n\tds_write_b32 %0, %1 offset:256\n\tds_write_b32 %0, %1 offset:512\n\tds_write_b32 %0, %1 offset:768\n\t"
                   "ds_write_b32 %0, %1 offset:1024\n\tds_write_b32 %0, %1 offset:1280\n\tds_write_b32 %0, %1 offset:1536\n\tds_write_b32 %0, %1 offset:1792"
                   : : "v"(addr), "v"(value) : "memory");
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
  if (blockIdx.x == 0) out[threadIdx.x] = rows[threadIdx.x];
}

template <int OP> static void run(const char *name, float value, float *out, int cus) {
  const int iters = 2000;
  hipEvent_t a, b;
  CHECK(hipEventCreate(&a));
  CHECK(hipEventCreate(&b));
  k_lds<OP><<<cus, 64 * WAVES>>>(out, iters, value);
  CHECK(hipDeviceSynchronize());
  float best = 1e30f;
  for (int rep = 0; rep < 5; rep++) {
    CHECK(hipEventRecord(a));
    k_lds<OP><<<cus, 64 * WAVES>>>(out, iters, value);
    CHECK(hipEventRecord(b));
    CHECK(hipEventSynchronize(b));
    float ms;
    CHECK(hipEventElapsedTime(&ms, a, b));
    best = ms < best ? ms : best;
  }
  float first;
  CHECK(hipMemcpy(&first, out, sizeof(float), hipMemcpyDeviceToHost));
  printf("%-34s %8.1f us per launch, %7.2f ns per wave instruction and CU  (first dword %g)\n", name, 1e3 * best,
         1e6 * best / ((double)iters * 8 * WAVES), first);
}

int main() {
  hipDeviceProp_t p;
  CHECK(hipGetDeviceProperties(&p, 0));
  float *out;
  CHECK(hipMalloc(&out, 64 * WAVES * sizeof(float)));
  printf("%s, %d CUs, one workgroup of %d waves each, 2000 x 8 LDS instructions per wave\n", p.name, p.multiProcessorCount, WAVES);
  run<2>("ds_write_b32", 1.0f, out, p.multiProcessorCount);
  run<1>("ds_add_u32", 1.4e-45f, out, p.multiProcessorCount);
  run<0>("ds_add_f32 (1.0)", 1.0f, out, p.multiProcessorCount);
  run<0>("ds_add_f32 (1e-3: rounding adds)", 1e-3f, out, p.multiProcessorCount);
  run<0>("ds_add_f32 (1e-41: denormals)", 1e-41f, out, p.multiProcessorCount);
  CHECK(hipFree(out));
  return 0;
}
