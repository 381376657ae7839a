// Does this runtime enforce hipFuncAttributeMaxDynamicSharedMemorySize at launch?  ("Host threads": the launchers set the attribute to
// their own call's bytes, so two host threads could interleave set, set, launch, launch.)  The worst answer is a launch error: the kernel touches
// nothing but the dynamic LDS it was launched with and one output word.
//   hipcc --offload-arch=gfx950 -O2 -o lds_attr_probe tools/lds_attr_probe.hip && ./lds_attr_probe
// The output recorded on an MI355X is profiles/host_threads/lds_attr_probe.txt.
#include <hip/hip_runtime.h>

#include <cstdio>

__global__ void probe_kernel(unsigned* out, unsigned words) {
  extern __shared__ unsigned lds[];
  for (unsigned i = threadIdx.x; i < words; i += blockDim.x) lds[i] = i;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = lds[words - 1] + 1;
}

static const char* launch(unsigned* d_out, size_t bytes) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(probe_kernel, dim3(1), dim3(256), bytes, nullptr, d_out, (unsigned)(bytes / 4));
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  unsigned got = 0;
  if (e == hipSuccess) e = hipMemcpy(&got, d_out, 4, hipMemcpyDeviceToHost);
  static char text[256];
  snprintf(text, sizeof text, "%s (out %u, want %u)", hipGetErrorString(e), got, (unsigned)(bytes / 4));
  return text;
}

int main() {
  int lds_max = 0, optin = 0;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { printf("no device\n"); return 2; }
  (void)hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, 0);
  optin = (int)prop.sharedMemPerBlockOptin;
  printf("%s: MaxSharedMemoryPerBlock %d, sharedMemPerBlockOptin %d, sharedMemPerBlock %zu\n", prop.gcnArchName, lds_max, optin, prop.sharedMemPerBlock);
  unsigned* d_out = nullptr;
  if (hipMalloc((void**)&d_out, 4) != hipSuccess) return 2;
  printf("A. no attribute set, launch 100 000 bytes: %s\n", launch(d_out, 100000));
  hipError_t e = hipFuncSetAttribute((const void*)probe_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 70000);
  printf("B. set 70 000: %s; launch 150 000 bytes: %s\n", hipGetErrorString(e), launch(d_out, 150000));
  hipFuncAttributes attr;
  e = hipFuncGetAttributes(&attr, (const void*)probe_kernel);
  printf("   hipFuncGetAttributes: %s, maxDynamicSharedSizeBytes %d\n", hipGetErrorString(e), attr.maxDynamicSharedSizeBytes);
  e = hipFuncSetAttribute((const void*)probe_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
  printf("C. set %d: %s; launch 150 000 bytes: %s\n", lds_max, hipGetErrorString(e), launch(d_out, 150000));
  e = hipFuncSetAttribute((const void*)probe_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max + 4096);
  printf("D. set %d (above the device's figure): %s\n", lds_max + 4096, hipGetErrorString(e));
  (void)hipGetLastError();
  (void)hipFree(d_out);
  return 0;
}
