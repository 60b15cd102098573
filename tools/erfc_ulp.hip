// The error of the device's fp64 erfc in ulps, against the host's erfcl, at 10^5 arguments in [-9, 9] (an even grid, so a run is
// reproducible): the measurement behind MQ_ERFC_ULP of csrc/sgp_mixture.hpp.  Prints one JSON object.
//   hipcc --offload-arch=gfx950 -O3 -o erfc_ulp tools/erfc_ulp.hip && ./erfc_ulp > profiles/mixture_quantile_erfc_ulp.json
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>

__global__ void erfc_kernel(const double* u, double* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = erfc(u[i]);
}

#define CHECK(call)                                                          \
  do {                                                                       \
    hipError_t e_ = (call);                                                  \
    if (e_ != hipSuccess) {                                                  \
      fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));             \
      return 1;                                                              \
    }                                                                        \
  } while (0)

int main() {
  const int n = 100000;
  const double lo = -9.0, hi = 9.0;
  std::vector<double> u(n), got(n);
  for (int i = 0; i < n; ++i) u[i] = lo + (hi - lo) * ((double)i + 0.5) / (double)n;
  double *du = nullptr, *dout = nullptr;
  CHECK(hipMalloc(&du, n * sizeof(double)));
  CHECK(hipMalloc(&dout, n * sizeof(double)));
  CHECK(hipMemcpy(du, u.data(), n * sizeof(double), hipMemcpyHostToDevice));
  erfc_kernel<<<(n + 255) / 256, 256>>>(du, dout, n);
  CHECK(hipGetLastError());
  CHECK(hipMemcpy(got.data(), dout, n * sizeof(double), hipMemcpyDeviceToHost));
  CHECK(hipFree(du));
  CHECK(hipFree(dout));
  double worst = 0.0, worst_u = 0.0, sum = 0.0, worst_tail = 0.0;  // worst_tail: over u >= 0 alone (the small values)
  for (int i = 0; i < n; ++i) {
    const long double ref = erfcl((long double)u[i]);
    int e = 0;
    frexpl(ref, &e);                                        // ref = m 2^e, 0.5 <= m < 1: one ulp of a double there is 2^(e - 53)
    const double ulps = (double)fabsl(((long double)got[i] - ref) / ldexpl(1.0L, e - 53));
    sum += ulps;
    if (ulps > worst) worst = ulps, worst_u = u[i];
    if (u[i] >= 0.0 && ulps > worst_tail) worst_tail = ulps;
  }
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  printf("{\"device\": \"%s\", \"function\": \"erfc (fp64, device library)\", \"reference\": \"erfcl (host, 64-bit significand)\", "
         "\"points\": %d, \"range\": [%.1f, %.1f], \"worst_ulp\": %.4f, \"worst_at\": %.17g, \"worst_ulp_nonnegative_argument\": %.4f, "
         "\"mean_ulp\": %.4f}\n",
         prop.name, n, lo, hi, worst, worst_u, worst_tail, sum / n);
  return 0;
}
