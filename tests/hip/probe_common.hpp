// Test-only probe of the device arithmetic (field_dev.hpp, unsat_dev.hpp, bucket_dev.hpp, coop_dev.hpp, ec_dev.hpp): every primitive behind
// its own tiny kernel, one lane per case, raw uint32 limbs in and out.  The product headers are included unchanged; nothing here
// is linked into libzkp_accel.so.  The reference is Python integer arithmetic (tests/field_ref.py).
//
// An op is a struct with  NIN / NOUT (words per case it reads / writes), LANES (1, or 4 for the quad-cooperative operations) and
//   static __device__ void run(const uint32_t* in, uint32_t* out, int role)
// `in` and `out` point at the case's own rows.  The out rows are copied to the device before the launch, so an operation whose
// operands live in memory (add_mem, quad_add_mem) finds them there.  No address depends on data: a wrong answer is a wrong number.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "coop_dev.hpp"

namespace probe {
using namespace zkp;

template <class Op>
__global__ void probe_kernel(int n, const uint32_t* in, int in_stride, uint32_t* out, int out_stride) {
  const int lane = blockIdx.x * blockDim.x + threadIdx.x;
  const int c = lane / Op::LANES;                            // blockDim is a multiple of 4: quads are never split
  if (c >= n) return;
  Op::run(in + (size_t)c * in_stride, out + (size_t)c * out_stride, lane % Op::LANES);
}

#define PROBE_HIP(x)                 \
  do {                               \
    hipError_t e_ = (x);             \
    if (e_ != hipSuccess) {          \
      st = (int)e_;                  \
      goto done;                     \
    }                                \
  } while (0)

// -2: the rows are too short for this operation (nothing is launched)
template <class Op>
int probe_launch(int n, const uint32_t* in, int in_stride, uint32_t* out, int out_stride) {
  if (n <= 0 || in_stride < Op::NIN || in_stride < 1 || out_stride < Op::NOUT) return -2;
  int st = 0;
  uint32_t *din = nullptr, *dout = nullptr;
  const size_t ib = (size_t)n * in_stride * 4, ob = (size_t)n * out_stride * 4;
  const int block = 64, lanes = n * Op::LANES;
  PROBE_HIP(hipMalloc(&din, ib));
  PROBE_HIP(hipMalloc(&dout, ob));
  PROBE_HIP(hipMemcpy(din, in, ib, hipMemcpyHostToDevice));
  PROBE_HIP(hipMemcpy(dout, out, ob, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(probe_kernel<Op>, dim3((lanes + block - 1) / block), dim3(block), 0, 0, n, din, in_stride, dout, out_stride);
  PROBE_HIP(hipGetLastError());
  PROBE_HIP(hipDeviceSynchronize());
  PROBE_HIP(hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost));
done:
  if (din) (void)hipFree(din);
  if (dout) (void)hipFree(dout);
  return st;
}

template <class P>
__device__ __forceinline__ Fu<P> ld_fu(const uint32_t* p) {
  Fu<P> r;
#pragma unroll
  for (int i = 0; i < Fu<P>::L; i++) r.v[i] = p[i];
  return r;
}
template <class P>
__device__ __forceinline__ void st_fu(uint32_t* p, const Fu<P>& a) {
#pragma unroll
  for (int i = 0; i < Fu<P>::L; i++) p[i] = a.v[i];
}
template <class P>
__device__ __forceinline__ Fp<P> ld_fp(const uint32_t* p) {
  Fp<P> r;
#pragma unroll
  for (int i = 0; i < P::N; i++) r.v[i] = p[i];
  return r;
}
template <class P>
__device__ __forceinline__ void st_fp(uint32_t* p, const Fp<P>& a) {
#pragma unroll
  for (int i = 0; i < P::N; i++) p[i] = a.v[i];
}

// dispatch helpers: `op` is the operation's name as the tests spell it
#define PROBE_OP(NAME, ...) \
  if (!strcmp(op, NAME)) return probe_launch<__VA_ARGS__>(n, in, in_stride, out, out_stride)
#define PROBE_ARGS const char *op, int field, int n, const uint32_t *in, int in_stride, uint32_t *out, int out_stride
constexpr int PROBE_UNKNOWN = -1;                            // this translation unit does not hold (op, field)

}  // namespace probe
