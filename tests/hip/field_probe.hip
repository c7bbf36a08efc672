// libzkp_field_probe.so: the one entry of the test-only arithmetic probe (see probe_common.hpp).  The operations themselves are
// in probe_fp.hip (saturated, built with and without ZKP_INLINE_MUL), probe_fu.hip, probe_g1.hip, probe_g2.hip and probe_ec.hip; the builder
// (tests/field_probe.py) compiles them as parallel objects.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

namespace probe {
#define PROBE_DECL(f) int f(const char* op, int field, int n, const uint32_t* in, int in_stride, uint32_t* out, int out_stride)
PROBE_DECL(probe_fp_inline);
PROBE_DECL(probe_fp_outline);
PROBE_DECL(probe_fu_9);
PROBE_DECL(probe_fu_14);
PROBE_DECL(probe_g1_c0);
PROBE_DECL(probe_g1_c1);
PROBE_DECL(probe_g2_c0_p0);
PROBE_DECL(probe_g2_c0_p1);
PROBE_DECL(probe_g2_c1_p0);
PROBE_DECL(probe_g2_c1_p1);
PROBE_DECL(probe_ec_c0_g1_p0);
PROBE_DECL(probe_ec_c0_g1_p1);
PROBE_DECL(probe_ec_c0_g1_p2);
PROBE_DECL(probe_ec_c0_g1_p3);
PROBE_DECL(probe_ec_c0_g2_p0);
PROBE_DECL(probe_ec_c0_g2_p1);
PROBE_DECL(probe_ec_c0_g2_p2);
PROBE_DECL(probe_ec_c0_g2_p3);
PROBE_DECL(probe_ec_c1_g1_p0);
PROBE_DECL(probe_ec_c1_g1_p1);
PROBE_DECL(probe_ec_c1_g1_p2);
PROBE_DECL(probe_ec_c1_g1_p3);
PROBE_DECL(probe_ec_c1_g2_p0);
PROBE_DECL(probe_ec_c1_g2_p1);
PROBE_DECL(probe_ec_c1_g2_p2);
PROBE_DECL(probe_ec_c1_g2_p3);
}  // namespace probe

// op: the operation's name ("fu_mul", "fu_sub<2>", "xyzz_madd_u", ...; "fp_*" / "fp2_*" take the prefix "inl:" or "ool:" for the
// inlined / out-of-line fp_mul).  field: 0 Bn254Fq, 1 Bn254Fr, 2 Bls381Fq, 3 Bls381Fr.  in / out: n rows of in_stride / out_stride
// uint32 words; the out rows are copied to the device too (operands of the in-memory operations).
// Returns the HIP status (0 = success), -1 for an (op, field) the probe does not hold, -2 for rows shorter than the operation needs.
extern "C" int zkp_probe_run(int device, const char* op, int field, int n, const uint32_t* in, int in_stride, uint32_t* out,
                             int out_stride) {
  using namespace probe;
  if (!op || !in || !out) return -2;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return (int)e;
  if (!strncmp(op, "inl:", 4)) return probe_fp_inline(op + 4, field, n, in, in_stride, out, out_stride);
  if (!strncmp(op, "ool:", 4)) return probe_fp_outline(op + 4, field, n, in, in_stride, out, out_stride);
  typedef int (*fn_t)(const char*, int, int, const uint32_t*, int, uint32_t*, int);
  const fn_t parts[] = {probe_fu_9,     probe_fu_14,    probe_g1_c0,    probe_g1_c1,
                        probe_g2_c0_p0, probe_g2_c0_p1, probe_g2_c1_p0, probe_g2_c1_p1,
                        probe_ec_c0_g1_p0, probe_ec_c0_g1_p1, probe_ec_c0_g1_p2, probe_ec_c0_g1_p3,
                        probe_ec_c0_g2_p0, probe_ec_c0_g2_p1, probe_ec_c0_g2_p2, probe_ec_c0_g2_p3,
                        probe_ec_c1_g1_p0, probe_ec_c1_g1_p1, probe_ec_c1_g1_p2, probe_ec_c1_g1_p3,
                        probe_ec_c1_g2_p0, probe_ec_c1_g2_p1, probe_ec_c1_g2_p2, probe_ec_c1_g2_p3};
  for (fn_t f : parts) {
    const int st = f(op, field, n, in, in_stride, out, out_stride);
    if (st != -1) return st;
  }
  return -1;
}
