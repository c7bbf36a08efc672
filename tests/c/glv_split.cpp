// CPU run of the scalar split as shipped: ckb_zkp_amd/csrc/glv.hpp included unchanged and compiled for the host alone
// (hipcc -x hip --cuda-host-only).  Reads "<curve> <64 hex digits>" lines (curve 0 = BN254, 1 = BLS12-381; the scalar is the
// canonical integer, most significant digit first) from stdin and prints "neg1 |k1| neg2 |k2|" (magnitudes as 40 hex digits)
// for each line.  Every check is done by the caller in Python integers (tests/test_glv_split.py).
#include "glv.hpp"

#include <cstdio>
#include <cstring>

static int hexval(char c) {
  if (c >= '0' && c <= '9') return c - '0';
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  if (c >= 'A' && c <= 'F') return c - 'A' + 10;
  return -1;
}

static void print5(const uint32_t* w) {
  for (int i = 4; i >= 0; i--) printf("%08x", w[i]);
}

int main() {
  char line[256];
  long n = 0;
  while (fgets(line, sizeof line, stdin)) {
    n++;
    int curve = -1;
    char hex[128];
    if (sscanf(line, "%d %127s", &curve, hex) != 2 || (curve != 0 && curve != 1) || strlen(hex) != 64) {
      fprintf(stderr, "line %ld: expected \"<0|1> <64 hex digits>\"\n", n);
      return 2;
    }
    uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 64; i++) {
      const int v = hexval(hex[63 - i]);
      if (v < 0) {
        fprintf(stderr, "line %ld: not a hex digit\n", n);
        return 2;
      }
      k[i >> 3] |= (uint32_t)v << (4 * (i & 7));
    }
    uint32_t k1[5], k2[5];
    int neg1 = -1, neg2 = -1;
    if (curve == 0) zkp::glv_decompose<zkp::GlvConst<zkp::Bn254Fq>>(k, k1, &neg1, k2, &neg2);
    else zkp::glv_decompose<zkp::GlvConst<zkp::Bls381Fq>>(k, k1, &neg1, k2, &neg2);
    printf("%d ", neg1);
    print5(k1);
    printf(" %d ", neg2);
    print5(k2);
    printf("\n");
  }
  return 0;
}
