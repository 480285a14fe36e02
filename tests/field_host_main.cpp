// The host half of the field-arithmetic check: csrc/field.h and csrc/field_test_ops.h compiled by g++ alone (no HIP), so
// that the host branch of reduce64 - what the native verifier and the host transcript run - sees the same cases as the
// device (tests/field_cases.py).  argv[1] is the field (0 KoalaBear, 1 BabyBear).  stdin: records of five u32 words
// {op, words in per case, words out per case, cases, aux} followed by the operand words; stdout: the result words of each
// record in order.  Any refusal is exit status 2 with a line on stderr.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "field_test_ops.h"

template <class PP>
static int run() {
  uint32_t hdr[5];
  std::vector<uint32_t> in, out;
  for (;;) {
    const size_t got = fread(hdr, 4, 5, stdin);
    if (got == 0) return 0;
    if (got != 5) { fprintf(stderr, "truncated record header\n"); return 2; }
    const int op = (int)hdr[0];
    int wi = 0, wo = 0;
    if (!p3r::field_test_shape(op, &wi, &wo) || (p3r::field_test_is_quintic(op) && !p3r::kHasQuintic<PP>)) {
      fprintf(stderr, "op %d is no operation of this field\n", op);
      return 2;
    }
    if ((uint32_t)wi != hdr[1] || (uint32_t)wo != hdr[2]) {
      fprintf(stderr, "op %d reads %d and writes %d words a case, got %u and %u\n", op, wi, wo, hdr[1], hdr[2]);
      return 2;
    }
    const size_t n = hdr[3];
    in.resize(n * wi);
    out.assign(n * wo, 0xFFFFFFFFu);
    if (fread(in.data(), 4, in.size(), stdin) != in.size()) { fprintf(stderr, "truncated operands of op %d\n", op); return 2; }
    for (size_t i = 0; i < n; ++i)
      if (!p3r::field_test_apply<PP>(op, in.data() + i * wi, out.data() + i * wo, hdr[4])) return 2;
    if (fwrite(out.data(), 4, out.size(), stdout) != out.size()) return 2;
  }
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s <0|1>\n", argv[0]); return 2; }
  return atoi(argv[1]) == 0 ? run<p3r::KoalaBearParams>() : run<p3r::BabyBearParams>();
}
