// Test seam for field.h as the DEVICE computes it: the __HIP_DEVICE_COMPILE__ branch of reduce64 / reduce64_lazy (REDC as
// one 64-bit multiply-add with a min fix-up) and everything whose range argument leans on it - dot2, sqr_times, cube, the
// extension products, the Frobenius tables, the inverses.  One case per lane through field_test_apply (field_test_ops.h),
// raw Montgomery words in and out.  Built into the knobs library only (plonky3_recursion_amd/knobs/libp3r_hip.so,
// -DP3R_TUNING_KNOBS: what tests and tuning tools load); the product library neither compiles nor exports it.
// Host arrays in, host arrays out, on the context's stream and pool.  tests/test_gpu_field_device.py.
#include "field_test_ops.h"
#include "test_seam.h"

namespace p3r {
namespace {
constexpr int kSeamBlock = 256;

template <class PP>
__global__ void __launch_bounds__(kSeamBlock)
k_test_field_op(int op, const uint32_t* __restrict__ in, int words_in, uint32_t* __restrict__ out, int words_out, size_t n, uint32_t aux) {
  const size_t i = (size_t)blockIdx.x * kSeamBlock + threadIdx.x;
  if (i >= n) return;
  field_test_apply<PP>(op, in + i * words_in, out + i * words_out, aux);
}

template <class PP>
void test_field_op(p3r_ctx* ctx, int op, const uint32_t* in, size_t words_in, uint32_t* out, size_t words_out, size_t n, uint32_t aux) {
  int wi = 0, wo = 0;
  if (!field_test_shape(op, &wi, &wo)) fail(P3R_EINVAL, "field_op %d is no operation", op);
  if (field_test_is_quintic(op) && !kHasQuintic<PP>) fail(P3R_EINVAL, "field_op %d: the quintic extension exists over KoalaBear only", op);
  if (words_in != (size_t)wi || words_out != (size_t)wo)
    fail(P3R_EINVAL, "field_op %d reads %d and writes %d words a case, got %zu and %zu", op, wi, wo, words_in, words_out);
  if (n > ((size_t)1 << 24)) fail(P3R_EINVAL, "at most 2^24 cases a call, got %zu", n);
  if (!n) return;
  if (!in || !out) fail(P3R_EINVAL, "NULL argument");
  DevBuf din(n * wi), res(n * wo);
  P3R_HIP(hipMemcpyAsync(din.p, in, n * wi * 4, hipMemcpyHostToDevice, ctx->stream));
  P3R_HIP(hipMemsetAsync(res.p, 0xFF, n * wo * 4, ctx->stream));   // a word the kernel did not write is in no field
  hipLaunchKernelGGL(k_test_field_op<PP>, dim3((unsigned)((n + kSeamBlock - 1) / kSeamBlock)), dim3(kSeamBlock), 0, ctx->stream,
                     op, din.p, wi, res.p, wo, n, aux);
  P3R_HIP(hipGetLastError());
  P3R_HIP(copy_sync(ctx->stream, out, res.p, n * wo * 4, hipMemcpyDeviceToHost));
}
}  // namespace
}  // namespace p3r

using namespace p3r;

extern "C" {
int p3r_test_field_op(p3r_ctx* ctx, int field_op, const uint32_t* in_words, size_t words_in_per_case, uint32_t* out_words,
                      size_t words_out_per_case, size_t n_cases, uint32_t aux) {
  return seam(ctx, [&] {
    if (ctx->cfg.field == P3R_FIELD_KOALA_BEAR) test_field_op<KoalaBearParams>(ctx, field_op, in_words, words_in_per_case, out_words, words_out_per_case, n_cases, aux);
    else test_field_op<BabyBearParams>(ctx, field_op, in_words, words_in_per_case, out_words, words_out_per_case, n_cases, aux);
  });
}
}
