// Test seam for the FP64 Poseidon2 permutations (poseidon2_f64.hip.h, poseidon2_w32_f64.hip.h) as the DEVICE computes them:
// v_fract_f64, the register pins and the compiler's contraction decisions are the device build's own, and a carried lane can
// be handed in at its stated maximum, which no product kernel does.  Built into the knobs library only
// (plonky3_recursion_amd/knobs/libp3r_hip.so, -DP3R_TUNING_KNOBS: what tests and tuning tools load); the product library
// neither compiles nor exports it.  Host arrays in, host arrays out, on the context's stream and pool.
// tests/test_gpu_p2f_device.py.
#include "poseidon2_w32_f64.hip.h"
#include "test_seam.h"

namespace p3r {
namespace {
constexpr int kSeamBlock = 256;

// one permutation per lane: `WIDTH` doubles in, every lane through p2f_store, canonical words out (row-major both ways)
template <class PP, int WIDTH, bool BUILTIN, unsigned MASK>
__global__ void __launch_bounds__(kSeamBlock)
k_test_p2f_permute(const double* __restrict__ states, size_t n, uint32_t* __restrict__ out, const double* __restrict__ tab) {
  const size_t i = (size_t)blockIdx.x * kSeamBlock + threadIdx.x;
  if (i >= n) return;
  double s[WIDTH];
#pragma unroll
  for (int k = 0; k < WIDTH; ++k) s[k] = states[i * WIDTH + k];
  if constexpr (WIDTH == P2_WIDTH) p2f_permute<PP, MASK>(s, tab);
  else p2wf_permute<PP, BUILTIN, MASK>(s, tab);
#pragma unroll
  for (int k = 0; k < WIDTH; ++k) out[i * WIDTH + k] = Fp<PP>::raw(p2f_store<PP>(s[k])).to_canonical();
}
template <class PP>
__global__ void __launch_bounds__(kSeamBlock) k_test_p2f_store(const double* __restrict__ x, size_t n, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kSeamBlock + threadIdx.x;
  if (i < n) out[i] = Fp<PP>::raw(p2f_store<PP>(x[i])).to_canonical();
}

using PermuteKernel = void (*)(const double*, size_t, uint32_t*, const double*);
// the masks the kernels instantiate (kernels.hip.h, kernels_stark.hip.h, kernels_mmcs4.hip.h), no others
template <class PP>
PermuteKernel permute_kernel(int width, uint32_t mask, bool general) {
  if (width == P2_WIDTH) {
    switch (mask) {
      case 0x0000u: return &k_test_p2f_permute<PP, P2_WIDTH, true, 0x0000u>;
      case 0x00FFu: return &k_test_p2f_permute<PP, P2_WIDTH, true, 0x00FFu>;
      case 0xFF00u: return &k_test_p2f_permute<PP, P2_WIDTH, true, 0xFF00u>;
      case 0xFFFFu: return &k_test_p2f_permute<PP, P2_WIDTH, true, 0xFFFFu>;
    }
    return nullptr;
  }
  switch (mask) {
    case 0x00000000u: return general ? &k_test_p2f_permute<PP, P2W_WIDTH, false, 0x00000000u> : &k_test_p2f_permute<PP, P2W_WIDTH, true, 0x00000000u>;
    case 0x000000FFu: return general ? &k_test_p2f_permute<PP, P2W_WIDTH, false, 0x000000FFu> : &k_test_p2f_permute<PP, P2W_WIDTH, true, 0x000000FFu>;
    case 0xFF000000u: return general ? &k_test_p2f_permute<PP, P2W_WIDTH, false, 0xFF000000u> : &k_test_p2f_permute<PP, P2W_WIDTH, true, 0xFF000000u>;
    case 0xFFFFFFFFu: return general ? &k_test_p2f_permute<PP, P2W_WIDTH, false, 0xFFFFFFFFu> : &k_test_p2f_permute<PP, P2W_WIDTH, true, 0xFFFFFFFFu>;
  }
  return nullptr;
}

template <class PP>
void test_permute(p3r_ctx* ctx, int width, uint32_t mask, int general, const double* states, size_t n, uint32_t* out) {
  if (width != P2_WIDTH && width != P2W_WIDTH) fail(P3R_EINVAL, "width must be 16 or 32, got %d", width);
  if (general != 0 && general != 1) fail(P3R_EINVAL, "general_diag must be 0 or 1");
  if (width == P2_WIDTH && general) fail(P3R_EINVAL, "the width-16 diagonal is not data: general_diag must be 0");
  const PermuteKernel kern = permute_kernel<PP>(width, mask, general != 0);
  if (!kern) fail(P3R_EINVAL, "carried mask 0x%x is not one the kernels instantiate", mask);
  if (width == P2W_WIDTH && !general) {
    // the BUILTIN instance has the built-in diagonal compiled in: only meaningful when that is the configured one
    const uint32_t* builtin = PP::FIELD_ID == 0 ? kDefaultDiagW32_koala_bear : kDefaultDiagW32_baby_bear;
    const uint32_t* diag = ctx->rc_canonical.data() + p2_num_constants<PP>() + p2w_num_rc<PP>();
    if (!std::equal(builtin, builtin + P2W_WIDTH, diag)) fail(P3R_EINVAL, "general_diag = 0 with a configured diagonal that is not the built-in one");
  }
  if (!n) return;
  if (!states || !out) fail(P3R_EINVAL, "NULL argument");
  const size_t cells = n * (size_t)width;
  DevBuf in(2 * cells), res(cells);
  P3R_HIP(hipMemcpyAsync(in.p, states, cells * 8, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(kern, dim3((unsigned)((n + kSeamBlock - 1) / kSeamBlock)), dim3(kSeamBlock), 0, ctx->stream,
                     reinterpret_cast<const double*>(in.p), n, res.p, width == P2_WIDTH ? ctx->rcd() : ctx->rcd_w32());
  P3R_HIP(hipGetLastError());
  P3R_HIP(copy_sync(ctx->stream, out, res.p, cells * 4, hipMemcpyDeviceToHost));
}

template <class PP>
void test_store(p3r_ctx* ctx, const double* x, size_t n, uint32_t* out) {
  if (!n) return;
  if (!x || !out) fail(P3R_EINVAL, "NULL argument");
  DevBuf in(2 * n), res(n);
  P3R_HIP(hipMemcpyAsync(in.p, x, n * 8, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_test_p2f_store<PP>, dim3((unsigned)((n + kSeamBlock - 1) / kSeamBlock)), dim3(kSeamBlock), 0, ctx->stream,
                     reinterpret_cast<const double*>(in.p), n, res.p);
  P3R_HIP(hipGetLastError());
  P3R_HIP(copy_sync(ctx->stream, out, res.p, n * 4, hipMemcpyDeviceToHost));
}
}  // namespace
}  // namespace p3r

using namespace p3r;

extern "C" {
int p3r_test_p2f_permute(p3r_ctx* ctx, int width, uint32_t carried_mask, int general_diag, const double* states, size_t n, uint32_t* out) {
  return seam(ctx, [&] {
    if (ctx->cfg.field == P3R_FIELD_KOALA_BEAR) test_permute<KoalaBearParams>(ctx, width, carried_mask, general_diag, states, n, out);
    else test_permute<BabyBearParams>(ctx, width, carried_mask, general_diag, states, n, out);
  });
}
int p3r_test_p2f_store(p3r_ctx* ctx, const double* x, size_t n, uint32_t* out) {
  return seam(ctx, [&] {
    if (ctx->cfg.field == P3R_FIELD_KOALA_BEAR) test_store<KoalaBearParams>(ctx, x, n, out);
    else test_store<BabyBearParams>(ctx, x, n, out);
  });
}
}
