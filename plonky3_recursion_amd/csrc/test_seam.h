// The wrapper of the p3r_test_* seam functions (tu_prims_test.hip, tu_p2f_test.hip; knobs library only): the context's
// device and pool for the call, errors into the context as the product's entry points report them.
#pragma once
#include "context.h"

namespace p3r {
namespace {
template <class Fn>
int seam(p3r_ctx* ctx, Fn&& fn) {
  try {
    if (!ctx) return P3R_EINVAL;
    (void)hipSetDevice(ctx->cfg.device);
    tls_pool() = ctx->pool;
    fn();
    return P3R_OK;
  } catch (const Error& e) {
    ctx->err = e.what();
    return e.code;
  } catch (const std::exception& e) {
    ctx->err = e.what();
    return P3R_EINVAL;
  }
}
}  // namespace
}  // namespace p3r
