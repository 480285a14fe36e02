// Test seam for device_prims.hip.h.  Built into the knobs library only (plonky3_recursion_amd/knobs/libp3r_hip.so,
// -DP3R_TUNING_KNOBS: what tests and tuning tools load); the product library neither compiles nor exports it.
// Host arrays in, host arrays out, on the context's stream and pool.  tests/test_gpu_device_prims.py.
#include "device_prims.hip.h"
#include "test_seam.h"

namespace p3r {
namespace {
struct LoadU64 {
  const uint64_t* p;
  __device__ uint64_t operator()(size_t i) const { return p[i]; }
};
}  // namespace
}  // namespace p3r

using namespace p3r;

extern "C" {
int p3r_test_exclusive_sum_u32(p3r_ctx* ctx, const uint32_t* in, uint32_t* out, size_t n, int in_place) {
  return seam(ctx, [&] {
    if (!n) return;
    DevBuf a(n), b(n);
    P3R_HIP(hipMemcpyAsync(a.p, in, n * 4, hipMemcpyHostToDevice, ctx->stream));
    uint32_t* dst = in_place ? a.p : b.p;
    prims::exclusive_sum<uint32_t>(ctx->stream, prims::LoadU32{a.p}, n, dst);
    P3R_HIP(copy_sync(ctx->stream, out, dst, n * 4, hipMemcpyDeviceToHost));
  });
}
int p3r_test_exclusive_sum_u64(p3r_ctx* ctx, const uint64_t* in, uint64_t* out, size_t n) {
  return seam(ctx, [&] {
    if (!n) return;
    DevBuf a(2 * n), b(2 * n);
    P3R_HIP(hipMemcpyAsync(a.p, in, n * 8, hipMemcpyHostToDevice, ctx->stream));
    prims::exclusive_sum<uint64_t>(ctx->stream, LoadU64{reinterpret_cast<const uint64_t*>(a.p)}, n, reinterpret_cast<uint64_t*>(b.p));
    P3R_HIP(copy_sync(ctx->stream, out, b.p, n * 8, hipMemcpyDeviceToHost));
  });
}
int p3r_test_reduce_max(p3r_ctx* ctx, const uint32_t* in, size_t n, uint32_t* out) {
  return seam(ctx, [&] {
    DevBuf a(n + 1), m(1);
    if (n) P3R_HIP(hipMemcpyAsync(a.p, in, n * 4, hipMemcpyHostToDevice, ctx->stream));
    prims::reduce_max(ctx->stream, prims::LoadU32{a.p}, n, m.p);
    P3R_HIP(copy_sync(ctx->stream, out, m.p, 4, hipMemcpyDeviceToHost));
  });
}
int p3r_test_sort_pairs(p3r_ctx* ctx, const uint32_t* keys, const uint32_t* vals, size_t n, int bits, uint32_t* keys_out, uint32_t* vals_out) {
  return seam(ctx, [&] {
    if (!n) return;
    DevBuf k(n), v(n), ko(n), vo(n);
    P3R_HIP(hipMemcpyAsync(k.p, keys, n * 4, hipMemcpyHostToDevice, ctx->stream));
    P3R_HIP(hipMemcpyAsync(v.p, vals, n * 4, hipMemcpyHostToDevice, ctx->stream));
    prims::sort_pairs(ctx->stream, k.p, ko.p, v.p, vo.p, n, bits);
    P3R_HIP(hipMemcpyAsync(keys_out, ko.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    P3R_HIP(copy_sync(ctx->stream, vals_out, vo.p, n * 4, hipMemcpyDeviceToHost));
  });
}
// The three idioms of the preparation pass.  The device copies of the outputs start as the caller's arrays and are read
// back whole (rank: n + 1, list: n), so the caller sees whatever a call touched - nothing, at n = 0.
// with_list = 0: ranks and count only; blocking = 1: the form that returns the count (*count), else the count is rank[n].
int p3r_test_select_marked(p3r_ctx* ctx, const uint32_t* marks, size_t n, int with_list, int blocking, uint32_t* rank, uint32_t* list,
                           size_t* count) {
  return seam(ctx, [&] {
    DevBuf m(n + 1), r(n + 1), l(n + 1);
    if (n) P3R_HIP(hipMemcpyAsync(m.p, marks, n * 4, hipMemcpyHostToDevice, ctx->stream));
    P3R_HIP(hipMemcpyAsync(r.p, rank, (n + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    if (n) P3R_HIP(hipMemcpyAsync(l.p, list, n * 4, hipMemcpyHostToDevice, ctx->stream));
    if (blocking) *count = prims::select_marked_count(ctx->stream, m.p, n, r.p, with_list ? l.p : nullptr);
    else prims::select_marked(ctx->stream, m.p, n, r.p, with_list ? l.p : nullptr);
    if (n) P3R_HIP(hipMemcpyAsync(list, l.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    P3R_HIP(copy_sync(ctx->stream, rank, r.p, (n + 1) * 4, hipMemcpyDeviceToHost));
  });
}
int p3r_test_ranks_of_u64(p3r_ctx* ctx, const uint64_t* in, uint64_t* out /* n + 1 */, size_t n) {
  return seam(ctx, [&] {
    DevBuf a(2 * (n + 1)), b(2 * (n + 1));
    if (n) P3R_HIP(hipMemcpyAsync(a.p, in, n * 8, hipMemcpyHostToDevice, ctx->stream));
    prims::ranks_of<uint64_t>(ctx->stream, LoadU64{reinterpret_cast<const uint64_t*>(a.p)}, n, reinterpret_cast<uint64_t*>(b.p));
    P3R_HIP(copy_sync(ctx->stream, out, b.p, (n + 1) * 8, hipMemcpyDeviceToHost));
  });
}
// first: n_keys cells, order: n, offs: n (lens = NULL: without lengths, offs is not touched)
int p3r_test_order_by_level(p3r_ctx* ctx, const uint32_t* keys, const uint32_t* lens, size_t n, int lbits, size_t n_keys, uint32_t* first,
                            uint32_t* order, uint32_t* offs) {
  return seam(ctx, [&] {
    DevBuf k(n + 1), ln(n + 1), f(n_keys + 1), o(n + 1), of(n + 1);
    P3R_HIP(hipMemcpyAsync(f.p, first, n_keys * 4, hipMemcpyHostToDevice, ctx->stream));
    if (n) {
      P3R_HIP(hipMemcpyAsync(k.p, keys, n * 4, hipMemcpyHostToDevice, ctx->stream));
      if (lens) P3R_HIP(hipMemcpyAsync(ln.p, lens, n * 4, hipMemcpyHostToDevice, ctx->stream));
      P3R_HIP(hipMemcpyAsync(o.p, order, n * 4, hipMemcpyHostToDevice, ctx->stream));
      P3R_HIP(hipMemcpyAsync(of.p, offs, n * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    prims::order_by_level(ctx->stream, k.p, n, lbits, f.p, o.p, lens ? ln.p : nullptr, lens ? of.p : nullptr);
    if (n) {
      P3R_HIP(hipMemcpyAsync(order, o.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
      P3R_HIP(hipMemcpyAsync(offs, of.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    P3R_HIP(copy_sync(ctx->stream, first, f.p, n_keys * 4, hipMemcpyDeviceToHost));
  });
}
}
