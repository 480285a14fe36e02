// C++ caller of p3r::witness_columns through include/p3r.hpp: a 16-bit range check whose derived columns - everything but
// the values themselves - are built on the device.
//
// One column v of 64 rows is uploaded, v[r] = 1021 r mod 2^16 with every eighth row zeroed.  A witness program derives the
// byte limbs lo = bits [0, 8) and hi = bits [8, 16) of v, the inverse witness w = 1 / v (0 for v = 0) and the is-zero flag
// z = 1 - v w.  A second one, with no input at all, derives the byte table t = 0 .. 255 from the row index.
// p3r::lookup_multiplicities then counts how often each byte is asked for, under the key c - x (exact for a single field,
// p3r.h); p3r::check_constraints confirms v = lo + 256 hi, v z = 0 and z = 1 - v w on the derived trace, and
// p3r::check_lookups that the counts balance the bus.  Nothing but v is computed on the host.
//
//   witness_program <koala-bear|baby-bear> <challenge degree>
//
// Output: "derived <width> columns, table <rows> rows", "zeros <count>", "bytes <asked for> <distinct>", then "ok".
// Exits non-zero if a step does not find what it should.
#include <cstdio>
#include <cstring>
#include <iostream>

#include "p3r.hpp"

static const uint32_t kShift = 1000003u;   // the constant c of the key c - x

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s <koala-bear|baby-bear> <challenge degree>\n", argv[0]);
    return 2;
  }
  try {
    const p3r::Field field = std::strcmp(argv[1], "koala-bear") == 0 ? p3r::Field::KoalaBear : p3r::Field::BabyBear;
    const uint32_t dc = (uint32_t)std::stoul(argv[2]);
    p3r::Context ctx(field, p3r::FriParams{}, 0, {}, 4, 0, dc);

    const size_t h = 64, ht = 256;
    std::vector<uint32_t> v(h);
    for (size_t r = 0; r < h; ++r) v[r] = r % 8 == 0 ? 0u : (uint32_t)(1021 * r % 65536);
    p3r_dmat* d_v = ctx.ptr(p3r_dmat_upload(ctx.raw(), v.data(), h, 1));

    // ---- the derived columns: lo, hi, w, z of the values; t of the table
    p3r::AirProgram derive, table;
    {
      const auto x = derive.local(0, 0);
      const auto w = derive.inv(x);
      derive.store(derive.bits(x, 0, 8), 0);
      derive.store(derive.bits(x, 8, 8), 1);
      derive.store(w, 2);
      derive.store(derive.constant(1) - x * w, 3);
      table.store(table.row(), 0);
    }
    p3r_dmat* d_w = p3r::witness_columns(ctx, derive, {d_v});
    p3r_dmat* d_t = p3r::witness_columns(ctx, table, {}, ht);
    std::cout << "derived " << p3r_dmat_width(d_w) << " columns, table " << p3r_dmat_height(d_t) << " rows\n";

    // ---- the constraints of the gadgets on the derived trace
    p3r::AirProgram air;
    {
      const auto x = air.local(0, 0), lo = air.local(1, 0), hi = air.local(1, 1), w = air.local(1, 2), z = air.local(1, 3);
      air.assert_zero(x - lo - air.constant(256) * hi);
      air.assert_zero(x * z);
      air.assert_zero(z + x * w - air.constant(1));
    }
    const p3r::ConstraintCheck cc = p3r::check_constraints(ctx, air, {d_v, d_w});
    if (!cc.satisfied()) throw std::runtime_error("the derived columns do not satisfy the gadgets' constraints");
    std::vector<uint32_t> derived(h * 4);
    ctx.check(p3r_dmat_download(ctx.raw(), d_w, derived.data()));
    size_t zeros = 0;
    for (size_t r = 0; r < h; ++r) zeros += derived[r * 4 + 3];
    std::cout << "zeros " << zeros << '\n';

    // ---- the bytes against the table: the counts on the device, and the bus they balance
    p3r::AirProgram asks, offers, receives;
    for (uint32_t limb = 0; limb < 2; ++limb) asks.lookup(asks.constant(1), asks.constant(kShift) - asks.local(0, limb));
    asks.end_lookup_column();
    offers.lookup(offers.constant(1), offers.constant(kShift) - offers.local(0, 0));
    offers.end_lookup_column();
    receives.lookup(-receives.local(1, 0), receives.constant(kShift) - receives.local(0, 0));
    receives.end_lookup_column();
    const p3r::LookupMultiplicities got = p3r::lookup_multiplicities(ctx, {&offers, {d_t}, {}}, {{&asks, {d_w}, {}}});
    if (got.n_missing) throw std::runtime_error("a limb is reported missing from the byte table");
    std::vector<uint32_t> m(ht);
    ctx.check(p3r_dmat_download(ctx.raw(), got.column, m.data()));
    size_t asked = 0, distinct = 0;
    for (uint32_t c : m) {
      asked += c;
      distinct += c != 0;
    }
    std::cout << "bytes " << asked << ' ' << distinct << '\n';
    const p3r::LookupCheck bus = p3r::check_lookups(ctx, {{&asks, {d_w}, {}}, {&receives, {d_t, got.column}, {}}});
    p3r_dmat_free(ctx.raw(), got.column);
    p3r_dmat_free(ctx.raw(), d_t);
    p3r_dmat_free(ctx.raw(), d_w);
    p3r_dmat_free(ctx.raw(), d_v);
    if (bus.n_unbalanced) throw std::runtime_error("the bus does not balance under the counts");
    if (asked != 2 * h) throw std::runtime_error("the counts do not add up to two limbs per row");
    std::cout << "ok" << std::endl;
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
