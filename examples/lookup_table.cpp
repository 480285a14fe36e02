// C++ caller of p3r::lookup_multiplicities through include/p3r.hpp: a range check, with the table's multiplicity column
// built on the device from the resident column it checks.
//
// A column v of 64 rows, v[r] = floor(r^2 / 3) mod 16, is checked against the table t = 0 .. 15 (16 rows, k = 4).  Both sides
// key a value x as c - x for a constant c, which is exact for a single field (p3r.h).  The query asks for c - v once per
// row; every table row offers c - t.  p3r::lookup_multiplicities returns the 16 x 1 column m of how often each t is asked
// for.  The bus - the query with multiplicity 1, the table with multiplicity -m read from that column - is then balanced,
// which p3r::check_lookups confirms.  Then v[37] is overwritten with 16, which the table does not hold, and the join
// reports that miss with its row.
//
//   lookup_table <koala-bear|baby-bear> <challenge degree>
//
// Output: "counts <m[0] .. m[15]>", "bus ok", "missing <count>" and per key "key first at query <q> row <r> term <t>,
// <n> records, net <DC words>"; then "ok".  Exits non-zero if a step does not find what it should.
#include <cstdio>
#include <cstring>
#include <iostream>

#include "p3r.hpp"

static const uint32_t kShift = 1000003u;   // the constant c of the key c - x

// the key of column 0 of matrix 0, with `multiplicity` as the term's multiplicity
static void range_term(p3r::AirProgram& air, p3r::AirProgram::Value multiplicity) {
  air.lookup(multiplicity, air.constant(kShift) - air.local(0, 0));
  air.end_lookup_column();
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s <koala-bear|baby-bear> <challenge degree>\n", argv[0]);
    return 2;
  }
  try {
    const p3r::Field field = std::strcmp(argv[1], "koala-bear") == 0 ? p3r::Field::KoalaBear : p3r::Field::BabyBear;
    const uint32_t dc = (uint32_t)std::stoul(argv[2]);
    p3r::Context ctx(field, p3r::FriParams{}, 0, {}, 4, 0, dc);

    const size_t h = 64, ht = 16, spoilt = 37;
    std::vector<uint32_t> v(h), t(ht);
    for (size_t r = 0; r < h; ++r) v[r] = (uint32_t)(r * r / 3 % ht);
    for (size_t r = 0; r < ht; ++r) t[r] = (uint32_t)r;
    p3r::AirProgram asks, offers, receives;
    range_term(asks, asks.constant(1));                // the query: every row asks once
    range_term(offers, offers.constant(1));            // the table in the join: every row is enabled
    range_term(receives, -receives.local(1, 0));       // the table on the bus: minus the count, from the column built below

    // ---- the counts, and the bus they balance
    p3r_dmat* d_v = ctx.ptr(p3r_dmat_upload(ctx.raw(), v.data(), h, 1));
    p3r_dmat* d_t = ctx.ptr(p3r_dmat_upload(ctx.raw(), t.data(), ht, 1));
    const p3r::LookupMultiplicities got = p3r::lookup_multiplicities(ctx, {&offers, {d_t}, {}}, {{&asks, {d_v}, {}}});
    std::vector<uint32_t> m(ht);
    ctx.check(p3r_dmat_download(ctx.raw(), got.column, m.data()));
    std::cout << "counts";
    for (uint32_t c : m) std::cout << ' ' << c;
    std::cout << '\n';
    if (got.n_missing) throw std::runtime_error("a value of the column is reported missing from the table");
    const p3r::LookupCheck bus = p3r::check_lookups(ctx, {{&asks, {d_v}, {}}, {&receives, {d_t, got.column}, {}}});
    p3r_dmat_free(ctx.raw(), got.column);
    p3r_dmat_free(ctx.raw(), d_v);
    if (bus.n_unbalanced) throw std::runtime_error("the bus does not balance under the counts");
    std::cout << "bus ok\n";

    // ---- one value out of range
    v[spoilt] = (uint32_t)ht;
    d_v = ctx.ptr(p3r_dmat_upload(ctx.raw(), v.data(), h, 1));
    const p3r::LookupMultiplicities off = p3r::lookup_multiplicities(ctx, {&offers, {d_t}, {}}, {{&asks, {d_v}, {}}});
    p3r_dmat_free(ctx.raw(), off.column);
    p3r_dmat_free(ctx.raw(), d_v);
    p3r_dmat_free(ctx.raw(), d_t);
    std::cout << "missing " << off.n_missing << '\n';
    for (const p3r_lookup_imbalance& e : off.missing) {
      std::cout << "key first at query " << e.instance << " row " << e.row << " term " << e.term << ", " << e.n_records << " records, net";
      for (uint32_t k = 0; k < dc; ++k) std::cout << ' ' << e.net[k];
      std::cout << '\n';
    }
    if (off.n_missing != 1 || off.missing[0].instance != 0 || off.missing[0].row != spoilt || off.missing[0].n_records != 1 ||
        off.missing[0].net[0] != 1 || off.missing[0].denominator[0] != kShift - ht)
      throw std::runtime_error("the value out of range was not located");
    std::cout << "ok" << std::endl;
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
