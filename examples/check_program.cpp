// C++ caller of the two trace checks through include/p3r.hpp: "is my trace right?" answered on the device, with a place.
//
// 1. A Fibonacci-style table of 64 rows, columns (a, b): a' = b and b' = a + b on every transition, a = 0 and b = 1 in the
//    first row, b = the public value in the last.  p3r::check_constraints passes it; then one cell is overwritten and the
//    check names the rows and the constraints the cell breaks.
// 2. Two tables on one bus with the reference's denominator bus_prefix + t0 + beta * t1 (challenges [bus_prefix, beta]):
//    a sender of 16 rows sends its tuple with the multiplicity in its third column, a receiver of 8 rows receives each
//    distinct tuple with minus the number of times it was sent.  p3r::check_lookups finds the bus balanced; then one send
//    is dropped (its multiplicity set to 0) and the check names the tuple's first record and what is missing.
//
//   check_program <koala-bear|baby-bear> <challenge degree>
//
// Output: "constraints ok", "constraint <k> fails first in row <r> (<n> rows)" per broken constraint and the report's
// "first failure: row <r> constraint <k>"; "bus ok", then "unbalanced <count>" and per key "key first at instance <p> row
// <r> term <t>, <n> records, net <DC words>"; then "ok".  Exits non-zero if a check does not find what was planted.
#include <cstdio>
#include <cstring>
#include <iostream>

#include "p3r.hpp"

static p3r::AirProgram fibonacci() {
  p3r::AirProgram air;
  const auto a = air.local(0, 0), b = air.local(0, 1), a_next = air.next(0, 0), b_next = air.next(0, 1);
  air.assert_zero(air.is_transition() * (a_next - b));              // constraint 0
  air.assert_zero(air.is_transition() * (b_next - (a + b)));        // constraint 1
  air.assert_zero(air.is_first_row() * a);                          // constraint 2
  air.assert_zero(air.is_first_row() * (b - air.constant(1)));      // constraint 3
  air.assert_zero(air.is_last_row() * (b - air.public_value(0)));   // constraint 4
  return air;
}

// multiplicity: column 2 of the table; the receiver's column holds the field's negatives
static p3r::AirProgram bus_interaction() {
  p3r::AirProgram air;
  air.lookup(air.local(0, 2), air.challenge(0) + air.local(0, 0) + air.challenge(1) * air.local(0, 1));
  air.end_lookup_column();
  return air;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s <koala-bear|baby-bear> <challenge degree>\n", argv[0]);
    return 2;
  }
  try {
    const p3r::Field field = std::strcmp(argv[1], "koala-bear") == 0 ? p3r::Field::KoalaBear : p3r::Field::BabyBear;
    const uint32_t dc = (uint32_t)std::stoul(argv[2]);
    const uint32_t p = field == p3r::Field::KoalaBear ? 0x7f000001u : 0x78000001u;
    p3r::Context ctx(field, p3r::FriParams{}, 0, {}, 4, 0, dc);

    // ---- 1. the constraints
    const size_t h = 64, wrong_row = 37;
    std::vector<uint32_t> fib(h * 2);
    uint32_t a = 0, b = 1;
    for (size_t r = 0; r < h; ++r) {
      fib[2 * r] = a;
      fib[2 * r + 1] = b;
      const uint32_t c = (uint32_t)(((uint64_t)a + b) % p);
      a = b;
      b = c;
    }
    const std::vector<uint32_t> publics = {fib[2 * (h - 1) + 1]};
    const p3r::AirProgram air = fibonacci();
    p3r_dmat* good = ctx.ptr(p3r_dmat_upload(ctx.raw(), fib.data(), h, 2));
    const p3r::ConstraintCheck pass = p3r::check_constraints(ctx, air, {good}, publics);
    p3r_dmat_free(ctx.raw(), good);
    if (!pass.satisfied() || pass.report.n_failures) throw std::runtime_error("the Fibonacci trace does not satisfy its own constraints");
    std::cout << "constraints ok\n";
    fib[2 * wrong_row + 1] = (fib[2 * wrong_row + 1] + 1) % p;   // b of row 37: breaks b' = a + b into it and a' = b, b' = a + b out of it
    p3r_dmat* bad = ctx.ptr(p3r_dmat_upload(ctx.raw(), fib.data(), h, 2));
    const p3r::ConstraintCheck found = p3r::check_constraints(ctx, air, {bad}, publics);
    p3r_dmat_free(ctx.raw(), bad);
    for (size_t k = 0; k < found.first_row.size(); ++k)
      if (found.n_failed[k]) std::cout << "constraint " << k << " fails first in row " << found.first_row[k] << " (" << found.n_failed[k] << " rows)\n";
    std::cout << "first failure: row " << found.report.first_row << " constraint " << found.report.first_constraint << '\n';
    if (found.report.first_row != wrong_row - 1 || found.report.first_constraint != 1 || found.report.n_failures != 3)
      throw std::runtime_error("the wrong cell was not located");

    // ---- 2. the bus
    const size_t hs = 16, hr = 8, dropped = 11;
    std::vector<uint32_t> sender(hs * 3), receiver(hr * 3, 0), challenges(2 * dc);
    for (uint32_t k = 0; k < 2 * dc; ++k) challenges[k] = 1000003u * (k + 1) % p;
    for (size_t r = 0; r < hr; ++r) {
      receiver[3 * r] = (uint32_t)r;
      receiver[3 * r + 1] = (uint32_t)(7 * r + 3);
    }
    for (size_t r = 0; r < hs; ++r) {   // tuple (r * 5) mod 8, sent once
      const size_t t = r * 5 % hr;
      sender[3 * r] = receiver[3 * t];
      sender[3 * r + 1] = receiver[3 * t + 1];
      sender[3 * r + 2] = 1;
      receiver[3 * t + 2] = (receiver[3 * t + 2] + p - 1) % p;
    }
    const p3r::AirProgram bus = bus_interaction();
    p3r_dmat* recv = ctx.ptr(p3r_dmat_upload(ctx.raw(), receiver.data(), hr, 3));
    p3r_dmat* send = ctx.ptr(p3r_dmat_upload(ctx.raw(), sender.data(), hs, 3));
    const p3r::LookupCheck balanced = p3r::check_lookups(ctx, {{&bus, {send}, {}}, {&bus, {recv}, {}}}, challenges);
    p3r_dmat_free(ctx.raw(), send);
    if (balanced.n_unbalanced) throw std::runtime_error("the bus does not balance");
    std::cout << "bus ok\n";
    sender[3 * dropped + 2] = 0;   // the send of row 11 is dropped: its tuple is received once more than it is sent
    send = ctx.ptr(p3r_dmat_upload(ctx.raw(), sender.data(), hs, 3));
    const p3r::LookupCheck off = p3r::check_lookups(ctx, {{&bus, {send}, {}}, {&bus, {recv}, {}}}, challenges);
    p3r_dmat_free(ctx.raw(), send);
    p3r_dmat_free(ctx.raw(), recv);
    std::cout << "unbalanced " << off.n_unbalanced << '\n';
    for (const p3r_lookup_imbalance& e : off.unbalanced) {
      std::cout << "key first at instance " << e.instance << " row " << e.row << " term " << e.term << ", " << e.n_records << " records, net";
      for (uint32_t k = 0; k < dc; ++k) std::cout << ' ' << e.net[k];
      std::cout << '\n';
    }
    // the tuple of row 11 is tuple 7, which row 3 sends too: its first record is the sender's row 3; two records are
    // left (one send, the receive of -2), and the net is -1
    if (off.n_unbalanced != 1 || off.unbalanced[0].instance != 0 || off.unbalanced[0].row != dropped - hr || off.unbalanced[0].n_records != 2 ||
        off.unbalanced[0].net[0] != p - 1)
      throw std::runtime_error("the dropped send was not located");
    std::cout << "ok" << std::endl;
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
