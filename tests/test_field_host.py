"""CPU: the field arithmetic of csrc/field.h as the HOST build computes it (the lo/hi/borrow branch of reduce64 that the
native verifier and the host transcript run), one operation at a time through csrc/field_test_ops.h, against the integer
reference of tests/field_ref.py at the edge operands and 2^14 random cases per operation of tests/field_cases.py.  Also
the reference's own checks: it is consistent with itself on random elements, and its array evaluation is its integer
evaluation.  tests/test_gpu_field_device.py runs the same cases through the device build."""
import random

import numpy as np
import pytest

import field_cases as FC
import field_ref as R


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = FC.build_host_program(tmp_path_factory.mktemp("field_host"))
    made = {}

    def get(field):
        if field not in made:
            cases = FC.build_cases(field)
            made[field] = (cases, FC.run_host_program(exe, field, cases), [FC.reference_words(field, c) for c in cases])
        return made[field]
    get.exe = exe
    return get


# ------------------------------------------------------------------ the reference against itself
def _random_elements(rng, E, n):
    return [[rng.randrange(E.p) for _ in range(E.d)] for _ in range(n)]


@pytest.mark.parametrize("field", FC.FIELDS)
def test_reference_is_consistent_with_itself(field):
    rng = random.Random(7)
    exts = [R.linear(field), R.quartic(field)] + ([R.quintic(field)] if R.PARAMS[field]["quintic"] else [])
    for E in exts:
        one = E.one(0)
        for a, b in zip(_random_elements(rng, E, 12), _random_elements(rng, E, 12)):
            assert any(b)
            binv = E.inv(b)
            assert E.mul(b, binv) == one                       # every nonzero element tried has an inverse
            assert E.mul(E.mul(a, b), binv) == a
            assert E.frobenius(E.mul(a, b), 1) == E.mul(E.frobenius(a, 1), E.frobenius(b, 1))
            assert E.frobenius(a, E.d) == a
            if E.d == 5:
                n = E.mul(a, E.norm_cofactor(a))
                assert not any(n[1:]), "a * norm_cofactor(a) lies in the base field"
                assert E.mul_c0(a, E.norm_cofactor(a)) == n[0]
                assert E.frobenius(E.frobenius(a, 1), 1) == E.frobenius(a, 2)
            if E.d == 4:
                n0, n1, d, odd0, odd1 = E.norm_tower(a)
                assert E.conj_x(a) == E.frobenius(a, 2)         # x -> -x is the Frobenius map squared
                assert odd0 == 0 and odd1 == 0                  # a * a(-x) lies in the quadratic subfield
                assert [d, 0, 0, 0] == E.pow(a, 1 + E.p + E.p**2 + E.p**3)   # d is the norm down to the base field
        # the sparse elements of the case set are invertible too
        for a in ([1] + [0] * (E.d - 1), [0] * (E.d - 1) + [E.p - 1]):
            assert E.mul(a, E.inv(a)) == one
        assert E.inv([0] * E.d) == [0] * E.d
    p = R.PARAMS[field]["p"]
    for bits in range(R.PARAMS[field]["two_adicity"] + 1):
        g = R.two_adic_generator(field, bits)
        assert pow(g, 1 << bits, p) == 1 and (bits == 0 or pow(g, 1 << (bits - 1), p) == p - 1)
    assert [R.bit_reverse(x, 3) for x in range(8)] == [0, 4, 2, 6, 1, 5, 3, 7] and R.bit_reverse(0, 0) == 0


@pytest.mark.parametrize("field", FC.FIELDS)
def test_array_evaluation_is_the_integer_evaluation(host, field):
    """The suites evaluate the reference on uint64 arrays; on the first and last rows and a stride of every launch that
    is what Python integers give (fewer rows where one case is a 155-bit exponentiation)."""
    cases, _, wants = host(field)
    for case, want in zip(cases, wants):
        n = case.inputs.shape[0]
        heavy = case.op.name.endswith(("_inv", "_pow", "_inv_given", "frobenius1", "frobenius2", "norm_cofactor"))
        rows = sorted(set(range(0, n, max(1, n // (3 if heavy else 40)))) | {n - 1})
        assert np.array_equal(want[rows], FC.reference_words_integers(field, case, rows)), (field, case.op.name, case.label)


# ------------------------------------------------------------------ the host build
@pytest.mark.parametrize("field", FC.FIELDS)
def test_host_field_operations_against_integers(host, field):
    cases, results, wants = host(field)
    got_totals = FC.totals(cases)
    for name, n in got_totals.items():
        print("%s %s %d" % (field, name, n))
    assert got_totals == FC.expected_totals(field)
    assert set(got_totals) == {o.name for o in FC.ops_of(field)}, "an operation of the table has no case"
    for case, got, want in zip(cases, results, wants):
        FC.check(field, case, got, want)


@pytest.mark.parametrize("field", FC.FIELDS)
def test_host_inverse_of_zero_is_pinned_to_zero(host, field):
    cases, results, _ = host(field)
    want = ["fp1_inv", "fp4_inv", "fp_inv"] + (["fp5_inv"] if R.PARAMS[field]["quintic"] else [])
    assert FC.check_inverse_of_zero(field, cases, results) == sorted(want)


def test_host_program_refuses_what_is_no_operation(host):
    quintic = FC.Case(FC.OPS["fp5_mul"], "refused", 0, np.zeros((1, 10), dtype=np.uint32))
    wrong_shape = FC.Case(FC.OPS["fp_add"]._replace(ins=["f"]), "refused", 0, np.zeros((1, 1), dtype=np.uint32))
    unknown = FC.Case(FC.OPS["fp_add"]._replace(id=31), "refused", 0, np.zeros((1, 2), dtype=np.uint32))
    for bad in (quintic, wrong_shape, unknown):
        with pytest.raises(AssertionError):
            FC.run_host_program(host.exe, "baby-bear", [bad])
