"""What tests/air_ref.py lacks for the verifier's side of a constraint program: 1 / (zeta^h - 1) on Python integers, the
three points at which a selector divides by zero, and the programs the host test evaluates.  air_ref.fold_at_point is
the folded value; nothing here calls the library under test."""
import air_ref
import field_ref


def inv_zh(field, dc, zeta, h):
    E = air_ref.ext_of(field, dc)
    return E.inv(E.sub(E.pow([int(v) for v in zeta], h), E.one(0)))


def forbidden_points(field, dc, log_height):
    """name -> zeta: 1, w_h^-1 and a point of the trace domain that is neither (when the domain has one)."""
    p = field_ref.PARAMS[field]["p"]
    w = field_ref.two_adic_generator(field, log_height)
    lift = lambda x: [x % p] + [0] * (dc - 1)
    pts = {"one": lift(1), "w_h_inverse": lift(pow(w, p - 2, p))}
    if log_height >= 2:
        pts["in_trace_domain"] = lift(pow(w, 2, p))
    return pts


def programs(field, dc):
    """name -> (AirBuilder, widths, n_public, n_challenges): a base-field transition with a public boundary value; a
    program over two matrices with LOCAL_EXT / NEXT_EXT, a challenge and all three selectors; one of degree 3 with NEG."""
    import plonky3_recursion_amd as p3r
    out = {}
    b = p3r.AirBuilder(field)
    a0, a1, n0, n1 = b.local(0, 0), b.local(0, 1), b.next(0, 0), b.next(0, 1)
    b.assert_zero(b.is_first_row() * (a0 - b.public(0)))
    b.assert_zero(b.is_transition() * (n0 - a1))
    b.assert_zero(b.is_transition() * (n1 - a0 - a1))
    b.assert_zero(b.is_last_row() * (a1 - b.public(1)))
    out["fibonacci"] = (b, [2], 2, 0)
    b = p3r.AirBuilder(field)
    s, s_next, f = b.local_ext(1, 0), b.next_ext(1, 0), b.local_ext(1, dc)
    d = b.challenge(0) + b.challenge(1) * b.local(0, 1)
    b.assert_zero(f * d - b.local(0, 0))
    b.assert_zero(b.is_first_row() * s)
    b.assert_zero(b.is_transition() * (s_next - s - f))
    b.assert_zero(b.is_last_row() * (s + f - b.challenge(2)))
    b.assert_zero(b.next(0, 2) - b.local(0, 2) * 7 + b.public(0))
    out["logup_ext_all_selectors"] = (b, [3, 2 * dc], 1, 3)
    b = p3r.AirBuilder(field)
    x = b.local(0, 0)
    b.assert_zero(-(x * x * x) + b.next(0, 0) + b.const(5))
    b.assert_zero(b.challenge(0) * x - b.next(0, 1))
    out["cubic_neg"] = (b, [2], 0, 1)
    return out
