"""Integer reference for the field arithmetic of csrc/field.h: the prime fields, the quartic binomial extension
F[x]/(x^4 - W), KoalaBear's quintic F[x]/(x^5 + x^2 - 1) and the degree-1 'extension'.  It owes nothing to field.h or to
the oracle: base arithmetic is `%`, extension elements are coefficient lists multiplied schoolbook and reduced by the
modulus, inverses are a^(p^D - 2) and Frobenius maps a^(p^K) by square-and-multiply.  Values are canonical residues;
Montgomery form is the callers' business.

Every function takes Python integers.  The same expressions also accept numpy uint64 arrays (one entry per case), which
is how the suites evaluate 2^14 cases of a 155-bit exponentiation in under a second: every intermediate stays below 2^63
(operands < 2^31, at most two products added before a `%`) and no expression goes below zero (a - b is written
a + (p - b)).  tests/test_field_host.py checks the array evaluation against the integer one."""

PARAMS = {
    # name: modulus, W of the quartic extension x^4 = W, multiplicative generator, two-adicity, has the quintic extension
    "koala-bear": dict(p=2**31 - 2**24 + 1, w=3, gen=3, two_adicity=24, quintic=True, field_id=0),
    "baby-bear": dict(p=2**31 - 2**27 + 1, w=11, gen=31, two_adicity=27, quintic=False, field_id=1),
}


# ------------------------------------------------------------------ base field
def add(a, b, p):
    return (a + b) % p


def sub(a, b, p):
    return (a + (p - b)) % p


def neg(a, p):
    return (p - a) % p


def mul(a, b, p):
    return a * b % p


def halve(a, p):
    return a * ((p + 1) // 2) % p


def one_like(a):
    return a - a + 1


def fpow(a, e, p):
    r, b = one_like(a), a
    while e:
        if e & 1:
            r = r * b % p
        b = b * b % p
        e >>= 1
    return r


def inv(a, p):
    """a^(p - 2): zero maps to zero."""
    return fpow(a, p - 2, p)


def two_adic_generator(field, bits):
    f = PARAMS[field]
    assert 0 <= bits <= f["two_adicity"]
    return pow(f["gen"], (f["p"] - 1) >> bits, f["p"])


def bit_reverse(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


# ------------------------------------------------------------------ extensions
class Ext:
    """F[x]/(m): degree 4 with m = x^4 - w, degree 5 with m = x^5 + x^2 - 1, degree 1 (the base field itself).
    Elements are lists of `d` coefficients, constant term first."""

    def __init__(self, p, d, w=None):
        assert (d == 4) == (w is not None) and d in (1, 4, 5)
        self.p, self.d, self.w = p, d, w

    def zero(self, like):
        return [like - like for _ in range(self.d)]

    def one(self, like):
        return [one_like(like)] + [like - like for _ in range(self.d - 1)]

    def add(self, a, b):
        return [add(x, y, self.p) for x, y in zip(a, b)]

    def sub(self, a, b):
        return [sub(x, y, self.p) for x, y in zip(a, b)]

    def neg(self, a):
        return [neg(x, self.p) for x in a]

    def scale(self, a, s):
        return [mul(x, s, self.p) for x in a]

    def halve(self, a):
        return [halve(x, self.p) for x in a]

    def mul(self, a, b):
        p, d = self.p, self.d
        t = [a[0] - a[0] for _ in range(2 * d - 1)]
        for i in range(d):
            for j in range(d):
                t[i + j] = (t[i + j] + a[i] * b[j] % p) % p
        for k in range(2 * d - 2, d - 1, -1):
            if d == 4:      # x^k = w x^(k-4)
                t[k - 4] = (t[k - 4] + self.w * t[k] % p) % p
            else:           # x^5 = 1 - x^2:  x^k = x^(k-5) - x^(k-3)
                t[k - 5] = (t[k - 5] + t[k]) % p
                t[k - 3] = (t[k - 3] + (p - t[k])) % p
        return t[:d]

    def pow(self, a, e):
        r, b = self.one(a[0]), a
        while e:
            if e & 1:
                r = self.mul(r, b)
            b = self.mul(b, b)
            e >>= 1
        return r

    def inv(self, a):
        """a^(p^d - 2): zero maps to zero."""
        return self.pow(a, self.p ** self.d - 2)

    def frobenius(self, a, k):
        return self.pow(a, self.p ** k)

    # --- the quintic's Itoh-Tsujii pieces, from their definitions
    def norm_cofactor(self, a):
        """a^(p + p^2 + p^3 + p^4): a times it is the norm, an element of the base field."""
        assert self.d == 5
        p = self.p
        return self.pow(a, p + p**2 + p**3 + p**4)

    def mul_c0(self, a, b):
        return self.mul(a, b)[0]

    # --- the quartic's norm tower, from automorphisms
    def conj_x(self, a):
        """x -> -x, the automorphism of order two (a^(p^2), checked in tests/test_field_host.py)."""
        assert self.d == 4
        return [a[0], neg(a[1], self.p), a[2], neg(a[3], self.p)]

    def norm_tower(self, a):
        """(n0, n1, d): N = a * a(-x) = n0 + n1 x^2 in the quadratic subfield, d = N * N(-x^2) = n0^2 - w n1^2 in the base
        field, read off the full products."""
        n = self.mul(a, self.conj_x(a))
        nbar = [n[0], n[1], neg(n[2], self.p), n[3]]
        return n[0], n[2], self.mul(n, nbar)[0], n[1], n[3]


def quartic(field):
    f = PARAMS[field]
    return Ext(f["p"], 4, f["w"])


def quintic(field):
    f = PARAMS[field]
    assert f["quintic"]
    return Ext(f["p"], 5)


def linear(field):
    return Ext(PARAMS[field]["p"], 1)
