"""GPU: the public challenger (p3r_challenger_*) against the CPU oracle's DuplexChallenger, word for word.  Random scripts
of observe / sample / sample_ext / sample_bits / grind run through Context.challenger() and through
oracle_lib.challenger_script; the proof-of-work witness must be the oracle's, which is the smallest.  Only `grind`
launches (k_grind); everything else is host state."""
import ctypes as C

import numpy as np
import pytest

import field_ref
import oracle_lib

pytestmark = pytest.mark.gpu
FIELDS = ["koala-bear", "baby-bear"]
P3R_EINVAL = -1
GRIND_BITS = (1, 4, 8, 12)
OBSERVE, SAMPLE, SAMPLE_EXT, SAMPLE_BITS, GRIND = 0, 1, 2, 3, 4


@pytest.fixture(scope="module")
def ctxs():
    import plonky3_recursion_amd as p3r
    made = {}

    def get(field, dc=4):
        if (field, dc) not in made:
            made[(field, dc)] = p3r.Context(field=field, challenge_degree=dc)
        return made[(field, dc)]
    yield get
    for c in made.values():
        c.close()


def run_library(ch, ops, args):
    out = []
    for op, a in zip(ops, args):
        if op == OBSERVE:
            ch.observe([a])
        elif op == SAMPLE:
            out.append(ch.sample())
        elif op == SAMPLE_EXT:
            out.extend(int(v) for v in ch.sample_ext())
        elif op == SAMPLE_BITS:
            out.append(ch.sample_bits(a))
        else:
            out.append(ch.grind(a))
    return np.array(out, dtype=np.uint32)


def random_script(field, rng, n=300):
    p = field_ref.PARAMS[field]["p"]
    ops, args = [], []
    # a grind with observations pending in the input buffer, and one directly after a sample
    for op, a in [(OBSERVE, 5), (OBSERVE, p - 1), (OBSERVE, 0), (GRIND, 4), (SAMPLE, 0), (GRIND, 8), (SAMPLE_EXT, 0), (GRIND, 1),
                  (OBSERVE, 7), (GRIND, 12)]:
        ops.append(op)
        args.append(a)
    grinds = 0
    while len(ops) < n:
        op = int(rng.choice([OBSERVE, OBSERVE, OBSERVE, SAMPLE, SAMPLE_EXT, SAMPLE_BITS, GRIND]))
        if op == GRIND and grinds >= 12:   # the oracle's search is sequential: a dozen more of them are enough
            op = OBSERVE
        grinds += op == GRIND
        a = {OBSERVE: int(rng.choice([0, p - 1, int(rng.integers(0, p))])), SAMPLE: 0, SAMPLE_EXT: 0,
             SAMPLE_BITS: int(rng.integers(0, 31)), GRIND: int(rng.choice(GRIND_BITS))}[op]
        ops.append(op)
        args.append(a)
    return ops, args


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("seed", [1, 2])
def test_random_scripts_equal_the_oracle(ctxs, oracle, field, seed):
    rng = np.random.default_rng(1000 * seed + len(field))
    ops, args = random_script(field, rng)
    want = oracle.challenger_script(field, ops, args)
    ch = ctxs(field).challenger()
    got = run_library(ch, ops, args)
    ch.free()
    assert got.shape == want.shape and np.array_equal(got, want)


def test_sample_ext_is_dc_consecutive_samples(ctxs):
    ch = ctxs("koala-bear", 5).challenger()
    ch.observe([1, 2, 3])
    twin = ch.clone()
    e = ch.sample_ext()
    assert e.shape == (5,) and [int(v) for v in e] == [twin.sample() for _ in range(5)]
    assert ch.sample() == twin.sample()
    # and the quartic context draws four
    c4 = ctxs("koala-bear").challenger()
    c4.observe([1, 2, 3])
    assert [int(v) for v in c4.sample_ext()] == [int(v) for v in e[:4]]


@pytest.mark.parametrize("field", FIELDS)
def test_a_clone_does_not_move_its_source(ctxs, oracle, field):
    ch = ctxs(field).challenger()
    ch.observe([9, 8, 7])
    first = ch.sample()
    twin = ch.clone()
    twin.observe([1])
    twin.sample_ext()
    twin.grind(4)
    assert first == int(oracle.challenger_script(field, [0, 0, 0, 1], [9, 8, 7, 0])[0])
    assert ch.sample() == int(oracle.challenger_script(field, [0, 0, 0, 1, 1], [9, 8, 7, 0, 0])[-1])


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("bits", [4, 8])
def test_check_witness_follows_the_oracle(ctxs, oracle, field, bits):
    pre_ops, pre_args = [OBSERVE, OBSERVE, SAMPLE], [3, 4, 0]
    out = oracle.challenger_script(field, pre_ops + [GRIND, SAMPLE], pre_args + [bits, 0])
    w, next_sample = int(out[1]), int(out[2])
    ch = ctxs(field).challenger()
    run_library(ch, pre_ops, pre_args)
    base = ch.clone()
    assert ch.grind(bits) == w
    assert ch.sample() == next_sample
    ok = base.clone()
    assert ok.check_witness(bits, w) and ok.sample() == next_sample
    # witness + 1: valid or not is the oracle's to say - observe it and look at the bits it would check
    o = oracle.challenger_script(field, pre_ops + [OBSERVE, SAMPLE_BITS, SAMPLE], pre_args + [w + 1, bits, 0])
    other = base.clone()
    assert other.check_witness(bits, w + 1) == (int(o[1]) == 0)
    assert other.sample() == int(o[2])
    # bits == 0: accepted, witness 0 from the search, the transcript untouched
    z = base.clone()
    assert z.check_witness(0, 12345) and z.grind(0) == 0 and z.sample() == base.clone().sample()


@pytest.mark.parametrize("field", FIELDS)
def test_refusals_leave_the_state_unchanged(ctxs, field):
    import plonky3_recursion_amd as p3r
    ctx, p = ctxs(field), field_ref.PARAMS[field]["p"]
    lib = ctx.lib
    ch = ctx.challenger()
    ch.observe([11, 12])
    twin = ch.clone()

    def refused(fn, what):
        with pytest.raises(p3r.P3rError) as e:
            fn()
        assert e.value.code == P3R_EINVAL, what
        assert str(e.value).split(": ", 1)[1].strip(), "a refusal carries a message: " + what

    refused(lambda: ch.observe([1, p, 2]), "non-canonical word: nothing of the call is observed")
    refused(lambda: ch.observe([0xFFFFFFFF]), "non-canonical word")
    refused(lambda: ch.sample_bits(31), "sample_bits > 30")
    refused(lambda: ch.grind(31), "grind bits > 30")
    refused(lambda: ch.check_witness(31, 0), "check_witness bits > 30")
    refused(lambda: ch.check_witness(4, p), "non-canonical witness")
    out = np.zeros(8, dtype=np.uint32)
    outp = out.ctypes.data_as(C.POINTER(C.c_uint32))
    ok = C.c_int()
    for rc in (lib.p3r_challenger_observe(None, outp, 1), lib.p3r_challenger_sample(None, outp, 1),
               lib.p3r_challenger_sample_ext(None, outp), lib.p3r_challenger_sample_bits(None, 3, outp),
               lib.p3r_challenger_check_witness(None, 3, 0, C.byref(ok)), lib.p3r_challenger_grind(ctx.h, None, 3, outp)):
        assert rc == P3R_EINVAL
    assert lib.p3r_challenger_clone(None) is None and lib.p3r_last_error(None)
    assert lib.p3r_challenger_create(None) is None
    lib.p3r_challenger_free(None)
    assert ch.sample() == twin.sample(), "the sample after the refused calls is the sample of a clone taken before them"
    assert ch.grind(4) == twin.grind(4)
