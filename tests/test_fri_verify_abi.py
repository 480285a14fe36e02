"""CPU: the host challenger (p3r_challenger_create_host) and the presence of the FRI verifier seam's entries.  No GPU is
touched: a handle is made from a p3r_config alone and must replay a transcript word for word as the CPU oracle's
DuplexChallenger does (fri_ref.ScriptChallenger), for both fields and both challenge degrees."""
import ctypes as C

import numpy as np
import pytest

import fri_ref
from fri_verify_ref import P3R_EINVAL, P3R_EUNSUPPORTED

CASES = [("koala-bear", 4), ("koala-bear", 5), ("baby-bear", 4)]


def test_the_new_symbols_exist():
    from plonky3_recursion_amd import _lib
    lib = _lib.load()
    for name in ("p3r_challenger_create_host", "p3r_fri_log_arity_cfg", "p3r_fri_verify_transcript", "p3r_fri_verify"):
        assert name in _lib.SIGNATURES and getattr(lib, name)
    assert _lib.P3R_EVERIFY == -7


@pytest.mark.parametrize("field,dc", CASES)
def test_host_challenger_is_the_oracles_word_for_word(oracle, field, dc):
    import plonky3_recursion_amd as p3r
    cfg, keep = p3r.make_config(field=field, challenge_degree=dc)
    ch = p3r.host_challenger(cfg)
    ref = fri_ref.ScriptChallenger(oracle, field, dc)
    p = p3r.device.MODULUS[field]
    rng = np.random.default_rng(dc)
    # a script that crosses the rate (8) in both directions: short and long absorbs, samples that drain the output
    # buffer, extension samples, bits, and proof-of-work checks that pass and fail
    for step in range(40):
        kind = step % 5
        if kind == 0:
            words = rng.integers(0, p, size=int(rng.integers(1, 20)), dtype=np.uint32)
            words[0] = p - 1
            ch.observe(words)
            ref.observe(words)
        elif kind == 1:
            assert ch.sample() == ref.sample(), step
        elif kind == 2:
            assert np.array_equal(ch.sample_ext(), ref.sample_ext()), step
        elif kind == 3:
            bits = int(rng.integers(1, 20))
            assert ch.sample_bits(bits) == ref.sample_bits(bits), (step, bits)
        else:
            # check_witness(bits, w) is observe(w) then sample_bits(bits) == 0
            bits, w = int(rng.integers(1, 4)), int(rng.integers(0, p))
            ok = ch.check_witness(bits, w)
            ref.observe([w])
            assert ok == (ref.sample_bits(bits) == 0), step
    # bits == 0: accepted, transcript untouched
    assert ch.check_witness(0, 5) and ch.sample() == ref.sample()
    # a clone goes its own way
    twin = ch.clone()
    ch.observe([1])
    ref2 = ref.clone()
    ref.observe([1])
    assert ch.sample() == ref.sample() and twin.sample() == ref2.sample()


def test_grind_on_a_host_handle_is_refused_and_moves_nothing():
    import plonky3_recursion_amd as p3r
    cfg, keep = p3r.make_config(field="baby-bear")
    ch, twin = p3r.host_challenger(cfg), p3r.host_challenger(cfg)
    ch.observe([7, 8, 9])
    twin.observe([7, 8, 9])
    with pytest.raises(p3r.P3rError) as e:
        ch.grind(3)
    assert e.value.code == P3R_EINVAL and "host challenger" in str(e.value)
    with pytest.raises(p3r.P3rError) as e:
        ch.observe([p3r.device.MODULUS["baby-bear"]])   # non-canonical: nothing of the call is observed
    assert e.value.code == P3R_EINVAL
    assert ch.sample() == twin.sample()


def test_bad_configurations_are_refused_with_a_message():
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import _lib
    lib = _lib.load()
    assert not lib.p3r_challenger_create_host(None)
    assert b"cfg is NULL" in lib.p3r_last_error(None)
    cfg, keep = p3r.make_config(field="baby-bear", challenge_degree=5)   # the quintic challenge field is KoalaBear's
    with pytest.raises(p3r.P3rError, match="quintic"):
        p3r.host_challenger(cfg)
    cfg, keep = p3r.make_config()
    cfg.abi_version += 1
    with pytest.raises(p3r.P3rError, match="abi_version"):
        p3r.host_challenger(cfg)
    cfg, keep = p3r.make_config(poseidon2_rc=[1, 2, 3])
    with pytest.raises(p3r.P3rError, match="poseidon2_rc_len"):
        p3r.host_challenger(cfg)
    assert lib.p3r_fri_log_arity_cfg(None, 0, 8, 2, -1) == -1


@pytest.mark.parametrize("schedule", [None, [1, 2, 3, 4, 1, 2]])
def test_log_arity_cfg_is_the_rule(schedule):
    import plonky3_recursion_amd as p3r
    for max_la in (1, 2, 4):
        cfg, keep = p3r.make_config(max_log_arity=max_la, fri_log_arities=schedule)
        for log_cur in range(1, 10):
            for log_final in range(0, log_cur):
                for log_next in range(-1, log_cur + 2):
                    for phase in (0, 3, 5, 6):
                        want = fri_ref.log_arity_rule(schedule or [], phase, max_la, log_cur, log_final, log_next)
                        assert p3r.fri_log_arity(cfg, phase, log_cur, log_final, log_next) == want
