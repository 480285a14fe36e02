"""GPU: p3r::AirProgram::lookup and p3r::logup_trace of include/p3r.hpp from compiled code (examples/logup_program.cpp),
in the manner of tests/test_gpu_quotient_program_cpp.py: the example builds the two interactions of a bus, a sender and a
receiver of a permutation of its tuples, and prints both permutation traces and table sums; they equal what the Python
layer gets from the same programs built by AirBuilder, the sums cancel, and with one received cell changed the example
exits non-zero."""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_open_points as ref

pytestmark = pytest.mark.gpu
ctxs = ref.ctxs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "logup_program")


def bus_interaction(p3r, field, receive):
    b = p3r.AirBuilder(field)
    d = b.challenge(0) + b.local(0, 0) + b.challenge(1) * b.local(0, 1)
    one = b.const(1)
    b.lookup(b.const(0) - one if receive else one, d)
    b.end_lookup_column()
    return b


def run_example(tmp_path, field, dc, h, sender, receiver, chal):
    case = tmp_path / "case.txt"
    case.write_text(" ".join(str(int(v)) for v in [h] + sender.reshape(-1).tolist() + receiver.reshape(-1).tolist() + chal.reshape(-1).tolist()))
    return subprocess.run([EXE, field, str(dc), str(case)], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("field,dc", ref.CTXS)
def test_cpp_lookup_programs_match_the_python_mirror_and_the_bus_balances(ctxs, tmp_path, field, dc):
    import plonky3_recursion_amd as p3r
    # unconditionally: the binary is not tracked, and the Makefile knows whether the headers or the source are newer
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "logup_program"], check=True)
    ctx, p, E, h = ctxs(field, dc), ref.P(field), ref.ext(field, dc), 32
    rng = np.random.default_rng(1570 + dc)
    sender = rng.integers(0, p, size=(h, 2), dtype=np.uint32)
    receiver = sender[rng.permutation(h)]
    chal = rng.integers(0, p, size=(2, dc), dtype=np.uint32)
    r = run_example(tmp_path, field, dc, h, sender, receiver, chal)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok" and len(lines) == 1 + 2 + 2 * h + 1
    info = ctx.lookup_program_info(bus_interaction(p3r, field, False), [2])
    assert lines[0].split() == ["info"] + [str(info[k]) for k in ("n_terms", "n_columns", "max_constraint_degree", "peak_live")]
    got_sums = [[int(v) for v in l.split()[1:]] for l in lines[1:3]]
    got = np.array([l.split() for l in lines[3:-1]], dtype=np.uint64).astype(np.uint32).reshape(2, h, 2 * dc)
    for t, (trace, receive) in enumerate(((sender, False), (receiver, True))):
        d = ctx.upload(trace)
        aux, total = ctx.logup_device(bus_interaction(p3r, field, receive), [d], challenges=chal)
        want = aux.download()
        for m in (d, aux):
            m.free()
        assert np.array_equal(got[t], want) and want.any() and got_sums[t] == [int(v) for v in total]
    assert any(got_sums[0]) and E.add(got_sums[0], got_sums[1]) == E.zero(0)
    # one received cell changed: the sums no longer cancel, and the example says so
    spoiled = receiver.copy()
    spoiled[3, 0] = (int(spoiled[3, 0]) + 1) % p
    r = run_example(tmp_path, field, dc, h, sender, spoiled, chal)
    assert r.returncode == 1 and "does not balance" in r.stderr
