"""Parity pins at the sizes the metric is quoted on: tests/golden/proof_digests_large.json (tools/gen_proof_digests.py
--large) holds, for layers of 2^14 to 2^20 rows under the reference examples' FRI defaults, the sha256 of the CPU oracle's
preprocessed commitment and proof bytes and one digest per decoded section of the proof.  The GPU side is
tests/test_gpu_large_digests.py, tests/test_gpu_headline.py and tests/test_gpu_bench.py; here, without a GPU: the
fixture's schema, that the generator still emits every pinned workload, that the oracle reproduces the entries small
enough for every run, and that the 2^20-row pin is the digest a device run recorded before the fixture existed."""
import importlib.util
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("gen_proof_digests", os.path.join(ROOT, "tools", "gen_proof_digests.py"))
gpd = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gpd)
PINS = json.load(open(gpd.LARGE_PATH))["cases"]
IDS = [c["name"] for c in gpd.LARGE_CASES]
HEX64 = re.compile(r"^[0-9a-f]{64}$")
KEYS = {"workload", "prep_commit", "proof_bytes", "proof", "sections", "circuit_seam", "oracle_seconds", "threads", "peak_rss_gb"}
SECTIONS = ["commitments.main", "commitments.permutation", "commitments.quotient", "commitments.random", "opened",
            "commit_phase_commits[0]", "final_poly", "commit_pow_witnesses", "query_pow_witness", "query_proofs[0]", "query_proofs"]


def test_the_fixture_holds_exactly_the_large_cases():
    assert list(PINS) == IDS
    assert len(open(gpd.LARGE_PATH, "rb").read()) < 64 << 10    # digests only: no proof bytes


@pytest.mark.parametrize("case", gpd.LARGE_CASES, ids=IDS)
def test_large_entry_schema(case):
    pin = PINS[case["name"]]
    assert set(pin) == KEYS
    for k in ("workload", "prep_commit", "proof"):
        assert HEX64.match(pin[k]), k
    assert isinstance(pin["proof_bytes"], int) and pin["proof_bytes"] > 0
    for k in SECTIONS:
        assert k in pin["sections"], k
    assert all(HEX64.match(v) for v in pin["sections"].values())
    # one commit-phase commitment per FRI round, numbered without gaps
    rounds = [k for k in pin["sections"] if k.startswith("commit_phase_commits[")]
    assert rounds == ["commit_phase_commits[%d]" % i for i in range(len(rounds))]
    assert ("random_opened_values" in pin["sections"]) == bool(case["prm"].get("zk"))
    assert (pin["circuit_seam"] is not None) == case["circuit"]
    assert pin["oracle_seconds"] > 0 and pin["threads"] >= 1 and pin["peak_rss_gb"] > 0


@pytest.mark.parametrize("case", gpd.LARGE_CASES, ids=IDS)
def test_generator_reproduces_the_pinned_workload(case):
    assert gpd.workload_digest(gpd.large_arrays(case)) == PINS[case["name"]]["workload"], \
        "the generator's arrays changed (harness/synth.cpp)"


@pytest.mark.parametrize("case", [c for c in gpd.LARGE_CASES if c["log_h"] <= 14], ids=lambda c: c["name"])
def test_oracle_reproduces_the_small_large_entries(oracle, case):
    """The whole entry - workload, preprocessed commitment, proof, sections, the circuit seam, `verify` - from the
    oracle, for the cases of at most 2^14 rows (seconds).  The taller cases take minutes each: they are re-derived by
    `tools/gen_proof_digests.py --check NAME` (or `--check all`), not in the suite."""
    got = gpd.large_entry(oracle, case)      # runs the oracle's verifier on its own proof as well
    assert gpd.compare_entries(PINS[case["name"]], got) == [], gpd.first_difference(PINS[case["name"]]["sections"], got["sections"])


def test_first_difference_names_the_phase():
    pin = PINS["kb_headline_14"]["sections"]
    assert gpd.first_difference(pin, dict(pin)) is None
    for k in ("commitments.quotient", "final_poly", "query_proofs"):
        other = dict(pin)
        other[k] = "0" * 64
        assert gpd.first_difference(pin, other) == k
    later = dict(pin, **{"commitments.quotient": "0" * 64, "query_proofs": "1" * 64})
    assert gpd.first_difference(pin, later) == "commitments.quotient"     # protocol order, not name order
    short = {k: v for k, v in pin.items() if k != "commit_phase_commits[2]"}
    assert gpd.first_difference(pin, short) == "commit_phase_commits[2]"   # another FRI schedule: a round is missing


def test_headline_pin_is_the_digest_an_earlier_device_run_recorded():
    """BENCH_r06.json keeps the bench's output as text; its line records `proof_sha256` of the device's 2^20-row
    KoalaBear headline proof, from a run made before this fixture existed."""
    text = open(os.path.join(ROOT, "BENCH_r06.json")).read()
    found = set(re.findall(r'proof_sha256\\*"\s*:\s*\\*"([0-9a-f]{64})', text))
    assert len(found) == 1, found
    assert PINS["kb_headline_20"]["proof"] == found.pop()
