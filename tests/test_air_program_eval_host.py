"""CPU: p3r_air_program_eval - the verifier's side of a constraint program - against integer arithmetic
(air_ref.fold_at_point, tests/air_eval_ref.py): programs with base cells, LOCAL_EXT / NEXT_EXT, publics, challenges and all
three selectors; log_height 0, 1 and 4; both fields; challenge degrees 4 and 5.  The three points where a selector or
the vanishing polynomial divides by zero are refused, as are index ranges and non-canonical words."""
import numpy as np
import pytest

import air_eval_ref
import air_ref
import field_ref

P3R_EINVAL, P3R_EUNSUPPORTED = -1, -5
CASES = [("koala-bear", 4), ("koala-bear", 5), ("baby-bear", 4)]


def draw(field, dc, widths, n_public, n_challenges, seed):
    p = field_ref.PARAMS[field]["p"]
    rng = np.random.default_rng(seed)
    w = sum(widths)
    u = lambda *shape: rng.integers(0, p, size=shape, dtype=np.uint32)
    return dict(local=u(w, dc), next=u(w, dc), zeta=u(dc), publics=u(n_public), challenges=u(n_challenges, dc), alpha=u(dc))


def per_matrix(flat, widths):
    out, at = [], 0
    for w in widths:
        out.append(flat[at:at + w])
        at += w
    return out


@pytest.mark.parametrize("field,dc", CASES)
@pytest.mark.parametrize("log_height", [0, 1, 4])
def test_folded_value_and_inverse_vanishing_against_integers(field, dc, log_height):
    import plonky3_recursion_amd as p3r
    cfg, keep = p3r.make_config(field=field, challenge_degree=dc)
    for k, (name, (b, widths, n_pub, n_ch)) in enumerate(sorted(air_eval_ref.programs(field, dc).items())):
        v = draw(field, dc, widths, n_pub, n_ch, 10 * log_height + k)
        folded, inv_zh = p3r.air_program_eval(cfg, b, widths, v["local"], v["next"], log_height, v["zeta"], v["publics"], v["challenges"], v["alpha"])
        want = air_ref.fold_at_point(field, dc, b.program(), per_matrix(v["local"], widths), per_matrix(v["next"], widths), v["zeta"],
                                     1 << log_height, v["publics"], v["challenges"], v["alpha"])
        assert [int(x) for x in folded] == [int(x) for x in want], name
        assert [int(x) for x in inv_zh] == air_eval_ref.inv_zh(field, dc, v["zeta"], 1 << log_height), name


@pytest.mark.parametrize("field,dc", CASES)
def test_division_by_zero_is_refused(field, dc):
    import plonky3_recursion_amd as p3r
    cfg, keep = p3r.make_config(field=field, challenge_degree=dc)
    b, widths, n_pub, n_ch = air_eval_ref.programs(field, dc)["logup_ext_all_selectors"]
    for log_height in (0, 1, 4):
        v = draw(field, dc, widths, n_pub, n_ch, log_height)
        for name, zeta in air_eval_ref.forbidden_points(field, dc, log_height).items():
            with pytest.raises(p3r.P3rError) as e:
                p3r.air_program_eval(cfg, b, widths, v["local"], v["next"], log_height, zeta, v["publics"], v["challenges"], v["alpha"])
            assert e.value.code == P3R_EINVAL and "zeta" in str(e.value), (name, str(e.value))


def test_what_else_is_refused():
    import plonky3_recursion_amd as p3r
    field, dc = "koala-bear", 4
    p = field_ref.PARAMS[field]["p"]
    cfg, keep = p3r.make_config(field=field, challenge_degree=dc)
    b, widths, n_pub, n_ch = air_eval_ref.programs(field, dc)["logup_ext_all_selectors"]
    v = draw(field, dc, widths, n_pub, n_ch, 3)

    def refused(code=P3R_EINVAL, text=None, program=b, ws=widths, log_height=4, use_cfg=cfg, **over):
        a = dict(v, **over)
        with pytest.raises(p3r.P3rError) as e:
            p3r.air_program_eval(use_cfg, program, ws, a["local"], a["next"], log_height, a["zeta"], a["publics"], a["challenges"], a["alpha"])
        assert e.value.code == code and (text is None or text in str(e.value)), str(e.value)

    refused(text="public value 0 of 0", publics=np.zeros(0, dtype=np.uint32))
    refused(text="challenge 2 of 2", challenges=v["challenges"][:2])
    for key in ("local", "next", "zeta", "publics", "challenges", "alpha"):
        bad = v[key].copy()
        bad.reshape(-1)[-1] = p
        refused(text="non-canonical", **{key: bad})
    refused(text="two-adicity", log_height=25)
    # what p3r_air_program_info refuses: a column out of range, an unknown op, no ASSERT_ZERO, a non-canonical constant
    refused(text="of matrix 1", ws=[3, 2 * dc - 1], local=v["local"][:-1], next=v["next"][:-1])
    prog = b.program().copy()
    prog[0, 0] = 21   # LOOKUP: unknown to a constraint program
    refused(text="unknown op", program=prog)
    refused(text="no ASSERT_ZERO", program=prog[:3] * 0 + np.array([[0, 1, 0]] * 3, dtype=np.uint32))
    refused(text="non-canonical constant", program=np.array([[0, p, 0], [20, 0, 0]], dtype=np.uint32))
    zk, keep2 = p3r.make_config(field=field, challenge_degree=dc, zk=1)
    refused(code=P3R_EUNSUPPORTED, use_cfg=zk)
    # more live values than the device interpreter takes: the host keeps all of them
    from plonky3_recursion_amd import _lib
    big = p3r.AirBuilder(field)
    cells = [big.local(0, c) for c in range(_lib.P3R_AIR_MAX_LIVE + 8)]
    acc = cells[0]
    for c in cells[1:]:
        acc = acc + c
    big.assert_zero(acc)
    w = [_lib.P3R_AIR_MAX_LIVE + 8]
    with pytest.raises(p3r.P3rError):
        p3r.air_program_info(cfg, big, w)
    vb = draw(field, dc, w, 0, 0, 9)
    folded, _ = p3r.air_program_eval(cfg, big, w, vb["local"], vb["next"], 2, vb["zeta"], (), (), vb["alpha"])
    assert [int(x) for x in folded] == [int(vb["local"][:, k].astype(np.uint64).sum() % p) for k in range(dc)]
