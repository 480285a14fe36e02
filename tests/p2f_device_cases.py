"""Run by tests/test_gpu_p2f_device.py with P3R_LIB_PATH = the knobs build of the library (the only one that exports the
p3r_test_p2f_* seam of csrc/tu_p2f_test.hip): the FP64 Poseidon2 permutations and p2f_store AS THE DEVICE COMPUTES THEM
(v_fract_f64, the register pins, the device compiler's contraction decisions) against integer arithmetic - Python ints
reduce the double states mod P, the oracle's integer permutation permutes the residues.  Edge states put the carried lanes at
their stated maxima (width 16: 2^36 - 1; width 32: p2wf_out_bound), which no product kernel can do."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_lib  # noqa: E402
import plonky3_recursion_amd as p3r  # noqa: E402

u32p, f64p = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
N_RANDOM = 1 << 12          # 64 wavefronts: one permutation per lane, no cross-lane structure
MASKS = {16: (0x0000, 0x00FF, 0xFF00, 0xFFFF), 32: (0x00000000, 0x000000FF, 0xFF000000, 0xFFFFFFFF)}
orc = oracle_lib.Oracle()


def bind(ctx):
    lib = ctx.lib
    lib.p3r_test_p2f_permute.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_int, f64p, C.c_size_t, u32p]
    lib.p3r_test_p2f_store.argtypes = [C.c_void_p, f64p, C.c_size_t, u32p]
    lib.p3r_test_p2f_permute.restype = lib.p3r_test_p2f_store.restype = C.c_int
    return lib


def carried_bound(field, width):
    p = oracle_lib.MODULUS[field]
    return (1 << 36) - 1 if width == 16 else 63 * ((13 * p + 9) // 10)   # p2f_permute's contract; p2wf_out_bound<PP>()


def states_for(rng, field, width, mask):
    """The seven edge patterns of tools/microbench/host_p2f_check.cpp, then N_RANDOM random states: fresh lanes in [0, P],
    carried lanes in [-C, C].  Python ints (an object array)."""
    p, c = oracle_lib.MODULUS[field], carried_bound(field, width)
    carried = [(mask >> i) & 1 for i in range(width)]
    edge = [
        [0] * width,
        [p - 1] * width,
        [p] * width,
        [c if carried[i] else p - 1 for i in range(width)],
        [-c if carried[i] else 0 for i in range(width)],
        [((c if i & 1 else -c) if carried[i] else (p if i & 1 else 0)) for i in range(width)],
        [-c if carried[i] else p for i in range(width)],
    ]
    fresh = rng.integers(0, p + 1, size=(N_RANDOM, width), dtype=np.int64)
    carr = rng.integers(-c, c + 1, size=(N_RANDOM, width), dtype=np.int64)
    rnd = np.where(np.array(carried, dtype=bool)[None, :], carr, fresh)
    return np.concatenate([np.array(edge, dtype=object), rnd.astype(object)], axis=0)


def device_permute(ctx, lib, width, mask, general, v):
    x = np.ascontiguousarray(v.astype(np.float64))
    assert all(int(a) == b for a, b in zip(x.reshape(-1)[:7 * width], v.reshape(-1)[:7 * width]))   # exact doubles
    out = np.empty(x.shape, dtype=np.uint32)
    ctx.check(lib.p3r_test_p2f_permute(ctx.h, width, mask, general, x.ctypes.data_as(f64p), x.shape[0], out.ctypes.data_as(u32p)))
    return out


def check_permute(field, ctx, lib, rng, width, general, w32, label):
    global checked
    p = oracle_lib.MODULUS[field]
    for mask in MASKS[width]:
        v = states_for(rng, field, width, mask)
        residues = (v % p).astype(np.uint32)             # Python-int arithmetic on the object array
        want = orc.permute(field, residues) if width == 16 else orc.p2w_permute(field, residues, w32=w32)
        got = device_permute(ctx, lib, width, mask, general, v)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (field, label, width, hex(mask), "first mismatching states", bad[:8].tolist(),
                               [int(t) for t in v[bad[0]]], got[bad[0]].tolist(), want[bad[0]].tolist())
        checked += 1


def store_cases(rng, p):
    xs = [0, 1, -1, p - 1, -(p - 1), p, -p]
    for k in (2, 3, 127, 255, 256, 511, 512):
        xs += [k * p, -k * p, k * p + 1, k * p - 1, -k * p + 1, -k * p - 1]
    h = (p - 1) // 2
    for d in (-1, 0, 1, 2):
        xs += [h + d, -(h + d)]
    xs += [(1 << 40) - 1, -((1 << 40) - 1)]
    xs += [int(t) for t in rng.integers(-(1 << 40) + 1, 1 << 40, size=N_RANDOM, dtype=np.int64)]
    return xs


checked = 0
for field in ("koala-bear", "baby-bear"):
    p = oracle_lib.MODULUS[field]
    rng = np.random.default_rng(20 + oracle_lib.FIELD_IDS[field])
    rc_w32, diag_builtin = oracle_lib.default_w32(field)

    # the library's own constants: width 16, width 32 with the built-in diagonal's forms and with the same diagonal as data
    ctx = p3r.Context(field=field, allow_unpinned_w32_defaults=True)
    lib = bind(ctx)
    check_permute(field, ctx, lib, rng, 16, 0, None, "width 16")
    check_permute(field, ctx, lib, rng, 32, 0, (rc_w32, diag_builtin), "builtin")
    check_permute(field, ctx, lib, rng, 32, 1, (rc_w32, diag_builtin), "general(builtin)")
    # only the masks the kernels instantiate, only the two widths
    x = np.zeros((1, 32), dtype=np.float64)
    out = np.zeros((1, 32), dtype=np.uint32)
    for width, mask, general in ((16, 0x0F0F, 0), (32, 0x0000FF00, 0), (32, 0x0000FF00, 1), (8, 0, 0), (16, 0, 1)):
        assert lib.p3r_test_p2f_permute(ctx.h, width, mask, general, x.ctypes.data_as(f64p), 1, out.ctypes.data_as(u32p)) != 0, (width, mask, general)

    # p2f_store alone
    xs = store_cases(rng, p)
    xd = np.array(xs, dtype=np.float64)
    assert all(int(a) == b for a, b in zip(xd, xs))
    got = np.empty(len(xs), dtype=np.uint32)
    ctx.check(lib.p3r_test_p2f_store(ctx.h, xd.ctypes.data_as(f64p), len(xs), got.ctypes.data_as(u32p)))
    want = [t % p for t in xs]
    bad = [i for i in range(len(xs)) if int(got[i]) != want[i]]
    assert not bad, (field, "p2f_store", [(xs[i], int(got[i]), want[i]) for i in bad[:8]])
    checked += 1
    ctx.close()

    # a general diagonal: random entries, random round constants
    rc2 = rng.integers(0, p, size=rc_w32.shape, dtype=np.uint32)
    diag2 = rng.integers(0, p, size=32, dtype=np.uint32)
    ctx = p3r.Context(field=field, poseidon2_w32_rc=rc2, poseidon2_w32_diag=diag2)
    lib = bind(ctx)
    check_permute(field, ctx, lib, rng, 32, 1, (rc2, diag2), "general(random)")
    # the BUILTIN instance has another diagonal compiled in than this context's
    assert lib.p3r_test_p2f_permute(ctx.h, 32, 0, 0, x.ctypes.data_as(f64p), 1, out.ctypes.data_as(u32p)) != 0
    ctx.close()

    # the adversarial diagonal: every entry (P-1)/2, the largest centred magnitude (if the library accepts it)
    diag3 = np.full(32, (p - 1) // 2, dtype=np.uint32)
    try:
        ctx = p3r.Context(field=field, poseidon2_w32_rc=rc2, poseidon2_w32_diag=diag3)
    except p3r.P3rError as e:
        print("(P-1)/2 diagonal refused by p3r_create:", e)
    else:
        lib = bind(ctx)
        check_permute(field, ctx, lib, rng, 32, 1, (rc2, diag3), "general((P-1)/2)")
        ctx.close()
print("p2f_device ok", checked)
