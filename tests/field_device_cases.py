"""Run by tests/test_gpu_field_device.py with P3R_LIB_PATH = the knobs build of the library (the only one that exports the
p3r_test_field_op seam of csrc/tu_field_test.hip): every case of tests/field_cases.py through field.h AS THE DEVICE
COMPUTES IT (REDC as one 64-bit multiply-add with a min fix-up, __umulhi, __brev), one case per lane, against the integer
reference of tests/field_ref.py and, where g++ is at hand, word for word against the host build of the same header
(reduce64_lazy excepted: on the host it is the full reduction).  One context per field."""
import ctypes as C
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_cases as FC  # noqa: E402
import plonky3_recursion_amd as p3r  # noqa: E402

u32p = C.POINTER(C.c_uint32)
P3R_EINVAL = -1


def bind(ctx):
    fn = ctx.lib.p3r_test_field_op
    fn.argtypes = [C.c_void_p, C.c_int, u32p, C.c_size_t, u32p, C.c_size_t, C.c_size_t, C.c_uint32]
    fn.restype = C.c_int
    return fn


def device_run(ctx, fn, case):
    n, wi, wo = case.inputs.shape[0], FC.words_in(case.op), FC.words_out(case.op)
    x = np.ascontiguousarray(case.inputs, dtype=np.uint32)
    out = np.zeros((n, wo), dtype=np.uint32)
    ctx.check(fn(ctx.h, case.op.id, x.ctypes.data_as(u32p), wi, out.ctypes.data_as(u32p), wo, n, case.aux))
    return out


host_exe, tmp = None, None
if shutil.which("g++"):
    tmp = tempfile.mkdtemp(prefix="field_host_")
    host_exe = FC.build_host_program(tmp)
else:
    print("field_device: no g++ here, the host build is not compared")

try:
    for field in FC.FIELDS:
        cases = FC.build_cases(field)
        totals = FC.totals(cases)
        assert totals == FC.expected_totals(field), (field, totals)
        assert set(totals) == {o.name for o in FC.ops_of(field)}
        assert max(c.inputs.shape[0] for c in cases) == (59049 if FC.params(field)["quintic"] else FC.N_RANDOM)
        assert any(c.inputs.shape[0] % 256 for c in cases), "a launch that is no multiple of the block"
        ctx = p3r.Context(field=field)
        fn = bind(ctx)
        t0 = time.time()
        results = [device_run(ctx, fn, c) for c in cases]
        t_dev = time.time() - t0
        for case, got in zip(cases, results):
            FC.check(field, case, got)
        pinned = FC.check_inverse_of_zero(field, cases, results)
        for name, n in totals.items():
            print("%s %s %d" % (field, name, n))
        print("%s: %d operations, %d cases in %d launches (%.2f s on the device side) equal the integer reference; "
              "inverse of zero pinned to zero for %s" % (field, len(totals), sum(totals.values()), len(cases), t_dev, ", ".join(pinned)))
        if host_exe:
            host = FC.run_host_program(host_exe, field, cases)
            words = 0
            for case, got, h in zip(cases, results, host):
                if case.op.name == "fp_reduce_lazy":
                    continue
                bad = np.flatnonzero((got != h).any(axis=1))
                assert bad.size == 0, (field, case.op.name, case.label, "host and device differ", case.inputs[bad[0]].tolist(),
                                       got[bad[0]].tolist(), h[bad[0]].tolist())
                words += got.size
            print("%s: host and device results agree word for word (%d words)" % (field, words))
        # refusals: no operation, an operation of another field, another layout
        x, out = np.zeros(16, dtype=np.uint32), np.zeros(16, dtype=np.uint32)
        xp, op_ = x.ctypes.data_as(u32p), out.ctypes.data_as(u32p)
        assert fn(ctx.h, 31, xp, 2, op_, 1, 1, 0) == P3R_EINVAL
        assert fn(ctx.h, FC.OPS["fp_add"].id, xp, 1, op_, 1, 1, 0) == P3R_EINVAL
        assert fn(ctx.h, FC.OPS["fp4_mul"].id, xp, 8, op_, 5, 1, 0) == P3R_EINVAL
        if not FC.params(field)["quintic"]:
            assert fn(ctx.h, FC.OPS["fp5_mul"].id, xp, 10, op_, 5, 1, 0) == P3R_EINVAL
        assert fn(ctx.h, FC.OPS["fp_add"].id, xp, 2, op_, 1, 0, 0) == 0    # no case: nothing to do
        ctx.close()
finally:
    if tmp:
        shutil.rmtree(tmp, ignore_errors=True)
print("field_device ok", "host compared" if host_exe else "host not compared")
