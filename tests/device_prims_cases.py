"""Run by tests/test_gpu_device_prims.py with P3R_LIB_PATH = the knobs build of the library (the only one that exports the
p3r_test_* seam of csrc/device_prims.hip.h): exclusive sums, maximum, the stable radix sort and the three idioms built on
them (select_marked, ranks_of, order_by_level) against numpy."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plonky3_recursion_amd as p3r  # noqa: E402

ctx = p3r.Context(field="koala-bear")
lib, h = ctx.lib, ctx.h
u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
lib.p3r_test_exclusive_sum_u32.argtypes = [C.c_void_p, u32p, u32p, C.c_size_t, C.c_int]
lib.p3r_test_exclusive_sum_u64.argtypes = [C.c_void_p, u64p, u64p, C.c_size_t]
lib.p3r_test_reduce_max.argtypes = [C.c_void_p, u32p, C.c_size_t, u32p]
lib.p3r_test_sort_pairs.argtypes = [C.c_void_p, u32p, u32p, C.c_size_t, C.c_int, u32p, u32p]
for f in (lib.p3r_test_exclusive_sum_u32, lib.p3r_test_exclusive_sum_u64, lib.p3r_test_reduce_max, lib.p3r_test_sort_pairs):
    f.restype = C.c_int


def p32(a):
    return a.ctypes.data_as(u32p)


rng = np.random.default_rng(5)
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 100_003, (1 << 20) + 3, 3_000_001]
checked = 0
for n in SIZES:
    a = rng.integers(0, 1 << 9, size=n, dtype=np.uint32)
    want = (np.cumsum(a, dtype=np.uint64) - a).astype(np.uint32)
    for in_place in (0, 1):
        out = np.empty(n, dtype=np.uint32)
        ctx.check(lib.p3r_test_exclusive_sum_u32(h, p32(a), p32(out), n, in_place))
        assert np.array_equal(out, want), ("exclusive_sum u32", n, in_place)
    # packed pair of counters, as the table ranks use it (a flag in the low word, a cell count in the high one)
    b = rng.integers(0, 2, size=n, dtype=np.uint64) | (rng.integers(0, 125, size=n, dtype=np.uint64) << np.uint64(32))
    out64 = np.empty(n, dtype=np.uint64)
    ctx.check(lib.p3r_test_exclusive_sum_u64(h, b.ctypes.data_as(u64p), out64.ctypes.data_as(u64p), n))
    assert np.array_equal(out64, np.cumsum(b, dtype=np.uint64) - b), ("exclusive_sum u64", n)
    m = np.zeros(1, dtype=np.uint32)
    big = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    ctx.check(lib.p3r_test_reduce_max(h, p32(big), n, p32(m)))
    assert int(m[0]) == int(big.max()), ("reduce_max", n)
    checked += 4
m = np.full(1, 7, dtype=np.uint32)
ctx.check(lib.p3r_test_reduce_max(h, p32(m), 0, p32(m)))
assert int(m[0]) == 0

for n in SIZES:
    for bits in (1, 5, 8, 9, 16, 17, 24, 27, 32):
        if n > 200_000 and bits not in (5, 17, 32):
            continue
        for style in ("uniform", "few", "high_bits"):
            if style == "uniform":
                keys = rng.integers(0, 1 << bits, size=n, dtype=np.uint64).astype(np.uint32)
            elif style == "few":      # long runs of equal digits: stability carries the order
                keys = rng.integers(0, min(1 << bits, 3), size=n, dtype=np.uint64).astype(np.uint32)
            else:                     # bits above `bits` are not part of the order
                keys = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
            vals = np.arange(n, dtype=np.uint32)[::-1].copy()
            ko, vo = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
            keep_k, keep_v = keys.copy(), vals.copy()
            ctx.check(lib.p3r_test_sort_pairs(h, p32(keys), p32(vals), n, bits, p32(ko), p32(vo)))
            mask = np.uint32((1 << bits) - 1) if bits < 32 else np.uint32(0xFFFFFFFF)
            order = np.argsort(keys & mask, kind="stable")
            assert np.array_equal(ko, keys[order]) and np.array_equal(vo, vals[order]), ("sort_pairs", n, bits, style)
            assert np.array_equal(keys, keep_k) and np.array_equal(vals, keep_v)
            checked += 1

# ---- the three idioms of the preparation pass: select_marked, ranks_of, order_by_level
lib.p3r_test_select_marked.argtypes = [C.c_void_p, u32p, C.c_size_t, C.c_int, C.c_int, u32p, u32p, C.POINTER(C.c_size_t)]
lib.p3r_test_ranks_of_u64.argtypes = [C.c_void_p, u64p, u64p, C.c_size_t]
lib.p3r_test_order_by_level.argtypes = [C.c_void_p, u32p, u32p, C.c_size_t, C.c_int, C.c_size_t, u32p, u32p, u32p]
for f in (lib.p3r_test_select_marked, lib.p3r_test_ranks_of_u64, lib.p3r_test_order_by_level):
    f.restype = C.c_int
IDIOM_SIZES = [0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 4097]   # 2048 = kScanTile: the tile offsets first matter
FILL = 0xABABABAB   # what an output holds before the call: a cell that still holds it was not touched
UNSET = 0xFFFFFFFF


def filled(n):
    return np.full(n, FILL, dtype=np.uint32)


for n in IDIOM_SIZES:
    for style in ("none", "all", "random"):
        marks = {"none": np.zeros(n, dtype=np.uint32), "all": np.ones(n, dtype=np.uint32),
                 "random": rng.integers(0, 2, size=n, dtype=np.uint32)}[style]
        want_rank = np.zeros(n + 1, dtype=np.uint32)   # the count at [n]
        want_rank[1:] = np.cumsum(marks, dtype=np.uint32)
        want_list = np.flatnonzero(marks).astype(np.uint32)
        for with_list in (0, 1):
            for blocking in (0, 1):
                rank, lst, count = filled(n + 1), filled(n), C.c_size_t(12345)
                ctx.check(lib.p3r_test_select_marked(h, p32(marks), n, with_list, blocking, p32(rank), p32(lst), C.byref(count)))
                case = ("select_marked", n, style, with_list, blocking)
                if n == 0:   # nothing launched, no buffer touched, count 0
                    assert np.array_equal(rank, filled(1)), case
                else:
                    assert np.array_equal(rank, want_rank), case
                    assert int(rank[n]) == len(want_list), case
                    k = len(want_list) if with_list else 0
                    assert np.array_equal(lst[:k], want_list[:k]) and np.array_equal(lst[k:], filled(n - k)), case
                if blocking:
                    assert count.value == len(want_list), case
                checked += 1

    # packed pair of counters: a flag in the low word, a count below 125 in the high one; the total at [n]
    b = rng.integers(0, 2, size=n, dtype=np.uint64) | (rng.integers(0, 125, size=n, dtype=np.uint64) << np.uint64(32))
    out64 = np.full(n + 1, 0xABABABABABABABAB, dtype=np.uint64)
    ctx.check(lib.p3r_test_ranks_of_u64(h, b.ctypes.data_as(u64p), out64.ctypes.data_as(u64p), n))
    want64 = np.zeros(n + 1, dtype=np.uint64)
    want64[1:] = np.cumsum(b, dtype=np.uint64)
    assert np.array_equal(out64, want64), ("ranks_of u64", n)
    assert int(out64[n]) == int(b.sum(dtype=np.uint64)), ("ranks_of u64 total", n)
    checked += 1

    for lbits in (1, 5, 9):
        for style in ("uniform", "three"):   # three distinct values: stability is what decides the order
            n_keys = 1 << lbits
            if style == "uniform":
                keys = rng.integers(0, n_keys, size=n, dtype=np.uint32)
            else:
                keys = rng.choice(rng.choice(n_keys, size=min(3, n_keys), replace=False), size=n).astype(np.uint32)
            lens = rng.integers(0, 300, size=n, dtype=np.uint32)
            want_order = np.argsort(keys, kind="stable").astype(np.uint32)
            want_first = np.full(n_keys, UNSET, dtype=np.uint32)
            sk = keys[want_order]
            for pos in range(n - 1, -1, -1):
                want_first[sk[pos]] = pos
            ls = lens[want_order]
            want_offs = (np.cumsum(ls, dtype=np.uint64) - ls).astype(np.uint32)
            for with_lens in (0, 1):
                first, order, offs = np.full(n_keys, UNSET, dtype=np.uint32), filled(n), filled(n)
                keep = keys.copy()
                ctx.check(lib.p3r_test_order_by_level(h, p32(keys), p32(lens) if with_lens else None, n, lbits, n_keys, p32(first),
                                                      p32(order), p32(offs)))
                case = ("order_by_level", n, lbits, style, with_lens)
                assert np.array_equal(order, want_order), case
                assert np.array_equal(first, want_first), case
                assert np.array_equal(offs, want_offs if with_lens else filled(n)), case
                assert np.array_equal(keys, keep), case
                checked += 1
ctx.close()
print("device_prims ok", checked)
