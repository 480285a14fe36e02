"""CPU: the hiding MMCS at the public commit/open seam - p3r_mmcs_open_batch, p3r_tree_salt_elems and
p3r_tree_num_matrices are declared in include/p3r.h, bound in _lib.py with the declared arity, and exported by the built
library (no compute calls: there is no GPU here)."""
import ctypes
import os
import re

import pytest

from test_abi import ROOT, header_symbols

NEW = {"p3r_mmcs_open_batch": 7, "p3r_tree_salt_elems": 1, "p3r_tree_num_matrices": 1}


def declared_arity(name):
    src = open(os.path.join(ROOT, "include/p3r.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, f"{name} is not declared in include/p3r.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", sorted(NEW))
def test_declared_bound_and_exported(name):
    from plonky3_recursion_amd import _lib
    assert name in header_symbols()
    assert declared_arity(name) == NEW[name]
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == NEW[name]
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} declared in include/p3r.h but not exported"


def test_abi_version_is_unchanged():
    """Nothing existing changes meaning for a plain MMCS and no struct changes: callers' literals stay valid."""
    from plonky3_recursion_amd import _lib
    src = open(os.path.join(ROOT, "include/p3r.h")).read()
    assert re.search(r"#define\s+P3R_ABI_VERSION\s+8\b", src) and _lib.P3R_ABI_VERSION == 8


def test_mirror_has_the_batched_opening():
    import plonky3_recursion_amd as p3r
    from plonky3_recursion_amd import device
    for attr in ("open_many", "salt_elems", "num_matrices", "open_batch"):
        assert hasattr(device.MerkleTree, attr)
    assert p3r.mmcs_verify is device.mmcs_verify
