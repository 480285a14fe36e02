"""The tree geometries walked by tests/test_mmcs_ref.py (CPU: mmcs_ref against the oracle) and
tests/test_gpu_mmcs_geometry.py (GPU: the device tree against mmcs_ref).  Test infrastructure.

A case is one commit: a name, the MMCS arity, the (height, width) of its matrices in commit order and the cap heights
it is committed under (the tree below a cap does not depend on the cap, so one reference tree serves them all).  The
contents are seeded by the case name; the matrices listed in `edge` hold the word P - 1 everywhere.

THE MATRIX SHORTER THAN THE CAP (height < 2^cap_height).  The reference's verifier (recursion/src/pcs/mmcs.rs
verify_batch_circuit) walks the height classes tallest first over the path levels plus the cap level and takes, per
level, the classes of exactly that height; a class shorter than the cap level is never reached, nothing checks that the
walk consumed every matrix, and the call succeeds.  So the reference ACCEPTS such a batch and its verifier leaves the
opened row of that matrix unconstrained; the native tree builder is not part of the reference, so what it would commit
is unpinned upstream.  The rule pinned here, which is what the oracle, the library and mmcs_ref all do:
  * the commit is accepted; the rows of such a matrix enter no digest of the cap or below it;
  * an opening still carries its row, at its own scale (index >> (log_max_height - log_height)), in commit order;
  * the verifiers (p3r_mmcs_verify, oracle.verify) accept the opening and ignore that row: changing it changes nothing.
A matrix exactly as tall as the cap (height == 2^cap_height) IS committed: it is injected after the last sibling."""
import zlib

import numpy as np

P = {"koala-bear": 0x7F000001, "baby-bear": 0x78000001}
FIELDS = ["koala-bear", "baby-bear"]


class Case:
    def __init__(self, group, name, shapes, caps=(0,), arity=2, edge=()):
        self.group, self.name, self.shapes, self.caps, self.arity, self.edge = group, name, list(shapes), list(caps), arity, edge
        self.hmax = max(s[0] for s in self.shapes)
        self.log_h = self.hmax.bit_length() - 1

    def mats(self, field):
        rng = np.random.default_rng(zlib.crc32(self.name.encode()))
        out = [rng.integers(0, P[field], size=s, dtype=np.uint32) for s in self.shapes]
        for k in self.edge:
            out[k] = np.full(self.shapes[k], P[field] - 1, dtype=np.uint32)
        return out

    def indices(self):
        """Every leaf up to 2^10 rows; above, the first ones, both sides of a 32-digest workgroup and of the middle, the last."""
        h = self.hmax
        if self.log_h <= 10:
            return list(range(h))
        return [0, 1, 31, 32, 33, h // 2 - 1, h // 2, h - 1]

    def short_for(self, cap_height):
        """Indices of the matrices shorter than a cap of 2^cap_height digests."""
        return [k for k, s in enumerate(self.shapes) if s[0] < (1 << cap_height)]

    def __repr__(self):
        return self.name


def _width(log_h):
    return 1 + log_h % 3


def group_a():
    """Height x cap, binary: one matrix at every log_h in 0..12 under every cap_height in 0..log_h."""
    return [Case("a", "a/h%02d" % lh, [(1 << lh, _width(lh))], caps=range(lh + 1), edge=(0,) if lh == 7 else ())
            for lh in range(13)]


def group_b():
    """Injection position, binary.  Tallest log_h in {5, 6, 10, 11}: a second matrix at every shorter height, and one
    tree with a matrix at every height.  For log_h 6 and 11 also under the caps that put the cap level on the injection
    level (cap == log of the second height), one level above it (cap one less) and one below it (cap one more: the
    second matrix is shorter than the cap); the every-height trees of 6 and 11 under every cap."""
    out = []
    for lh in (5, 6, 10, 11):
        for s in range(lh):
            caps = [0]
            if lh in (6, 11):
                caps = sorted({0} | {c for c in (s - 1, s, s + 1) if 0 <= c <= lh})
            out.append(Case("b", "b/h%02d+s%02d" % (lh, s), [(1 << lh, 2), (1 << s, _width(s))], caps=caps,
                            edge=(1,) if (lh, s) == (6, 2) else ()))
        out.append(Case("b", "b/h%02d+all" % lh, [(1 << s, _width(s)) for s in range(lh, -1, -1)],
                        caps=range(lh + 1) if lh in (6, 11) else [0]))
    return out


def group_c():
    """Regime boundary, binary: the layers around the largest one the several-levels-per-launch kernel takes (2^15 nodes).
    Under a 2^16 tree the one-permutation-per-lane kernel writes the 2^15 layer and the 2^14 layer is the first level of
    the following launch: an injection at each."""
    caps = [0, 1]
    return [Case("c", "c/h15", [(1 << 15, 1)], caps=caps),
            Case("c", "c/h16", [(1 << 16, 1)], caps=caps, edge=(0,)),
            Case("c", "c/h17", [(1 << 17, 1)], caps=caps),
            Case("c", "c/h16+s15", [(1 << 16, 1), (1 << 15, 1)], caps=caps),
            Case("c", "c/h16+s14", [(1 << 16, 1), (1 << 14, 1)], caps=caps),
            Case("c", "c/h17+s16+s15+s14", [(1 << 17, 1), (1 << 14, 1), (1 << 16, 1), (1 << 15, 1)], caps=caps)]


JOB_ORDER = [(64, 2), (32, 19), (4, 9), (2, 1), (1, 30)]   # the widest-first job order differs from the class order


def group_d():
    """Leaf rows, binary: total widths 1..25 (every remainder of the rate 8, up to three full blocks and one cell) at one
    row, two rows, one wavefront and two workgroups of rows; the same totals split over several matrices of one class;
    several one-workgroup classes in one launch, in both commit orders."""
    out = []
    for h in (1, 2, 64, 512):
        for w in range(1, 26):
            out.append(Case("d", "d/h%d/w%02d" % (h, w), [(h, w)], edge=(0,) if (h, w) == (64, 9) else ()))
        for split in ((3, 5), (7, 2, 8), (8, 8, 1)):
            out.append(Case("d", "d/h%d/split%s" % (h, "+".join(map(str, split))), [(h, w) for w in split]))
    out.append(Case("d", "d/job_order", JOB_ORDER))
    out.append(Case("d", "d/job_order_shortest_first", JOB_ORDER[::-1]))
    return out


def group_e():
    """Arity 4: one matrix at every log_h in 0..12; for log_h in {5, 6, 9} a second matrix at every shorter height (a
    bridge where that height falls between quaternary layers) and one tree with a matrix at every height."""
    out = [Case("e", "e/h%02d" % lh, [(1 << lh, _width(lh))], arity=4, edge=(0,) if lh == 4 else ()) for lh in range(13)]
    for lh in (5, 6, 9):
        for s in range(lh):
            out.append(Case("e", "e/h%02d+s%02d" % (lh, s), [(1 << lh, 2), (1 << s, _width(s))], arity=4))
        out.append(Case("e", "e/h%02d+all" % lh, [(1 << s, _width(s)) for s in range(lh, -1, -1)], arity=4))
    return out


GROUPS = {"a": group_a(), "b": group_b(), "c": group_c(), "d": group_d(), "e": group_e()}
ALL = [c for g in "abcde" for c in GROUPS[g]]


def perms(oracle, field):
    """(width-16, width-32) permutation callables over the oracle's golden-pinned permutations."""
    return (lambda s: oracle.permute(field, s)), (lambda s: oracle.p2w_permute(field, s))


def reference_tree(oracle, field, case, _cache={}):
    """mmcs_ref's tree of a case, built once per (field, case) and left unchanged."""
    import mmcs_ref
    key = (field, case.name)
    if key not in _cache:
        p16, p32 = perms(oracle, field)
        mats = case.mats(field)
        _cache[key] = mmcs_ref.commit4(p32, mats) if case.arity == 4 else mmcs_ref.commit2(p16, mats)
    return _cache[key]


def walk_device(p3r, oracle, field, cases):
    """Commits every case on the device under each of its caps and compares the cap, every opening of case.indices()
    (p3r_mmcs_open_batch) and three single openings (p3r_mmcs_open) with mmcs_ref's tree.  Returns the mismatches as
    sentences (empty: all equal).  One context at a time; every tree is freed."""
    out = []
    keys = sorted({(c.arity, cap) for c in cases for cap in c.caps})
    for arity, cap_height in keys:
        ctx = p3r.Context(field=field, cap_height=cap_height, mmcs_arity=arity, allow_unpinned_w32_defaults=True)
        try:
            for case in cases:
                if case.arity != arity or cap_height not in case.caps:
                    continue
                ref = reference_tree(oracle, field, case)
                indices = case.indices()
                want_opened, want_proofs = ref.open_many(indices, cap_height)
                cap, tree = ctx.commit(case.mats(field))
                try:
                    bad = np.argwhere((cap != ref.cap(cap_height)).any(axis=1))
                    if bad.size:
                        out.append("%s cap %d: cap entry %d differs (layer %d, node %d)"
                                   % (case.name, cap_height, bad[0, 0], ref.n_levels(cap_height), bad[0, 0]))
                    opened, _, proofs = tree.open_many(indices)
                    diff = first_difference(case, ref, cap_height, indices, opened, proofs, want_opened, want_proofs)
                    if diff:
                        out.append(diff)
                    for k in sorted({0, len(indices) // 2, len(indices) - 1}):
                        one_opened, one_proof = tree.open_batch(indices[k])
                        if not (np.array_equal(one_opened, opened[k]) and np.array_equal(one_proof, proofs[k])):
                            out.append("%s cap %d: the single opening of index %d differs from the batched one"
                                       % (case.name, cap_height, indices[k]))
                finally:
                    tree.free()
        finally:
            ctx.close()
    return out


def first_difference(case, ref, cap_height, indices, opened, proofs, want_opened, want_proofs):
    """None when equal; else a sentence naming the case and the first differing opened row or sibling (its level, the layer it
    was read from and the node)."""
    if opened.shape != want_opened.shape or proofs.shape != want_proofs.shape:
        return "%s cap %d: opening shapes %s %s, expected %s %s" % (case.name, cap_height, opened.shape, proofs.shape,
                                                                  want_opened.shape, want_proofs.shape)
    bad = np.argwhere(opened != want_opened)
    if bad.size:
        i, col = bad[0]
        return "%s cap %d: opened row of index %d differs at word %d" % (case.name, cap_height, indices[i], col)
    bad = np.argwhere((proofs != want_proofs).any(axis=2))
    if bad.size:
        # the lowest level first: a wrong digest there explains everything above it
        i, k = min(map(tuple, bad), key=lambda t: (t[1], t[0]))
        level, node = ref.sibling_nodes(int(indices[i]), cap_height)[k]
        made = "the leaf digests"
        if level:
            inj = ref.levels[level - 1].inject_h
            made = "built by level %d%s" % (level - 1, ", which injects height %d" % inj if inj else "")
        return ("%s cap %d: sibling %d of index %d differs: layer %d (%d nodes; %s), read by level %d, node %d"
                % (case.name, cap_height, k, indices[i], level, ref.layers[level].shape[0], made, level, node))
    return None
