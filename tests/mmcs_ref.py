"""The MMCS Merkle trees on Python and NumPy, from the permutation only.  Test infrastructure.

A plain statement of what `MerkleTreeMmcs` commits to, written from include/p3r.h and the reference's statements of the
tree (the in-circuit verifier recursion/src/pcs/mmcs.rs, the compression rows of circuit/src/ops/mmcs.rs); it shares no
code with the oracle's tree (oracle/hash.hpp) or the library's (csrc/mmcs4.h, csrc/mmcs_impl.hip.h).  The only primitive
is a permutation callable `perm(states[n, width]) -> states[n, width]` on canonical words; a layer is one batched call.

  digest          8 words.
  leaf sponge     overwrite mode: the state starts at zero, each chunk of `rate` cells overwrites state[0 .. len(chunk))
                  and the state is permuted; no padding, an exact multiple of the rate costs no extra permutation; the
                  digest is state[0 .. 8).  Binary tree: width 16, rate 8.  Arity-4 tree: width 32, rate 24.
  height class    the matrices of one height in commit order (tallest first is a STABLE sort); a class's row i is the
                  concatenation of their rows i, and the class has one digest per row.
  compression     truncated permutation: perm(children concatenated, zero chunks above them)[0 .. 8).
  injection       after the level that produces a layer of the class's height: node = compress(node, class digest)
                  (arity 4: compress(node, class digest, 0, 0)).
  binary tree     layer 0 = the digests of the tallest class; layer l + 1 halves layer l; the cap of height c is the
                  layer of 2^c nodes.  Layers below the cap do not depend on the cap, so ONE tree serves every cap.
  arity-4 tree    a level compresses 4 children, or 2 (a bridge) when a class still to be injected is taller than the
                  next quaternary layer; a layer of 2 or 3 nodes is padded to 4 with zero digests; one root.
  opening         for a leaf index: every matrix's row at its own scale (index >> (log_max_height - log_height)) in
                  commit order, then per level the step - 1 siblings in ascending position, the node's own left out.
"""
import numpy as np

DIGEST = 8


def log2_exact(n):
    if n < 1 or n & (n - 1):
        raise ValueError("%d is not a power of two" % n)
    return n.bit_length() - 1


def sponge(perm, width, rate, rows):
    """Digests [n, 8] of rows [n, w] under the overwrite-mode sponge."""
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    state = np.zeros((rows.shape[0], width), dtype=np.uint32)
    for at in range(0, rows.shape[1], rate):
        chunk = rows[:, at:at + rate]
        state[:, :chunk.shape[1]] = chunk
        state = np.asarray(perm(state), dtype=np.uint32).reshape(-1, width)
    return np.ascontiguousarray(state[:, :DIGEST])


def compress(perm, width, children):
    """perm(children[0] | children[1] | .. | 0 ..)[0 .. 8) for every node; children: [n, 8] arrays."""
    state = np.zeros((children[0].shape[0], width), dtype=np.uint32)
    for k, c in enumerate(children):
        state[:, DIGEST * k:DIGEST * (k + 1)] = c
    return np.ascontiguousarray(np.asarray(perm(state), dtype=np.uint32).reshape(-1, width)[:, :DIGEST])


def height_classes(mats):
    """{height: rows of the class [height, total width]}, tallest first; inside a class, commit order."""
    order = sorted(range(len(mats)), key=lambda i: -mats[i].shape[0])   # sorted() is stable
    groups = {}
    for i in order:
        groups.setdefault(mats[i].shape[0], []).append(np.asarray(mats[i], dtype=np.uint32))
    return {h: np.concatenate(v, axis=1) for h, v in groups.items()}


class Level:
    """One level: `step` children per node, taken from layer `layer`, after `bits` index bits; `inject_h`: the height of
    the class folded in after the level (0: none)."""

    def __init__(self, step, bits, inject_h):
        self.step, self.bits, self.inject_h = step, bits, inject_h

    def __repr__(self):
        return "Level(step=%d, bits=%d, inject_h=%d)" % (self.step, self.bits, self.inject_h)


class Tree:
    """`layers[l]`: [n_l, 8] digests (arity 4: at the padded length); `levels[l]` leads from layers[l] to layers[l + 1]."""

    def __init__(self, arity, mats, layers, levels):
        self.arity, self.mats, self.layers, self.levels = arity, mats, layers, levels
        self.log_max_h = log2_exact(max(m.shape[0] for m in mats))

    def n_levels(self, cap_height=0):
        """Levels below a cap of 2^cap_height digests."""
        if self.arity == 4:
            if cap_height:
                raise ValueError("the arity-4 tree has one root")
            return len(self.levels)
        if not 0 <= cap_height <= self.log_max_h:
            raise ValueError("cap_height %d exceeds log2 of the tallest matrix (%d)" % (cap_height, self.log_max_h))
        return self.log_max_h - cap_height

    def cap(self, cap_height=0):
        return self.layers[self.n_levels(cap_height)][:1 << cap_height]

    def proof_len(self, cap_height=0):
        return sum(lv.step - 1 for lv in self.levels[:self.n_levels(cap_height)])

    def sibling_nodes(self, index, cap_height=0):
        """[(level, node)] of the siblings of one opening, in proof order: sibling k is layers[level][node]."""
        out = []
        for l, lv in enumerate(self.levels[:self.n_levels(cap_height)]):
            idx = index >> lv.bits
            pos = idx & (lv.step - 1)
            out += [(l, idx - pos + j) for j in range(lv.step) if j != pos]
        return out

    def open_many(self, indices, cap_height=0):
        """(opened[n, total width], proofs[n, proof_len, 8]) for the leaf indices."""
        idx = np.asarray(indices, dtype=np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >> self.log_max_h):
            raise ValueError("open index out of range")
        rows = [np.asarray(m, dtype=np.uint32)[idx >> (self.log_max_h - log2_exact(m.shape[0]))] for m in self.mats]
        opened = np.concatenate(rows, axis=1)
        sib = []
        for l, lv in enumerate(self.levels[:self.n_levels(cap_height)]):
            at = idx >> lv.bits
            pos = at & (lv.step - 1)
            for slot in range(lv.step - 1):          # ascending position, the node's own left out
                sib.append(self.layers[l][at - pos + slot + (slot >= pos)])
        proofs = np.stack(sib, axis=1) if sib else np.zeros((idx.size, 0, DIGEST), dtype=np.uint32)
        return opened, proofs

    def open(self, index, cap_height=0):
        opened, proofs = self.open_many([index], cap_height)
        return opened[0], proofs[0]


def commit2(perm16, mats):
    """The binary tree down to its root; `Tree.cap(c)` / `open(.., c)` cut it at a cap of 2^c digests.  A class shorter
    than the cap sits above the cut: its rows enter no digest below the cap (mmcs_cases.py states the rule)."""
    classes = height_classes(mats)
    hmax = next(iter(classes))
    log_h = log2_exact(hmax)
    for h in classes:
        log2_exact(h)
    layers = [sponge(perm16, 16, 8, classes[hmax])]
    levels = []
    for l in range(log_h):
        n = hmax >> (l + 1)
        node = compress(perm16, 16, [layers[-1][0::2], layers[-1][1::2]])
        if n in classes:
            node = compress(perm16, 16, [node, sponge(perm16, 16, 8, classes[n])])
        layers.append(node)
        levels.append(Level(2, l, n if n in classes else 0))
    return Tree(2, list(mats), layers, levels)


def next_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def padded4(n):
    """Allocated length of a layer of n logical nodes: a multiple of 4, except the root."""
    return n if n <= 1 else max(4, -(-n // 4) * 4)


def schedule4(heights):
    """[(step, logical nodes of the new layer, its padded length, injected height or 0)] of the arity-4 tree.
    Derivation: the layers above the leaves want to shrink by 4; a class can only be injected into a layer whose
    power-of-two size is its own, so when the tallest class still waiting is taller than the next quaternary layer the
    level shrinks by 2 instead (a bridge) and the class is met on the way."""
    waiting = sorted(set(heights), reverse=True)
    top = next_pow2(waiting[0])
    waiting = [h for h in waiting if next_pow2(h) != top]       # the leaf hash takes the tallest class
    cur = padded4(max(heights))
    out = []
    while cur > 1:
        if cur < 4:
            step = 2
        else:
            step = 2 if waiting and next_pow2(waiting[0]) > next_pow2(cur // 4) else 4
        logical = cur // step
        cur = padded4(logical)
        inject = 0
        if waiting and next_pow2(waiting[0]) == next_pow2(logical):
            inject = waiting.pop(0)
        out.append((step, logical, cur, inject))
    return out


def commit4(perm32, mats):
    """The arity-4 tree (one root)."""
    classes = height_classes(mats)
    hmax = next(iter(classes))
    leaf = np.zeros((padded4(hmax), DIGEST), dtype=np.uint32)
    leaf[:hmax] = sponge(perm32, 32, 24, classes[hmax])
    layers, levels, bits = [leaf], [], 0
    for step, logical, padded, inject in schedule4([m.shape[0] for m in mats]):
        kids = layers[-1][:step * logical].reshape(logical, step, DIGEST)
        node = compress(perm32, 32, [kids[:, k] for k in range(step)])
        if inject:
            if inject != logical:
                raise ValueError("matrix heights must be powers of two")
            node = compress(perm32, 32, [node, sponge(perm32, 32, 24, classes[inject])])
        nxt = np.zeros((padded, DIGEST), dtype=np.uint32)
        nxt[:logical] = node
        layers.append(nxt)
        levels.append(Level(step, bits, inject))
        bits += 2 if step == 4 else 1
    return Tree(4, list(mats), layers, levels)
