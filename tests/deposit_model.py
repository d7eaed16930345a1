"""Python restatement of the deposit statement, independent of csrc/: the 24-field row of a deposit at a given index of an
append-only tree (oracle.hashes: Poseidon, Grumpkin; client/merkle.ts:146-222 for the tree) and the rule by which a log of proved
deposits is checked one after another.  Python ints throughout; nothing of the package under test is imported.

  row   = old_root | new_root | commitment | amount | index | owner_x | owner_y | randomness | siblings[depth]
  owner = secret_key * G, commitment = H(owner_x, owner_y, amount, randomness)
  sibling l of slot i in the tree of the first i leaves: with p = i >> l, node (l, p - 1) when p is odd -- a subtree of leaves
  below i, complete -- and the level default when p is even (nothing to the right of slot i exists yet)
  old_root = the path from the empty leaf 0, new_root = the path from the commitment, over those siblings
"""
from oracle import hashes as H

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
DEPTH = 16
ROW_FIELDS = 8 + DEPTH
OK, BAD_AMOUNT, STALE_ROOT, BAD_INDEX, BAD_PROOF = range(5)
NAMES = ["OK", "BAD_AMOUNT", "STALE_ROOT", "BAD_INDEX", "BAD_PROOF"]


def commitment_of(record):
    sk, amount, randomness = record
    owner = H.fixed_base_scalar_mul(sk)
    return owner, H.poseidon_hash4(owner[0], owner[1], amount % R, randomness % R)


def row_from_parts(owner, amount, randomness, index, siblings, commitment=None):
    """the row over given siblings, whatever tree they come from (the circuit does not care)"""
    c = H.poseidon_hash4(owner[0], owner[1], amount % R, randomness % R) if commitment is None else commitment
    old_root = H.compute_merkle_root(0, index, siblings)
    new_root = H.compute_merkle_root(c, index, siblings)
    return [old_root, new_root, c, amount % R, index, owner[0], owner[1], randomness % R] + list(siblings)


class Tree:
    """append-only tree kept level by level; append() recomputes the one path the new leaf touches"""

    def __init__(self, depth=DEPTH):
        self.depth = depth
        self.dflt = H.default_hashes(depth)
        self.levels = [[] for _ in range(depth + 1)]

    @property
    def size(self):
        return len(self.levels[0])

    def root(self):
        return self.levels[self.depth][0] if self.size else self.dflt[self.depth]

    def append(self, leaf):
        i = self.size
        self.levels[0].append(leaf % R)
        for l in range(self.depth):
            p = (i >> l) & ~1
            lv = self.levels[l]
            node = H.poseidon_hash2(lv[p], lv[p + 1] if p + 1 < len(lv) else self.dflt[l])
            up = self.levels[l + 1]
            if (p >> 1) < len(up):
                up[p >> 1] = node
            else:
                up.append(node)
        return i

    def siblings_for_append(self, index):
        """the siblings of slot `index` in the tree of the first `index` leaves; needs index <= size.  Every node read covers
        leaves below `index` only, so later appends do not change the answer"""
        assert index <= self.size and index < (1 << self.depth)
        out = []
        for l in range(self.depth):
            p = index >> l
            out.append(self.levels[l][p - 1] if p & 1 else self.dflt[l])
        return out

    def row(self, record, index):
        owner, c = commitment_of(record)
        return row_from_parts(owner, record[1], record[2], index, self.siblings_for_append(index), c)


def rows_for_deposits(records, leaves_so_far=(), depth=DEPTH):
    """appends leaves_so_far, then the records' commitments one by one; returns (tree, rows of the records)"""
    t = Tree(depth)
    for leaf in leaves_so_far:
        t.append(leaf)
    rows = []
    for rec in records:
        i = t.size
        owner, c = commitment_of(rec)
        sibs = t.siblings_for_append(i)
        old_root = H.compute_merkle_root(0, i, sibs)
        assert old_root == t.root()
        t.append(c)                                  # the path of the new leaf: its top is new_root
        rows.append([old_root, t.root(), c, rec[1] % R, i, owner[0], owner[1], rec[2] % R] + sibs)
    return t, rows


def word(v):
    return int(v).to_bytes(32, "big")


def check_chain(pws, proof_ok, start_root, start_index, lamports=None):
    """pws: public witnesses as bytes (12-byte header, then old_root | new_root | commitment | amount | index); proof_ok[i]: what the
    batch verifier decided for instruction i; start_root: 32 bytes.  Returns (codes, end_root bytes, end_index).  Words are compared
    as bytes; the first failing check in the order amount, root, index, proof names the result; a rejected instruction advances
    nothing."""
    root, count, codes = bytes(start_root), int(start_index), []
    for i, pw in enumerate(pws):
        w = [bytes(pw[12 + 32 * k:44 + 32 * k]) for k in range(5)]
        if lamports is not None and w[3] != word(lamports[i]):
            codes.append(BAD_AMOUNT)
        elif w[0] != root:
            codes.append(STALE_ROOT)
        elif count >= (1 << 64) or w[4] != word(count):
            codes.append(BAD_INDEX)
        elif not proof_ok[i]:
            codes.append(BAD_PROOF)
        else:
            codes.append(OK)
            root, count = w[1], count + 1
    return codes, root, count
