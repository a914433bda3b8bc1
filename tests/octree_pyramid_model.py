"""A numpy model of k_octree's count-pyramid path (csrc/extract.hip, oct_pyramid), step by step as the
kernel takes them:

* every candidate's root, `(int)(x / hX)` in float32, clamped to [0, nIni) as the kernel clamps it, and
  its descent from the root's box by DivideNode's arithmetic in float32 (`hx = (int)ceil((x1 - x0) / 2)`,
  `x < (float)(x0 + hx)`, and the same in y): the box (d, gx, gy) it lies in at every depth d;
* the count pyramid: candidates per box, depths 0..D;
* the rounds, which read counts only: a node is (box, count, creation sequence); phase 1 splits every
  node that holds several candidates, phase 2 the largest (count, sequence) first until the list holds N;
  both stop on `size >= N or size == prevSize`;
* the fallback: a round that SELECTS a node of depth D with several candidates for splitting ends the
  path (phase 2 counts such a node as one child while it looks for the walk's stop, as the kernel does:
  the stop it finds is then either right or at or past that node).  A level of more than 65535
  candidates (the counters are 16 bit) and D = 0 never enter the path;
* final ownership: each candidate descends from its root through the split boxes to a listed node, and
  a node's pick is its first maximum response in candidate order.

`run(...)` returns (selected candidate indices in list order, path, deepest node split): path 0 for an
empty level, 1 when the pyramid path finished, 2 when the block runs the generic path -- the model then
gives what the same rounds give with no depth limit, which is what the generic path computes.
"""
import numpy as np

import octree_literal as lit

F = np.float32
MAX_DEPTH = 6  # kOctMaxDepth
COUNTER_MAX = 0xFFFF


def pyramid_counters(nIni, D):
    """oct_pyr_counters: 16-bit counters of depths 0..D, depth 0 padded to an even count."""
    return ((nIni + 1) & ~1) + nIni * ((4 ** (D + 1) - 4) // 3)


class Descent:
    """Every candidate's box per depth, computed depth by depth as the kernel's registers hold it."""

    def __init__(self, x, y, minX, maxX, minY, maxY):
        self.x, self.y = np.asarray(x, F), np.asarray(y, F)
        _, self.nIni, self.hX = lit.root_count(minX, maxX, minY, maxY)
        root = (self.x / self.hX).astype(np.int64) if len(self.x) else np.zeros(0, np.int64)
        self.root = np.clip(root, 0, self.nIni - 1)
        self.x0 = (self.hX * self.root.astype(F)).astype(np.int64)
        self.x1 = (self.hX * (self.root + 1).astype(F)).astype(np.int64)
        self.y0 = np.zeros(len(self.x), np.int64)
        self.y1 = np.full(len(self.x), maxY - minY, np.int64)
        self.boxes = [(self.root.copy(), np.zeros(len(self.x), np.int64))]  # [d] -> (gx, gy) per candidate

    def depth(self, d):
        while len(self.boxes) <= d:
            gx, gy = self.boxes[-1]
            hx = np.ceil((self.x1 - self.x0).astype(F) / F(2)).astype(np.int64)
            hy = np.ceil((self.y1 - self.y0).astype(F) / F(2)).astype(np.int64)
            dx = ~(self.x < (self.x0 + hx).astype(F))
            dy = ~(self.y < (self.y0 + hy).astype(F))
            self.x0, self.x1 = np.where(dx, self.x0 + hx, self.x0), np.where(dx, self.x1, self.x0 + hx)
            self.y0, self.y1 = np.where(dy, self.y0 + hy, self.y0), np.where(dy, self.y1, self.y0 + hy)
            self.boxes.append((2 * gx + dx, 2 * gy + dy))
        return self.boxes[d]

    def counts(self, d):
        """{(gx, gy): candidates} of depth d."""
        gx, gy = self.depth(d)
        keys, n = np.unique(np.stack([gx, gy], 1), axis=0, return_counts=True)
        return {(int(a), int(b)): int(c) for (a, b), c in zip(keys, n)}


class FellBack(Exception):
    pass


def rounds(desc, N, D):
    """The node list [(d, gx, gy, count, seq)] in list order and the set of split boxes; D None: no limit.
    Raises FellBack when a round selects a node of depth D that holds several candidates."""
    pyr = {}

    def count(d, gx, gy):
        if d not in pyr:
            pyr[d] = desc.counts(d)
        return pyr[d].get((gx, gy), 0)

    def kids(n):
        d, gx, gy = n[:3]
        return [(d + 1, 2 * gx + (q & 1), 2 * gy + (q >> 1), count(d + 1, 2 * gx + (q & 1), 2 * gy + (q >> 1))) for q in range(4)]

    deep = (lambda n: False) if D is None else (lambda n: n[0] >= D)
    nodes = [(0, i, 0, count(0, i, 0), i) for i in range(desc.nIni) if count(0, i, 0) > 0]
    seq = desc.nIni
    split_boxes = set()
    phase = 1
    while True:
        S = len(nodes)
        if phase == 1:
            chosen = [n for n in nodes if n[3] > 1]
        else:
            order = sorted((n for n in nodes if n[3] > 1), key=lambda n: (n[3], n[4]), reverse=True)
            size, m = S, len(order) - 1
            for j, n in enumerate(order):
                size += (1 if deep(n) else sum(k[3] > 0 for k in kids(n))) - 1
                if size >= N:
                    m = j
                    break
            chosen = order[:m + 1]
        if any(deep(n) for n in chosen):
            raise FellBack()
        created, nexp = [], 0
        for n in chosen:  # in list order (phase 1) or processing order (phase 2): the sequence follows it
            split_boxes.add(n[:3])
            for k in kids(n):
                if k[3] > 0:
                    created.append(k + (seq,))
                    seq += 1
                    nexp += k[3] > 1
        gone = {n[:3] for n in chosen}
        nodes = created[::-1] + [n for n in nodes if n[:3] not in gone]
        if len(nodes) >= N or len(nodes) == S:
            return nodes, split_boxes
        if phase == 1 and len(nodes) + 3 * nexp > N:
            phase = 2


def run(x, y, response, minX, maxX, minY, maxY, N, D):
    """(indices in list order, path, deepest node split or -1)."""
    x, y = np.asarray(x, F), np.asarray(y, F)
    response = np.asarray(response, F)
    if len(x) == 0:
        return np.zeros(0, np.int64), 0, -1
    desc = Descent(x, y, minX, maxX, minY, maxY)
    path = 1
    try:
        if D == 0 or len(x) > COUNTER_MAX:
            raise FellBack()
        nodes, split_boxes = rounds(desc, N, D)
    except FellBack:
        path = 2
        nodes, split_boxes = rounds(desc, N, None)
    # ownership: descend while the box is a split one
    owner = np.full(len(x), -1, np.int64)
    index_of = {n[:3]: i for i, n in enumerate(nodes)}
    deepest = max([b[0] for b in split_boxes], default=-1)
    for d in range(deepest + 2):
        gx, gy = desc.depth(d)
        for k in np.flatnonzero(owner < 0):
            i = index_of.get((d, int(gx[k]), int(gy[k])))
            if i is not None:
                owner[k] = i
    assert (owner >= 0).all()
    index = np.zeros(len(nodes), np.int64)
    for i in range(len(nodes)):
        mine = np.flatnonzero(owner == i)
        index[i] = mine[int(np.argmax(response[mine]))]
    return index, path, deepest
