"""A literal restatement of ORBextractor::DistributeOctTree and ExtractorNode::DivideNode (reference
src/ORBextractor.cc:501-815), statement by statement, with a trace of the rounds it took.  It pins
oracle.distribute_octree (oracle/orb_oracle.cpp) and, through tests/test_gpu_octree.py, k_octree, which is
written in a very different structure; this file follows the reference's.

Arithmetic.  Every value the reference holds in a `float` is an np.float32 here, and every operation on
floats rounds to float once, as the compiled reference does:

* `nIni = round(static_cast<float>(maxX-minX)/(maxY-minY))` (:567): a float division, then C round (half
  away from zero).
* `hX = static_cast<float>(maxX-minX)/nIni` (:570): float.
* a root's `UL.x = hX*static_cast<float>(i)`, `UR.x = hX*static_cast<float>(i+1)` (:583-584): float
  products truncated by cv::Point2i's constructor.
* `vpIniNodes[kp.pt.x/hX]` (:598): a float division truncated to the index.
* `halfX = ceil(static_cast<float>(UR.x-UL.x)/2)` (:503-504): float division, ceil, truncation.
* `kp.pt.x<n1.UR.x`, `kp.pt.y<n1.BR.y` (:537-544): the float coordinate against the int boundary
  converted to float, strict.  Coordinates and boundaries are integers below 4096, so every conversion
  is exact.
* the list is a std::list with push_front (:666-696, :743-770): a round's children stand in front of
  everything older, the last created first, and a node that is not split keeps its place.
* `lNodes.size()+nToExpand*3 > N` (:720) switches to the second loop, which sorts the splittable nodes
  ascending and walks them from the back (:733-735), erasing each after its children were pushed, and
  breaks as soon as the list holds N nodes (:781).
* both loops finish on `size >= N || size == prevSize` (:714, :785).  The second condition also ends
  the search while nodes still hold several points: a node whose points all fall in one child is
  replaced by that child and the list does not grow.
* the first maximum response of a node's keys, in candidate order (:796-812).

Two deviations from the reference, which the oracle and the library share:

1. The sort at :733 is over pair<int, ExtractorNode*>: equal sizes are ordered by HEAP ADDRESS there,
   which no restatement can reproduce.  Here equal sizes are ordered by creation sequence (roots 0 ..
   nIni - 1, then every child in the order it is pushed), so among equal sizes the node created last
   is split first.
2. `nIni` clamps to 1.  On a tall image the quotient rounds to 0, hX is infinite and
   `vpIniNodes.resize(0)` is indexed out of bounds (:590, :598).

The root index is NOT clamped here (nor in the reference): `root` in the result is int(x / hX) as
computed, and the scenes assert that it stays below nIni.

distribute() returns a dict: `index` (the selected candidates, in list order), `x`, `y`, `score` of
those, `root` (per candidate), `nIni`, `hX`, `roots_erased`, and `trace`, one entry per round:
  phase      1 (:628-717) or 2 (:723-788)
  before     list size when the round began (prevSize)
  after      list size when it ended
  M          splittable nodes when it began (phase 2: the length of the sorted vector)
  split      nodes it divided
  exit       'N' (size >= N), 'stuck' (size == prevSize), 'phase2' (:720 switched), 'next'
  broke      phase 2 only: the walk broke at :781 with nodes of the sorted vector left over
  distinct_sizes  phase 2 only: how many different sizes the sorted vector held
  stuck_multi  at a 'stuck' exit: nodes of the final list that still hold several points
"""
import numpy as np

F = np.float32


def c_round(v):
    """C round(): half away from zero."""
    v = float(v)
    return int(np.floor(v + 0.5)) if v >= 0 else -int(np.floor(-v + 0.5))


def root_count(minX, maxX, minY, maxY):
    """(nIni as the reference computes it, nIni clamped to 1, hX)."""
    raw = c_round(F(maxX - minX) / F(maxY - minY))
    n = max(raw, 1)
    return raw, n, F(maxX - minX) / F(n)


class Node:
    __slots__ = ("x0", "y0", "x1", "y1", "keys", "seq")

    def __init__(self, x0, y0, x1, y1, keys, seq):
        self.x0, self.y0, self.x1, self.y1, self.keys, self.seq = x0, y0, x1, y1, keys, seq


def child_boxes(x0, y0, x1, y1):
    """n1..n4's (UL.x, UL.y, BR.x, BR.y) of DivideNode (:508-529)."""
    hx = int(np.ceil(F(x1 - x0) / F(2)))
    hy = int(np.ceil(F(y1 - y0) / F(2)))
    return [(x0, y0, x0 + hx, y0 + hy), (x0 + hx, y0, x1, y0 + hy), (x0, y0 + hy, x0 + hx, y1),
            (x0 + hx, y0 + hy, x1, y1)]


def divide(n, x, y):
    """DivideNode: the four children's key arrays (candidate order kept), n1..n4."""
    boxes = child_boxes(n.x0, n.y0, n.x1, n.y1)
    bx, by = F(boxes[0][2]), F(boxes[0][3])  # n1.UR.x, n1.BR.y
    right = ~(x[n.keys] < bx)
    low = ~(y[n.keys] < by)
    q = right.astype(np.int8) + 2 * low.astype(np.int8)
    return [(b, n.keys[q == d]) for d, b in enumerate(boxes)]


def distribute(x, y, response, minX, maxX, minY, maxY, N):
    """x, y relative to (minX, minY), as ComputeKeyPointsOctTree hands them over, in candidate order."""
    x = np.asarray(x, F)
    y = np.asarray(y, F)
    response = np.asarray(response, F)
    nIni_raw, nIni, hX = root_count(minX, maxX, minY, maxY)
    out = dict(nIni_raw=nIni_raw, nIni=nIni, hX=hX, trace=[], roots_erased=0, root=np.zeros(0, np.int64))
    if len(x) == 0:  # the caller's vToDistributeKeys is empty: the reference returns an empty vector
        out.update(index=np.zeros(0, np.int64), x=x, y=y, score=response)
        return out
    root = (x / hX).astype(np.int64)  # :598, truncation, not clamped
    out["root"] = root
    assert root.min() >= 0 and root.max() < nIni, "vpIniNodes indexed out of bounds"
    seq = 0
    nodes = []
    for i in range(nIni):  # :580-591
        nodes.append(Node(int(hX * F(i)), 0, int(hX * F(i + 1)), maxY - minY, np.flatnonzero(root == i), seq))
        seq += 1
    out["roots_erased"] = sum(len(n.keys) == 0 for n in nodes)
    nodes = [n for n in nodes if len(n.keys) > 0]  # :606-617

    def push_children(n, created, expand):
        nonlocal seq
        for box, keys in divide(n, x, y):
            if len(keys) > 0:
                c = Node(box[0], box[1], box[2], box[3], keys, seq)
                seq += 1
                created.append(c)
                if len(keys) > 1:
                    expand.append(c)

    finish = False
    while not finish:  # :628
        prev = len(nodes)
        expand, created, kept = [], [], []
        for n in nodes:  # :642-708, new nodes go to the front and are not visited
            if len(n.keys) == 1:
                kept.append(n)
            else:
                push_children(n, created, expand)
        split = prev - len(kept)
        nodes = created[::-1] + kept
        entry = dict(phase=1, before=prev, after=len(nodes), M=split, split=split, broke=False)
        out["trace"].append(entry)
        if len(nodes) >= N or len(nodes) == prev:  # :714
            finish = True
            entry["exit"] = "N" if len(nodes) >= N else "stuck"
        elif len(nodes) + 3 * len(expand) > N:  # :720
            entry["exit"] = "phase2"
            while not finish:  # :723
                prev = len(nodes)
                prev_expand = sorted(expand, key=lambda n: (len(n.keys), n.seq))  # deviation 1
                expand, created, gone = [], [], set()
                size, broke = prev, False
                for j in range(len(prev_expand) - 1, -1, -1):  # :735
                    n = prev_expand[j]
                    before = len(created)
                    push_children(n, created, expand)
                    gone.add(id(n))
                    size += len(created) - before - 1
                    if size >= N:  # :781
                        broke = j > 0
                        break
                nodes = created[::-1] + [n for n in nodes if id(n) not in gone]
                assert len(nodes) == size
                entry = dict(phase=2, before=prev, after=size, M=len(prev_expand), split=len(gone), broke=broke,
                             distinct_sizes=len({len(n.keys) for n in prev_expand}))
                out["trace"].append(entry)
                if size >= N or size == prev:  # :785
                    finish = True
                    entry["exit"] = "N" if size >= N else "stuck"
                else:
                    entry["exit"] = "next"
        else:
            entry["exit"] = "next"
    last = out["trace"][-1]
    last["stuck_multi"] = sum(len(n.keys) > 1 for n in nodes) if last["exit"] == "stuck" else 0
    index = np.zeros(len(nodes), np.int64)
    for i, n in enumerate(nodes):  # :796-812
        r = response[n.keys]
        index[i] = n.keys[int(np.argmax(r))]  # argmax: the first maximum
    out.update(index=index, x=x[index], y=y[index], score=response[index], final_sizes=[len(n.keys) for n in nodes])
    return out


def leaves(W, H, depth):
    """The node rectangles (x0, y0, x1, y1), relative to the border box of width W and height H, after
    `depth` full splits of every root: where a scene has to put points to fill chosen nodes."""
    _, nIni, hX = root_count(0, W, 0, H)
    boxes = [(int(hX * F(i)), 0, int(hX * F(i + 1)), H) for i in range(nIni)]
    for _ in range(depth):
        boxes = [c for b in boxes for c in child_boxes(*b)]
    return boxes
