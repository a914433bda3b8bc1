"""Scenes for the covisibility table, one per path: every script drives a player `p` that applies each call
to the literal restatement (tests/covis_literal.py) and, in tests/test_covis.py, to the library, comparing
as it goes.  A script asserts on the literal's own results that its input reaches the branch it is about.

A row entry is (point id or -1, octave, flags); flags are covis_literal.STEREO | CLOSE.
"""
import covis_literal as CL

S, C = CL.STEREO, CL.CLOSE


def ent(pids, octave=0, flags=C):
    return [(int(p), octave, flags) for p in pids]


class Fill:
    """Points nobody else observes (nObs 1: counted in nMPs, never redundant)."""

    def __init__(self, start):
        self.next = start

    def __call__(self, n, octave=0, flags=C):
        r = ent(range(self.next, self.next + n), octave, flags)
        self.next += n
        return r


class Pair:
    """Applies every call to the library's class and to the literal and compares the results exactly; after
    every mutating call the whole read-back (rows, nObs, bad) is compared with the literal's state."""

    def __init__(self, dev, lit=None):
        self.dev, self.lit = dev, lit or CL.Table()

    def set_keyframe(self, kf, entries):
        self.lit.set_keyframe(kf, entries)
        self.dev.set_keyframe(kf, [e[0] for e in entries], [e[1] for e in entries], [e[2] for e in entries])
        self.check_state()

    def erase_keyframe(self, kf):
        self.lit.erase_keyframe(kf)
        self.dev.erase_keyframe(kf)
        self.check_state()

    def set_points_bad(self, ids):
        self.lit.set_points_bad(ids)
        self.dev.set_points_bad(ids)
        self.check_state()

    def update_connections(self, kf, th=15):
        want = self.lit.update_connections(kf, th)
        got = self.dev.update_connections(kf, th)
        assert got == want, ("update_connections", kf, got, want)
        return want

    def vote(self, pids):
        want = self.lit.vote(pids)
        wb, counter, kmax, mx = self.dev.vote(pids)
        got = (wb.tolist(), counter, kmax, mx)
        assert got == want, ("vote", got, want)
        return want

    def local_points(self, kfs):
        want = self.lit.local_points(kfs)
        got = self.dev.local_points(kfs)
        assert got == want, ("local_points", kfs, got, want)
        return want

    def cull(self, cands, not_erase, monocular):
        trace = []
        want = self.lit.cull(cands, not_erase, monocular, trace)
        got = self.dev.cull(cands, not_erase, monocular)
        assert got == want, ("cull", got, want, trace)
        self.check_state()
        return want[0], want[1], {t[0]: t[1:] for t in trace}

    def check_state(self):
        rows, pts = self.lit.state()
        live, _, npts = self.dev.size()
        assert live == len(rows)
        assert npts == (max(pts) + 1 if pts else 0)
        for k, (pid, octs, flags) in rows.items():
            g = self.dev.read_keyframe(k)
            assert g[0].tolist() == pid and g[1].tolist() == octs and g[2].tolist() == flags, ("row", k)
        ids = sorted(pts)
        nobs, bad = self.dev.read_points(ids)
        assert nobs.tolist() == [pts[i][0] for i in ids], "nObs"
        assert bad.tolist() == [pts[i][1] for i in ids], "bad"


class LitOnly:
    """Plays a script on the literal alone and logs every call with what the reference's objects hold after
    it: the operations file of tests/test_covis_shim.py."""

    def __init__(self):
        self.lit = CL.Table()
        self.log = []
        self.all_kfs = {}

    def graph(self):
        """Of every keyframe ever seen: weights, the ordered vectors, parent, children, isBad; and the bad points."""
        g = {}
        for k, kf in sorted(self.all_kfs.items()):
            g[k] = dict(weights=[(c.mnId, w) for c, w in CL.by_id(kf.mConnectedKeyFrameWeights)],
                        ordered=[c.mnId for c in kf.mvpOrderedConnectedKeyFrames],
                        ordered_w=list(kf.mvOrderedWeights),
                        parent=-1 if kf.mpParent is None else kf.mpParent.mnId,
                        children=[c.mnId for c in CL.by_id(kf.mspChildrens)], bad=int(kf.mbBad))
        pts = {i: int(p.mbBad) for i, p in sorted(self.lit.points.items())}
        return g, pts

    def set_keyframe(self, kf, entries):
        k = self.lit.set_keyframe(kf, entries)
        self.all_kfs[kf] = k
        self.log.append(("set", kf, list(entries), list(k.mvuRight), list(k.mvDepth)))

    def erase_keyframe(self, kf):
        raise AssertionError("the shim scenes erase keyframes through KeyFrameCulling only")

    def set_points_bad(self, ids):
        self.lit.set_points_bad(ids)
        self.log.append(("bad", list(ids)))

    def update_connections(self, kf, th=15):
        assert th == 15
        r = self.lit.update_connections(kf)
        self.log.append(("update", kf, self.graph()))
        return r

    def cull(self, cands, not_erase, monocular):
        trace = []
        v, bad = self.lit.cull(cands, not_erase, monocular, trace)
        self.log.append(("cull", list(cands), [int(x) for x in not_erase], int(monocular), self.graph()))
        return v, bad, {t[0]: t[1:] for t in trace}

    def check_state(self):
        pass


# ------------------------------------------------------------------ UpdateConnections
def script_update_connections(p):
    f = Fill(5000)
    me = list(range(100, 158))  # keyframe 5: 58 points, two -1 slots, two of its points bad
    p.set_keyframe(5, ent(me[:30]) + [(-1, 0, C)] + ent(me[30:]) + [(-1, 1, S | C)])
    p.set_keyframe(1, ent(me[2:22]) + f(25))                    # 20 shared
    p.set_keyframe(2, ent(me[10:25], 1, S | C) + f(30))         # 15: exactly th
    p.set_keyframe(3, ent(me[0:2]) + ent(me[30:44]) + f(30))    # 14 + the two bad ones
    p.set_keyframe(4, ent(me[40:55]) + f(28))                   # 15: equal to keyframe 2
    p.set_keyframe(6, ent(me[55:58]) + ent([900, 901, 902]) + f(40))   # 3
    p.set_keyframe(7, f(45))                                    # nothing shared with anybody
    p.set_keyframe(8, ent(me[22:42]) + f(25))                   # 20: equal to keyframe 1
    p.set_keyframe(9, ent([900, 901, 902]) + f(40))             # 3 with keyframe 6 only
    p.set_points_bad(me[0:2])
    counter, ordered = p.update_connections(5)
    assert counter == [(1, 20), (2, 15), (3, 14), (4, 15), (6, 3), (8, 20)], counter
    assert ordered == [(8, 20), (1, 20), (4, 15), (2, 15)], ordered  # equal weights: descending id
    # nothing reaches th and keyframes 5 and 9 tie at 3: the smallest id, alone
    counter, ordered = p.update_connections(6)
    assert counter == [(5, 3), (9, 3)] and ordered == [(5, 3)], (counter, ordered)
    assert p.update_connections(7) == ([], [])  # no shared point at all
    # a replaced row, then an erased one
    p.set_keyframe(2, ent(me[10:20], 2, C) + f(35))
    counter, ordered = p.update_connections(5)
    assert (2, 10) in counter and ordered == [(8, 20), (1, 20), (4, 15)], (counter, ordered)
    p.erase_keyframe(8)
    counter, ordered = p.update_connections(5)
    assert ordered == [(1, 20), (4, 15)] and all(k != 8 for k, _ in counter)
    # another threshold: 14 now passes
    _, ordered = p.update_connections(5, th=14)
    assert ordered == [(1, 20), (4, 15), (3, 14)], ordered


# ------------------------------------------------------------------ vote / local points
def script_vote_local(p):
    f = Fill(7000)
    a, b, c = list(range(300, 320)), list(range(320, 340)), list(range(340, 352))
    p.set_keyframe(10, ent(a) + ent(c) + f(20))
    p.set_keyframe(11, ent(b[:12]) + [(-1, 0, C)] + ent(c[:6]) + f(30))
    p.set_keyframe(12, f(5) + ent(c[:3], 1, S | C) + ent(b[12:]) + ent(a[:10]) + f(25))
    p.set_keyframe(13, f(40))
    p.set_points_bad([a[0], b[0]])
    # the frame: 12 points of keyframe 11 (one bad), 11 of keyframe 12 other than those, -1 slots, an unseen id
    frame = b[:12] + [-1] + b[12:] + a[10:13] + [-1, 999999]
    wb, counter, kmax, mx = p.vote(frame)
    assert sum(wb) == 1 and wb[0] == 1
    assert dict(counter)[11] == 11 and dict(counter)[12] == 8 and dict(counter)[10] == 3, counter
    # a tie for pKFmax: eight points of keyframe 11 and eight of keyframe 12
    wb, counter, kmax, mx = p.vote(b[1:9] + b[12:20])
    assert counter == [(11, 8), (12, 8)] and kmax == 11 and mx == 8, (counter, kmax, mx)
    assert p.vote([-1, -1]) == ([0, 0], [], None, 0)
    assert p.vote([]) == ([], [], None, 0)
    # c[0..2] are in keyframes 10, 11 and 12: once each, where first met
    lp = p.local_points([12, 10, 11])
    assert len(lp) == len(set(lp)) and a[0] not in lp and b[0] not in lp
    assert lp.index(c[0]) == 5 and lp.index(c[2]) == 7, lp[:10]
    lp2 = p.local_points([11, 12, 10])
    assert sorted(lp2) == sorted(lp) and lp2 != lp
    assert p.local_points([]) == []
    assert p.local_points([13])[:2] == [p.lit.kfs[13].mvpMapPoints[0].mnId, p.lit.kfs[13].mvpMapPoints[1].mnId]


# ------------------------------------------------------------------ KeyFrameCulling
CULL_ORDER = [0, 3, 4, 5, 6, 7, 8, 16, 9, 10, 11, 12, 13, 14, 15]


def build_cull_table(p):
    """Background keyframes 20, 21, 22 (and 23 for some) observe pools of points; a candidate holding a pool
    point then finds three other observers and nObs = 4.  Every candidate has 40 features."""
    f = Fill(9000)
    P = lambda k: list(range(1000 + 100 * k, 1000 + 100 * k + 40))  # noqa: E731
    pA, pB, pC, pE, pE2, pG, pI, pJ, pL, pM, p0 = (P(k) for k in range(11))
    T = [2300, 2301, 2302]
    D = [2400, 2401, 2402]
    bg = pA[:36] + pB[:37] + pI[:37] + pJ[:36] + pM[:30] + p0
    # 20 sees pC / pG / pL in stereo (nObs 2), so those points pass nObs > 3 with only two other observers
    p.set_keyframe(20, ent(bg) + ent(pC, 0, S | C) + ent(pE, 3) + ent(pE2, 3) + ent(pG, 0, S | C) + ent(pL, 0, S | C))
    p.set_keyframe(21, ent(bg) + ent(pC) + ent(pE, 3) + ent(pE2, 3) + ent(pG) + ent(pL))
    p.set_keyframe(22, ent(bg))
    # the third observer of pC[:37]; of pE at level + 1 (36 points) and level + 2 (the rest); of pE2 at level + 1
    p.set_keyframe(23, ent(pC[:37]) + ent(pE[:36], 3) + ent(pE[36:], 4) + ent(pE2[:37], 3) + ent(D, 0, S | C))
    p.set_keyframe(0, ent(p0))                                  # id 0: redundant but never judged
    p.set_keyframe(3, ent(pA[:36]) + f(4))                      # 36 of 40: exactly 0.9 nMPs, kept
    p.set_keyframe(4, ent(pB[:37]) + f(3))                      # 37 of 40: culled
    p.set_keyframe(5, ent(pC))                                  # 37 with three others, 3 with exactly two
    p.set_keyframe(6, ent(pE, 2))                               # octave rule: 36 at level + 1, 4 at level + 2
    p.set_keyframe(7, ent(pE2[:37], 2) + f(3))                  # 37 at exactly level + 1
    p.set_keyframe(8, [(-1, 0, C)] * 37 + ent(T))               # nMPs = 0 once T is bad (the second call)
    # two stereo observations (nObs 4 > 3) but one other observer: not redundant
    p.set_keyframe(16, ent(D, 0, S | C) + f(37))
    p.set_keyframe(9, ent(pG[:37]) + f(3))                      # cascade 1: culled ...
    p.set_keyframe(10, ent(pG[:37]) + f(3))                     # ... which leaves this one two observers
    # cascade 2: T is seen by 8, 11 (stereo) and 12; culling 11 leaves nObs 2, T goes bad, 12 shrinks to 37
    p.set_keyframe(11, ent(pI[:37]) + ent(T, 0, S | C))
    p.set_keyframe(12, ent(pJ[:36]) + ent(T) + f(1))
    p.set_keyframe(13, ent(pL[:37]) + f(3))                     # not_erase: redundant, stays
    p.set_keyframe(14, ent(pL[:37]) + f(3))                     # needs 13's observations to be redundant
    # the close gate: 30 close redundant + 10 far fillers
    p.set_keyframe(15, ent(pM[:30]) + f(10, 0, 0))
    return dict(T=T, D=D)


def script_cull(p, monocular):
    info = build_cull_table(p)
    ne = [k == 13 for k in CULL_ORDER]
    v, bad, tr = p.cull(CULL_ORDER, ne, monocular)
    V = dict(zip(CULL_ORDER, v))
    assert V[0] == 0 and 0 not in tr                         # id 0 skipped
    assert tr[3] == (40, 36) and V[3] == 0                   # exactly 0.9 nMPs
    assert tr[4] == (40, 37) and V[4] == 1                   # one above
    assert tr[5] == (40, 37) and V[5] == 1                   # exactly 3 others count, exactly 2 do not
    assert tr[6] == (40, 36) and V[6] == 0                   # level + 2 does not count
    assert tr[7] == (40, 37) and V[7] == 1                   # level + 1 does
    assert tr[8] == (3, 0) and V[8] == 0
    assert tr[16] == (40, 0) and V[16] == 0                  # nObs 4 > 3, one other observer
    assert tr[9] == (40, 37) and V[9] == 1
    assert tr[10] == (40, 0) and V[10] == 0                  # cascade 1: nObs still 4, two observers left
    assert tr[11] == (40, 37) and V[11] == 1
    assert set(info["T"]) <= set(bad) and bad == sorted(bad)  # cascade 2: T went bad (with the culled rows' own points)
    assert tr[12] == (37, 36) and V[12] == 1                 # ... and the shrunken nMPs flips the verdict
    assert tr[13] == (40, 37) and V[13] == 2                 # to be erased: observations stay
    assert tr[14] == (40, 37) and V[14] == 1                 # and still count here
    if monocular:
        assert tr[15] == (40, 30) and V[15] == 0
    else:
        assert tr[15] == (30, 30) and V[15] == 1             # only close points count
    # nMPs = 0: keyframe 8 again, its three points now bad
    v, bad, tr = p.cull([8, 13], [False, False], monocular)
    assert tr[8] == (0, 0) and tr[13] == (40, 0) and v == [0, 0] and bad == []  # 14 is gone: two observers
    # the table after culling answers the other queries
    p.update_connections(3)
    p.local_points([3, 12, 8] if 12 in p.lit.kfs else [3, 8])


# ------------------------------------------------------------------ sizes, growth, compaction
def script_sizes(p):
    """Row lengths 0, 1, 63, 64, 65 and one past a workgroup's width; point ids that straddle a bitmap word;
    the point tables and the pool grow, and the pool compacts, in the middle of the scene."""
    base = list(range(20, 20 + 1100))  # ids 20..1119: crosses the words at 32, 64, ...
    p.set_keyframe(1, [])
    p.set_keyframe(2, ent(base[11:12]))             # id 31
    p.set_keyframe(3, ent(base[:63]))
    p.set_keyframe(4, ent(base[:64], 1))
    p.set_keyframe(5, ent(base[:65], 0, S | C))
    p.set_keyframe(6, ent(base, 1))                 # 1100 features
    p.set_keyframe(7, ent(base[30:48]) + ent([70000, 70001]))   # the point tables grow past 65,536
    counter, ordered = p.update_connections(6)
    assert counter == [(2, 1), (3, 63), (4, 64), (5, 65), (7, 18)], counter
    assert p.update_connections(1) == ([], [])
    assert p.update_connections(2)[1] == [(3, 1)]
    v, bad, tr = p.cull([1, 6, 3], [False] * 3, True)
    assert tr[1] == (0, 0) and tr[6][0] == 1100 and tr[6][1] == 63 and tr[3] == (63, 63) and v == [0, 0, 1]
    # 70 rows of 1,000 fresh points each: past the pool's first 65,536 entries
    for k in range(70):
        p.set_keyframe(100 + k, ent(range(100000 + 500 * k, 100000 + 500 * k + 1000)))
    assert len(p.update_connections(135)[0]) == 2
    for k in range(0, 70, 2):   # then more dead than live: compaction
        p.erase_keyframe(100 + k)
    for k in range(1, 40, 2):
        p.erase_keyframe(100 + k)
    counter, ordered = p.update_connections(6)
    assert counter == [(2, 1), (4, 64), (5, 65), (7, 18)], counter
    lp = p.local_points([141, 6, 143])
    assert len(lp) == 1000 + 1100 + 1000
    wb, counter, kmax, mx = p.vote(base[:70] + [70000])
    assert kmax == 6 and mx == 70
    v, bad, tr = p.cull([141, 4], [False, False], True)
    assert tr[4] == (64, 19) and v == [0, 0], (tr, v)  # three others: 18 points with 5, 6, 7 and id 31 with 2, 5, 6


# ------------------------------------------------------------------ the object graph (tests/test_covis_shim.py)
def script_graph(p):
    """A trajectory: keyframe k sees points 20k .. 20k + 99 (every point is seen by five keyframes), with
    UpdateConnections on insertion as ProcessNewKeyFrame does, then once more for all as after a fusion; the
    spanning tree is the chain.  Culling then removes keyframes that have children (their children find new
    parents among the covisibles), turns private points bad, and holds one keyframe by mbNotErase."""
    for k in range(10):
        extra = ent(range(3000 + 10 * k, 3000 + 10 * k + 3), 1, S | C) if k in (3, 6) else []
        p.set_keyframe(k, ent(range(20 * k, 20 * k + 100)) + extra)
        p.update_connections(k)
    for k in range(10):
        p.update_connections(k)
    kfs = dict(p.lit.kfs)  # (the table forgets a culled keyframe; the objects stay)
    assert [kfs[k].mpParent.mnId for k in range(1, 10)] == list(range(0, 9))
    v, bad, tr = p.cull([0, 3, 4, 5, 6, 7], [0, 0, 0, 1, 0, 0], True)
    assert v == [0, 1, 1, 0, 0, 0] and bad == [3030, 3031, 3032]
    assert kfs[4].mpParent is kfs[2] and kfs[5].mpParent is kfs[2]  # the culled keyframes' children moved up
    # three more views of keyframe 7's points make it redundant; mbNotErase holds it, then lets go
    for k in (20, 21, 22):
        p.set_keyframe(k, ent(range(140, 240)))
        p.update_connections(k)
    v, bad, tr = p.cull([7, 8], [1, 0], True)
    assert v[0] == 2 and kfs[7].mbToBeErased and not kfs[7].mbBad and tr[7] == (100, 100)
    v, bad, tr = p.cull([7, 8], [0, 0], True)
    assert v[0] == 1 and kfs[7].mbBad and kfs[8].mpParent is not kfs[7]
