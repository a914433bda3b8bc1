"""Inputs shared by tests/test_kfdb.py and tests/test_kfdb_shim.py: a keyframe "trajectory" over a
synthetic vocabulary, and a script runner that plays one list of operations on the library's
KeyFrameDatabase and on the literal restatement (tests/kfdb_literal.py) alike.

`transform` is any callable list-of-descriptor-arrays -> list of (words, values, ...): the GPU
tests pass ORBVocabulary.transform_sets, the CPU checks of the scenes pass the oracle's transform
(bit-identical, tests/test_voc.py), so a scene's properties are asserted without a GPU.
"""
import numpy as np

from orb_slam2_commit_amd import synth

N_KF = 200
LOOP_FROM, LOOP_SHIFT = 150, 130  # keyframes 150.. revisit the places of keyframes 20..


def small_voc():
    """k = 10, L = 3: about 1,000 words."""
    return synth.vocabulary(seed=23, k=10, L=3, p_short=0.0, p_stop=0.02)


def place_descriptors(rng, vd, leaves, place, n=150, width=60, step=4, noise_bits=6):
    """n descriptors near the vocabulary leaves leaves[place*step : place*step + width]: keyframes
    at neighbouring places share most of their words."""
    pick = leaves[place * step + rng.integers(0, width, n)]
    bits = np.unpackbits(vd[pick], axis=1)
    for r in range(n):
        bits[r, rng.choice(256, noise_bits, replace=False)] ^= 1
    return np.packbits(bits, axis=1)


def place_of(i):
    return i if i < LOOP_FROM else i - LOOP_SHIFT


def neighbours_by_index(i, ids):
    """The 10 nearest in index, nearest first."""
    out = []
    for d in range(1, 11):
        for j in (i - d, i + d):
            if 0 <= j < len(ids) and len(out) < 10:
                out.append(ids[j])
    return out


def trajectory(transform, seed=7, query_places=(52, 55, 49)):
    """200 keyframes along a path that closes a loop, their neighbour lists, and query frames."""
    text, vd, leaf = small_voc()
    leaves = np.flatnonzero(leaf)
    rng = np.random.default_rng(seed)
    desc = [place_descriptors(rng, vd, leaves, place_of(i)) for i in range(N_KF)]
    qdesc = [place_descriptors(rng, vd, leaves, p) for p in query_places]
    out = transform(desc + qdesc)
    bows = [(np.asarray(t[0], np.uint32), np.asarray(t[1], np.float64)) for t in out]
    ids = list(range(N_KF))
    return dict(text=text, ids=ids, bows=bows[:N_KF], queries=bows[N_KF:], qdesc=qdesc,
                neigh={i: neighbours_by_index(i, ids) for i in ids})


class Pair:
    """The library's database and the restatement, driven together."""

    def __init__(self, db, lit):
        self.db, self.lit = db, lit

    def add(self, i, bow):
        self.db.add(i, bow)
        self.lit.add(i, bow)

    def erase(self, i):
        self.db.erase(i)
        self.lit.erase(i)

    def set_neighbours(self, neigh):
        self.db.set_neighbours(neigh)
        for k, v in neigh.items():
            self.lit.set_neighbours(k, v)

    def reloc(self, fid, bow):
        got = self.db.DetectRelocalizationCandidates(fid, bow)
        want = self.lit.DetectRelocalizationCandidates(fid, bow)
        assert got == want, (fid, got, want)
        return want

    def loop(self, kid, bow, connected, min_score):
        got = self.db.DetectLoopCandidates(kid, bow, connected, min_score)
        want = self.lit.DetectLoopCandidates(kid, bow, connected, min_score)
        assert got == want, (kid, got, want)
        return want

    def check_scores(self, bow, ids=None):
        ids = sorted(self.lit.live) if ids is None else list(ids)
        got = self.db.score(bow, ids)
        want = np.array([self.lit.score(bow, i) for i in ids], np.float64)
        np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
        return want

    def check_state(self):
        """All six members of every id ever seen, floats by bit pattern."""
        ids = sorted(self.lit.kfs)
        if not ids:
            return
        got = self.db.read_state(ids)
        want = [self.lit.kfs[i].state() for i in ids]
        for c, (name, dt) in enumerate([("mnRelocQuery", np.uint64), ("mnRelocWords", np.int32),
                                        ("mRelocScore", np.float32), ("mnLoopQuery", np.uint64),
                                        ("mnLoopWords", np.int32), ("mLoopScore", np.float32)]):
            w = np.array([x[c] for x in want], dt)
            g = got[name]
            if dt == np.float32:
                w, g = w.view(np.uint32), g.view(np.uint32)
            bad = np.flatnonzero(w != g)
            assert len(bad) == 0, (name, [(ids[b], g[b], w[b]) for b in bad[:5]])


class LitOnly(Pair):
    """The restatement alone, logging every operation with its expected result: the CPU checks of
    the scenes use it as is, the shim test replays the log through the C++ driver."""

    def __init__(self, lit):
        self.db, self.lit, self.log = None, lit, []

    def add(self, i, bow):
        self.lit.add(i, bow)
        self.log.append(("add", i, bow))

    def erase(self, i):
        self.lit.erase(i)
        self.log.append(("erase", i))

    def set_neighbours(self, neigh):
        for k, v in neigh.items():
            self.lit.set_neighbours(k, v)
        self.log.append(("neigh", dict(neigh)))

    def reloc(self, fid, bow):
        want = self.lit.DetectRelocalizationCandidates(fid, bow)
        self.log.append(("reloc", fid, bow, want))
        return want

    def loop(self, kid, bow, connected, min_score):
        want = self.lit.DetectLoopCandidates(kid, bow, connected, min_score)
        self.log.append(("loop", kid, bow, list(connected), float(np.float32(min_score)), want))
        return want

    def check_scores(self, bow, ids=None):
        ids = sorted(self.lit.live) if ids is None else list(ids)
        want = np.array([self.lit.score(bow, i) for i in ids], np.float64)
        self.log.append(("score", bow, ids, want))
        return want

    def check_state(self):
        ids = sorted(self.lit.kfs)
        self.log.append(("state", ids, [self.lit.kfs[i].state() for i in ids]))


# ------------------------------------------------------------------------------------- scripts
def script_reloc(p, sc):
    """Three relocalization queries in a row on the trajectory (frame ids 7, 8, 9)."""
    for i in sc["ids"]:
        p.add(i, sc["bows"][i])
    p.set_neighbours(sc["neigh"])
    C = p.lit.counters
    for q, fid in enumerate((7, 8, 9)):
        before = dict(C)
        cand = p.reloc(fid, sc["queries"][q])
        assert len(cand) >= 2
        p.check_state()
        p.check_scores(sc["queries"][q])
        if q == 0:
            first = {k: C[k] - before.get(k, 0) for k in C}
    # queries 2 and 3 added scores left by an earlier query, one even became pBestKF's score; and
    # several entries named a pBestKF that was already listed
    assert C["reloc_stale_score_accumulated"] > first.get("reloc_stale_score_accumulated", 0)
    assert C["reloc_stale_best"] > first.get("reloc_stale_best", 0)
    assert C["reloc_dedup_dropped"] > 0 and C["reloc_not_scored"] > 0 and C["reloc_below_retain"] > 0


ORDER_GROUP = (1050, 1041, 1020, 1035)  # added in this order; identical BowVectors


def script_order(p, sc):
    """Ids added in a non-monotonic order, one erased from the middle, one erased and added again:
    among keyframes whose first common word with the query is the same, the add sequence decides."""
    q = sc["queries"][0]
    order = [int(x) for x in np.random.default_rng(5).permutation(40) + 30]  # trajectory keyframes 30..69
    half = len(order) // 2
    for i in order[:half]:
        p.add(i, sc["bows"][i])
    for g in ORDER_GROUP:  # four copies of the query's own vector: the best score, all retained
        p.add(g, q)
    for i in order[half:]:
        p.add(i, sc["bows"][i])
    p.erase(1020)            # from the middle of the group
    p.erase(order[3])
    p.erase(1050)            # the first of the group goes to the back
    p.add(1050, q)
    cand = p.reloc(3, q)
    p.check_state()
    # no neighbour lists: every scored keyframe stands for itself.  The three survivors share every
    # word with the query, so their first common word is the same (the query's first word); they come
    # out in add order 1041, 1035, 1050 -- neither id order nor the order they were first added in
    grp = [c for c in cand if c in ORDER_GROUP]
    assert grp == [1041, 1035, 1050], cand
    firsts = {c: min(set(map(int, p.lit.kfs[c].mBowVec[0])) & set(map(int, q[0]))) for c in cand}
    assert len({firsts[c] for c in grp}) == 1
    assert grp != sorted(grp) and grp != [g for g in ORDER_GROUP if g in grp]
    return cand


LOOP_KF = 185
LOOP_CONNECTED = [181, 182, 183, 184, 186, 187, 188, 189, 190, 52, 53, 54, 55, 56, 57]


def script_loop(p, sc):
    """DetectLoopCandidates for keyframe 185 (not yet in the database, as LoopClosing calls it) with
    15 connected keyframes and minScore as DetectLoop computes it; then a query nothing can pass."""
    for i in sc["ids"]:
        if i != LOOP_KF:
            p.add(i, sc["bows"][i])
    p.set_neighbours(sc["neigh"])
    qb = sc["bows"][LOOP_KF]
    lit, C = p.lit, p.lit.counters
    assert len(LOOP_CONNECTED) == 15
    min_score = float(np.float32(min(p.check_scores(qb, LOOP_CONNECTED))))
    pre = {i: lit.kfs[i].state() for i in LOOP_CONNECTED}
    cand = p.loop(LOOP_KF, qb, LOOP_CONNECTED, min_score)
    p.check_state()
    assert cand and not set(cand) & set(LOOP_CONNECTED)
    shared = [i for i in LOOP_CONNECTED if set(map(int, lit.kfs[i].mBowVec[0])) & set(map(int, qb[0]))]
    assert len(shared) >= 10
    for i in shared:  # one word, query id untouched
        assert lit.kfs[i].mnLoopWords == 1 and lit.kfs[i].mnLoopQuery == pre[i][3] == 0
    assert C["loop_connected_reset"] > 0 and C["loop_below_min_score"] > 0 and C["loop_not_scored"] > 0
    n_below = C["loop_below_min_score"]
    assert p.loop(LOOP_KF + 1000, qb, LOOP_CONNECTED, 2.0) == []  # above every score
    assert C["loop_no_match"] == 1 and C["loop_below_min_score"] > n_below
    assert any(k.mnLoopQuery == LOOP_KF + 1000 for k in lit.kfs.values())  # the state moved on all the same
    p.check_state()
    return cand
