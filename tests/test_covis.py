"""The covisibility table on the GPU (orbx_covis_*, orb_slam2_commit_amd.CovisibilityMap) against the literal
restatement of tests/covis_literal.py, on the scenes of tests/covis_scenes.py.

Every comparison is exact (integers and id lists): KFcounter, the ordered lists and pKFmax, the local point
lists, the culling verdicts and went-bad lists, and after every mutating call the full read-back of rows,
nObs and bad against the literal's state.

CPU: hand-computed cases of the restatement, the scenes' own branch asserts on the restatement alone, the
ABI symbols, the argument refusals and the loud failure without a GPU.  The covis entry points pass no
struct, so orbx_sizeof has no entry for them.
"""
import ctypes as C

import numpy as np
import pytest

import covis_literal as CL
import covis_scenes as S

SYMBOLS = ["orbx_covis_create", "orbx_covis_destroy", "orbx_covis_clear", "orbx_covis_check_row",
           "orbx_covis_set_keyframe", "orbx_covis_erase_keyframe", "orbx_covis_set_points_bad", "orbx_covis_size",
           "orbx_covis_read_keyframe", "orbx_covis_read_points", "orbx_covis_update_connections", "orbx_covis_vote",
           "orbx_covis_local_points", "orbx_covis_cull"]


class LitPair(S.Pair):
    """The scripts on the literal alone: only their own asserts run."""

    def __init__(self):
        self.lit = CL.Table()

    def set_keyframe(self, kf, entries):
        self.lit.set_keyframe(kf, entries)

    def erase_keyframe(self, kf):
        self.lit.erase_keyframe(kf)

    def set_points_bad(self, ids):
        self.lit.set_points_bad(ids)

    def update_connections(self, kf, th=15):
        return self.lit.update_connections(kf, th)

    def vote(self, pids):
        return self.lit.vote(pids)

    def local_points(self, kfs):
        return self.lit.local_points(kfs)

    def cull(self, cands, not_erase, monocular):
        trace = []
        v, bad = self.lit.cull(cands, not_erase, monocular, trace)
        return v, bad, {t[0]: t[1:] for t in trace}

    def check_state(self):
        pass


SCRIPTS = [("update_connections", S.script_update_connections), ("vote_local", S.script_vote_local),
           ("cull_monocular", lambda p: S.script_cull(p, True)), ("cull_stereo", lambda p: S.script_cull(p, False)),
           ("sizes", S.script_sizes)]


# ------------------------------------------------------------------------------------ CPU
def test_literal_update_connections_by_hand():
    """By hand.  A = {1, 2, 3}; B = {1, 2}; C = {3}; D = {2, 3, 9}.  With th = 2, UpdateConnections(A) counts
    B 2, C 1, D 2: the counter keeps all three, the ordered list holds D then B (equal weight, descending id),
    B and D receive A as a connection, A's first connection makes D its parent.  With th = 15 nothing passes
    and B, the smallest id among the maxima, is connected alone."""
    t = CL.Table()
    for k, pts in ((10, [1, 2, 3]), (11, [1, 2]), (12, [3]), (13, [2, 3, 9])):
        t.set_keyframe(k, S.ent(pts))
    assert t.update_connections(10, th=2) == ([(11, 2), (12, 1), (13, 2)], [(13, 2), (11, 2)])
    A, B, D = t.kfs[10], t.kfs[11], t.kfs[13]
    assert A.mpParent is D and A in D.mspChildrens and not A.mbFirstConnection
    assert B.mvpOrderedConnectedKeyFrames == [A] and B.mvOrderedWeights == [2] and t.kfs[12].GetWeight(A) == 0
    t2 = CL.Table()
    for k, pts in ((10, [1, 2, 3]), (11, [1, 2]), (12, [3]), (13, [2, 3, 9])):
        t2.set_keyframe(k, S.ent(pts))
    assert t2.update_connections(10) == ([(11, 2), (12, 1), (13, 2)], [(11, 2)])
    assert t2.kfs[13].mConnectedKeyFrameWeights == {} and t2.kfs[10].mpParent is t2.kfs[11]


def test_literal_culling_by_hand():
    """By hand, monocular.  Points 1..10 are seen by X, Y, Z and K (nObs 4, three others): K = {1..10} has
    nRedundant 10 of nMPs 11 (10 > 9.9) and is culled.  L = {1..9, 50}: those points now have nObs 4 with L, the
    others X, Y, Z: 9 redundant of 10, 9 > 9.0 is false: kept.  With K holding a stereo point 60 alone
    (nObs 2) the point goes bad when K leaves."""
    t = CL.Table()
    for k in (20, 21, 22):
        t.set_keyframe(k, S.ent(range(1, 11)))
    t.set_keyframe(5, S.ent(range(1, 11)) + [(60, 0, CL.STEREO | CL.CLOSE), (-1, 0, 0)])
    t.set_keyframe(6, S.ent(list(range(1, 10)) + [50]))
    assert t.points[60].nObs == 2 and t.points[1].nObs == 5
    trace = []
    v, bad = t.cull([5, 6], [False, False], True, trace)
    assert trace == [(5, 11, 10), (6, 10, 9)] and v == [1, 0] and bad == [60]
    assert 5 not in t.kfs and t.points[1].nObs == 4 and t.points[60].mbBad and t.points[60].nObs == 0
    # stereo gate: far points do not count; mbNotErase: reported, observations stay
    t = CL.Table()
    for k in (20, 21, 22):
        t.set_keyframe(k, S.ent(range(1, 11)))
    t.set_keyframe(5, S.ent(range(1, 10)) + S.ent([70, 71], 0, 0))
    trace = []
    assert t.cull([5], [True], True, trace) == ([0], []) and trace == [(5, 11, 9)]
    trace = []
    assert t.cull([5], [True], False, trace) == ([2], []) and trace == [(5, 9, 9)]
    assert 5 in t.kfs and t.points[1].nObs == 4


def test_literal_vote_and_local_points_by_hand():
    t = CL.Table()
    t.set_keyframe(1, S.ent([5, 6, 7]))
    t.set_keyframe(2, S.ent([7, 8, 5]))
    t.set_points_bad([6])
    assert t.vote([5, 6, -1, 8]) == ([0, 1, 0, 0], [(1, 1), (2, 2)], 2, 2)
    assert t.vote([5, 7]) == ([0, 0], [(1, 2), (2, 2)], 1, 2)  # a tie: the smallest id
    assert t.local_points([2, 1]) == [7, 8, 5] and t.local_points([1, 2]) == [5, 7, 8]
    assert t.state()[0][1][0] == [5, -1, 7]  # the bad point's slot is what EraseMapPointMatch leaves


@pytest.mark.parametrize("name,script", SCRIPTS, ids=[s[0] for s in SCRIPTS])
def test_scenes_reach_their_branches(name, script):
    script(LitPair())


def test_abi_symbols():
    from orb_slam2_commit_amd import CovisibilityMap, _lib
    L = _lib.lib()
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and getattr(L, s) is not None, s
    assert CovisibilityMap.STEREO == CL.STEREO == 1 and CovisibilityMap.CLOSE == CL.CLOSE == 2
    f = CovisibilityMap.flags([1.0, -1.0, 5.0, -1.0], [1.0, 1.0, 3.0, -1.0], CL.TH_DEPTH)
    assert f.tolist() == [3, 2, 1, 0]
    assert [CL.flags_to_stereo_depth(int(x)) for x in f] == [(1.0, 1.0), (-1.0, 1.0), (1.0, 3.0), (-1.0, -1.0)]


def test_row_check_on_the_host():
    """orbx_covis_check_row is the check set_keyframe applies before any device call."""
    from orb_slam2_commit_amd import _lib
    from orb_slam2_commit_amd._lib import ptr
    L = _lib.lib()

    def chk(p, o, f, n=None):
        p, o, f = np.asarray(p, np.int32), np.asarray(o, np.int32), np.asarray(f, np.uint8)
        return L.orbx_covis_check_row(ptr(p), ptr(o), ptr(f), len(p) if n is None else n)

    assert chk([3, -1, 7, -1], [0, 1, 7, 63], [0, 1, 2, 3]) == 0
    assert L.orbx_covis_check_row(None, None, None, 0) == 0
    assert chk([3, 7, 3], [0, 0, 0], [0, 0, 0]) == -1            # a point twice
    assert chk([-2], [0], [0]) == -1 and chk([1 << 26], [0], [0]) == -1
    assert chk([1], [-1], [0]) == -1 and chk([1], [64], [0]) == -1
    assert chk([1], [0], [4]) == -1
    assert chk([1], [0], [0], n=-1) == -1
    assert L.orbx_covis_check_row(None, None, None, 1) == -1


def test_argument_checks_before_the_device():
    """Null handles, null outputs and negative sizes are refused with ORBX_ERR_ARG before any device call; the
    refusals that need a live handle (unknown and duplicate ids) are in test_gpu_refusals."""
    from orb_slam2_commit_amd import _lib
    from orb_slam2_commit_amd._lib import ptr
    L = _lib.lib()
    a32, a64, a8 = np.zeros(4, np.int32), np.zeros(4, np.int64), np.zeros(4, np.uint8)
    n = C.c_int()
    k, m = C.c_int64(), C.c_int32()
    assert L.orbx_covis_create(0, None) == -1
    h = C.c_void_p()
    assert L.orbx_covis_create(-1, C.byref(h)) == -1 and not h.value
    assert L.orbx_covis_destroy(None) == -1 and L.orbx_covis_clear(None) == -1
    assert L.orbx_covis_set_keyframe(None, 1, 4, ptr(a32), ptr(a32), ptr(a8)) == -1
    assert L.orbx_covis_erase_keyframe(None, 1) == -1
    assert L.orbx_covis_set_points_bad(None, ptr(a32), 4) == -1
    assert L.orbx_covis_size(None, None, None, None) == -1
    assert L.orbx_covis_read_keyframe(None, 1, ptr(a32), ptr(a32), ptr(a8), 4, C.byref(n)) == -1
    assert L.orbx_covis_read_points(None, ptr(a32), 4, ptr(a32), ptr(a8)) == -1
    assert L.orbx_covis_update_connections(None, 1, 15, ptr(a64), ptr(a32), 4, C.byref(n), ptr(a64), ptr(a32), 4,
                                           C.byref(n)) == -1
    assert L.orbx_covis_vote(None, ptr(a32), 4, ptr(a8), ptr(a64), ptr(a32), 4, C.byref(n), C.byref(k),
                             C.byref(m)) == -1
    assert L.orbx_covis_local_points(None, ptr(a64), 4, ptr(a32), 4, C.byref(n)) == -1
    assert L.orbx_covis_cull(None, ptr(a64), 4, ptr(a8), 1, ptr(a8), ptr(a32), 4, C.byref(n)) == -1


def test_no_gpu_fails_loudly():
    from orb_slam2_commit_amd import CovisibilityMap, OrbxError, _lib
    L = _lib.lib()
    if L.orbx_device_count() > 0:
        CovisibilityMap(0).close()
        return
    h = C.c_void_p()
    assert L.orbx_covis_create(0, C.byref(h)) == -4 and not h.value
    with pytest.raises(OrbxError) as e:
        CovisibilityMap(0)
    assert e.value.code == -4


# ------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name,script", SCRIPTS, ids=[s[0] for s in SCRIPTS])
def test_gpu_scenes(gpu, name, script):
    from orb_slam2_commit_amd import CovisibilityMap
    cm = CovisibilityMap(0)
    try:
        p = S.Pair(cm)
        script(p)
        p.check_state()
        cm.clear()
        assert cm.size() == (0, 0, 0)
        # the handle after clear: the same scene once more on the same tables
        p = S.Pair(cm)
        if name != "sizes":
            script(p)
    finally:
        cm.close()


@pytest.mark.gpu
def test_gpu_refusals(gpu):
    """Unknown and duplicate ids, bad rows and short buffers on a live handle; none of them changes the table."""
    from orb_slam2_commit_amd import CovisibilityMap, OrbxError
    cm = CovisibilityMap(0)
    try:
        p = S.Pair(cm)
        p.set_keyframe(1, S.ent([5, 6, 7]))
        p.set_keyframe(2, S.ent([7, 8, 5]))

        def refused(code, fn, *a):
            with pytest.raises(OrbxError) as e:
                fn(*a)
            assert e.value.code == code, (fn.__name__, e.value.code)
            p.check_state()

        refused(-1, cm.set_keyframe, 3, [4, 4], [0, 0], [0, 0])       # a point twice in a row
        refused(-1, cm.set_keyframe, -1, [4], [0], [0])
        refused(-1, cm.set_keyframe, 3, [4], [64], [0])
        refused(-1, cm.erase_keyframe, 9)                             # not live
        refused(-1, cm.update_connections, 9)
        refused(-1, cm.read_keyframe, 9)
        refused(-1, cm.read_points, [100000])                         # never seen
        refused(-1, cm.local_points, [1, 9])
        refused(-1, cm.local_points, [1, 2, 1])                       # a keyframe twice
        refused(-1, cm.cull, [2, 2], [0, 0], True)
        refused(-1, cm.cull, [9], [0], True)
        refused(-1, cm.vote, [5, -2])
        refused(-1, cm.set_points_bad, [-1])
        refused(-2, cm.local_points, [1, 2], 2)                       # four distinct points, room for two
        assert cm.local_points([1, 2]) == [5, 6, 7, 8]
        p.erase_keyframe(1)
        refused(-1, cm.update_connections, 1)                         # erased: no longer live
        p.set_keyframe(1, S.ent([5]))                                 # and back under the same id
        assert p.update_connections(1) == ([(2, 1)], [(2, 1)])
    finally:
        cm.close()
