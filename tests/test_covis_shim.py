"""The C++ shim's KeyFrame::UpdateConnections() and LocalMapping::KeyFrameCulling() (shim/include/Objects.h,
LocalMapping.h, tests/cpp/test_covis.cpp) against the literal restatement (tests/covis_literal.py).

The scenes of tests/covis_scenes.py are played on the restatement, which logs every operation with the object
graph it leaves; the C++ driver replays the log on KeyFrame / MapPoint / Map / LocalMapping objects through the
reference's signatures and writes, after every UpdateConnections() and KeyFrameCulling(), every keyframe's
mConnectedKeyFrameWeights, ordered vectors, parent, children and isBad() and every point's isBad(), all
compared exactly.  CPU: the driver and the shim build, export the reference's members, and throw without a
device.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

import covis_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "shim", "build", "test_covis")


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "shim")])
    return EXE


def test_covis_shim_abi(exe):
    r = subprocess.run([exe, "abi"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "abi ok" in r.stdout


def test_covis_shim_exports_reference_members(exe):
    out = subprocess.check_output(["nm", "-DC", "--defined-only", os.path.join(ROOT, "shim", "liborbx_shim.so")]).decode()
    for sym in ["ORB_SLAM2::KeyFrame::UpdateConnections()",
                "ORB_SLAM2::KeyFrame::SetBadFlag()",
                "ORB_SLAM2::LocalMapping::KeyFrameCulling()"]:
        assert sym in out, sym


def serialise(log):
    out = []
    for op in log:
        k = op[0]
        if k == "set":
            ent = op[2]
            n = len(ent)
            out += [struct.pack("<Iqi", 1, op[1], n), np.array([e[0] for e in ent], "<i4").tobytes(),
                    np.array([e[1] for e in ent], "<i4").tobytes(), np.array(op[3], "<f4").tobytes(),
                    np.array(op[4], "<f4").tobytes()]
        elif k == "bad":
            out += [struct.pack("<Ii", 2, len(op[1])), np.array(op[1], "<i4").tobytes()]
        elif k == "update":
            out.append(struct.pack("<Iq", 3, op[1]))
        elif k == "cull":
            out += [struct.pack("<Ii", 4, len(op[1])), np.array(op[1], "<i8").tobytes(),
                    np.array(op[2], np.uint8).tobytes(), struct.pack("<i", op[3])]
        else:
            raise AssertionError(k)
    out.append(struct.pack("<I", 0))
    return b"".join(out)


def graph_words(graph):
    """A logged graph as the int64 words the driver's dump writes."""
    g, pts = graph
    w = [len(g)]
    for k in sorted(g):
        e = g[k]
        w += [k, e["bad"], e["parent"], len(e["weights"])]
        for i, x in e["weights"]:
            w += [i, x]
        w += [len(e["ordered"])] + e["ordered"] + [len(e["ordered_w"])] + e["ordered_w"]
        w += [len(e["children"])] + e["children"]
    w.append(len(pts))
    for i in sorted(pts):
        w += [i, pts[i]]
    return w


def compare(log, raw):
    got = np.frombuffer(raw, "<i8").tolist()
    pos = n = 0
    for op in log:
        if op[0] not in ("update", "cull"):
            continue
        want = graph_words(op[-1])
        assert got[pos:pos + len(want)] == want, (n, op[0], op[1])
        pos += len(want)
        n += 1
    assert pos == len(got)
    return n


def test_log_round_trip_format():
    """The operations file the driver reads and the dump it writes: sizes add up for a small hand-made log."""
    p = S.LitOnly()
    p.set_keyframe(1, S.ent([5, 6]))
    p.set_keyframe(2, S.ent([6, 5, 9]))
    p.update_connections(1)
    p.cull([1], [0], True)
    raw = serialise(p.log)
    assert len(raw) == (16 + 4 * 8) + (16 + 4 * 12) + 12 + (8 + 8 + 1 + 4) + 4
    w = graph_words(p.log[2][-1])
    # two keyframes: 1 (parent 2: first connection) and 2 (child 1); three points
    assert w == [2, 1, 0, 2, 1, 2, 2, 1, 2, 1, 2, 0, 2, 0, -1, 1, 1, 2, 1, 1, 1, 2, 1, 1, 3, 5, 0, 6, 0, 9, 0]


@pytest.mark.gpu
def test_gpu_covis_shim_graph_scene(gpu, exe, tmp_path):
    p = S.LitOnly()
    S.script_graph(p)
    fin, fout = str(tmp_path / "ops.in"), str(tmp_path / "ops.out")
    with open(fin, "wb") as f:
        f.write(serialise(p.log))
    r = subprocess.run([exe, "run", fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert compare(p.log, open(fout, "rb").read()) == 23 + 3


@pytest.mark.gpu
@pytest.mark.parametrize("monocular", [True, False])
def test_gpu_covis_shim_cull_scene(gpu, exe, tmp_path, monocular):
    """The culling scene's verdicts, cascades and bad points through LocalMapping::KeyFrameCulling()."""
    p = S.LitOnly()
    S.build_cull_table(p)
    ne = [k == 13 for k in S.CULL_ORDER]
    v, bad, _ = p.cull(S.CULL_ORDER, ne, monocular)
    assert 1 in v and 2 in v and bad
    fin, fout = str(tmp_path / "ops.in"), str(tmp_path / "ops.out")
    with open(fin, "wb") as f:
        f.write(serialise(p.log))
    r = subprocess.run([exe, "run", fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert compare(p.log, open(fout, "rb").read()) == 1
