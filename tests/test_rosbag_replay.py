"""Recorded multi-target data (the reference's test/test_multiple_targets.bag, extracted to
tests/golden/multiple_targets_tf.npz) replayed through the ingest policy: on CPU with the policy
restatement + oracle, on the GPU with the product, compared tick by tick.  The bag reader is checked
on a rosbag v2 file written from the fixture (the bag itself is not part of the repository)."""
import os
import struct

import numpy as np
import pytest

import oracle
from oracle.ingest_policy import RefIngest
from target_estimation_amd import rosbag_tf
from conftest import ROOT, model_path

FIX = os.path.join(ROOT, "tests", "golden", "multiple_targets_tf.npz")


def load_fixture():
    a = np.load(FIX)
    return [dict(recv_time=float(a["recv_time"][i]), stamp=float(a["stamp"][i]), frame_id=a["frame_id"][i].decode(),
                 child_frame_id=a["child_frame_id"][i].decode(), pose=a["pose"][i].copy()) for i in range(len(a["stamp"]))]


def _time(t):
    """(sec, nsec) that the reader turns back into exactly the float t."""
    sec = int(t)
    base = int(round((t - sec) * 1e9))
    for d in range(1000):
        for nsec in (base - d, base + d):
            if float(sec) + 1e-9 * float(nsec) == t:
                return sec, nsec
    raise ValueError(t)


def write_bag(path, fx):
    """A rosbag v2 file as the ROS recorder lays it out: bag header record (padded to 4 KB), one uncompressed chunk holding the
    /tf connection and one TFMessage per transform, the chunk's index record, then the index section (connection record and
    chunk-info record) that the bag header points to."""
    def field(name, value):
        return struct.pack("<I", len(name) + 1 + len(value)) + name.encode() + b"=" + value

    def record(fields, data):
        header = b"".join(field(k, v) for k, v in fields)
        return struct.pack("<I", len(header)) + header + struct.pack("<I", len(data)) + data

    def text(s):
        b = s.encode()
        return struct.pack("<I", len(b)) + b

    conn_data = b"".join(field(k, v.encode()) for k, v in (("topic", "/tf"), ("type", "tf2_msgs/TFMessage"), ("md5sum", "94810edda583a504dfda3829e70d7eec"),
                                                            ("message_definition", "geometry_msgs/TransformStamped[] transforms\n")))
    conn = record([("op", b"\x07"), ("conn", struct.pack("<I", 0)), ("topic", b"/tf")], conn_data)
    chunk, offsets, times = conn, [], []
    for seq, t in enumerate(fx):
        sec, nsec = _time(t["recv_time"])
        ssec, snsec = _time(t["stamp"])
        msg = struct.pack("<IIII", 1, seq, ssec, snsec) + text(t["frame_id"]) + text(t["child_frame_id"]) + struct.pack("<7d", *t["pose"])
        offsets.append(len(chunk))
        times.append((sec, nsec))
        chunk += record([("op", b"\x02"), ("conn", struct.pack("<I", 0)), ("time", struct.pack("<II", sec, nsec))], msg)
    magic = b"#ROSBAG V2.0\n"
    header_len = 4096
    chunk_pos = len(magic) + header_len
    chunk_rec = record([("op", b"\x05"), ("compression", b"none"), ("size", struct.pack("<I", len(chunk)))], chunk)
    index = record([("op", b"\x04"), ("ver", struct.pack("<I", 1)), ("conn", struct.pack("<I", 0)), ("count", struct.pack("<I", len(fx)))],
                   b"".join(struct.pack("<IIi", s, n, o) for (s, n), o in zip(times, offsets)))
    index_pos = chunk_pos + len(chunk_rec) + len(index)
    info = record([("op", b"\x06"), ("ver", struct.pack("<I", 1)), ("chunk_pos", struct.pack("<Q", chunk_pos)),
                   ("start_time", struct.pack("<II", *min(times))), ("end_time", struct.pack("<II", *max(times))), ("count", struct.pack("<I", 1))],
                  struct.pack("<II", 0, len(fx)))
    fields = [("op", b"\x03"), ("index_pos", struct.pack("<Q", index_pos)), ("conn_count", struct.pack("<I", 1)), ("chunk_count", struct.pack("<I", 1))]
    head = record(fields, b"")
    head = record(fields, b" " * (header_len - len(head)))
    assert len(head) == header_len
    with open(path, "wb") as f:
        f.write(magic + head + chunk_rec + index + conn + info)


@pytest.fixture(scope="module")
def bag(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bag") / "test_multiple_targets.bag")
    write_bag(path, load_fixture())
    return path


def test_reader_reproduces_the_fixture(bag):
    tr = rosbag_tf.read_tf(bag)
    fx = load_fixture()
    assert len(tr) == len(fx) == 572
    for a, b in zip(tr, fx):
        assert a["child_frame_id"] == b["child_frame_id"] and a["frame_id"] == b["frame_id"]
        assert a["stamp"] == b["stamp"] and a["recv_time"] == b["recv_time"]
        np.testing.assert_array_equal(a["pose"], b["pose"])


def test_reader_agrees_with_the_bags_own_index(bag):
    """Independent of the reader's walk over the chunks: the bag's INDEX section (written by the ROS recorder) declares how
    many messages the /tf connection holds; the reader must have decoded exactly that many, each TFMessage consumed to its
    last byte (parse_tf_message raises otherwise).  Stored in the fixture when it was made; re-derived here on the bag
    written from the fixture."""
    a = np.load(FIX)
    assert int(a["tf_messages_declared_by_the_bag_index"]) == int(a["tf_messages_decoded"]) == 572
    assert int(a["bag_conn_count"]) == 1 and int(a["bag_chunk_count"]) == 1
    declared, conns, chunks = rosbag_tf.declared_counts(bag)
    stats = {}
    rosbag_tf.read_tf(bag, stats=stats)
    assert declared == {"/tf": stats["messages"]} and (conns, chunks) == (1, 1)
    assert stats["messages"] == int(a["tf_messages_decoded"])


def test_fixture_contents_and_cpu_replay(models):
    fx = load_fixture()
    names = sorted({t["child_frame_id"] for t in fx})
    assert names == ["target_0", "target_1", "target_2"]
    assert {t["frame_id"] for t in fx} == {"camera_depth_optical_frame"}
    q = np.array([t["pose"][3:] for t in fx])
    np.testing.assert_allclose(np.linalg.norm(q, axis=1), 1.0, atol=1e-12)
    m = models["angular_velocities"]
    ref = RefIngest(m["model"], m["Q"], m["R"], m["P"], expiration_time=2.0)
    seen = []
    rosbag_tf.replay(fx, ref, 1.0 / 50.0, on_tick=lambda k, t, res: seen.append(tuple(res[0].tolist())))
    assert (0, 1) in seen or (0, 1, 2) in seen
    assert any(2 in s for s in seen)
    # while target_0 is visible and recently measured, its filtered position stays close to the measurement
    last = {}
    for t in fx:
        last[t["child_frame_id"]] = t["pose"]
    ids, poses = ref.tick(1.0 / 50.0, fx[-1]["recv_time"])
    for i, p in zip(ids, poses):
        assert np.linalg.norm(p[:3] - last["target_%d" % i][:3]) < 0.25


@pytest.mark.gpu
def test_gpu_replay_matches_policy_oracle(models):
    te = pytest.importorskip("target_estimation_amd")
    fx = load_fixture()
    m = models["angular_velocities"]
    dt = 1.0 / 50.0
    mgr = te.TargetManager()
    ing = te.MeasurementIngest(mgr, m["model"], m["Q"], m["R"], m["P"], expiration_time=2.0)
    ref = RefIngest(m["model"], m["Q"], m["R"], m["P"], expiration_time=2.0)
    got, want = [], []
    n1 = rosbag_tf.replay(fx, ing, dt, on_tick=lambda k, t, res: got.append(res))
    n2 = rosbag_tf.replay(fx, ref, dt, on_tick=lambda k, t, res: want.append(res))
    assert n1 == n2 > 1000
    for (ids, poses), (rids, rposes) in zip(got, want):
        np.testing.assert_array_equal(ids, rids)
        np.testing.assert_allclose(poses, rposes, atol=1e-8)
    assert max(len(g[0]) for g in got) == 3
    ing.close(); mgr.close()
