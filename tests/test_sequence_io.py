"""The host threads of the overlapped sequence loop (streammos_amd.sequence_io) without a GPU: order, ring bound,
malformed input, sequences without ground truth."""
import os
import queue
import threading

import numpy as np
import pytest

from streammos_amd import kitti, sequence_io, synth


def _write_sequence(root, n, labels=True, points=120):
    seq = root / "seq"
    (seq / "velodyne").mkdir(parents=True)
    if labels:
        (seq / "labels").mkdir()
    for k in range(n):
        scan, lab = synth.synthetic_scan(k, 4, points // 4, with_labels=True)
        scan.tofile(seq / "velodyne" / ("%06d.bin" % k))
        if labels:
            # instance bits in the high half, a static and a moving id
            (np.where(lab == 2, 252, 40) | (k << 16)).astype(np.uint32).tofile(seq / "labels" / ("%06d.label" % k))
    return seq, sorted(os.listdir(seq / "velodyne"))


def test_reader_delivers_frames_in_order_within_its_ring(tmp_path):
    seq, files = _write_sequence(tmp_path, 9)
    before = threading.active_count()
    with sequence_io.ScanReader(str(seq), files, ring=3, pin=False) as reader:
        got = []
        held = [reader.get(), reader.get(), reader.get()]
        with pytest.raises(queue.Empty):            # all three slots held by the consumer: the reader waits
            reader.get(timeout=0.3)
        for fr in held:
            got.append(fr)
            reader.release(fr)
        while True:
            fr = reader.get()
            if fr is None:
                break
            got.append(fr)
            assert reader.peak_filled <= 3
            want_scan = np.fromfile(seq / "velodyne" / files[fr.index], dtype=np.float32).reshape(-1, 4)
            want_label = np.fromfile(seq / "labels" / (files[fr.index][:-4] + ".label"), dtype=np.uint32)
            assert np.array_equal(fr.scan.numpy(), want_scan)
            assert np.array_equal(fr.label.numpy().view(np.uint32), want_label)
            reader.release(fr)
        assert [fr.index for fr in got] == list(range(9))
        assert reader.peak_filled <= 3 and reader.max_points == 120
        assert reader.get() is None
    assert threading.active_count() == before


def _expect_value_error(seq, files, name):
    before = threading.active_count()
    reader = sequence_io.ScanReader(str(seq), files, ring=2, pin=False)
    try:
        with pytest.raises(ValueError, match=name):
            for _ in range(len(files) + 1):
                fr = reader.get(timeout=30)
                if fr is None:
                    break
                reader.release(fr)
    finally:
        reader.close()
    assert threading.active_count() == before


def test_truncated_scan_raises_naming_the_file(tmp_path):
    seq, files = _write_sequence(tmp_path, 5)
    path = seq / "velodyne" / files[3]
    data = path.read_bytes()
    path.write_bytes(data[:-6])
    _expect_value_error(seq, files, files[3])


def test_label_of_the_wrong_length_raises_naming_the_file(tmp_path):
    seq, files = _write_sequence(tmp_path, 5)
    path = seq / "labels" / (files[2][:-4] + ".label")
    np.zeros(119, dtype=np.uint32).tofile(path)
    _expect_value_error(seq, files, files[2][:-4] + ".label")


def test_unknown_semantic_id_raises_naming_the_file(tmp_path):
    seq, files = _write_sequence(tmp_path, 5)
    path = seq / "labels" / (files[4][:-4] + ".label")
    words = np.fromfile(path, dtype=np.uint32)
    words[17] = (7 << 16) | kitti.learning_map_lut().shape[0]        # one past the map; instance bits must not hide it
    words.tofile(path)
    _expect_value_error(seq, files, files[4][:-4] + ".label")


def test_sequence_without_labels_yields_no_ground_truth(tmp_path):
    seq, files = _write_sequence(tmp_path, 4, labels=False)
    with sequence_io.ScanReader(str(seq), files, ring=2, pin=False) as reader:
        n = 0
        while True:
            fr = reader.get(timeout=30)
            if fr is None:
                break
            assert fr.label is None and fr.scan.shape == (120, 4)
            reader.release(fr)
            n += 1
    assert n == 4


def test_writer_runs_jobs_in_order_and_hands_back_the_error(tmp_path):
    before = threading.active_count()
    writer = sequence_io.SlotWriter(range(2))
    done = []
    for k in range(3):
        slot = writer.take()
        writer.submit(slot, None, lambda k=k: done.append(k))
    slot = writer.take()

    def fail():
        raise ValueError("frame 3 does not fit")
    writer.submit(slot, None, fail)
    with pytest.raises(ValueError, match="does not fit"):
        while True:
            writer.take()
    writer.submit(0, None, lambda: done.append(4))        # dropped: the writer stopped at the error
    writer.close()
    assert done == [0, 1, 2] and isinstance(writer.error, ValueError)
    assert threading.active_count() == before
