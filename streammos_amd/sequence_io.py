"""Host threads of the overlapped sequence loop (run_sequence(device_preprocess=True); DESIGN.md "The sequence loop").

``ScanReader`` reads a sequence's ``velodyne/*.bin`` (and ``labels/*.label``) in frame order on a thread of its own,
straight into a ring of host buffers (pinned when a GPU is present, so that the uploads are asynchronous copies).
``SlotWriter`` runs the label-file writes on a thread of its own, in submission order.  Neither thread enqueues GPU
work: the caller's thread is the only one that does; the threads only wait on events it hands them.  An exception
on either thread is handed to the caller (``ScanReader.get`` raises it; ``SlotWriter.error`` holds it and the free-slot
queue wakes the caller), and ``close()`` always joins the thread.
"""
import collections
import os
import queue
import threading

import numpy as np
import torch

from . import kitti

Frame = collections.namedtuple("Frame", "index slot scan label")     # scan [n,4] float32, label [n] int32 words or None
_END = object()


class _Failure:
    def __init__(self, exc):
        self.exc = exc


def _read_exact(path, out):
    """Reads the whole file into the numpy array `out` (its exact byte size)."""
    view = memoryview(out).cast("B")
    with open(path, "rb", buffering=0) as f:
        got = 0
        while got < view.nbytes:
            k = f.readinto(view[got:])
            if not k:
                break
            got += k
        if got != view.nbytes or f.read(1):
            raise ValueError("%s: the file changed size while the sequence was read" % path)


class ScanReader:
    """Frames of one sequence, in order, from a thread that stays up to `ring` frames ahead of the consumer.

    ``get()`` returns the next ``Frame`` (None after the last); its ``scan`` / ``label`` are views of ring slot
    ``frame.slot``.  ``release(frame, event)`` hands the slot back: it is refilled only once `event` (the CUDA event
    recorded behind the copies that read it; None when nothing is in flight) has completed.  Malformed input raises a
    ValueError naming the file, in ``get()``, at the frame it belongs to."""

    def __init__(self, seq_dir, files, ring=6, labels=None, pin=None):
        self.paths = [os.path.join(seq_dir, "velodyne", f) for f in files]
        if labels is None:
            labels = os.path.isdir(os.path.join(seq_dir, "labels"))
        self.label_paths = [os.path.join(seq_dir, "labels", f[:-4] + ".label") for f in files] if labels else None
        self.ring = int(ring)
        if self.ring < 1:
            raise ValueError("ScanReader: ring must hold at least one frame")
        self.max_points = max([os.stat(p).st_size // 16 for p in self.paths], default=0)
        self._map_n = kitti.learning_map_lut().shape[0]
        pin = torch.cuda.is_available() if pin is None else bool(pin)
        cap = max(self.max_points, 1)
        self._scan_buf = [torch.empty(cap * 4, dtype=torch.float32, pin_memory=pin) for _ in range(self.ring)]
        self._label_buf = [torch.empty(cap, dtype=torch.int32, pin_memory=pin) for _ in range(self.ring)] if labels else None
        self._events = [None] * self.ring
        self._free = queue.Queue()
        for k in range(self.ring):
            self._free.put(k)
        self._ready = queue.Queue()
        self._stop = threading.Event()
        self._filled = 0
        self.peak_filled = 0                 # most slots ever filled and not yet handed back (<= ring)
        self._lock = threading.Lock()
        self._thread = threading.Thread(target=self._run, name="smos-scan-reader", daemon=True)
        self._thread.start()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _run(self):
        try:
            for i in range(len(self.paths)):
                k = self._free.get()
                if k is None or self._stop.is_set():
                    return
                with self._lock:
                    self._filled += 1
                    self.peak_filled = max(self.peak_filled, self._filled)
                ev, self._events[k] = self._events[k], None
                if ev is not None:
                    ev.synchronize()                # the upload that read this slot has completed
                self._ready.put(self._read(i, k))
            self._ready.put(_END)
        except BaseException as e:                  # handed to the consumer; the thread ends
            self._ready.put(_Failure(e))

    def _read(self, i, k):
        path = self.paths[i]
        size = os.stat(path).st_size
        if size % 16:
            raise ValueError("%s: %d bytes is not a whole number of 16-byte points (x, y, z, intensity)" % (path, size))
        n = size // 16
        if n > self.max_points:
            raise ValueError("%s: the file grew while the sequence was read" % path)
        scan = self._scan_buf[k][:n * 4]
        _read_exact(path, scan.numpy())
        label = None
        if self.label_paths is not None:
            lpath = self.label_paths[i]
            lsize = os.stat(lpath).st_size
            if lsize != 4 * n:
                raise ValueError("%s: %d bytes of labels for a scan of %d points (%s)" % (lpath, lsize, n, path))
            label = self._label_buf[k][:n]
            words = label.numpy().view(np.uint32)
            _read_exact(lpath, words)
            sem = words & 0xFFFF
            bad = np.flatnonzero(sem >= self._map_n)
            if bad.size:
                raise ValueError("%s: semantic id %d (point %d) is outside the learning map (ids < %d)"
                                 % (lpath, int(sem[bad[0]]), int(bad[0]), self._map_n))
        return Frame(i, k, scan.view(n, 4), label)

    def get(self, timeout=None):
        """The next frame (None when the sequence is done).  Raises what the reader thread raised; queue.Empty after
        `timeout` seconds without a frame."""
        item = self._ready.get(timeout=timeout)
        if isinstance(item, _Failure):
            self._ready.put(item)                   # every later get() raises it too
            raise item.exc
        if item is _END:
            self._ready.put(item)
            return None
        return item

    def release(self, frame, event=None):
        self._events[frame.slot] = event
        with self._lock:
            self._filled -= 1
        self._free.put(frame.slot)

    def close(self):
        self._stop.set()
        self._free.put(None)
        self._thread.join()


class SlotWriter:
    """Runs ``submit(slot, event, write)`` jobs in order on a thread of its own: waits for `event` (the copy that filled
    the slot's host buffer), calls ``write()`` and puts `slot` on ``free``.  The first exception stops the thread: it is
    kept in ``error``, later jobs are dropped and None is put on ``free`` to wake a caller waiting for a slot."""

    def __init__(self, slots):
        self.free = queue.Queue()
        for k in slots:
            self.free.put(k)
        self.error = None
        self._work = queue.Queue()
        self._thread = threading.Thread(target=self._run, name="smos-label-writer", daemon=True)
        self._thread.start()

    def _run(self):
        while True:
            job = self._work.get()
            if job is None:
                return
            slot, event, write = job
            try:
                if event is not None:
                    event.synchronize()
                write()
            except BaseException as e:
                self.error = e
                self.free.put(None)
                return
            self.free.put(slot)

    def submit(self, slot, event, write):
        self._work.put((slot, event, write))

    def take(self):
        """A free slot; waits while every slot is in flight.  Raises the writer's error."""
        slot = self.free.get()
        if slot is None:
            raise self.error
        return slot

    def close(self):
        """Lets the jobs already submitted finish (unless one failed) and joins the thread."""
        self._work.put(None)
        self._thread.join()
