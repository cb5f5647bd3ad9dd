"""Device-side validation preprocessing (row f1): raw scans + pose differences in, network inputs out.

Host equivalent: ``streammos_amd.preprocess.build_sample`` (itself bit-exact against the reference's DataloadVal
arithmetic).  Only the raw scans cross PCIe; compaction, padding, TTA flips, quantisation and the point feature are
computed by csrc/preprocess.hip.  No host synchronisation: the number of in-range points stays on the device (the
un-padding of the labels is a kernel too).
"""
import ctypes

import numpy as np
import torch

from . import _lib, preprocess


def check_in_range_counts(counts, frame_point_num):
    """Host copy of a window's ``in_range_counts`` -> the host path's error (preprocess.pad_scan) for a scan that leaves no
    padding."""
    for t, c in enumerate(counts):
        if c >= frame_point_num:
            raise ValueError("scan %d of the window has %d in-range points, frame_point_num=%d leaves no padding "
                             "(the reference asserts pad_length > 0)" % (t, c, frame_point_num))


class DevicePreprocessor:
    def __init__(self, device, spec=None, frame_point_num=160000, tta=True):
        self.device = torch.device(device)
        self.spec = spec or preprocess.VoxelSpec()
        self.N = int(frame_point_num)
        signs = preprocess.TTA_SIGNS if tta else preprocess.TTA_SIGNS[:1]
        self.V = len(signs)
        self._sx = _lib.f32_array([s[0] for s in signs])
        self._sy = _lib.f32_array([s[1] for s in signs])
        sp = self.spec
        self._range6 = _lib.f64_array([sp.range_x[0], sp.range_x[1], sp.range_y[0], sp.range_y[1], sp.range_z[0], sp.range_z[1]])
        self._bev3 = _lib.i64_array(sp.bev_shape)
        h, w = sp.rv_shape
        phi_hi, phi_lo = 180.0 * np.pi / 180.0, -180.0 * np.pi / 180.0          # datasets/utils.py:176
        th_lo, th_hi = sp.RV_theta[0] * np.pi / 180.0, sp.RV_theta[1] * np.pi / 180.0
        self._rv4 = _lib.f64_array([phi_hi, (phi_hi - phi_lo) / w, th_hi, (th_hi - th_lo) / h])

    def build(self, scans, pose_diffs, strict=False):
        """scans: list of T device tensors [n_t, 4] float32, current scan first; pose_diffs: list of T 4x4 float64
        arrays (inv(P_cur) * P_t; None / identity for the current scan).  Returns the infer() inputs plus what is
        needed to un-pad the current scan's labels.

        A scan with >= frame_point_num in-range points does not fit (the reference asserts pad_length > 0,
        datasets/data_StreamMOS.py:563-566; the host path raises in preprocess.pad_scan).  The kernels never write out
        of bounds -- surplus points are dropped -- and the per-scan in-range counts stay on the device in
        ``in_range_counts``; ``check_capacity`` turns them into the host path's error.  strict=True checks at once
        (one stream synchronisation); the streaming runner checks when it reads the labels back anyway."""
        T, N, V = len(scans), self.N, self.V
        dev = self.device
        xyzi = torch.empty((V, T, 7, N, 1), dtype=torch.float32, device=dev)
        coord = torch.empty((V, T, N, 3, 1), dtype=torch.float32, device=dev)
        sphere = torch.empty((V, T, N, 2, 1), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        first = None
        counts = torch.zeros(T, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            for t, (scan, pose) in enumerate(zip(scans, pose_diffs)):
                if not (scan.is_cuda and scan.dtype == torch.float32 and scan.is_contiguous() and scan.shape[1] == 4):
                    raise RuntimeError("DevicePreprocessor: scans must be contiguous float32 [n, 4] GPU tensors")
                n = scan.shape[0]
                moved = torch.empty_like(scan)
                mask = torch.empty(n, dtype=torch.int32, device=dev)
                pd = None
                if pose is not None and not np.array_equal(np.asarray(pose), np.eye(4)):
                    pd = _lib.f64_array(np.asarray(pose, dtype=np.float64).reshape(-1)[:16])
                _lib.call("smos_prep_transform_mask", scan.data_ptr(), n, pd, self._range6, moved.data_ptr(), mask.data_ptr(),
                          stream)
                prefix = torch.cumsum(mask, 0, dtype=torch.int32)
                _lib.call("smos_prep_emit", moved.data_ptr(), mask.data_ptr(), prefix.data_ptr(), n, t, T, N, V, self._sx, self._sy,
                          self._range6, self._bev3, self._rv4, xyzi.data_ptr(), coord.data_ptr(), sphere.data_ptr(), stream)
                if n > 0:
                    counts[t:t + 1].copy_(prefix[-1:])
                if t == 0:
                    first = (mask, prefix, n)
        built = {"pcds_xyzi": xyzi, "pcds_coord": coord, "pcds_sphere_coord": sphere, "mask": first[0], "prefix": first[1],
                 "n_raw": first[2], "in_range_counts": counts, "n_live": counts[0:1]}
        if strict:
            self.check_capacity(built)
        return built

    def check_capacity(self, built):
        """Raises like preprocess.pad_scan when a scan of `built` left no padding (synchronises the stream)."""
        check_in_range_counts(built["in_range_counts"].cpu().tolist(), self.N)

    def unpad_labels(self, labels, built):
        """labels [N] uint8 of the padded sample -> [n_raw] uint8 for the raw scan (0 where out of range)."""
        raw = torch.empty(built["n_raw"], dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.call("smos_prep_unpad_labels", labels.data_ptr(), labels.shape[0], built["mask"].data_ptr(),
                      built["prefix"].data_ptr(), built["n_raw"], raw.data_ptr(),
                      torch.cuda.current_stream(self.device).cuda_stream)
        return raw


def check_train_counts(counts):
    """Host copy of ``in_range_counts`` [B, 3, T] -> the error of the host path's reference (``np.random.choice`` raises on an
    empty frame) for a (sample, window, frame) without in-range points."""
    counts = np.asarray(counts).reshape(-1, preprocess.TRAIN_WINDOWS, preprocess.TRAIN_FRAMES - preprocess.TRAIN_WINDOWS + 1)
    for b, w, t in zip(*np.nonzero(counts == 0)):
        raise ValueError("sample %d, window %d, frame %d has no point inside the range: nothing to resample from (the frame "
                         "was written as the padding point with label 0)" % (b, w, t))


class _RowStaging:
    """Checks and uploads of the five scans / label arrays of a training sample (needs ``self.device``)."""

    def _stage(self, arrays, dtype):
        """Host arrays -> one device tensor through pinned staging (one copy; the pinned block goes back to torch's caching
        host allocator, which re-uses it only after the copy has run: no host wait)."""
        total = sum(a.shape[0] for a in arrays)
        staged = torch.empty((total,) + tuple(arrays[0].shape[1:]), dtype=dtype, pin_memory=True)
        at = 0
        for a in arrays:
            staged[at:at + a.shape[0]].copy_(torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a))
            at += a.shape[0]
        return staged.to(self.device, non_blocking=True)

    def _check_rows(self, items, what, np_dtypes, torch_dtypes, trailing):
        if len(items) != preprocess.TRAIN_FRAMES:
            raise RuntimeError("%s: a training sample has %d %s, got %d" % (type(self).__name__, preprocess.TRAIN_FRAMES, what, len(items)))
        on_dev = [torch.is_tensor(s) and s.is_cuda for s in items]
        for s, dev in zip(items, on_dev):
            shape_ok = getattr(s, "ndim", None) == 1 + len(trailing) and tuple(s.shape[1:]) == trailing and s.shape[0] >= 1
            if dev:
                ok = s.dtype in torch_dtypes and s.is_contiguous() and s.device == self.device
            else:
                ok = isinstance(s, np.ndarray) and s.dtype in np_dtypes and s.flags["C_CONTIGUOUS"]
            if not (ok and shape_ok):
                raise RuntimeError("%s: %s must be contiguous %s arrays of shape [n >= 1%s], on the host (numpy) "
                                   "or on %s" % (type(self).__name__, what, np_dtypes[0].__name__, "".join(", %d" % d for d in trailing), self.device))

    def _device_rows(self, items, torch_dtype, trailing):
        """Five checked host arrays or device tensors -> (device pointers, lengths, tensors kept alive).  The host arrays
        among them go up in one copy; a device tensor is used where it lies."""
        lengths = [int(s.shape[0]) for s in items]
        host = [s for s in items if not torch.is_tensor(s)]
        keep = [s for s in items if torch.is_tensor(s)]
        ptrs = [s.data_ptr() if torch.is_tensor(s) else None for s in items]
        if host:
            whole = self._stage(host, torch_dtype)
            keep.append(whole)
            step = whole.element_size() * int(np.prod(trailing, dtype=np.int64))
            at = 0
            for i, s in enumerate(items):
                if ptrs[i] is None:
                    ptrs[i] = whole.data_ptr() + at * step
                    at += lengths[i]
        return ptrs, lengths, keep


class DeviceTrainPreprocessor(_RowStaging):
    """Training samples built on the device (row f2, csrc/train_prep.hip): raw scans, label words and poses in, the batch dict
    of ``AttNet.forward`` out.  Host equivalent: ``streammos_amd.preprocess.build_train_sample``.  Only the scans (16 bytes a
    point) and label words (4 bytes a point) cross PCIe; nothing is read back, the per-frame in-range counts stay on the device
    (``check_counts`` is the one synchronising call).  Copy-paste augmentation is a stage of its own in front of this one
    (``DeviceCopyPaste``, or the host's): the builder takes scans and label words as they are;
    ``build_batch(paste=DeviceCopyPaste(...))`` runs it on the device first.  ``paste_labels`` then names the labels of the
    pasted points, e.g. {"pcds_target": (0, 1, 2), "pcds_bf_target": (2, 2, 2)}; without it the LUT is unchanged.

    The random draws are either explicit (``preprocess.TrainDraws`` with device or host ``words`` / ``noise``) or come from a
    seed: Philox4x32-10 inside the kernels for the resampling words and the noise, ``preprocess.seeded_scalars`` on the host
    for the five per-sample scalars.  The same (seed, sample_index) gives the same bits on every run."""

    T = preprocess.TRAIN_FRAMES - preprocess.TRAIN_WINDOWS + 1
    W = preprocess.TRAIN_WINDOWS

    def __init__(self, device, spec=None, frame_point_num=130000, aug=None, label_maps=None, paste_labels=None):
        from . import kitti
        self.device = torch.device(device)
        self.spec = spec or preprocess.VoxelSpec()
        self.N = int(frame_point_num)
        if self.N <= 0:
            raise RuntimeError("DeviceTrainPreprocessor: frame_point_num must be positive, got %d" % self.N)
        self.aug = aug or preprocess.AugParam()
        maps = dict(label_maps or {"pcds_target": kitti.learning_map_lut()})
        if not 1 <= len(maps) <= 4:
            raise RuntimeError("DeviceTrainPreprocessor: 1..4 label maps, got %d" % len(maps))
        self.paste_label_base = None
        if paste_labels is not None:       # the three label ids of pasted points, directly past the longest map
            try:
                maps, self.paste_label_base = preprocess.paste_label_maps(maps, paste_labels)
            except ValueError as e:
                raise RuntimeError("DeviceTrainPreprocessor: %s" % e)
        self.target_names = list(maps)
        lut_len = max(int(np.asarray(m).shape[0]) for m in maps.values())
        lut = np.zeros((len(maps), lut_len), dtype=np.int32)
        for i, m in enumerate(maps.values()):
            lut[i, :np.asarray(m).shape[0]] = np.asarray(m)
        self._lut = torch.from_numpy(lut).to(self.device)
        sp = self.spec
        self._range6 = _lib.f64_array([sp.range_x[0], sp.range_x[1], sp.range_y[0], sp.range_y[1], sp.range_z[0], sp.range_z[1]])
        self._bev3 = _lib.i64_array(sp.bev_shape)
        self.bev_target_shape = (sp.bev_shape[0] // 2, sp.bev_shape[1] // 2, 1)
        h, w = sp.rv_shape
        phi_hi, phi_lo = 180.0 * np.pi / 180.0, -180.0 * np.pi / 180.0          # datasets/utils.py:176
        th_lo, th_hi = sp.RV_theta[0] * np.pi / 180.0, sp.RV_theta[1] * np.pi / 180.0
        self._rv4 = _lib.f64_array([phi_hi, (phi_hi - phi_lo) / w, th_hi, (th_hi - th_lo) / h])
        self._work = {}            # stream -> scratch tensor (a stream runs its builds one after the other)

    # ---- buffers ----------------------------------------------------------------------------------------------------------
    def output_shapes(self):
        n = self.N
        shapes = {}
        for i in range(self.W):
            shapes["pcds_xyzi_%d" % i] = ((self.T, 7, n, 1), torch.float32)
            shapes["pcds_coord_%d" % i] = ((self.T, n, 3, 1), torch.float32)
            shapes["pcds_sphere_coord_%d" % i] = ((self.T, n, 2, 1), torch.float32)
            shapes["pcds_bev_target_%d" % i] = (self.bev_target_shape, torch.int64)
            for name in self.target_names:
                shapes["%s_%d" % (name, i)] = ((n, 1), torch.int64)
        shapes["in_range_counts"] = ((self.W, self.T), torch.int32)
        return shapes

    def alloc_batch(self, batch_size):
        """Uninitialised batch tensors (leading batch dimension) that ``build(out=..., batch_slot=b)`` fills slice by slice."""
        return {k: torch.empty((int(batch_size),) + tuple(shape), dtype=dtype, device=self.device)
                for k, (shape, dtype) in self.output_shapes().items()}

    def _check_draw(self, value, what, shape, np_dtype, torch_dtypes):
        if torch.is_tensor(value) and value.is_cuda:
            ok = value.dtype in torch_dtypes and value.is_contiguous() and tuple(value.shape) == shape and value.device == self.device
        else:
            ok = isinstance(value, np.ndarray) and value.dtype == np_dtype and value.shape == shape
        if not ok:
            raise RuntimeError("DeviceTrainPreprocessor: draws.%s must be %s of shape %s, on the host (numpy) or on %s"
                               % (what, np.dtype(np_dtype).name, list(shape), self.device))

    def _draw_tensor(self, value, shape, torch_dtype):
        if torch.is_tensor(value):
            return value
        return self._stage([np.ascontiguousarray(value).reshape((1,) + shape)], torch_dtype)

    # ---- draws ------------------------------------------------------------------------------------------------------------
    def seeded_draws(self, seed, sample_index=0):
        """The draws ``build(seed=seed, sample_index=sample_index)`` uses, as explicit ``TrainDraws`` with device tensors:
        smos_train_prep_draws for the words and the noise, ``preprocess.seeded_scalars`` for the five scalars."""
        seed, sample_index = self._check_seed(seed, sample_index)
        words = torch.empty((self.W, self.T, self.N), dtype=torch.int32, device=self.device)
        noise = torch.empty((self.W, self.T * self.N, 3), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.call("smos_train_prep_draws", seed, sample_index, self.N, float(self.aug.noise_mean), float(self.aug.noise_std),
                      words.data_ptr(), noise.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
        return preprocess.TrainDraws(words, noise, *preprocess.seeded_scalars(seed, sample_index, self.aug))

    @staticmethod
    def _check_seed(seed, sample_index):
        seed, sample_index = int(seed), int(sample_index)
        if not (0 <= seed < 2 ** 64 and 0 <= sample_index < 2 ** 64):
            raise RuntimeError("DeviceTrainPreprocessor: seed and sample_index are unsigned 64-bit integers")
        return seed, sample_index

    # ---- building ---------------------------------------------------------------------------------------------------------
    def build(self, scans, label_words, poses, draws=None, seed=None, sample_index=0, out=None, batch_slot=0, aligned=False):
        """One sample.  scans: 5 [n_k, 4] float32 arrays in ``meta_list_raw`` order (numpy, uploaded through pinned staging, or
        contiguous tensors already on the device); label_words: their [n_k] uint32 words (numpy uint32 / int32, or int32
        device tensors); poses: 5 4x4 float64.  Exactly one of ``draws`` (explicit) and ``seed`` (with ``sample_index``).
        ``out``: batch tensors as ``alloc_batch`` returns them (any batch stride; each sample slice contiguous): the sample is
        written into slice ``batch_slot``; without ``out`` a batch of one is allocated.  Returns the dict of batch tensors.
        aligned=True: the scans already went through the first alignment (the state in which the reference's copy-paste
        augmentation edits them); only the windows' second alignment is applied.
        Every argument is checked before the first launch; an argument error is a RuntimeError."""
        if (draws is None) == (seed is None):
            raise RuntimeError("DeviceTrainPreprocessor.build: give either draws or seed, not both and not neither")
        if len(scans) != preprocess.TRAIN_FRAMES or len(label_words) != preprocess.TRAIN_FRAMES:
            raise RuntimeError("DeviceTrainPreprocessor: a training sample has %d scans and label arrays, got %d and %d"
                               % (preprocess.TRAIN_FRAMES, len(scans), len(label_words)))
        if len(poses) != preprocess.TRAIN_FRAMES:
            raise RuntimeError("DeviceTrainPreprocessor: a training sample has %d poses, got %d" % (preprocess.TRAIN_FRAMES, len(poses)))
        for s, w in zip(scans, label_words):
            if getattr(s, "ndim", None) != 2 or getattr(w, "ndim", None) != 1 or s.shape[0] != w.shape[0]:
                raise RuntimeError("DeviceTrainPreprocessor: a scan [n, 4] needs n label words, got shapes %s and %s"
                                   % (list(getattr(s, "shape", ())), list(getattr(w, "shape", ()))))
        poses = [np.asarray(p, dtype=np.float64) for p in poses]
        if any(p.shape != (4, 4) for p in poses):
            raise RuntimeError("DeviceTrainPreprocessor: poses are 4x4 matrices")
        N, W, T = self.N, self.W, self.T
        if out is None:
            out, batch_slot = self.alloc_batch(1), 0
        slices = {}
        for k, (shape, dtype) in self.output_shapes().items():
            t = out.get(k)
            if not (torch.is_tensor(t) and t.device == self.device and t.dtype == dtype and tuple(t.shape[1:]) == tuple(shape)
                    and 0 <= batch_slot < t.shape[0] and t[batch_slot].is_contiguous()):
                raise RuntimeError("DeviceTrainPreprocessor.build: out[%r] must be a %s tensor [B > %d, %s] on %s with contiguous "
                                   "samples" % (k, dtype, batch_slot, ", ".join(str(d) for d in shape), self.device))
            slices[k] = t[batch_slot]
        self._check_rows(scans, "scans", (np.float32,), (torch.float32,), (4,))
        self._check_rows(label_words, "label words", (np.uint32, np.int32), (torch.int32,), ())
        if draws is not None:
            self._check_draw(draws.words, "words", (W, T, N), np.uint32, (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32") else ()))
            self._check_draw(draws.noise, "noise", (W, T * N, 3), np.float64, (torch.float64,))
        else:
            seed, sample_index = self._check_seed(seed, sample_index)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            if draws is not None:
                words = self._draw_tensor(draws.words, (W, T, N), torch.int32)
                noise = self._draw_tensor(draws.noise, (W, T * N, 3), torch.float64)
                words_ptr, noise_ptr, seed, sample_index = words.data_ptr(), noise.data_ptr(), 0, 0
                shift, scale, h_flip, v_flip, theta_z = draws.shift, draws.scale, draws.h_flip, draws.v_flip, draws.theta_z
            else:
                words_ptr = noise_ptr = None
                shift, scale, h_flip, v_flip, theta_z = preprocess.seeded_scalars(seed, sample_index, self.aug)
            scan_ptrs, lengths, keep_s = self._device_rows(scans, torch.float32, (4,))
            word_ptrs, _, keep_w = self._device_rows(label_words, torch.int32, ())
            work_bytes = _lib.query("smos_train_prep_work_bytes", max(lengths))
            if work_bytes < 0:
                raise RuntimeError("DeviceTrainPreprocessor: a scan of %d points is too large" % max(lengths))
            work = self._work.get(stream.cuda_stream)
            if work is None or work.numel() < work_bytes:
                work = self._work[stream.cuda_stream] = torch.empty(work_bytes, dtype=torch.uint8, device=self.device)
            inv0 = np.linalg.inv(poses[0])
            first = np.stack([np.eye(4) if aligned else inv0.dot(p) for p in poses]).reshape(-1)
            second = np.stack([np.linalg.inv(poses[w]).dot(poses[0]) for w in range(W)]).reshape(-1)
            ang = float(theta_z) * np.pi / 180.0
            vp5, vp3 = ctypes.c_void_p * preprocess.TRAIN_FRAMES, ctypes.c_void_p * W
            targets = (ctypes.c_void_p * (len(self.target_names) * W))(
                *[slices["%s_%d" % (name, w)].data_ptr() for name in self.target_names for w in range(W)])
            _lib.call("smos_train_prep_build", vp5(*scan_ptrs), vp5(*word_ptrs), _lib.i64_array(lengths), _lib.f64_array(first),
                      _lib.f64_array(second), self._range6, self._bev3, self._rv4, N, words_ptr, noise_ptr, seed, sample_index,
                      float(self.aug.noise_mean), float(self.aug.noise_std), _lib.f64_array(shift), float(scale), int(v_flip),
                      int(h_flip), float(np.cos(ang)), float(np.sin(ang)), self._lut.data_ptr(), len(self.target_names),
                      self._lut.shape[1], vp3(*[slices["pcds_xyzi_%d" % w].data_ptr() for w in range(W)]),
                      vp3(*[slices["pcds_coord_%d" % w].data_ptr() for w in range(W)]),
                      vp3(*[slices["pcds_sphere_coord_%d" % w].data_ptr() for w in range(W)]), targets,
                      vp3(*[slices["pcds_bev_target_%d" % w].data_ptr() for w in range(W)]), slices["in_range_counts"].data_ptr(),
                      work.data_ptr(), work.numel(), stream.cuda_stream)
            for t in keep_s + keep_w + ([words, noise] if draws is not None else []):   # read by the launches above
                t.record_stream(stream)
        return out

    def build_batch(self, samples, draws=None, seed=None, first_sample_index=0, out=None, aligned=False, paste=None, paste_draws=None):
        """samples: list of (scans, label_words, poses); draws: one ``TrainDraws`` per sample, or seed: sample b uses
        ``sample_index = first_sample_index + b``.  Returns the dict ``AttNet.forward`` / ``StreamMOS_seg.AttNet.forward``
        consume (keys ``pcds_xyzi_i``, ``pcds_coord_i``, ``pcds_sphere_coord_i``, one target per label map and
        ``pcds_bev_target_i`` for i = 0..2, plus ``in_range_counts`` [B, 3, 3]), on the device, each sample written straight
        into its slice.  paste: a ``DeviceCopyPaste``; every sample then goes through ``paste.apply`` (with ``paste_draws[b]``,
        or seeded like the rest) and is built with aligned=True; the dict gains ``paste_status``, one int32 tensor per sample.
        The builder must have been made with ``paste_labels``."""
        if (draws is None) == (seed is None):
            raise RuntimeError("DeviceTrainPreprocessor.build_batch: give either draws or seed, not both and not neither")
        if draws is not None and len(draws) != len(samples):
            raise RuntimeError("DeviceTrainPreprocessor.build_batch: %d samples, %d draws" % (len(samples), len(draws)))
        if paste is not None:
            if aligned:
                raise RuntimeError("DeviceTrainPreprocessor.build_batch: copy-paste takes raw scans (it aligns them itself)")
            if self.paste_label_base is None or paste.label_base != self.paste_label_base:
                raise RuntimeError("DeviceTrainPreprocessor.build_batch: the builder needs paste_labels, and its label base (%s) must "
                                   "be the paste stage's (%d)" % (self.paste_label_base, paste.label_base))
            if (paste_draws is None) != (draws is None) or (paste_draws is not None and len(paste_draws) != len(samples)):
                raise RuntimeError("DeviceTrainPreprocessor.build_batch: explicit draws need one PasteDraws per sample, seeded ones none")
        elif paste_draws is not None:
            raise RuntimeError("DeviceTrainPreprocessor.build_batch: paste_draws without paste")
        if out is None:
            out = self.alloc_batch(len(samples))
        status = []
        for b, (scans, label_words, poses) in enumerate(samples):
            if paste is not None:
                scans, label_words, st = paste.apply(scans, label_words, poses, draws=None if paste_draws is None else paste_draws[b],
                                                     seed=seed, sample_index=first_sample_index + b)
                status.append(st)
            self.build(scans, label_words, poses, draws=None if draws is None else draws[b], seed=seed,
                       sample_index=first_sample_index + b, out=out, batch_slot=b, aligned=aligned or paste is not None)
        if paste is not None:
            out["paste_status"] = status
        return out

    def check_counts(self, built):
        """Raises if a frame of `built` had no point inside the range (synchronises the stream: the one host read)."""
        check_train_counts(built["in_range_counts"].cpu().numpy())


def check_padding_stays_out(poses, spec):
    """The fixed-length layout of DeviceCopyPaste marks a removed point with the padding point p = (-1000, -1000, -4000), and
    relies on the builder's range filter to drop it in every window.  Window 0 filters p itself: z = -4000 is below any range.
    Windows 1 and 2 filter R p + t with (R, t) = inv(P_w) P_0, rounded to float32.  |R p + t| >= s_min(R) |p| - |t|, and a point
    inside the range box is at most the box's farthest corner away from the origin, so p stays out whenever
    s_min(R) |p| - |t| exceeds that radius (by 1 m here, far more than the float32 rounding of values near 4000, 2.5e-4).
    Raises for poses that do not satisfy this -- a translation of kilometres between the frames of one sample, or a pose
    whose rotation block is far from a rotation."""
    pad = float(np.linalg.norm(np.array(preprocess.PASTE_PAD[:3], dtype=np.float64)))
    radius = float(np.sqrt(sum(max(abs(lo), abs(hi)) ** 2 for lo, hi in (spec.range_x, spec.range_y, spec.range_z))))
    poses = [np.asarray(p, dtype=np.float64) for p in poses]
    if not (spec.range_z[0] > preprocess.PAD_Z):
        raise RuntimeError("DeviceCopyPaste: the range's lower z bound %s does not exclude the padding point" % (spec.range_z[0],))
    for w in range(1, preprocess.TRAIN_WINDOWS):
        m = np.linalg.inv(poses[w]).dot(poses[0])
        if not np.isfinite(m).all():
            raise RuntimeError("DeviceCopyPaste: pose %d is not finite" % w)
        s_min = float(np.linalg.svd(m[:3, :3], compute_uv=False).min())
        if not s_min * pad - float(np.linalg.norm(m[:3, 3])) > radius + 1.0:
            raise RuntimeError("DeviceCopyPaste: the poses of frames 0 and %d could carry the padding point of a removed row back "
                               "into the range (translation %.1f m, smallest singular value %.3g)"
                               % (w, float(np.linalg.norm(m[:3, 3])), s_min))


class DeviceObjectBank:
    """The object bank of the copy-paste augmentation, uploaded once: the objects' points concatenated ([P, 4] float32) and the
    footprint of each box scaled by 1.05 ([B, 4, 2] float64, compute_box_3d in float64 on the host) on the device; the offsets
    into the points, yaw, categories and the per-category index lists stay on the host, where the scalar draws are made and
    the launches get their pointers."""

    def __init__(self, device, objects):
        self.device = torch.device(device)
        self.objects = list(objects)
        if not self.objects or not all(isinstance(o, preprocess.PasteObject) for o in self.objects):
            raise RuntimeError("DeviceObjectBank: a non-empty list of preprocess.PasteObject")
        self.sizes = [int(o.pcds.shape[0]) for o in self.objects]
        if min(self.sizes) < 1:
            raise RuntimeError("DeviceObjectBank: an object without points")
        self.offsets = np.concatenate(([0], np.cumsum(self.sizes))).astype(np.int64)
        self.categories = [[i for i, o in enumerate(self.objects) if o.cate == c] for c in preprocess.PASTE_CATEGORIES]
        self.points = torch.from_numpy(np.concatenate([o.pcds for o in self.objects])).to(self.device)
        self.footprints = torch.from_numpy(np.stack([preprocess.paste_box_footprint(o) for o in self.objects])).to(self.device)

    @classmethod
    def from_dir(cls, device, object_dir):
        """The reference's layout: one folder per category with .npz files (pcds, center, size, yaw, cate); files of sequence
        08 are skipped (copy_paste.py:82).  Files are taken in sorted order."""
        import os
        objects = []
        for c in preprocess.PASTE_CATEGORIES:
            folder = os.path.join(object_dir, c)
            for name in sorted(os.listdir(folder)):
                if name.endswith(".npz") and name.split("_")[0] != "08":
                    with np.load(os.path.join(folder, name)) as z:
                        objects.append(preprocess.PasteObject(z["pcds"], z["center"], z["size"], z["yaw"], str(z["cate"])))
        return cls(device, objects)

    def __len__(self):
        return len(self.objects)


class DeviceCopyPaste(_RowStaging):
    """Copy-paste augmentation on the device (csrc/copy_paste.hip): raw scans, label words, poses and an object bank in, the
    five edited scans in the fixed-length layout ``DeviceTrainPreprocessor.build(aligned=True)`` consumes out.  Host equivalent:
    ``preprocess.copy_paste_sample``.  One launch per sample and four per object, nothing is read back.

    label_base: pasted points get the label word label_base + motion label; it must be the length of the longest label map of
    the builder that consumes the result (``DeviceTrainPreprocessor(..., paste_labels=...).paste_label_base``)."""

    def __init__(self, bank, spec=None, label_base=360, max_objects=preprocess.PASTE_MAX_OBJECTS):
        self.bank = bank
        self.device = bank.device
        self.spec = spec or preprocess.VoxelSpec()
        self.label_base = int(label_base)
        self.max_objects = int(max_objects)
        if not (0 <= self.label_base and self.label_base + 2 <= 0xFFFF):
            raise RuntimeError("DeviceCopyPaste: label_base %d + 2 does not fit the low half of a label word" % self.label_base)
        if not 0 <= self.max_objects <= 256:
            raise RuntimeError("DeviceCopyPaste: 0..256 objects a sample")
        c, s = preprocess.paste_rotations()
        self._cos, self._sin = _lib.f64_array(c), _lib.f64_array(s)
        self._work = {}

    def _check_draws(self, draws, need_noise):
        if not isinstance(draws, preprocess.PasteDraws):
            raise RuntimeError("DeviceCopyPaste: draws is a preprocess.PasteDraws")
        if not (len(draws.velocity) == draws.count and draws.count <= 256):
            raise RuntimeError("DeviceCopyPaste: %d objects, %d velocities (at most 256 objects)" % (draws.count, len(draws.velocity)))
        for i in range(draws.count):
            if not 0 <= draws.index[i] < len(self.bank):
                raise RuntimeError("DeviceCopyPaste: object %d: bank index %d outside 0..%d" % (i, draws.index[i], len(self.bank) - 1))
            if sorted(draws.order[i].tolist()) != list(range(preprocess.PASTE_TRIALS)):
                raise RuntimeError("DeviceCopyPaste: object %d: the trial order is not a permutation of 0..19" % i)
            if not np.isfinite(draws.velocity[i]):
                raise RuntimeError("DeviceCopyPaste: object %d: velocity %r" % (i, draws.velocity[i]))
        if need_noise:
            if draws.noise is None or len(draws.noise) != draws.count:
                raise RuntimeError("DeviceCopyPaste: explicit draws carry one noise array per object")
            for i, nz in enumerate(draws.noise):
                shape = (preprocess.TRAIN_FRAMES, self.bank.sizes[draws.index[i]], 3)
                if torch.is_tensor(nz) and nz.is_cuda:
                    ok = nz.dtype == torch.float64 and nz.is_contiguous() and tuple(nz.shape) == shape and nz.device == self.device
                else:
                    ok = isinstance(nz, np.ndarray) and nz.dtype == np.float64 and nz.shape == shape
                if not ok:
                    raise RuntimeError("DeviceCopyPaste: object %d: noise must be float64 of shape %s, on the host (numpy) or on %s"
                                       % (i, list(shape), self.device))

    def seeded_draws(self, seed, sample_index=0):
        """The draws ``apply(seed=seed, sample_index=sample_index)`` uses, as explicit ``PasteDraws`` with device noise:
        ``preprocess.seeded_paste_scalars`` for the host scalars, smos_copy_paste_draws for the noise."""
        seed, sample_index = DeviceTrainPreprocessor._check_seed(seed, sample_index)
        index, velocity, order = preprocess.seeded_paste_scalars(seed, sample_index, self.bank.categories, self.max_objects)
        noise = []
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            for i, b in enumerate(index):
                nz = torch.empty((preprocess.TRAIN_FRAMES, self.bank.sizes[b], 3), dtype=torch.float64, device=self.device)
                _lib.call("smos_copy_paste_draws", seed, sample_index, i, self.bank.sizes[b], nz.data_ptr(), stream)
                noise.append(nz)
        return preprocess.PasteDraws(index, velocity, order, noise)

    def apply(self, scans, label_words, poses, draws=None, seed=None, sample_index=0):
        """scans: 5 raw [n_k, 4] float32 arrays (numpy or device tensors), label_words: their [n_k] words, poses: 5 4x4 float64,
        as ``DeviceTrainPreprocessor.build`` takes them.  Exactly one of ``draws`` (PasteDraws with noise) and ``seed``.
        Returns (scans', words', status): five [n_k + M, 4] float32 and five [n_k + M] int32 device tensors in the fixed-length
        layout (M = the points of all drawn objects; views of one allocation each) -- first-aligned, to be built with
        aligned=True -- and status [count] int32 on the device: the accepted trial of each object or -1.
        Every argument is checked before the first launch; an argument error is a RuntimeError."""
        if (draws is None) == (seed is None):
            raise RuntimeError("DeviceCopyPaste.apply: give either draws or seed, not both and not neither")
        F = preprocess.TRAIN_FRAMES
        if len(scans) != F or len(label_words) != F or len(poses) != F:
            raise RuntimeError("DeviceCopyPaste: a training sample has %d scans, label arrays and poses" % F)
        for s, w in zip(scans, label_words):
            if getattr(s, "ndim", None) != 2 or getattr(w, "ndim", None) != 1 or s.shape[0] != w.shape[0]:
                raise RuntimeError("DeviceCopyPaste: a scan [n, 4] needs n label words, got shapes %s and %s"
                                   % (list(getattr(s, "shape", ())), list(getattr(w, "shape", ()))))
        poses = [np.asarray(p, dtype=np.float64) for p in poses]
        if any(p.shape != (4, 4) for p in poses):
            raise RuntimeError("DeviceCopyPaste: poses are 4x4 matrices")
        check_padding_stays_out(poses, self.spec)
        self._check_rows(scans, "scans", (np.float32,), (torch.float32,), (4,))
        self._check_rows(label_words, "label words", (np.uint32, np.int32), (torch.int32,), ())
        if draws is None:
            seed, sample_index = DeviceTrainPreprocessor._check_seed(seed, sample_index)
            index, velocity, order = preprocess.seeded_paste_scalars(seed, sample_index, self.bank.categories, self.max_objects)
            draws = preprocess.PasteDraws(index, velocity, order, None)
            self._check_draws(draws, need_noise=False)
            noise = [None] * draws.count
        else:
            self._check_draws(draws, need_noise=True)
            seed = sample_index = 0
            noise = draws.noise
        bank = self.bank
        sizes = [bank.sizes[b] for b in draws.index]
        slots = int(sum(sizes))
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            scan_ptrs, lengths, keep_s = self._device_rows(scans, torch.float32, (4,))
            word_ptrs, _, keep_w = self._device_rows(label_words, torch.int32, ())
            work_bytes = _lib.query("smos_copy_paste_work_bytes", lengths[0])
            if work_bytes < 0:
                raise RuntimeError("DeviceCopyPaste: a scan of %d points is too large" % lengths[0])
            work = self._work.get(stream.cuda_stream)
            if work is None or work.numel() < work_bytes:
                work = self._work[stream.cuda_stream] = torch.empty(work_bytes, dtype=torch.uint8, device=self.device)
            rows = [n + slots for n in lengths]
            total = int(sum(rows))
            pts = torch.empty((total, 4), dtype=torch.float32, device=self.device)
            words = torch.empty(total, dtype=torch.int32, device=self.device)
            ang = torch.empty((total, 2), dtype=torch.float32, device=self.device)
            flags = torch.empty(total, dtype=torch.uint8, device=self.device)
            status = torch.empty(max(draws.count, 1), dtype=torch.int32, device=self.device)[:draws.count]
            inv0 = np.linalg.inv(poses[0])
            first = np.stack([inv0.dot(p) for p in poses])
            vp5 = ctypes.c_void_p * F
            n5 = _lib.i64_array(lengths)
            _lib.call("smos_copy_paste_begin", vp5(*scan_ptrs), vp5(*word_ptrs), n5, _lib.f64_array(first.reshape(-1)), slots,
                      draws.count, pts.data_ptr(), words.data_ptr(), ang.data_ptr(), flags.data_ptr(), status.data_ptr(),
                      stream.cuda_stream)
            first0 = _lib.f64_array(first[0].reshape(-1))
            keep_n, slot = [], 0
            for i, b in enumerate(draws.index):
                m, at = sizes[i], slot
                slot += m
                if m < preprocess.PASTE_MIN_POINTS:       # copy_paste.py:195: its slot keeps the padding point
                    continue
                obj = bank.objects[b]
                vx, vy = preprocess.paste_velocity_xy(obj, draws.velocity[i])
                nz = noise[i]
                if nz is not None and not torch.is_tensor(nz):
                    nz = self._stage([np.ascontiguousarray(nz)], torch.float64)
                if nz is not None:
                    keep_n.append(nz)
                _lib.call("smos_copy_paste_object", scan_ptrs[0], word_ptrs[0], first0, n5, slots, pts.data_ptr(), words.data_ptr(),
                          ang.data_ptr(), flags.data_ptr(), status.data_ptr(), draws.count, i,
                          bank.points.data_ptr() + int(bank.offsets[b]) * 16, m, at, bank.footprints.data_ptr() + b * 64,
                          _lib.f64_array([vx * t * 0.1 for t in range(F)]), _lib.f64_array([vy * t * 0.1 for t in range(F)]),
                          (ctypes.c_uint8 * preprocess.PASTE_TRIALS)(*draws.order[i].tolist()), self._cos, self._sin,
                          None if nz is None else nz.data_ptr(), seed, sample_index,
                          self.label_base + preprocess.paste_motion_label(draws.velocity[i]), work.data_ptr(), work.numel(),
                          stream.cuda_stream)
            for t in keep_s + keep_w + keep_n:       # read by the launches above
                t.record_stream(stream)
        out_scans, out_words, at = [], [], 0
        for r in rows:
            out_scans.append(pts[at:at + r])
            out_words.append(words[at:at + r])
            at += r
        return out_scans, out_words, status
