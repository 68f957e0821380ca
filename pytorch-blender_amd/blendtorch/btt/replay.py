"""HBM-resident replay of rendered frames.

The reference replays recordings from disk. :class:`FileDataset` unpickles every
``.btr`` message on every epoch, in DataLoader workers, and collates on the host
(pkg_pytorch/blendtorch/btt/dataset.py:119-153, file.py:81-132).
:class:`DeviceReplayBuffer` keeps the raw u8 frames in GPU memory instead. An
MI355X has 288 GB of HBM3E, which holds about 230k 640x480 RGBA frames. Every
epoch after the first then runs at HBM speed without touching the host:

* ``from_recordings(prefix)``: the ``.btr`` files are memory-mapped, and each
  message is scanned in place by the native pickle codec (zero-copy views, no
  unpickling of the image). The image bytes are staged through a pinned buffer
  into the device store in large chunks.
* ``extend(images, **meta)``: append frames (ring semantics: the oldest are
  overwritten once ``capacity`` is reached). The frames can be device tensors,
  e.g. a :class:`~blendtorch.btt.gpu.DeviceLoader` with
  ``DecodeConfig.raw()`` output, or host arrays.
* ``sample(B, decode)`` / ``batches(B, decode)``: draw random (or shuffled)
  indices on the device and decode them with ONE fused gather+decode kernel
  (``ops.decode_gather``: the kernel reads frame ``index[b]`` straight from the
  store; the gathered u8 batch is never materialised). Per-item metadata
  (``btid``, ``frameid``, ``xy``, ...) is gathered on the device too.
* ``DecodeConfig(crop=ops.Crop(...))``: the same launch also draws a window
  per image (Philox, next to the index draw) and decodes through it: random
  crop + mirror, or with ``Crop(frame_size, pad=4)`` the random shift of
  DrQ / RAD (replicate padding).  The batch reports its windows as
  ``batch['crop']``; a graphed sampler draws fresh ones on every replay.
* ``sample_transitions(B, decode, stack=k, stride=S)``: frame-stacked
  transitions for pixel-based RL (``obs``, ``next_obs``, the metadata at both
  ends) assembled by the sample kernel from frames stored once; episode
  starts come from a one-byte ``first`` metadata column.  ``nstep=n,
  gamma=g`` adds the n-step return, its bootstrap discount and the stack n
  steps later, in the same launch.
* ``DeviceReplayBuffer(..., priority_alpha=a)`` + ``sample_transitions(...,
  prioritized=True)``: prioritized experience replay.  The priorities are
  integer masses in a 64-ary sum tree in HBM; a small launch in front of the
  transition launch draws the anchors by tree descent (stratified) and the
  importance weights, ``update_priorities`` writes TD errors back.

On a CPU device the same API runs with the fp32 reference ops (tests, hosts
without a GPU). On a GPU device the HIP kernels are required and fail loudly
if the extension is missing.
"""
from __future__ import annotations

import mmap
from glob import glob
from typing import Dict, Iterator, Optional

import numpy as np
import torch

from .. import ops
from ..ops import DecodeConfig

__all__ = ['DeviceReplayBuffer']


def _as_tensor(x, device):
    if isinstance(x, torch.Tensor):
        return x.to(device)
    return torch.as_tensor(np.asarray(x), device=device)


class DeviceReplayBuffer:
    """Ring buffer of raw u8 ``H x W x C`` frames (+ numeric metadata) on one device.

    Params
    ------
    capacity: int
        Frames held; the store is ``capacity x H x W x C`` bytes, allocated
        on the first ``extend`` (when the frame shape is known).
    device: torch.device / str
        Where frames live (``'cuda:N'`` for HBM, ``'cpu'`` for the reference path).
    image_key: str
        Message key of the image when filling from recordings / loaders.
    priority_alpha: float, optional
        Keep a priority per stored transition (prioritized experience replay,
        Schaul et al. 2016): ``sample_transitions(prioritized=True)`` draws in
        proportion to ``priority ** priority_alpha`` and
        ``update_priorities`` writes TD errors back.  ``None``: nothing is
        allocated and nothing changes.
    first_key, priority_stride:
        The episode-start column and the frames per environment step of the
        transitions the priorities are kept for (``sample_transitions``'s
        ``first_key`` and ``stride``); ``extend`` needs that column then.
    """

    def __init__(self, capacity: int, device=None, image_key: str = 'image', seed: Optional[int] = None,
                 priority_alpha: Optional[float] = None, first_key: str = 'first', priority_stride: int = 1):
        if capacity < 1:
            raise ValueError('capacity must be >= 1')
        self.capacity = int(capacity)
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.image_key = image_key
        self.store: Optional[torch.Tensor] = None     # [capacity, H, W, C] u8
        self.meta: Dict[str, torch.Tensor] = {}
        self._size = 0
        self._next = 0
        # sampler state of the fused kernel: Philox key and counter (host-side
        # for eager sampling: one launch per batch; graphed samplers keep a
        # device counter the captured graph advances itself)
        self.seed = int(torch.initial_seed() if seed is None else seed) & (2 ** 64 - 1)
        self._ctr = 0
        # device int64 (head, size) for graphed transition samplers; None until one exists
        self._state: Optional[torch.Tensor] = None
        if self.device.type == 'cuda':
            ops.hip_ext()   # fail loudly here, not at the first sample()
        # prioritized replay (None: nothing is allocated): the mass tree of ops.priority_tree over the slots,
        # kept eligible-or-zero by extend() for transitions of `priority_stride` with episode starts `first_key`
        self.priority_alpha = None if priority_alpha is None else float(priority_alpha)
        self.first_key, self.priority_stride = first_key, int(priority_stride)
        self._levels = self._max_mass = self._beta = None
        if self.priority_alpha is not None:
            if not 0.0 <= self.priority_alpha <= 16.0:
                raise ValueError('priority_alpha must lie in [0, 16]')
            if not 1 <= self.priority_stride < self.capacity:
                raise ValueError('priority_stride must lie in [1, capacity)')
            self._levels = ops.priority_tree(np.zeros(self.capacity, np.uint32), device=self.device)
            self._max_mass = torch.from_numpy(np.array([ops.PRIORITY_ONE], np.uint32)).to(self.device)
            self._beta = [None, torch.zeros(1, dtype=torch.float32, device=self.device)]   # host value, device scalar

    # -- filling ---------------------------------------------------------------
    def __len__(self):
        return self._size

    @property
    def frame_shape(self):
        return None if self.store is None else tuple(self.store.shape[1:])

    @property
    def nbytes(self):
        return 0 if self.store is None else self.store.numel()

    def _alloc(self, shape, meta):
        self.store = torch.empty((self.capacity,) + tuple(shape), dtype=torch.uint8, device=self.device)
        for k, v in meta.items():
            v = _as_tensor(v, self.device)
            self.meta[k] = torch.zeros((self.capacity,) + tuple(v.shape[1:]), dtype=v.dtype, device=self.device)

    def extend(self, images, **meta):
        """Append ``n`` frames (u8 ``[n,H,W,C]`` or ``[n,H,W]``; tensor or ndarray)
        and per-frame metadata arrays of leading length ``n``."""
        imgs = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images))
        if imgs.dtype != torch.uint8:
            raise TypeError('frames must be uint8')
        if imgs.dim() == 3:
            imgs = imgs.unsqueeze(-1)
        n = int(imgs.shape[0])
        meta = {k: v for k, v in meta.items() if v is not None}
        if self.store is None:
            self._alloc(imgs.shape[1:], {k: v[:1] if len(v) else v for k, v in meta.items()})
        if tuple(imgs.shape[1:]) != self.frame_shape:
            raise ValueError(f'frame shape {tuple(imgs.shape[1:])} != store {self.frame_shape}')
        if set(meta) != set(self.meta):
            raise ValueError(f'metadata keys {sorted(meta)} != {sorted(self.meta)}')
        if n > self.capacity:   # only the newest `capacity` frames survive
            imgs = imgs[n - self.capacity:]
            meta = {k: v[n - self.capacity:] for k, v in meta.items()}
            n = self.capacity
        if self._levels is not None:
            self._first_column()
        pos, start = 0, self._next
        while pos < n:
            k = min(n - pos, self.capacity - self._next)
            self.store[self._next:self._next + k].copy_(imgs[pos:pos + k], non_blocking=True)
            for key, v in meta.items():
                self.meta[key][self._next:self._next + k].copy_(_as_tensor(v[pos:pos + k], self.device))
            self._next = (self._next + k) % self.capacity
            pos += k
        self._size = min(self.capacity, self._size + n)
        if self._levels is not None and n:   # the appended slots and the steps before them change eligibility
            args = (self.capacity, start, n, self._next, self._size, self.priority_stride)
            if self.device.type == 'cuda':
                ops.priority_extend(self._levels, self.capacity, self._max_mass, *args[1:], self._first_column())
            else:
                ops.reference_priority_extend([lev.numpy() for lev in self._levels], int(self._max_mass.numpy()[0]),
                                              *args, self._first_column().numpy())
        if self._state is not None:   # a graphed transition sampler reads the ring state from the device
            self._state.copy_(torch.tensor([self._next, self._size], dtype=torch.int64))
        return self

    # -- priorities ------------------------------------------------------------
    def _first_column(self):
        first = self.meta.get(self.first_key)
        if first is None or first.dim() != 1 or first.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f'a prioritized buffer needs a uint8 / bool [capacity] metadata column {self.first_key!r} '
                             '(episode starts): extend(frames, ..., %s=flags)' % self.first_key)
        return first

    def _need_priorities(self):
        if self._levels is None:
            raise ValueError('this buffer keeps no priorities: DeviceReplayBuffer(..., priority_alpha=...)')

    @property
    def priority_mass(self) -> torch.Tensor:
        """uint32 [capacity], read-only: the mass of the transition anchored at
        each slot (``ops.reference_priority_mass``; 0: may not be drawn)."""
        self._need_priorities()
        return self._levels[0][:self.capacity].clone()

    def update_priorities(self, index, priority):
        """Write priorities (TD errors; float32) back for the anchors ``index``
        of a batch: slot ``index[b]`` takes mass ``clamp(rint(priority[b] **
        priority_alpha * 65536), 1, 2**32 - 1)``.  Of duplicate anchors the
        last entry wins; an anchor that may not be drawn stays excluded.  On a
        GPU one launch per 1024 entries, no host sync."""
        self._need_priorities()
        index = _as_tensor(index, self.device).to(torch.int64).reshape(-1)
        priority = _as_tensor(priority, self.device).to(torch.float32).reshape(-1)
        if index.numel() != priority.numel():
            raise ValueError('update_priorities: one priority per index')
        for s in range(0, int(index.numel()), ops.MAX_PRIORITY_B):
            i, p = index[s:s + ops.MAX_PRIORITY_B], priority[s:s + ops.MAX_PRIORITY_B]
            if self.device.type == 'cuda':
                ops.priority_update(self._levels, self.capacity, self._max_mass, i, p, self.priority_alpha)
            else:
                mx = ops.reference_priority_update([lev.numpy() for lev in self._levels], int(self._max_mass.numpy()[0]),
                                                   i.numpy(), p.numpy(), self.priority_alpha)
                self._max_mass.numpy()[0] = mx
        return self

    def _priority_draw(self, B, ctr, beta, advance):
        """(index, prob, weight) of a prioritized batch at Philox counter ``ctr``; beta: a value or a device scalar."""
        if isinstance(beta, torch.Tensor):
            beta_t = beta
        else:
            if self._beta[0] != float(beta):      # the device scalar follows the host value
                self._beta[0] = float(beta)
                self._beta[1].fill_(float(beta))
            beta_t = self._beta[1]
        if self.device.type == 'cuda':
            idx, _, prob, weight = ops.priority_draw(self._levels, self.capacity, self._max_mass, B, seed=self.seed,
                                                     counter=ctr, beta=beta_t, advance=advance)
            return idx, prob, weight
        idx, mass, prob = ops.reference_priority_draw([lev.numpy() for lev in self._levels], self.seed, int(ctr), B)
        weight = ops.reference_priority_weights(mass, float(beta_t[0])).astype(np.float32)
        return torch.from_numpy(idx), torch.from_numpy(prob), torch.from_numpy(weight)

    def fill_from(self, batches, max_items: int):
        """Append frames from an iterable of batch dicts (e.g. a
        ``DeviceLoader(..., decode=DecodeConfig.raw())``) until ``max_items``."""
        got = 0
        for b in batches:
            img = b[self.image_key]
            take = min(len(img), max_items - got)
            meta = {k: v[:take] for k, v in b.items()
                    if k != self.image_key and isinstance(v, (torch.Tensor, np.ndarray))}
            self.extend(img[:take], **meta)
            got += take
            if got >= max_items:
                break
        return self

    @classmethod
    def from_recordings(cls, record_path_prefix: str, device=None, capacity: Optional[int] = None,
                        image_key: str = 'image', meta_keys=('btid', 'frameid'), chunk: int = 64):
        """Load every ``{prefix}_*.btr`` recording (FileRecorder format) into a
        new buffer.  Images are located in the memory-mapped files by the
        native codec (no unpickling of pixel data) and uploaded ``chunk``
        frames at a time through pinned memory."""
        from .file import FileReader
        from .. import _native
        fnames = sorted(glob(f'{record_path_prefix}_*.btr'))
        assert fnames, f'Found no recording files with prefix {record_path_prefix}'
        spans = []
        for f in fnames:
            offs = FileReader.read_offsets(f)
            spans.append((f, offs))
        total = sum(len(o) for _, o in spans)
        buf = cls(capacity or max(1, total), device=device, image_key=image_key)
        pin = None
        stage_imgs, stage_meta = [], {k: [] for k in meta_keys}

        def flush():
            nonlocal pin
            if not stage_imgs:
                return
            arr = np.stack(stage_imgs)
            t = torch.from_numpy(arr)
            if buf.device.type == 'cuda':
                if pin is None or pin.shape[1:] != t.shape[1:] or pin.shape[0] < len(t):
                    pin = torch.empty((chunk,) + tuple(t.shape[1:]), dtype=torch.uint8).pin_memory()
                pin[:len(t)].copy_(t)
                t = pin[:len(t)]
            buf.extend(t, **{k: np.asarray(v) for k, v in stage_meta.items() if v})
            if buf.device.type == 'cuda':
                torch.cuda.current_stream(buf.device).synchronize()   # `pin` is reused
            stage_imgs.clear()
            for v in stage_meta.values():
                v.clear()

        for fname, offs in spans:
            with open(fname, 'rb') as fp, mmap.mmap(fp.fileno(), 0, access=mmap.ACCESS_READ) as mm:
                view = memoryview(mm)
                ends = list(offs[1:]) + [len(mm)]
                for o, e in zip(offs, ends):
                    msg = view[int(o):int(e)]
                    try:
                        item = _native.fast_loads(msg)
                    except ValueError:   # outside the codec's fast path
                        import pickle
                        item = pickle.loads(msg)
                    img = np.asarray(item[image_key])
                    stage_imgs.append(np.array(img, dtype=np.uint8, copy=True))
                    for k in meta_keys:
                        if k in item:
                            stage_meta[k].append(item[k])
                    del item, img, msg
                    if len(stage_imgs) == chunk:
                        flush()
                flush()
                view.release()
        return buf

    def save_recordings(self, record_path_prefix: str, files: int = 1, chunk: int = 64):
        """Write the stored frames (oldest first) as ``.btr`` recordings,
        ``{prefix}_{i:02d}.btr`` for i < ``files``: one message per frame,
        ``{image_key: u8 HxWxC, **metadata}``. The files are the format
        ``FileRecorder`` writes, so ``FileDataset`` (CPU) and
        :meth:`from_recordings` (GPU) read them back. This is how a stream
        consumed on the GPU path gets recorded."""
        from .file import FileRecorder
        n = self._size
        start = self._next if n == self.capacity else 0   # ring order: oldest first
        order = [(start + i) % self.capacity for i in range(n)]
        per = [order[i::files] for i in range(files)]
        paths = []
        for fi, idxs in enumerate(per):
            path = FileRecorder.filename(record_path_prefix, fi)
            with FileRecorder(path, max_messages=max(1, len(idxs))) as rec:
                for s in range(0, len(idxs), chunk):
                    sel = torch.as_tensor(idxs[s:s + chunk], dtype=torch.int64, device=self.device)
                    imgs = self.store.index_select(0, sel).cpu().numpy()
                    meta = {k: v.index_select(0, sel).cpu().numpy() for k, v in self.meta.items()}
                    for j in range(len(imgs)):
                        item = {self.image_key: imgs[j]}
                        for k, v in meta.items():
                            item[k] = v[j].item() if v[j].ndim == 0 else v[j]
                        rec.save(item, is_pickled=False)
            paths.append(path)
        return paths

    # -- sampling --------------------------------------------------------------
    def _fused(self, decode: DecodeConfig):
        return self.device.type == 'cuda' and not decode.colour_kernel and self.store.is_contiguous()

    def _decode(self, idx: torch.Tensor, decode: DecodeConfig):
        if self.device.type == 'cuda' and not decode.colour_kernel:
            return ops.decode_gather(self.store, idx, decode)
        imgs = self.store.index_select(0, idx)
        if self.device.type == 'cuda':
            return ops.decode(imgs, decode)
        return ops.reference_decode(imgs, decode)

    def _windows(self, B: int, crop, windows, ctr: int) -> np.ndarray:
        """int32 [B, 3] windows of a sample on the reference path: the given ones (validated),
        else what the fused kernel draws at Philox counter ``ctr`` (ops.replay_windows)."""
        H, W = self.frame_shape[:2]
        crop.check_frame(H, W)
        if windows is None:
            return ops.replay_windows(crop, H, W, B, seed=self.seed, counter=ctr)
        win = windows.detach().cpu().numpy() if isinstance(windows, torch.Tensor) else np.asarray(windows)
        if win.shape != (B, 3) or win.dtype.kind not in 'iu':
            raise ValueError(f'windows must be integers [{B}, 3] (y0, x0, mirrored)')
        ops._check_windows(win.astype(np.int64), crop, H, W)
        return np.ascontiguousarray(win, dtype=np.int32)

    @staticmethod
    def _no_resize(decode: DecodeConfig):
        if decode.resize is not None:
            raise ValueError('DeviceReplayBuffer: a resize is not supported on the replay path; '
                             'use ops.decode(store[index], cfg, window=windows)')

    def gather(self, idx: torch.Tensor, decode: DecodeConfig = DecodeConfig(), windows=None, _counter=None):
        """Decoded frames ``idx`` (device int tensor) + their metadata.  On a
        GPU: one fused launch decodes the frames and gathers every metadata
        column (``ops.replay_sample`` with given indices).

        With ``decode.crop`` the frames are decoded through windows inside
        the same launch and the batch carries ``batch['crop']`` (int32 [B, 3]:
        y0, x0, mirrored; ``ops.crop_points`` maps coordinates into them).  A
        random crop draws its windows at the buffer's Philox counter, which
        then advances by the batch size; ``windows`` ([B, 3], host values or a
        tensor; eager use only) gives them instead."""
        if self._size == 0:
            raise IndexError('empty replay buffer')
        idx = idx.to(self.device, torch.int64)
        self._no_resize(decode)
        crop = decode.crop
        if crop is None:
            if windows is not None:
                raise ValueError('crop windows given for a config without a crop')
            if self._fused(decode):
                img, idx, meta = ops.replay_sample(self.store, self._size, int(idx.numel()), decode, index=idx,
                                                   meta=self.meta)
                return {self.image_key: img, **meta, 'index': idx}
            out = {self.image_key: self._decode(idx, decode)}
            for k, v in self.meta.items():
                out[k] = v.index_select(0, idx)
            out['index'] = idx
            return out
        B = int(idx.numel())
        ctr = _counter
        if ctr is None:
            ctr = self._ctr
            if crop.kind == 'random' and windows is None:   # the windows are drawn: the counter moves on
                self._ctr += B
        if self.device.type == 'cuda':
            img, idx, meta, win = ops.replay_sample(self.store, self._size, B, decode, seed=self.seed, counter=ctr,
                                                    index=idx, meta=self.meta, windows=windows)
            return {self.image_key: img, **meta, 'index': idx, 'crop': win}
        win = self._windows(B, crop, windows, ctr)
        out = {self.image_key: ops.reference_decode(self.store.index_select(0, idx), decode, crop=win)}
        for k, v in self.meta.items():
            out[k] = v.index_select(0, idx)
        out['index'] = idx
        out['crop'] = torch.from_numpy(win).to(self.device)
        return out

    def sample(self, batch_size: int, decode: DecodeConfig = DecodeConfig(), generator=None, _counter=None):
        """Uniform random batch (with replacement).  On a GPU (no ``generator``)
        ONE fused launch draws the indices (Philox), decodes the frames and
        gathers their metadata; with a ``torch.Generator`` the indices come
        from ``torch.randint`` instead.

        With ``decode.crop`` the same launch also draws the windows
        (``batch['crop']``).  A CPU buffer then draws indices and windows with
        the numpy references of the kernel's Philox draws
        (``ops.philox_indices`` / ``ops.philox_windows``): a CPU buffer and a
        GPU buffer with the same seed and call sequence return the same
        batches.  With a ``generator`` only the indices come from it."""
        if self._size == 0:
            raise IndexError('empty replay buffer')
        self._no_resize(decode)
        if generator is None and self._fused(decode):
            ctr = _counter
            if ctr is None:
                ctr, self._ctr = self._ctr, self._ctr + batch_size
            if decode.crop is not None:
                img, idx, meta, win = ops.replay_sample(self.store, self._size, batch_size, decode, seed=self.seed,
                                                        counter=ctr, meta=self.meta)
                return {self.image_key: img, **meta, 'index': idx, 'crop': win}
            img, idx, meta = ops.replay_sample(self.store, self._size, batch_size, decode, seed=self.seed,
                                               counter=ctr, meta=self.meta)
            return {self.image_key: img, **meta, 'index': idx}
        if decode.crop is not None and generator is None and self.device.type != 'cuda':
            # the fused sample on the reference path: one counter for indices and windows
            ctr, self._ctr = self._ctr, self._ctr + batch_size
            idx = torch.from_numpy(ops.philox_indices(self.seed, ctr, batch_size, self._size))
            return self.gather(idx, decode, _counter=ctr)
        idx = torch.randint(0, self._size, (batch_size,), device=self.device, generator=generator)
        return self.gather(idx, decode)

    def graphed_sampler(self, batch_size: int, decode: DecodeConfig = DecodeConfig(), warmup: int = 3):
        """``sample(batch_size, decode)`` captured once as a HIP graph.

        A batch-8 sample is a handful of small launches (index draw, offset
        scale, the fused gather+decode, one gather per metadata key), so its
        cost is launch overhead. Replaying the captured graph issues all of
        them at once. The returned callable replays the graph and returns the
        same static output dict every time: consume (or clone) a batch before
        the next call. The number of stored frames is frozen into the graph,
        so capture again after ``extend``.
        """
        if self.device.type != 'cuda':
            return lambda: self.sample(batch_size, decode)
        # the captured sample reads its Philox counter from device memory and
        # advances it there: every replay draws new indices
        counter = torch.tensor([self._ctr], dtype=torch.int64, device=self.device)
        self._ctr += 1 << 40          # disjoint from later eager draws
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(warmup):   # allocations, LUT upload, kernel selection outside the capture
                self.sample(batch_size, decode, _counter=counter)
        torch.cuda.current_stream(self.device).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = self.sample(batch_size, decode, _counter=counter)

        def replay():
            graph.replay()
            return out
        replay.graph = graph
        return replay

    # -- frame-stacked transitions ------------------------------------------------
    def _transitions(self, B, idx, decode, stack, stride, first_key, next_keys, shared_window, _counter,
                     nstep=None, gamma=0.99, reward_key='reward', done_key=None, prioritized=False, beta=0.4):
        if self._size == 0:
            raise IndexError('empty replay buffer')
        if prioritized:
            self._need_priorities()
            if int(stride) != self.priority_stride or first_key != self.first_key:
                raise ValueError(f'the priorities are kept for stride = {self.priority_stride} and first_key = '
                                 f'{self.first_key!r} (the constructor\'s)')
            if not 1 <= B <= ops.MAX_PRIORITY_B:
                raise ValueError(f'a prioritized batch holds 1 .. {ops.MAX_PRIORITY_B} transitions')
        ops._transition_cfg(decode, 'DeviceReplayBuffer transitions')
        first = self.meta.get(first_key)
        if first is None or first.dim() != 1 or first.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f'transitions need a uint8 / bool [capacity] metadata column {first_key!r} '
                             '(episode starts): extend(frames, ..., %s=flags)' % first_key)
        next_keys = tuple(next_keys)
        for k in next_keys:
            if k not in self.meta:
                raise ValueError(f'next_keys: no metadata column {k!r}')
        stack, stride = int(stack), int(stride)
        if not 1 <= stack <= ops.MAX_STACK or B * (stack + 1) > ops.MAX_STACK_TABLE:
            raise ValueError(f'stack must lie in [1, {ops.MAX_STACK}] with batch * (stack + 1) <= {ops.MAX_STACK_TABLE}')
        if not 1 <= stride < self.capacity:
            raise ValueError('stride must lie in [1, capacity)')
        if self._size <= stride:
            raise ValueError(f'transitions need more than stride = {stride} stored frames: {self._size}')
        reward = done = None
        if nstep is not None:
            nstep, _ = ops._nstep_args(nstep, gamma)
            if B * (stack + nstep) > ops.MAX_STACK_TABLE:
                raise ValueError(f'n-step transitions need batch * (stack + nstep) <= {ops.MAX_STACK_TABLE}')
            reward = self.meta.get(reward_key)
            if reward is None or reward.dim() != 1 or reward.dtype != torch.float32:
                raise ValueError(f'n-step returns need a float32 [capacity] metadata column {reward_key!r} '
                                 '(the reward of the step taken from each frame)')
            if done_key is not None:
                done = self.meta.get(done_key)
                if done is None or done.dim() != 1 or done.dtype not in (torch.uint8, torch.bool):
                    raise ValueError(f'done_key: no uint8 / bool [capacity] metadata column {done_key!r}')
        crop = decode.crop
        ctr = _counter
        if ctr is None:
            ctr = self._ctr
            if idx is None or (crop is not None and crop.kind == 'random'):   # something is drawn
                self._ctr += B
        prio = None
        if prioritized:
            # the anchors come from the priority tree, drawn in front of the transition launch at the same
            # counter; that launch then takes them as given ones.  A device counter moves on by B once: behind
            # the transition launch if it draws windows, else in the draw.
            windows_drawn = crop is not None and crop.kind == 'random'
            idx, *prio = self._priority_draw(B, ctr, beta, advance=isinstance(ctr, torch.Tensor) and not windows_drawn)
        if self.device.type == 'cuda':
            if not self.store.is_contiguous():
                raise ValueError('transitions need a contiguous store')
            out, info = ops.replay_transitions(
                self.store, self._next, self._size, B, decode, stack=stack, stride=stride, first=first, seed=self.seed,
                counter=ctr, index=idx, meta=self.meta, next_meta={k: self.meta[k] for k in next_keys},
                shared_window=shared_window, state=self._state if isinstance(ctr, torch.Tensor) else None,
                nstep=nstep, gamma=gamma, reward=reward, done=done)
            batch = {'obs': out[0], 'next_obs': out[1], **info['meta']}
            batch.update({'next_' + k: v for k, v in info['next_meta'].items()})
            batch.update(index=info['index'], next_index=info['next_index'], valid=info['valid'])
            if crop is not None:
                batch.update(crop=info['crop'], next_crop=info['next_crop'])
            if nstep is not None:
                batch.update({k: info[k] for k in ('nstep_return', 'nstep_discount', 'nstep_steps')})
            if prio is not None:
                batch.update(prob=prio[0], weight=prio[1])
            return batch
        # the reference path: the numpy references of the kernel's draws + reference_decode
        ring = (self._next, self._size, self.capacity, stride, stack, first.numpy())
        nkw = {} if nstep is None else dict(nstep=nstep, done=None if done is None else done.numpy())
        if idx is None:
            anchor, succ, table, valid = ops.philox_transitions(self.seed, ctr, B, *ring, **nkw)
        else:
            anchor, succ, table, valid = ops.given_transitions(idx.cpu().numpy(), *ring, **nkw)
        tables = (table[:, :stack], table[:, 1:]) if nstep is None else table
        H, W = self.frame_shape[:2]
        wins = None
        if crop is not None:
            crop.check_frame(H, W)
            wins = ops.transition_windows(crop, H, W, B, seed=self.seed, counter=ctr, shared_window=shared_window)
        sides = []
        for d in (0, 1):
            planes = [ops.reference_decode(self.store.index_select(0, torch.from_numpy(tables[d][:, f].copy())), decode,
                                           crop=None if wins is None else wins[d]) for f in range(stack)]
            sides.append(torch.cat(planes, dim=1))
        anchor, succ = torch.from_numpy(anchor), torch.from_numpy(succ)
        batch = {'obs': sides[0], 'next_obs': sides[1]}
        batch.update({k: v.index_select(0, anchor) for k, v in self.meta.items()})
        batch.update({'next_' + k: self.meta[k].index_select(0, succ) for k in next_keys})
        batch.update(index=anchor, next_index=succ, valid=torch.from_numpy(valid))
        if wins is not None:
            batch.update(crop=torch.from_numpy(wins[0].copy()), next_crop=torch.from_numpy(wins[1].copy()))
        if nstep is not None:
            _, steps, ret, disc = ops.nstep_transitions(anchor.numpy(), valid, self._next, self._size, self.capacity,
                                                        stride, nstep, gamma, reward.numpy(), first.numpy(),
                                                        done=nkw['done'])
            batch.update(nstep_return=torch.from_numpy(ret), nstep_discount=torch.from_numpy(disc),
                         nstep_steps=torch.from_numpy(steps))
        if prio is not None:
            batch.update(prob=prio[0], weight=prio[1])
        return batch

    def sample_transitions(self, batch_size: int, decode: DecodeConfig = DecodeConfig(), stack: int = 1,
                           stride: int = 1, first_key: str = 'first', next_keys=(), shared_window: bool = False,
                           _counter=None, nstep=None, gamma: float = 0.99, reward_key: str = 'reward', done_key=None,
                           prioritized: bool = False, beta=0.4):
        """A batch of frame-stacked transitions out of the frame-once store.

        Storage convention (nothing about ``extend`` changes): an RL loop
        appends ``stride`` frames per environment step, one per environment
        and always in the same order (``stride = len(vec_env)``, 1 for a single
        environment), so the same environment's previous step of ring slot s
        is ``(s - stride) mod capacity``.  The one-byte metadata column
        ``first_key`` (uint8 / bool) is non-zero where a frame is the first
        observation after a reset; terminal observations are stored like any
        other frame, and the frame after one is a ``first`` frame.

        Returns ``obs`` and ``next_obs`` (``[B, stack * Cout, h, w]``, NCHW:
        the last ``stack`` frames ending at the anchor, resp. one step later,
        oldest first along channels; a stack that reaches back over an
        episode start, or past the oldest stored frame, repeats that frame),
        every metadata column at the anchor (action, reward, done ...),
        ``'next_' + key`` at the successor for ``next_keys``, ``index`` /
        ``next_index`` (the anchor's and the successor's slot) and ``valid``.
        No transition crosses a reset: an anchor whose successor is a
        ``first`` frame is redrawn, up to 16 times (``ops.philox_transitions``);
        ``valid`` is False for an image that found none (its ``next_index`` is
        its ``index``): mask it out of the loss.

        With ``decode.crop`` one window serves all frames of a stack and the
        two stacks take independent windows (``crop`` / ``next_crop``), as DrQ
        augments them, unless ``shared_window``.  On a GPU all of it is ONE
        launch (``ops.replay_transitions``); a CPU buffer with the same seed
        and call sequence returns the same batches.  Colour-kernel, resize
        and NHWC configs raise ``ValueError`` (NHWC: channel-stacked
        channels-last output needs another store pattern).

        ``nstep`` = n in [1, 16] makes them n-step transitions, still in the
        one launch.  Storage convention: the float32 column ``reward_key``
        holds at each frame the reward of the step taken FROM it, and the
        optional uint8 / bool column ``done_key`` is non-zero where that step
        terminated the episode; terminal observations are stored as frames
        (the frame after one is a ``first`` frame).  From each anchor the
        walk takes m <= n steps, stopping at the episode's end and at the
        newest stored step.  ``next_obs``, ``next_index`` and the
        ``'next_' + key`` columns are then taken m steps after the anchor,
        and the batch also holds ``nstep_return`` (float32: ``r_t + gamma
        r_{t+1} + ... + gamma^(m-1) r_{t+m-1}``), ``nstep_discount``
        (float32: ``gamma^m``, the factor of the bootstrap term) and
        ``nstep_steps`` (int32: m; 0 where ``valid`` is False).  With a done
        column ``nstep_discount`` is 0 after a termination: the target is
        ``nstep_return + nstep_discount * Q(next_obs)`` with no further
        mask.  Without one the walk merely truncates at the episode's end
        (time-limit semantics: the last observation still bootstraps).
        ``index`` and ``valid`` are the 1-step ones whatever ``nstep`` is;
        ``ops.nstep_transitions`` is the reference.

        ``prioritized`` (a buffer built with ``priority_alpha``): the anchors
        are drawn in proportion to their priority instead -- stratified, one
        per ``batch_size``-th of the total mass, by a small launch in front
        of the transition launch (``ops.priority_draw``), which then takes
        them as given anchors at the same counter: windows, stacks and n-step
        returns are what :meth:`gather_transitions` gives for them.  The
        batch gains ``prob`` (float32: mass / total mass) and ``weight``
        (float32: the importance-sampling weight ``(N prob)^-beta`` divided
        by the batch maximum).  New transitions enter with the largest
        priority written so far; :meth:`update_priorities` writes TD errors
        back.  ``valid`` is all True unless no stored transition is eligible.
        The Philox counter advances by ``batch_size`` per sample."""
        return self._transitions(int(batch_size), None, decode, stack, stride, first_key, next_keys, shared_window,
                                 _counter, nstep, gamma, reward_key, done_key, prioritized=bool(prioritized), beta=beta)

    def gather_transitions(self, idx: torch.Tensor, decode: DecodeConfig = DecodeConfig(), stack: int = 1,
                           stride: int = 1, first_key: str = 'first', next_keys=(), shared_window: bool = False,
                           _counter=None, nstep=None, gamma: float = 0.99, reward_key: str = 'reward', done_key=None):
        """:meth:`sample_transitions` at given anchors ``idx`` (slots).
        ``valid`` is False where the anchor is among the newest ``stride``
        frames, is not stored, or its successor is a ``first`` frame.  A random
        crop draws its windows at the buffer's Philox counter."""
        idx = idx.to(self.device, torch.int64).reshape(-1)
        return self._transitions(int(idx.numel()), idx, decode, stack, stride, first_key, next_keys, shared_window,
                                 _counter, nstep, gamma, reward_key, done_key)

    def graphed_transition_sampler(self, batch_size: int, decode: DecodeConfig = DecodeConfig(), stack: int = 1,
                                   stride: int = 1, first_key: str = 'first', next_keys=(),
                                   shared_window: bool = False, warmup: int = 3, nstep=None, gamma: float = 0.99,
                                   reward_key: str = 'reward', done_key=None, prioritized: bool = False, beta=0.4):
        """:meth:`sample_transitions` captured once as a HIP graph.  The
        Philox counter lives in device memory (as in :meth:`graphed_sampler`)
        and so does the ring state: the kernel reads ``(head, size)`` from a
        device tensor that ``extend`` refreshes once such a sampler exists, so
        ONE capture serves a buffer that grows every environment step.  The
        returned callable replays the graph and returns the same static
        output dict every time.  ``prioritized``: both launches are captured;
        the callable's ``.beta`` is the device float32 scalar the draw reads
        (``sampler.beta.fill_(b)`` anneals it between replays)."""
        kw = dict(stack=stack, stride=stride, first_key=first_key, next_keys=next_keys, shared_window=shared_window,
                  nstep=nstep, gamma=gamma, reward_key=reward_key, done_key=done_key)
        beta_t = None
        if prioritized:
            self._need_priorities()
            beta_t = torch.full((1,), float(beta), dtype=torch.float32, device=self.device)
            kw.update(prioritized=True, beta=beta_t)
        if self.device.type != 'cuda':
            def sample():
                return self.sample_transitions(batch_size, decode, **kw)
            sample.beta = beta_t
            return sample
        if self._state is None:
            self._state = torch.tensor([self._next, self._size], dtype=torch.int64, device=self.device)
        counter = torch.tensor([self._ctr], dtype=torch.int64, device=self.device)
        self._ctr += 1 << 40          # disjoint from later eager draws
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self.sample_transitions(batch_size, decode, _counter=counter, **kw)
        torch.cuda.current_stream(self.device).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = self.sample_transitions(batch_size, decode, _counter=counter, **kw)

        def replay():
            graph.replay()
            return out
        replay.graph = graph
        replay.counter = counter
        replay.beta = beta_t
        return replay

    def batches(self, batch_size: int, decode: DecodeConfig = DecodeConfig(), shuffle: bool = True,
                drop_last: bool = True, epochs: int = 1, generator=None) -> Iterator[dict]:
        """Epochs over the stored frames (a device-side permutation each epoch)."""
        for _ in range(epochs):
            order = (torch.randperm(self._size, device=self.device, generator=generator) if shuffle
                     else torch.arange(self._size, device=self.device))
            stop = self._size - (self._size % batch_size if drop_last else 0)
            for s in range(0, stop, batch_size):
                yield self.gather(order[s:s + batch_size], decode)
