"""Crop, mirror and replicate pad inside the fused replay sample
(csrc/gpu/kernels.hip ``replay_sample_crop``) and through ``DeviceReplayBuffer``.

Kernel: every launch goes into SENTINEL-filled buffers (tests/decode_oracle.py)
and the WHOLE image buffer -- 256-byte guards included -- is compared bit for bit
(bf16 / f16 as raw bytes) with the CPU ``ops.reference_decode(store[index], cfg,
crop=windows)``; the index, window and metadata outputs sit between guards too.
"""
import dataclasses

import numpy as np
import pytest
import torch

from decode_oracle import ELEM, GUARD, SENTINEL, dense_dst, frames
from blendtorch import ops
from blendtorch.btt.replay import DeviceReplayBuffer
from blendtorch.ops import Crop, DecodeConfig

pytestmark = pytest.mark.gpu

DTYPES = ('float32', 'bfloat16', 'float16', 'uint8')
LAYOUTS = ('nchw', 'nhwc')
PPT = {'float32': 4, 'bfloat16': 8, 'float16': 8, 'uint8': 16}
CMAPS = {3: ['rgb', 'bgr'], 4: ['rgb', 'bgr', 'rgba', (3,)]}
SEED, CTR = 0x9E3779B97F4A7C15, (3 << 32) | 77
MAX_REPLAY_B = 1024       # kernels.h: kMaxReplayB


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    ops.hip_ext()  # must load: no silent fallback
    return torch.device('cuda', 0)


def _vcfg(channels, dtype, layout, crop, flip=False):
    """Gamma + normalisation (u8: gamma only), as test_gpu_crop._vcfg."""
    if dtype == 'uint8':
        return DecodeConfig(channels=channels, gamma=2.2, dtype='uint8', layout=layout, crop=crop, flip=flip)
    return DecodeConfig.densityopt(channels=channels, gamma=2.2, dtype=dtype, layout=layout, crop=crop, flip=flip)


def _bytes(t):
    return t.contiguous().view(torch.uint8).reshape(t.shape[0], -1).numpy()


class _Launch:
    """One replay_sample launch with a crop on guard-filled buffers, through the binding.

    index / win: given indices / windows, or None: drawn at (SEED, CTR).  shift: byte shift of the output base."""

    def __init__(self, store, cfg, B, index=None, win=None, shift=0, max_grid=0, cmap=None):
        self.store, self.cfg, self.B, self.shift, self.max_grid = store, cfg, B, shift, max_grid
        self.N, self.H, self.W, self.Cin = store.shape
        self.crop = cfg.crop
        self.key = (SEED + self.crop.seed) & (2 ** 64 - 1)
        self.index = None if index is None else [int(v) for v in index]
        self.win = None if win is None else [tuple(int(v) for v in r) for r in win]
        self.cmap = cfg.cmap if cmap is None else cmap
        h, w = self.crop.size
        self.img_bytes = h * w * cfg.cout * ELEM[cfg.dtype]
        self.bufs, self.dst = dense_dst(B, self.img_bytes, shift=shift)
        rng = np.random.default_rng(self.N + B)
        self.metas = [rng.normal(size=(self.N, 3)).astype(np.float32),
                      rng.integers(0, 256, size=(self.N, 5), dtype=np.uint8)]

    def want_index(self):
        return np.asarray(self.index) if self.index is not None else ops.philox_indices(SEED, CTR, self.B, self.N)

    def want_win(self):
        if self.win is not None:
            return np.asarray(self.win, np.int32)
        return ops.replay_windows(self.crop, self.H, self.W, self.B, seed=SEED, counter=CTR)

    def expected(self):
        x = torch.from_numpy(self.store[self.want_index()])
        ref = _bytes(ops.reference_decode(x, self.cfg, crop=self.want_win()))
        buf = np.full(self.bufs[0], SENTINEL, np.uint8)
        for b, (_, off) in enumerate(self.dst):
            assert off >= GUARD // 2 and off + self.img_bytes <= len(buf) - GUARD // 2
            buf[off:off + self.img_bytes] = ref[b]
        return buf

    def run(self, dev, B=None, crop_size=None):
        ext = ops.hip_ext()
        B = self.B if B is None else B
        store = torch.from_numpy(self.store).to(dev)
        out = torch.full((self.bufs[0],), SENTINEL, dtype=torch.uint8, device=dev)
        nbytes = [12, 5]
        msrc = [torch.from_numpy(m).to(dev) for m in self.metas]
        mdst = [torch.full((2 * GUARD + self.B * nb,), SENTINEL, dtype=torch.uint8, device=dev) for nb in nbytes]
        idx_out = torch.full((self.B + 64,), -1, dtype=torch.int64, device=dev)
        crop_out = torch.full((3 * self.B + 64,), -7, dtype=torch.int32, device=dev)
        idx_in = torch.tensor(self.index, dtype=torch.int64, device=dev) if self.index is not None else None
        win_in = torch.tensor(self.win, dtype=torch.int32, device=dev).reshape(-1) if self.win is not None else None
        c = self.crop
        try:
            ext.replay_sample(store.data_ptr(), self.N, out.data_ptr() + self.dst[0][1],
                              ops.device_lut(self.cfg, dev).data_ptr(), B, self.H, self.W, self.Cin, self.cfg.cout,
                              self.cmap, int(self.cfg.flip), ops.OUT_DTYPES[self.cfg.dtype],
                              ops.LAYOUTS[self.cfg.layout], SEED, 0, CTR, idx_in.data_ptr() if idx_in is not None else 0,
                              idx_out.data_ptr(), [m.data_ptr() for m in msrc], [m.data_ptr() + GUARD for m in mdst],
                              nbytes, ops._stream(dev), ops.table_only(self.cfg, dev), max_grid=self.max_grid,
                              crop_size=list(c.size if crop_size is None else crop_size), crop_mode=c.mode,
                              crop_origin=list(c.origin or ()), crop_pad=c.pad, mirror=c.mirror, x_align=c.x_align,
                              window_key=self.key, windows_in=win_in.data_ptr() if win_in is not None else 0,
                              crop_out=crop_out.data_ptr())
        finally:
            torch.cuda.synchronize()
        return (out.cpu().numpy(), idx_out.cpu().numpy(), crop_out.cpu().numpy(), [m.cpu().numpy() for m in mdst])

    def check(self, dev, what=''):
        out, idx, win, mdst = self.run(dev)
        where = f'{what} {self.cfg.channels} Cin {self.Cin} {self.cfg.dtype} {self.cfg.layout} windows {self.want_win().tolist()}'
        want = self.want_index()
        assert np.array_equal(idx[:self.B], want) and (idx[self.B:] == -1).all(), where
        assert np.array_equal(win[:3 * self.B].reshape(-1, 3), self.want_win()) and (win[3 * self.B:] == -7).all(), where
        exp = self.expected()
        if not np.array_equal(out, exp):
            bad = np.flatnonzero(out != exp)
            img = [b for b, (_, off) in enumerate(self.dst) if off <= bad[0] < off + self.img_bytes]
            raise AssertionError(f'{where}: {len(bad)} bytes differ, first at {bad[0]} '
                                 f'({"image %d + %d" % (img[0], bad[0] - self.dst[img[0]][1]) if img else "GUARD"}): '
                                 f'got {out[bad[0]]:#x}, expected {exp[bad[0]]:#x}')
        for got, m in zip(mdst, self.metas):
            row = m[want].reshape(self.B, -1).view(np.uint8).reshape(-1)
            assert np.array_equal(got[GUARD:-GUARD], row), where
            assert (got[:GUARD] == SENTINEL).all() and (got[-GUARD:] == SENTINEL).all(), where


# the origin classes of test_gpu_crop.W416 (window 4 x 16 in 7 x 32 frames): x0 over every residue of
# 3 * x0 mod 4, the first and last legal columns, y0 the first and last rows, every x0 mirrored and not
W416 = [
    [(0, 0, 0), (3, 1, 1), (0, 2, 0)],
    [(3, 3, 1), (0, 5, 0), (3, 16, 1)],
    [(3, 0, 1), (0, 1, 0), (3, 2, 1)],
    [(0, 3, 0), (3, 5, 1), (0, 16, 0)],
]
INDEX = [5, 0, 5]


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_given_window_matrix(dev, dtype, layout):
    """6 frames of 7 x 32, indices with a repeat: the 4 x 16 window at every origin class (once upside down),
    the 3 x 12 window (vector for f32 only) and an output base off by one element (scalar)."""
    es = ELEM[dtype]
    assert {(3 * x0) % 4 for w in W416 for _, x0, _ in w} == {0, 1, 2, 3}
    assert {(x0, m) for w in W416 for _, x0, m in w} >= {(0, 0), (0, 1), (16, 0), (16, 1)}
    for Cin in (3, 4):
        store = frames(6, 7, 32, Cin, seed=100 + Cin)
        for ch in CMAPS[Cin]:
            cfg = _vcfg(ch, dtype, layout, Crop((4, 16)))
            for i, win in enumerate(W416):
                _Launch(store, cfg, 3, INDEX, win).check(dev, f'4x16 #{i}')
            _Launch(store, dataclasses.replace(cfg, flip=True), 3, INDEX, W416[1]).check(dev, '4x16 flip_all')
            small = _vcfg(ch, dtype, layout, Crop((3, 12)))
            assert (12 % PPT[dtype] == 0) == (dtype == 'float32')
            _Launch(store, small, 3, INDEX, [(4, 20, 1), (0, 0, 0), (2, 7, 1)]).check(dev, '3x12')
            _Launch(store, cfg, 3, INDEX, [(0, 2, 1), (3, 16, 0), (2, 3, 1)], shift=es).check(dev, 'dst + 1 element')


def _straddles(win, w, W, ppt):
    """Which kinds of pixel groups the windows hold: a group's first source column is x0 + j (x0 + w - ppt - j
    mirrored: the same set), j a multiple of ppt."""
    kinds = set()
    for _, x0, _ in win:
        for j in range(0, w, ppt):
            xs = x0 + j
            kinds.add('inside' if xs >= 0 and xs + ppt <= W else ('left' if xs < 0 else 'right'))
    return kinds


PAD_FULL = [(-3, -3, 0), (3, 3, 1), (0, -1, 1), (-2, 2, 0)]
PAD_416 = [(-2, -2, 0), (5, 32 + 2 - 16, 1), (0, -2, 1), (3, 32 + 2 - 16, 0)]


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_pad_matrix(dev, dtype, layout):
    """Windows that leave the frame: 7 x 32 with pad 3 and 4 x 16 with pad 2, on every side and at corners."""
    for ppt in (4, 8, 16):
        assert _straddles(PAD_FULL, 32, 32, ppt) == {'left', 'right', 'inside'}
        assert _straddles(PAD_416, 16, 32, ppt) >= ({'left', 'right', 'inside'} if ppt < 16 else {'left', 'right'})
    for Cin in (3, 4):
        store = frames(6, 7, 32, Cin, seed=400 + Cin)
        for ch in CMAPS[Cin]:
            full = _vcfg(ch, dtype, layout, Crop((7, 32), pad=3))
            _Launch(store, full, 4, [5, 0, 5, 2], PAD_FULL).check(dev, '7x32 pad 3')
            part = _vcfg(ch, dtype, layout, Crop((4, 16), pad=2))
            _Launch(store, part, 4, [1, 1, 4, 3], PAD_416).check(dev, '4x16 pad 2')
        _Launch(store, _vcfg('bgr', dtype, layout, Crop((7, 32), pad=3), flip=True), 4, [5, 0, 5, 2],
                PAD_FULL).check(dev, '7x32 pad 3 flip_all')
        _Launch(store, _vcfg('rgb', dtype, layout, Crop((7, 32), pad=3)), 4, [5, 0, 5, 2], PAD_FULL,
                shift=ELEM[dtype]).check(dev, '7x32 pad 3, scalar')
        # a window larger than the frame: every border pixel replicated
        _Launch(store, _vcfg('rgb', dtype, layout, Crop((7 + 6, 32 + 16), pad=8)), 2, [3, 0],
                [(-8, -8, 1), (-2, -8, 0)]).check(dev, '13x48 of 7x32')


DRAW_CROPS = [Crop((4, 16), mirror=0.5, seed=1), Crop((7, 32), pad=3, mirror=0.5, seed=2),
              Crop((3, 12), mirror=0.5, seed=3), Crop((4, 16), mirror=0.5, x_align=4, seed=1),
              Crop((4, 16), mode='center', x_align=4), Crop((3, 8), origin=(4, 21))]


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_drawn_windows(dev, dtype, layout):
    """windows_in null: indices and windows from the device's Philox draws (or the centre / fixed window)."""
    B = 12
    for crop in DRAW_CROPS:
        ref = ops.replay_windows(crop, 7, 32, B, seed=SEED, counter=CTR)
        if crop.kind == 'random':
            assert set(ref[:, 2]) == {0, 1}
            assert len(set(ref[:, 1] % 4)) >= (3 if crop.x_align == 1 else 1), ref[:, 1]
        for Cin, ch in ((3, 'bgr'), (4, 'rgba')):
            store = frames(6, 7, 32, Cin, seed=500 + Cin)
            _Launch(store, _vcfg(ch, dtype, layout, crop), B).check(dev, f'drawn {crop}')
    # drawn windows for given indices: the counter is read even with index_in
    store = frames(6, 7, 32, 4, seed=504)
    _Launch(store, _vcfg('rgb', dtype, layout, DRAW_CROPS[1]), 5, index=[5, 0, 5, 2, 2]).check(dev, 'given index')
    # table-mode value table (no normalisation): the kernels' table-only instantiations
    tab = DecodeConfig.unit(channels='rgb', gamma=2.2, dtype=dtype, layout=layout, crop=DRAW_CROPS[1]) \
        if dtype != 'uint8' else DecodeConfig(channels='rgb', gamma=2.2, dtype=dtype, layout=layout, crop=DRAW_CROPS[1])
    _Launch(store, tab, B).check(dev, 'table mode')
    _Launch(store, dataclasses.replace(tab, crop=DRAW_CROPS[0]), B).check(dev, 'table mode')


@pytest.mark.parametrize('dtype,layout,Cin,ch', [('float32', 'nchw', 3, 'bgr'), ('bfloat16', 'nhwc', 4, 'rgba'),
                                                ('uint8', 'nhwc', 4, 'rgb'), ('float16', 'nchw', 3, 'rgb')])
def test_grid_stride_loop(dev, dtype, layout, Cin, ch):
    """One block (max_grid = 1) over 3 windows of 16 x 64 in 20 x 96 frames, with and without a pad."""
    assert 3 * 16 * 64 // PPT[dtype] >= 192 and 3 * 16 * 64 // 4 > 256
    store = frames(4, 20, 96, Cin, seed=300 + Cin)
    _Launch(store, _vcfg(ch, dtype, layout, Crop((16, 64))), 3, [3, 0, 3], [(4, 32, 1), (0, 0, 0), (3, 17, 1)],
            max_grid=1).check(dev, 'grid 1')
    _Launch(store, _vcfg(ch, dtype, layout, Crop((16, 64), mirror=0.5, pad=5)), 3, max_grid=1).check(dev, 'grid 1 drawn')
    _Launch(store, _vcfg(ch, dtype, layout, Crop((16, 64), pad=5)), 3, [1, 2, 1], [(-5, -5, 1), (9, 37, 0), (0, 33, 1)],
            max_grid=1, shift=ELEM[dtype]).check(dev, 'grid 1 scalar')


def test_more_images_than_lanes(dev):
    """B = 300 windows of 2 x 16 in 3 x 20 frames: the prologue's per-image loop strides past 256 lanes."""
    store = frames(9, 3, 20, 4, seed=31, ramp=False)
    for dtype, layout in (('float32', 'nchw'), ('uint8', 'nhwc')):
        crop = Crop((2, 16), mirror=0.5, pad=1, seed=8)
        ref = ops.philox_windows(SEED, CTR, 300, crop, 3, 20)
        assert not np.array_equal(ref[:44], ref[256:]) and set(ref[256:, 2]) == {0, 1}
        _Launch(store, _vcfg('rgba', dtype, layout, crop), 300).check(dev, 'B 300')
        _Launch(store, _vcfg('rgba', dtype, layout, crop), 300, max_grid=1).check(dev, 'B 300 one block')


@pytest.mark.parametrize('what', ['window > padded frame', 'B = kMaxReplayB + 1', 'bad channel map', 'pad with x_align'])
def test_rejected_on_the_host_before_any_launch(dev, what):
    store = frames(6, 7, 32, 3, seed=1)
    cfg = _vcfg('rgb', 'float32', 'nchw', Crop((4, 16), pad=1))
    l = _Launch(store, cfg, 3, INDEX, [(3, 16, 0), (-1, -1, 1), (0, 0, 1)])
    kw = {}
    if what == 'window > padded frame':
        kw = dict(crop_size=[7 + 2 + 1, 16])
    elif what == 'B = kMaxReplayB + 1':
        # (no buffer of that size exists: a launch would write far past the guards)
        kw = dict(B=MAX_REPLAY_B + 1)
    elif what == 'bad channel map':
        l = _Launch(store, cfg, 3, INDEX, l.win, cmap=[0, 3, 1])
    else:
        l.crop = Crop((4, 16), x_align=4)               # a legal Crop ...
        object.__setattr__(l.crop, 'pad', 1)            # ... made illegal behind the dataclass's back
    res = None
    with pytest.raises(RuntimeError, match='invalid'):
        res = l.run(dev, **kw)
    assert res is None
    # nothing was written: the same rejected call on buffers we keep
    ext = ops.hip_ext()
    out = torch.full((l.bufs[0],), SENTINEL, dtype=torch.uint8, device=dev)
    idx_out = torch.full((16,), -1, dtype=torch.int64, device=dev)
    crop_out = torch.full((48,), -7, dtype=torch.int32, device=dev)
    st = torch.from_numpy(store).to(dev)
    c = l.crop
    with pytest.raises(RuntimeError, match='invalid'):
        ext.replay_sample(st.data_ptr(), 6, out.data_ptr() + GUARD, ops.device_lut(cfg, dev).data_ptr(),
                          kw.get('B', 3), 7, 32, 3, 3, l.cmap, 0, 0, 0, SEED, 0, CTR, 0, idx_out.data_ptr(), [], [], [],
                          ops._stream(dev), 0, crop_size=kw.get('crop_size', list(c.size)), crop_mode='random',
                          crop_pad=c.pad, x_align=c.x_align, window_key=1, crop_out=crop_out.data_ptr())
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((idx_out == -1).all()) and bool((crop_out == -7).all())
    # and the well-formed launch runs
    _Launch(store, cfg, 3, INDEX, [(3, 16, 0), (-1, -1, 1), (0, 0, 1)]).check(dev, 'legal')


# ---- ops.replay_sample and DeviceReplayBuffer ---------------------------------------------------------------------

def test_ops_replay_sample_with_and_without_a_crop(dev):
    """Without a crop: the 3-tuple, and indices and bytes identical to a direct binding call made before and
    after a cropped call (no state shared between the two paths)."""
    N, H, W = 9, 20, 96
    store_np = frames(N, H, W, 4, seed=12)
    store = torch.from_numpy(store_np).to(dev)
    plain = DecodeConfig.unit(channels='rgb', gamma=2.2)
    ext = ops.hip_ext()

    def direct():
        out = torch.empty(plain.out_shape(5, H, W), dtype=torch.float32, device=dev)
        idx = torch.empty(5, dtype=torch.int64, device=dev)
        ext.replay_sample(store.data_ptr(), N, out.data_ptr(), ops.device_lut(plain, dev).data_ptr(), 5, H, W, 4, 3,
                          plain.cmap, 0, 0, 0, SEED, 0, CTR, 0, idx.data_ptr(), [], [], [], ops._stream(dev),
                          ops.table_only(plain, dev))
        torch.cuda.synchronize()
        return out.cpu(), idx.cpu()

    before = direct()
    res = ops.replay_sample(store, N, 5, plain, seed=SEED, counter=CTR)
    assert len(res) == 3
    crop = Crop((8, 32), mirror=0.5, pad=4, seed=5)
    cfg = dataclasses.replace(plain, crop=crop)
    meta = {'frameid': torch.arange(N, device=dev) * 3}
    img, idx, mo, win = ops.replay_sample(store, N, 5, cfg, seed=SEED, counter=CTR, meta=meta)
    after = direct()
    for a in (after, (res[0].cpu(), res[1].cpu())):
        assert torch.equal(a[0], before[0]) and torch.equal(a[1], before[1])
    assert np.array_equal(before[1].numpy(), ops.philox_indices(SEED, CTR, 5, N))
    # the cropped call: the same indices, the reference windows, the reference images
    assert torch.equal(idx.cpu(), before[1]) and torch.equal(mo['frameid'].cpu(), before[1] * 3)
    assert win.dtype == torch.int32 and np.array_equal(win.cpu().numpy(), ops.philox_windows(SEED, CTR, 5, crop, H, W))
    assert img.shape == (5, 3, 8, 32)
    assert torch.equal(img.cpu(), ops.reference_decode(torch.from_numpy(store_np)[before[1]], cfg, crop=win.cpu()))
    # a device counter advances by B behind a cropped launch, also with given indices and a random crop
    ctr = torch.tensor([CTR], dtype=torch.int64, device=dev)
    ops.replay_sample(store, N, 5, cfg, seed=SEED, counter=ctr)
    assert int(ctr) == CTR + 5
    _, _, _, w2 = ops.replay_sample(store, N, 3, cfg, seed=SEED, counter=ctr, index=torch.tensor([1, 1, 8]))
    assert int(ctr) == CTR + 8 and np.array_equal(w2.cpu().numpy(), ops.philox_windows(SEED, CTR + 5, 3, crop, H, W))
    fixed = dataclasses.replace(plain, crop=Crop((8, 32), mode='center'))
    ops.replay_sample(store, N, 3, fixed, seed=SEED, counter=ctr, index=torch.tensor([1, 1, 8]))
    assert int(ctr) == CTR + 8                          # nothing drawn: nothing advances
    # given windows: verbatim, validated on the host
    given = [[-4, -4, 1], [16, 68, 0], [0, 0, 0]]
    img, idx, _, win = ops.replay_sample(store, N, 3, cfg, index=torch.tensor([1, 1, 8]), windows=given)
    assert win.cpu().tolist() == given
    assert torch.equal(img.cpu(), ops.reference_decode(torch.from_numpy(store_np)[[1, 1, 8]], cfg, crop=given))
    for bad in ([[-5, 0, 0]] + given[1:], [[0, 69, 0]] + given[1:], [[0, 0, 2]] + given[1:], given[:2]):
        with pytest.raises(ValueError):
            ops.replay_sample(store, N, 3, cfg, index=torch.tensor([1, 1, 8]), windows=bad)
    with pytest.raises(ValueError):
        ops.replay_sample(store, N, 3, plain, index=torch.tensor([1, 1, 8]), windows=given)
    with pytest.raises(ValueError):
        ops.replay_sample(store, N, 3, cfg, index=torch.tensor([1, 1, 8]))       # drawn windows need the counter


BUF_CFGS = [
    DecodeConfig.unit(channels='rgb', gamma=2.2, crop=Crop((8, 32), mirror=0.5, seed=4)),
    DecodeConfig.densityopt(channels='bgr', dtype='bfloat16', layout='nhwc', crop=Crop((20, 96), pad=4, mirror=0.5)),
    DecodeConfig.unit(channels='rgba', dtype='float16', crop=Crop((7, 30), mode='center')),
]


def _buffers(dev, seed=321):
    f = frames(9, 20, 96, 4, seed=44)
    rng = np.random.default_rng(3)
    meta = dict(frameid=np.arange(9) * 7, xy=rng.normal(size=(9, 2)).astype(np.float32))
    out = []
    for d in ('cpu', dev):
        rb = DeviceReplayBuffer(9, device=d, seed=seed)
        rb.extend(f, **meta)
        out.append(rb)
    return out


def _same(a, b):
    assert set(a) == set(b) and 'crop' in a
    assert a['image'].shape == b['image'].shape and a['image'].dtype == b['image'].dtype
    assert torch.equal(a['image'].view(torch.uint8), b['image'].cpu().view(torch.uint8))
    for k in a:
        if k != 'image':
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k].cpu()), k


@pytest.mark.parametrize('cfg', BUF_CFGS, ids=['f32-crop', 'bf16-shift', 'f16-center'])
def test_gpu_buffer_equals_cpu_buffer(dev, cfg):
    cpu, gpu = _buffers(dev)
    for _ in range(2):
        _same(cpu.sample(5, cfg), gpu.sample(5, cfg))
    idx = torch.tensor([8, 0, 8, 3])
    _same(cpu.gather(idx, cfg), gpu.gather(idx.to(dev), cfg))
    assert cpu._ctr == gpu._ctr == 10 + (4 if cfg.crop.kind == 'random' else 0)
    for a, b in zip(cpu.batches(4, cfg, shuffle=False, drop_last=False), gpu.batches(4, cfg, shuffle=False, drop_last=False)):
        _same(a, b)
    if cfg.crop.pad:
        win = [[-4, -4, 1], [4, 4, 0], [0, -3, 1], [2, 0, 0]]
        a, b = cpu.gather(idx, cfg, windows=win), gpu.gather(idx.to(dev), cfg, windows=torch.tensor(win, device=dev))
        assert a['crop'].tolist() == win
        _same(a, b)
        with pytest.raises(ValueError):
            gpu.gather(idx.to(dev), cfg, windows=[[-5, 0, 0]] + win[1:])
    assert cpu._ctr == gpu._ctr
    # a torch.Generator draws the indices; the windows stay the buffer's Philox draw
    c0 = gpu._ctr
    b = gpu.sample(4, cfg, generator=torch.Generator(device=dev).manual_seed(1))
    want = ops.replay_windows(cfg.crop, 20, 96, 4, seed=gpu.seed, counter=c0)
    assert np.array_equal(b['crop'].cpu().numpy(), want)
    _same(cpu.gather(b['index'].cpu(), cfg, windows=want), b)


def test_graphed_sampler_draws_fresh_windows(dev, monkeypatch):
    cfg = BUF_CFGS[0]
    cpu, gpu = _buffers(dev, seed=99)
    c0 = gpu._ctr
    sampler = gpu.graphed_sampler(4, cfg, warmup=3)
    c = c0 + 3 * 4                                      # the warm-up samples moved the device counter
    seen = []
    for k in range(3):
        b = sampler()
        torch.cuda.synchronize()
        idx = ops.philox_indices(gpu.seed, c + 4 * k, 4, 9)
        win = ops.philox_windows(gpu.seed, c + 4 * k, 4, cfg.crop, 20, 96)
        assert np.array_equal(b['index'].cpu().numpy(), idx), k
        assert np.array_equal(b['crop'].cpu().numpy(), win), k
        ref = ops.reference_decode(cpu.store[torch.from_numpy(idx)], cfg, crop=win)
        assert torch.equal(b['image'].cpu(), ref), k
        assert torch.equal(b['frameid'].cpu(), cpu.meta['frameid'][torch.from_numpy(idx)])
        seen.append(win.tolist())
    assert seen[0] != seen[1] != seen[2]
    # given windows come from the host: refused while a capture is running
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    with pytest.raises(RuntimeError, match='capture'):
        gpu.gather(torch.arange(4, device=dev), cfg, windows=[[0, 0, 0]] * 4)
