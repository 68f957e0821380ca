"""Resized crop inside the fused decode (csrc/gpu/kernels.hip ``decode_resize``)
and through the stream loader.

Kernel: as tests/test_gpu_crop.py -- every launch is compared bit for bit (bf16 /
f16 as raw bits) over its WHOLE destination buffers, the 256-byte guards of
sentinel bytes before, between and behind the images included, with the CPU
``ops.reference_decode(..., window=)``.  Buffers and frames come from
tests/decode_oracle.py.

Loader: stamped 64x32 cubesim frames of one fixed pose, batch 4, 10 batches, one
producer (arrival order = draw order), as tests/test_gpu_crop.py.
"""
import dataclasses
import struct

import numpy as np
import pytest
import torch

from decode_oracle import ELEM, GUARD, SENTINEL, dense_dst, frames, scattered_dst
from blendtorch import btt, ops
from blendtorch.btt.gpu import DeviceLoader
from blendtorch.ops import Crop, DecodeConfig, ResizedCrop
from blendtorch.transport import shm, zmq

pytestmark = pytest.mark.gpu

DTYPES = ('float32', 'bfloat16', 'float16', 'uint8')
LAYOUTS = ('nchw', 'nhwc')
PPT = {'float32': 4, 'bfloat16': 8, 'float16': 8, 'uint8': 16}
CMAPS = {3: ['rgb', 'bgr'], 4: ['rgb', 'bgr', 'rgba', (3,)]}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    ops.hip_ext()  # must load: no silent fallback
    return torch.device('cuda', 0)


def _vcfg(channels, dtype, layout, size, **kw):
    """Gamma + normalisation (u8: gamma only), as test_gpu_crop._vcfg, with a resize (or what ``kw`` gives)."""
    kw = kw or dict(resize=ResizedCrop(size))
    if dtype == 'uint8':
        return DecodeConfig(channels=channels, gamma=2.2, dtype='uint8', layout=layout, **kw)
    return DecodeConfig.densityopt(channels=channels, gamma=2.2, dtype=dtype, layout=layout, **kw)


def _bytes(t):
    return t.contiguous().view(torch.uint8).reshape(t.shape[0], -1).numpy()


_ref_cache = {}


class _Launch:
    """One decode_resize launch on guard-filled buffers, and what it must leave in them.

    win: (y0, x0, h, w, mirrored) per image; srcs: per-image source pointers with unequal
    strides (else one dense source); dsts: per-image destinations in two buffers (else one
    dense destination); shift: byte shift per destination (dsts), or of the dense base."""

    def __init__(self, store, cfg, win, flip=None, flip_bits=0, srcs=False, dsts=False, shift=None, max_grid=0,
                 src_shift=0):
        self.store, self.cfg, self.win = store, cfg, [tuple(int(v) for v in r) for r in win]
        self.flip, self.flip_bits, self.srcs, self.dsts, self.max_grid = flip, flip_bits, srcs, dsts, max_grid
        self.src_shift = src_shift
        self.B, self.H, self.W, self.Cin = store.shape
        oh, ow = cfg.resize.size
        self.img_bytes = oh * ow * cfg.cout * ELEM[cfg.dtype]
        if dsts:
            self.bufs, self.dst = scattered_dst([(b % 2, b // 2) for b in range(self.B)], self.img_bytes, nbufs=2,
                                                shift=shift)
        else:
            self.bufs, self.dst = dense_dst(self.B, self.img_bytes, shift=shift or 0)

    def flags(self):
        return [int(bool((self.flip is not None and self.flip[b]) or (self.flip_bits >> b) & 1)) for b in range(self.B)]

    def reference(self):
        # computed once per (frames, config, windows, flips) and shared between the launches that need it
        key = (self.store.tobytes(), self.store.shape, self.cfg, tuple(self.win), tuple(self.flags()))
        if key not in _ref_cache:
            ref = _bytes(ops.reference_decode(torch.from_numpy(self.store), self.cfg, flip=self.flags(), window=self.win))
            ref.setflags(write=False)
            _ref_cache[key] = ref
        return _ref_cache[key]

    def expected(self):
        ref = self.reference()
        bufs = [np.full(n, SENTINEL, np.uint8) for n in self.bufs]
        for b, (k, off) in enumerate(self.dst):
            assert off >= GUARD // 2 and off + self.img_bytes <= len(bufs[k]) - GUARD // 2
            bufs[k][off:off + self.img_bytes] = ref[b]
        return bufs

    def run(self, dev, B=None, win=None):
        ext = ops.hip_ext()
        fb = self.H * self.W * self.Cin
        # unequal strides: 16-byte aligned frames with gaps of 48 and 80 bytes (sentinel bytes between them)
        pos = [n * fb + 16 * (0, 3, 8)[n % 3] + 16 * 8 * (n // 3) for n in range(self.B)] if self.srcs else \
            [n * fb for n in range(self.B)]
        flat = np.full(self.src_shift + pos[-1] + fb, 0x5A, np.uint8)
        for n, p in enumerate(pos):
            flat[self.src_shift + p:self.src_shift + p + fb] = self.store[n].reshape(-1)
        src = torch.from_numpy(flat).to(dev)
        assert src.data_ptr() % 256 == 0
        outs = [torch.full((n,), SENTINEL, dtype=torch.uint8, device=dev) for n in self.bufs]
        ft = torch.tensor(list(self.flip), dtype=torch.uint8, device=dev) if self.flip is not None else None
        base = src.data_ptr() + self.src_shift
        k0, off0 = self.dst[0]
        win = self.win if win is None else win
        ext.decode(0 if self.srcs else base, 0, 0 if self.dsts else outs[k0].data_ptr() + off0,
                   ops.device_lut(self.cfg, dev).data_ptr(), ft.data_ptr() if ft is not None else 0,
                   self.B if B is None else B, self.H, self.W, self.Cin, self.cfg.cout, self.cfg.cmap, 0,
                   ops.OUT_DTYPES[self.cfg.dtype], ops.LAYOUTS[self.cfg.layout], ops._stream(dev),
                   srcs=[base + p for p in pos] if self.srcs else [],
                   dsts=[outs[k].data_ptr() + off for k, off in self.dst] if self.dsts else [],
                   flip_bits=[self.flip_bits] if self.flip_bits else [], max_grid=self.max_grid,
                   resize_size=list(self.cfg.resize.size), window=[v for r in win for v in r])
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in outs]

    def check(self, dev, what=''):
        got, exp = self.run(dev), self.expected()
        for k, (g, e) in enumerate(zip(got, exp)):
            if not np.array_equal(g, e):
                bad = np.flatnonzero(g != e)
                where = [b for b, (kk, off) in enumerate(self.dst) if kk == k and off <= bad[0] < off + self.img_bytes]
                raise AssertionError(f'{what} {self.cfg.channels} Cin {self.Cin} windows {self.win} flips {self.flags()}: '
                                     f'buffer {k}: {len(bad)} bytes differ, first at {bad[0]} '
                                     f'({"image %d" % where[0] if where else "GUARD"}): got {g[bad[0]]:#x}, '
                                     f'expected {e[bad[0]]:#x}')


# B = 3 frames of 7 x 32, output 4 x 16.  Identity windows (4, 16) at x0 over every residue of 3 * x0 mod 4
# (0, 1, 2, 3, 5) and at 16, the last legal column, on the first and the last legal rows; upscales from (2, 5)
# and (1, 1); downscales from (7, 32) and (7, 31) (vertical scale 1.75: adjacent output rows share source rows;
# horizontal >= 1.9: columns are skipped); a window ending on the frame's last row and column.  Every window
# class runs mirrored and not; image 1 of the first launch is flipped AND mirrored; sources dense / per image,
# destinations dense / per image.
W416 = [
    dict(win=[(0, 0, 4, 16, 0), (3, 1, 4, 16, 1), (0, 2, 4, 16, 0)], flip_bits=0b011),
    dict(win=[(3, 3, 4, 16, 1), (0, 5, 4, 16, 0), (3, 16, 4, 16, 1)], flip=[1, 0, 0], srcs=True, dsts=True),
    dict(win=[(3, 0, 4, 16, 1), (0, 1, 4, 16, 0), (3, 2, 4, 16, 1)], flip=[0, 1, 0], flip_bits=0b100, srcs=True),
    dict(win=[(0, 3, 4, 16, 0), (3, 5, 4, 16, 1), (0, 16, 4, 16, 0)], flip_bits=0b110, dsts=True),
    dict(win=[(1, 3, 2, 5, 0), (6, 31, 1, 1, 1), (0, 0, 7, 32, 0)], flip_bits=0b010, srcs=True),
    dict(win=[(5, 27, 2, 5, 1), (0, 0, 1, 1, 0), (0, 0, 7, 32, 1)], flip=[1, 1, 0], dsts=True),
    dict(win=[(0, 0, 7, 31, 0), (0, 1, 7, 31, 1), (2, 9, 5, 23, 0)], flip_bits=0b101),
    dict(win=[(0, 1, 7, 31, 1), (0, 0, 7, 31, 0), (2, 9, 5, 23, 1)], flip=[0, 0, 1], srcs=True, dsts=True),
]


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_resize_window_matrix(dev, dtype, layout):
    """B = 3, H = 7, W = 32 -> 4 x 16: every window class, the 3 x 12 output (staged for f32 only), and a
    destination off by one element and a source off by 4 bytes (one pixel per thread), for both source
    layouts and every channel map."""
    es = ELEM[dtype]
    for Cin in (3, 4):
        store = frames(3, 7, 32, Cin, seed=100 + Cin)
        for ch in CMAPS[Cin]:
            cfg = _vcfg(ch, dtype, layout, (4, 16))
            for i, kw in enumerate(W416):
                _Launch(store, cfg, **kw).check(dev, f'4x16 #{i}')
            small = _vcfg(ch, dtype, layout, (3, 12))
            assert (12 % PPT[dtype] == 0) == (dtype == 'float32')
            _Launch(store, small, [(4, 20, 3, 12, 1), (0, 0, 7, 32, 0), (2, 7, 2, 5, 1)], flip_bits=0b101,
                    srcs=True).check(dev, '3x12')
            _Launch(store, small, [(1, 9, 6, 23, 0), (4, 20, 3, 12, 1), (6, 31, 1, 1, 1)], flip=[0, 1, 1],
                    dsts=True).check(dev, '3x12 dsts')
            # one destination off by one element: the launch leaves the staged path
            _Launch(store, cfg, [(3, 16, 4, 16, 1), (0, 0, 7, 32, 0), (1, 5, 2, 5, 1)], flip_bits=0b001, dsts=True,
                    shift=[0, es, 0]).check(dev, 'dst + 1 element')
            _Launch(store, cfg, [(0, 2, 7, 30, 1), (3, 16, 4, 16, 0), (2, 3, 1, 1, 1)], flip=[1, 1, 0],
                    shift=es).check(dev, 'dense dst + 1')
        # a source base off by 4 bytes (one pixel per thread too)
        _Launch(store, _vcfg('bgr', dtype, layout, (4, 16)), W416[4]['win'], flip_bits=0b010,
                src_shift=4).check(dev, 'src + 4')


# 40 x 96 frames, outputs 37 x 32 and 64 x 48 (several bands and a ragged last one for any band height up to 32),
# 9 x 32 from 40 rows (vertical scale 4.4: the rows between taps are skipped).  Window heights 5 (many output rows
# per source-row pair: bands share rows), 37 (identity rows for the 37-row output) and 40.
BANDS = [
    ((37, 32), [(0, 0, 37, 96, 0), (3, 33, 5, 32, 1), (0, 8, 40, 64, 0)]),
    ((64, 48), [(35, 1, 5, 95, 1), (2, 0, 37, 48, 0), (0, 0, 40, 96, 1)]),
    ((9, 32), [(0, 0, 40, 96, 0), (0, 64, 40, 32, 1), (31, 5, 9, 64, 0)]),
]


@pytest.mark.parametrize('max_grid', [1, 0])
@pytest.mark.parametrize('dtype,layout,Cin,ch', [('float32', 'nchw', 3, 'bgr'), ('bfloat16', 'nhwc', 4, 'rgba'),
                                                ('float32', 'nhwc', 4, 'rgb'), ('float16', 'nchw', 3, 'rgb')])
def test_bands_and_grid_stride(dev, dtype, layout, Cin, ch, max_grid):
    """max_grid = 1: one block walks every band of every image, restaging its rows each time."""
    store = frames(3, 40, 96, Cin, seed=300 + Cin)
    for size, win in BANDS:
        cfg = _vcfg(ch, dtype, layout, size)
        _Launch(store, cfg, win, flip_bits=0b011, max_grid=max_grid, srcs=True).check(dev, f'{size} grid {max_grid}')
        _Launch(store, cfg, win[::-1], flip=[0, 0, 1], max_grid=max_grid, dsts=True).check(dev, f'{size} grid {max_grid}')


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_identity_resize_equals_the_crop(dev, dtype, layout):
    for Cin in (3, 4):
        x = torch.from_numpy(frames(3, 7, 32, Cin, seed=200 + Cin)).to(dev)
        for ch in CMAPS[Cin]:
            for (y0, x0, m) in ((0, 0, 0), (3, 5, 1), (2, 16, 1)):
                rcfg = _vcfg(ch, dtype, layout, (4, 16))
                ccfg = _vcfg(ch, dtype, layout, None, crop=Crop((4, 16)))
                a = ops.decode(x, rcfg, flip=[0, 1, 1], window=(y0, x0, 4, 16, m))
                b = ops.decode(x, ccfg, flip=[0, 1, 1], crop=[(y0, x0, m)] * 3)
                assert a.shape == b.shape and a.dtype == b.dtype
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (Cin, ch, y0, x0, m)


def test_ops_decode_with_a_resize(dev):
    """The public call: windows from ops.resized_windows, output allocated or given."""
    store = frames(5, 20, 96, 4, seed=7)
    rc = ResizedCrop((8, 32), scale=(0.1, 1.0), mirror=0.5, seed=2795)
    cfg = DecodeConfig.unit(channels='rgb', gamma=2.2, resize=rc)
    win = ops.resized_windows(rc, 20, 96, 5)
    x = torch.from_numpy(store).to(dev)
    ref = ops.reference_decode(torch.from_numpy(store), cfg, flip=[1, 0, 0, 1, 0], window=win)
    got = ops.decode(x, cfg, flip=[1, 0, 0, 1, 0], window=win)
    assert got.shape == (5, 3, 8, 32) and torch.equal(got.cpu(), ref)
    out = torch.zeros_like(got)
    assert ops.decode(x, cfg, flip=[1, 0, 0, 1, 0], out=out, window=torch.from_numpy(win)) is out and torch.equal(out, got)
    with pytest.raises(ValueError):
        ops.decode(x, cfg)                                                  # a resize config needs its windows
    with pytest.raises(ValueError):
        ops.decode(x, DecodeConfig.unit(channels='rgb'), window=win)
    with pytest.raises(ValueError):
        ops.decode(x, cfg, window=win, out=torch.zeros(5, 3, 20, 96, device=dev))
    with pytest.raises(ValueError):
        ops.decode(x, cfg, window=win[:4])
    x65 = torch.zeros(65, 4, 8, 4, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match='64'):
        ops.decode(x65, cfg, window=(0, 0, 4, 8, 0))
    with pytest.raises(ValueError):
        ops.decode_gather(x, torch.arange(5, device=dev), cfg)
    from blendtorch.btt.replay import DeviceReplayBuffer
    buf = DeviceReplayBuffer(8, device=dev)
    buf.extend(x)
    with pytest.raises(ValueError, match='resize'):
        buf.sample(4, cfg)


@pytest.mark.parametrize('what', ['y0 = -1', 'x0 + w = W + 1', 'h = 0', 'y0 + h = H + 1', 'B = 65'])
def test_rejected_on_the_host_before_any_launch(dev, what):
    cfg = _vcfg('rgb', 'float32', 'nchw', (4, 16))
    if what == 'B = 65':
        l = _Launch(frames(65, 7, 32, 3, seed=1), cfg, [(0, 0, 7, 32, 0)] * 65)
    else:
        bad = {'y0 = -1': (-1, 4, 4, 16, 0), 'x0 + w = W + 1': (2, 17, 4, 16, 1), 'h = 0': (2, 4, 0, 16, 0),
               'y0 + h = H + 1': (4, 4, 4, 16, 0)}
        l = _Launch(frames(3, 7, 32, 3, seed=1), cfg, [(3, 16, 4, 16, 0), bad[what], (0, 0, 7, 32, 1)])
    outs = None
    with pytest.raises(RuntimeError, match='invalid'):
        outs = l.run(dev)
    assert outs is None
    # the same launch with legal windows runs (the rejection was the window's), and a rejected one writes nothing
    if what != 'B = 65':
        _Launch(l.store, cfg, [(3, 16, 4, 16, 0), (3, 16, 4, 16, 1), (0, 0, 7, 32, 1)]).check(dev, 'legal')
    touched = torch.full((l.bufs[0],), SENTINEL, dtype=torch.uint8, device=dev)
    src = torch.from_numpy(l.store).to(dev)
    with pytest.raises(RuntimeError, match='invalid'):
        ops.hip_ext().decode(src.data_ptr(), 0, touched.data_ptr() + GUARD, ops.device_lut(cfg, dev).data_ptr(), 0, l.B,
                             7, 32, 3, 3, cfg.cmap, 0, 0, 0, ops._stream(dev), resize_size=[4, 16],
                             window=[v for r in l.win for v in r])
    torch.cuda.synchronize()
    assert bool((touched == SENTINEL).all())


# ---- the stream loader ------------------------------------------------------------------------------------------

B, NBATCH = 4, 10
RES, FH, FW = '64x32', 32, 64
POSE = ['--rotation', '0.6', '0.4', '0.9']
# seed 8855: of the 40 windows it draws on 32 x 64 frames 2 are lower than the 16-row output and 36 higher,
# 19 are mirrored and 31 sizes differ (seed 8853 draws no window lower than 16 rows);
# test_the_loader_stream_is_varied holds it to that
RC = ResizedCrop((16, 16), scale=(0.1, 1.0), mirror=0.5, seed=8855)
_frame_cache = {}


def _args(*extra):
    return ['--mode', 'rgba', '--resolution', RES, '--stamp', *POSE, *extra]


def _frame(port):
    """The fixed pose's 32 x 64 x 4 frame through the CPU path, once."""
    if RES not in _frame_cache:
        with btt.BlenderLauncher(producer='cubesim', num_instances=1, named_sockets=['DATA'], start_port=port,
                                 proto='ipc', instance_args=[_args('--shm', '8', '--shm-layout', 'interleaved')]) as bl:
            s = zmq.Context().socket(zmq.PULL)
            s.connect(bl.launch_info.addresses['DATA'][0])
            assert s.poll(20000)
            _frame_cache[RES] = np.ascontiguousarray(shm.resolve(s.recv_pyobj())['image'])
            s.close()
        assert _frame_cache[RES].shape == (FH, FW, 4)
        _frame_cache[RES].setflags(write=False)
    return _frame_cache[RES]


def _reference(frame, cfg, btid, seq, win):
    f = frame.copy()
    f.reshape(-1)[:16] = np.frombuffer(struct.pack('<2sHIQ', b'BT', btid, 0, seq), np.uint8)
    return ops.reference_decode(torch.from_numpy(f[None]), cfg, flip=[0], window=[win])[0]


def _run(dev, port, cfg, producers, **kw):
    """[(btid, seq, window, decoded image (cpu))] in arrival order, and the loader's stats."""
    out = []
    with btt.BlenderLauncher(producer='cubesim', num_instances=len(producers), named_sockets=['DATA'],
                             start_port=port, proto='ipc', instance_args=producers) as bl:
        dl = DeviceLoader(bl.launch_info.addresses['DATA'], batch_size=B, max_items=B * NBATCH, device=dev,
                          decode=cfg, **kw)
        for b in dl:
            img = b['image'].cpu()
            assert tuple(img.shape) == tuple(cfg.out_shape(B, FH, FW))
            win = b['window']
            assert isinstance(win, torch.Tensor) and win.dtype == torch.int32 and tuple(win.shape) == (B, 5)
            assert 'crop' not in b
            for k in range(B):
                out.append((int(b['btid'][k]), int(b['seq'][k]), tuple(int(v) for v in win[k]), img[k]))
        st = dict(dl.stats)
    assert len(out) == B * NBATCH and st['bad'] == 0 and st['batches'] == NBATCH
    return out, st


def _check_images(got, frame, cfg):
    for btid, seq, win, img in got:
        assert torch.equal(img.view(torch.uint8), _reference(frame, cfg, btid, seq, win).view(torch.uint8)), (btid, seq, win)


_CFGS = {
    'f32-nchw': lambda rc: DecodeConfig.unit(channels='rgb', gamma=2.2, resize=rc),
    'bf16-nhwc': lambda rc: DecodeConfig.unit(channels='rgb', gamma=2.2, dtype='bfloat16', layout='nhwc', resize=rc),
}


def test_the_loader_stream_is_varied():
    """(no GPU work) the 40 windows of the loader tests: up- and downscales, both mirror states, many sizes."""
    want = ops.resized_windows(RC, FH, FW, B * NBATCH)
    assert (want[:, 2] < 16).any() and (want[:, 2] > 16).any()
    assert 10 <= want[:, 4].sum() <= 30 and len({(h, w) for h, w in want[:, 2:4]}) > 10


@pytest.mark.parametrize('path', ['rgb_a', 'interleaved', 'copy'])
@pytest.mark.parametrize('cfg', list(_CFGS))
def test_loader_resizes_what_it_reports(dev, free_port, cfg, path):
    cfg = _CFGS[cfg](RC)
    frame = _frame(free_port)
    want = ops.resized_windows(RC, FH, FW, B * NBATCH)
    area = int((want[:, 2].astype(np.int64) * want[:, 3]).sum())
    if path == 'rgb_a':      # a producer that always writes rgb_a: every slot is read in place as packed RGB
        got, st = _run(dev, free_port + 5, cfg, [_args('--shm', '8', '--shm-layout', 'planar')])
        assert st['planar_frames'] == B * NBATCH and st['direct_batches'] == st['batches'] and st['staged_frames'] == 0, st
        assert st['image_bytes'] == area * 3, st
    elif path == 'interleaved':
        got, st = _run(dev, free_port + 5, cfg, [_args('--shm', '8')], shm_alpha='interleaved')
        assert st['planar_frames'] == 0 and st['direct_batches'] == st['batches'] and st['staged_frames'] == 0, st
        assert st['image_bytes'] == area * 4, st
    else:
        got, st = _run(dev, free_port + 5, cfg, [_args('--shm', '8')], h2d='copy')
        assert st['direct_batches'] == 0 and st['passthrough_batches'] == 0, st
        assert st['image_bytes'] == B * NBATCH * FH * FW * 4, st         # the copy path moves whole frames
    # one producer: arrival order is the draw order
    assert [g[1] for g in got] == sorted(g[1] for g in got)
    assert np.array_equal(np.array([g[2] for g in got], np.int32), want)
    _check_images(got, frame, cfg)


@pytest.mark.parametrize('rc', [ResizedCrop((16, 16), mode='center'), ResizedCrop((16, 24), mode='full'),
                                ResizedCrop((8, 40), mode='center'), ResizedCrop((12, 20), window=(9, 37, 15, 21))])
def test_loader_center_full_and_fixed_windows(dev, free_port, rc):
    cfg = _CFGS['f32-nchw'](rc)
    frame = _frame(free_port)
    got, st = _run(dev, free_port + 5, cfg, [_args('--shm', '8')])
    want = tuple(int(v) for v in ops.resized_windows(rc, FH, FW, 1)[0])
    assert want[4] == 0 and {g[2] for g in got} == {want}
    if rc.kind == 'full':
        assert want == (0, 0, FH, FW, 0)
    assert st['direct_batches'] == st['batches'], st
    _check_images(got, frame, cfg)


def test_mixed_fleet_stays_direct_with_a_resize(dev, free_port):
    cfg = _CFGS['f32-nchw'](RC)
    frame = _frame(free_port)
    # as test_gpu_crop: a ring producer and a paced inline producer, both source layouts in one group
    got, st = _run(dev, free_port + 5, cfg, [_args('--shm', '4'), _args('--fps', '200')], launch_depth=0)
    assert st['direct_batches'] == st['batches'], st
    assert 0 < st['planar_frames'] < st['frames'] and st['shm_frames'] < st['frames'], st
    assert {g[0] for g in got} == {0, 1}
    assert np.array_equal(np.array([g[2] for g in got], np.int32), ops.resized_windows(RC, FH, FW, B * NBATCH))
    _check_images(got, frame, cfg)


def test_window_larger_than_the_frame_fails_the_stream(dev, free_port):
    cfg = _CFGS['f32-nchw'](ResizedCrop((16, 16), window=(0, 0, FH + 1, FW)))
    with btt.BlenderLauncher(producer='cubesim', num_instances=1, named_sockets=['DATA'], start_port=free_port,
                             proto='ipc', instance_args=[_args('--shm', '8')]) as bl:
        dl = DeviceLoader(bl.launch_info.addresses['DATA'], batch_size=B, max_items=B * NBATCH, device=dev, decode=cfg)
        n = 0
        with pytest.raises(RuntimeError, match=r'33x64 resize window.*32x64'):
            for _ in dl:
                n += 1
        assert n == 0 and dl.stats['batches'] == 0
