"""Crop + mirror inside the fused decode (csrc/gpu/kernels.hip ``decode_crop``)
and through the stream loader.

Kernel: every launch is compared bit for bit (bf16 / f16 as raw bits) over its
WHOLE destination buffers -- 256-byte guards of sentinel bytes before, between
and behind the images included -- with the CPU ``ops.reference_decode(...,
crop=)``.  The buffers and frames come from tests/decode_oracle.py.

Loader: stamped 64x32 cubesim frames of one fixed pose, batch 4, 10 batches, one
producer (arrival order = draw order), as tests/test_gpu_planar_alpha.py.
"""
import dataclasses
import struct

import numpy as np
import pytest
import torch

from decode_oracle import ELEM, GUARD, SENTINEL, dense_dst, frames, scattered_dst
from blendtorch import btt, ops
from blendtorch.btt.gpu import DeviceLoader
from blendtorch.ops import Crop, DecodeConfig
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


def _vcfg(channels, dtype, layout, size):
    """Gamma + normalisation (u8: gamma only), as test_decode_family._vcfg, with a crop."""
    if dtype == 'uint8':
        return DecodeConfig(channels=channels, gamma=2.2, dtype='uint8', layout=layout, crop=Crop(size))
    return DecodeConfig.densityopt(channels=channels, gamma=2.2, dtype=dtype, layout=layout, crop=Crop(size))


def _bytes(t):
    return t.contiguous().view(torch.uint8).reshape(t.shape[0], -1).numpy()


class _Launch:
    """One decode_crop launch on guard-filled buffers, and what it must leave in them.

    srcs: per-image source pointers with unequal strides (else one dense source);
    dsts: per-image destinations in two buffers (else one dense destination);
    shift: byte shift per destination (dsts), or of the dense base."""

    def __init__(self, store, cfg, win, flip=None, flip_bits=0, srcs=False, dsts=False, shift=None, max_grid=0,
                 src_shift=0):
        self.store, self.cfg, self.win = store, cfg, [tuple(int(v) for v in r) for r in win]
        self.flip, self.flip_bits, self.srcs, self.dsts, self.max_grid = flip, flip_bits, srcs, dsts, max_grid
        self.src_shift = src_shift
        self.B, self.H, self.W, self.Cin = store.shape
        h, w = cfg.crop.size
        self.img_bytes = h * w * cfg.cout * ELEM[cfg.dtype]
        if dsts:
            self.bufs, self.dst = scattered_dst([(b % 2, b // 2) for b in range(self.B)], self.img_bytes, nbufs=2,
                                                shift=shift)
        else:
            self.bufs, self.dst = dense_dst(self.B, self.img_bytes, shift=shift or 0)

    def flags(self):
        return [int(bool((self.flip is not None and self.flip[b]) or (self.flip_bits >> b) & 1)) for b in range(self.B)]

    def expected(self):
        ref = _bytes(ops.reference_decode(torch.from_numpy(self.store), self.cfg, flip=self.flags(), crop=self.win))
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
                   crop_size=list(self.cfg.crop.size), crop=[v for r in win for v in r])
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


# window (4, 16) of 7 x 32 frames: x0 over every residue of x0 * 3 mod 4 and x0 * 4 mod 16 and the first and
# last legal columns, y0 the first and last legal rows; every x0 mirrored and not; image 1 of the first
# launch is flipped AND mirrored; sources dense / per image, destinations dense / per image
W416 = [
    dict(win=[(0, 0, 0), (3, 1, 1), (0, 2, 0)], flip_bits=0b011),
    dict(win=[(3, 3, 1), (0, 5, 0), (3, 16, 1)], flip=[1, 0, 0], srcs=True, dsts=True),
    dict(win=[(3, 0, 1), (0, 1, 0), (3, 2, 1)], flip=[0, 1, 0], flip_bits=0b100, srcs=True),
    dict(win=[(0, 3, 0), (3, 5, 1), (0, 16, 0)], flip_bits=0b110, dsts=True),
]


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_crop_window_matrix(dev, dtype, layout):
    """B = 3, H = 7, W = 32: the 4 x 16 window at every origin class, the 3 x 12 window (vector for f32 only),
    and a destination off by one element (scalar), for both source layouts and every channel map."""
    es = ELEM[dtype]
    for Cin in (3, 4):
        store = frames(3, 7, 32, Cin, seed=100 + Cin)
        for ch in CMAPS[Cin]:
            cfg = _vcfg(ch, dtype, layout, (4, 16))
            for i, kw in enumerate(W416):
                _Launch(store, cfg, **kw).check(dev, f'4x16 #{i}')
            small = _vcfg(ch, dtype, layout, (3, 12))
            assert (12 % PPT[dtype] == 0) == (dtype == 'float32')
            _Launch(store, small, [(4, 20, 1), (0, 0, 0), (2, 7, 1)], flip_bits=0b101, srcs=True).check(dev, '3x12')
            _Launch(store, small, [(1, 9, 0), (4, 20, 1), (0, 3, 1)], flip=[0, 1, 1], dsts=True).check(dev, '3x12 dsts')
            # one destination off by one element: the launch leaves the vector path
            _Launch(store, cfg, [(3, 16, 1), (0, 0, 0), (1, 5, 1)], flip_bits=0b001, dsts=True,
                    shift=[0, es, 0]).check(dev, 'dst + 1 element')
            _Launch(store, cfg, [(0, 2, 1), (3, 16, 0), (2, 3, 1)], flip=[1, 1, 0], shift=es).check(dev, 'dense dst + 1')
        # a source base off by 4 bytes (scalar too)
        _Launch(store, _vcfg('bgr', dtype, layout, (4, 16)), W416[0]['win'], flip_bits=0b010,
                src_shift=4).check(dev, 'src + 4')


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_full_frame_window_is_the_plain_decode(dev, dtype, layout):
    for Cin in (3, 4):
        store = frames(3, 7, 32, Cin, seed=200 + Cin)
        for ch in CMAPS[Cin]:
            cfg = _vcfg(ch, dtype, layout, (7, 32))
            win = [(0, 0, 0)] * 3
            _Launch(store, cfg, win, flip=[0, 1, 0], flip_bits=0b100).check(dev, 'full frame')
            x = torch.from_numpy(store).to(dev)
            plain = ops.decode(x, dataclasses.replace(cfg, crop=None), flip=[0, 1, 1])
            cropped = ops.decode(x, cfg, flip=[0, 1, 1], crop=win)
            assert cropped.shape == plain.shape and cropped.dtype == plain.dtype
            assert torch.equal(cropped.view(torch.uint8), plain.view(torch.uint8))


@pytest.mark.parametrize('dtype,layout,Cin,ch', [('float32', 'nchw', 3, 'bgr'), ('bfloat16', 'nhwc', 4, 'rgba'),
                                                ('float32', 'nhwc', 4, 'rgb'), ('float16', 'nchw', 3, 'rgb')])
def test_grid_stride_loop(dev, dtype, layout, Cin, ch):
    """One block (max_grid = 1) over B = 3 windows of 16 x 64 in 20 x 96 frames: 3 * 1024 / PPT groups on 256 lanes."""
    assert 3 * 16 * 64 // PPT[dtype] > 256
    store = frames(3, 20, 96, Cin, seed=300 + Cin)
    cfg = _vcfg(ch, dtype, layout, (16, 64))
    _Launch(store, cfg, [(4, 32, 1), (0, 0, 0), (3, 17, 1)], flip_bits=0b011, max_grid=1, srcs=True).check(dev, 'grid 1')
    _Launch(store, cfg, [(0, 5, 0), (4, 31, 1), (2, 32, 0)], flip=[0, 0, 1], max_grid=1, dsts=True).check(dev, 'grid 1')


def test_ops_decode_with_a_crop(dev):
    """The public call: windows from ops.crop_windows, output allocated or given."""
    store = frames(5, 20, 96, 4, seed=7)
    crop = Crop((8, 32), mirror=0.5, seed=2795, x_align=4)
    cfg = DecodeConfig.unit(channels='rgb', gamma=2.2, crop=crop)
    win = ops.crop_windows(crop, 20, 96, 5)
    x = torch.from_numpy(store).to(dev)
    ref = ops.reference_decode(torch.from_numpy(store), cfg, flip=[1, 0, 0, 1, 0], crop=win)
    got = ops.decode(x, cfg, flip=[1, 0, 0, 1, 0], crop=win)
    assert got.shape == (5, 3, 8, 32) and torch.equal(got.cpu(), ref)
    out = torch.zeros_like(got)
    assert ops.decode(x, cfg, flip=[1, 0, 0, 1, 0], out=out, crop=torch.from_numpy(win)) is out and torch.equal(out, got)
    with pytest.raises(ValueError):
        ops.decode(x, cfg)                                                  # a crop config needs its windows
    with pytest.raises(ValueError):
        ops.decode(x, DecodeConfig.unit(channels='rgb'), crop=win)
    with pytest.raises(ValueError):
        ops.decode(x, cfg, crop=win, out=torch.zeros(5, 3, 20, 96, device=dev))
    with pytest.raises(ValueError):
        ops.decode_gather(x, torch.arange(5, device=dev), cfg)


@pytest.mark.parametrize('what', ['y0 = -1', 'x0 = -1', 'y0 + h = H + 1', 'x0 + w = W + 1', 'B = 65'])
def test_rejected_on_the_host_before_any_launch(dev, what):
    cfg = _vcfg('rgb', 'float32', 'nchw', (4, 16))
    if what == 'B = 65':
        l = _Launch(frames(65, 7, 32, 3, seed=1), cfg, [(0, 0, 0)] * 65)
    else:
        bad = {'y0 = -1': (-1, 4, 0), 'x0 = -1': (2, -1, 0), 'y0 + h = H + 1': (4, 4, 0), 'x0 + w = W + 1': (2, 17, 1)}
        l = _Launch(frames(3, 7, 32, 3, seed=1), cfg, [(3, 16, 0), bad[what], (0, 0, 1)])
    outs = None
    with pytest.raises(RuntimeError, match='invalid'):
        outs = l.run(dev)
    assert outs is None
    # the same launch with legal windows runs (the rejection was the window's), and a rejected one writes nothing
    if what != 'B = 65':
        ok = _Launch(l.store, cfg, [(3, 16, 0), (3, 16, 1), (0, 0, 1)])
        ok.check(dev, 'legal')
    touched = torch.full((l.bufs[0],), SENTINEL, dtype=torch.uint8, device=dev)
    src = torch.from_numpy(l.store).to(dev)
    with pytest.raises(RuntimeError, match='invalid'):
        ops.hip_ext().decode(src.data_ptr(), 0, touched.data_ptr() + GUARD, ops.device_lut(cfg, dev).data_ptr(), 0, l.B,
                             7, 32, 3, 3, cfg.cmap, 0, 0, 0, ops._stream(dev), crop_size=[4, 16],
                             crop=[v for r in l.win for v in r])
    torch.cuda.synchronize()
    assert bool((touched == SENTINEL).all())


# ---- the stream loader ------------------------------------------------------------------------------------------

B, NBATCH = 4, 10
RES, FH, FW = '64x32', 32, 64
POSE = ['--rotation', '0.6', '0.4', '0.9']
CROP = Crop((FH // 2, FW // 2), mirror=0.5, seed=8853)
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
    return ops.reference_decode(torch.from_numpy(f[None]), cfg, flip=[0], crop=[win])[0]


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
            win = b['crop']
            assert isinstance(win, torch.Tensor) and win.dtype == torch.int32 and tuple(win.shape) == (B, 3)
            for k in range(B):
                out.append((int(b['btid'][k]), int(b['seq'][k]), tuple(int(v) for v in win[k]), img[k]))
        st = dict(dl.stats)
    assert len(out) == B * NBATCH and st['bad'] == 0 and st['batches'] == NBATCH
    return out, st


def _check_images(got, frame, cfg):
    for btid, seq, win, img in got:
        assert torch.equal(img.view(torch.uint8), _reference(frame, cfg, btid, seq, win).view(torch.uint8)), (btid, seq)


_CFGS = {
    'f32-nchw': lambda crop: DecodeConfig.unit(channels='rgb', gamma=2.2, crop=crop),
    'bf16-nhwc': lambda crop: DecodeConfig.unit(channels='rgb', gamma=2.2, dtype='bfloat16', layout='nhwc', crop=crop),
}


@pytest.mark.parametrize('path', ['rgb_a', 'interleaved', 'copy'])
@pytest.mark.parametrize('cfg', list(_CFGS))
def test_loader_crops_what_it_reports(dev, free_port, cfg, path):
    cfg = _CFGS[cfg](CROP)
    frame = _frame(free_port)
    h, w = CROP.size
    if path == 'rgb_a':      # a producer that always writes rgb_a: every slot is read in place as packed RGB
        got, st = _run(dev, free_port + 5, cfg, [_args('--shm', '8', '--shm-layout', 'planar')])
        assert st['planar_frames'] == B * NBATCH and st['direct_batches'] == st['batches'] and st['staged_frames'] == 0, st
        assert st['image_bytes'] == B * NBATCH * h * w * 3, st
    elif path == 'interleaved':
        got, st = _run(dev, free_port + 5, cfg, [_args('--shm', '8')], shm_alpha='interleaved')
        assert st['planar_frames'] == 0 and st['direct_batches'] == st['batches'] and st['staged_frames'] == 0, st
        assert st['image_bytes'] == B * NBATCH * h * w * 4, st
    else:
        got, st = _run(dev, free_port + 5, cfg, [_args('--shm', '8')], h2d='copy')
        assert st['direct_batches'] == 0 and st['passthrough_batches'] == 0, st
        assert st['image_bytes'] == B * NBATCH * FH * FW * 4, st         # the copy path moves whole frames
    # one producer: arrival order is the draw order
    assert [g[1] for g in got] == sorted(g[1] for g in got)
    want = ops.crop_windows(CROP, FH, FW, B * NBATCH)
    assert np.array_equal(np.array([g[2] for g in got], np.int32), want)
    assert 0 < want[:, 2].sum() < len(want) and len({tuple(r[:2]) for r in want}) > 10
    _check_images(got, frame, cfg)


def test_loader_reads_planar_slots_on_request(dev, free_port):
    """The ring hint is unchanged: an RGB-only direct crop still asks for rgb_a frames."""
    cfg = _CFGS['f32-nchw'](CROP)
    frame = _frame(free_port)
    got, st = _run(dev, free_port + 5, cfg, [_args('--shm', '8')])
    h, w = CROP.size
    assert st['planar_frames'] > 0 and st['direct_batches'] == st['batches'], st
    assert st['image_bytes'] == h * w * (3 * st['planar_frames'] + 4 * (B * NBATCH - st['planar_frames'])), st
    _check_images(got, frame, cfg)


@pytest.mark.parametrize('crop', [Crop((16, 32), mode='center', x_align=4), Crop((15, 21), origin=(9, 37)),
                                  Crop((32, 64), mode='center')])
def test_loader_center_and_fixed_windows(dev, free_port, crop):
    cfg = _CFGS['f32-nchw'](crop)
    frame = _frame(free_port)
    got, st = _run(dev, free_port + 5, cfg, [_args('--shm', '8')])
    want = tuple(int(v) for v in ops.crop_windows(crop, FH, FW, 1)[0])
    assert want[2] == 0 and {g[2] for g in got} == {want}
    assert st['direct_batches'] == st['batches'], st
    _check_images(got, frame, cfg)


def test_identity_decode_with_a_crop_takes_the_kernel(dev, free_port):
    cfg = DecodeConfig.raw(channels='rgba', crop=CROP)
    frame = _frame(free_port)
    got, st = _run(dev, free_port + 5, cfg, [_args('--shm', '8')], h2d='copy')
    assert st['passthrough_batches'] == 0, st
    _check_images(got, frame, cfg)


def test_mixed_fleet_stays_direct_with_a_crop(dev, free_port):
    cfg = _CFGS['f32-nchw'](CROP)
    frame = _frame(free_port)
    # as test_gpu_planar_alpha: a ring producer and a paced inline producer, both source layouts in one group
    got, st = _run(dev, free_port + 5, cfg, [_args('--shm', '4'), _args('--fps', '200')], launch_depth=0)
    assert st['direct_batches'] == st['batches'], st
    assert 0 < st['planar_frames'] < st['frames'] and st['shm_frames'] < st['frames'], st
    assert {g[0] for g in got} == {0, 1}
    assert np.array_equal(np.array([g[2] for g in got], np.int32), ops.crop_windows(CROP, FH, FW, B * NBATCH))
    _check_images(got, frame, cfg)


def test_window_larger_than_the_frame_fails_the_stream(dev, free_port):
    cfg = _CFGS['f32-nchw'](Crop((FH + 1, FW), mirror=0.5))
    with btt.BlenderLauncher(producer='cubesim', num_instances=1, named_sockets=['DATA'], start_port=free_port,
                             proto='ipc', instance_args=[_args('--shm', '8')]) as bl:
        dl = DeviceLoader(bl.launch_info.addresses['DATA'], batch_size=B, max_items=B * NBATCH, device=dev, decode=cfg)
        n = 0
        with pytest.raises(RuntimeError, match=r'33x64 crop window.*32x64'):
            for _ in dl:
                n += 1
        assert n == 0 and dl.stats['batches'] == 0
