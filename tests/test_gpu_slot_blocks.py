"""Block-mask reads with a slot mirror: the kernel (csrc/gpu/kernels.hip
``decode_delta_blocks``) and the stream loader (``DeviceLoader(slot_mirror=
True)`` over producers that report changed blocks).

Kernel: images of H = 40, W = 192 (3 column blocks) per launch -- image 0
without a mirror, flipped and upright images mixed, per-image destinations --
with bands of 8 rows (5 bands) and of 16 rows (16, 16 and 8 rows: the last band
is partial).  The host frames (pinned, device-mapped) hold the true bytes inside
each image's set blocks and POISON outside them; the mirrors hold the true
bytes outside and poison inside.  The outputs, compared bit for bit with
``ops.reference_decode`` of the true frames over their whole guard-filled
buffers, therefore prove that nothing outside a set block is taken from the
host and nothing inside from the mirror; afterwards every mirror equals its
true frame and the guards around the mirrors hold.

Loader: stamped 128x64 cubesim frames, random poses, from two 4-slot rings,
batch 4, 12 batches, and from two 24-slot rings in batches of 40 (more than one
block launch holds); the oracle is the same frames through the CPU path.
"""
import ctypes

import numpy as np
import pytest
import torch

from decode_oracle import ELEM, GUARD, SENTINEL, frames, scattered_dst
from blendtorch import btt, ops
from blendtorch.btt.gpu import DeviceLoader
from blendtorch.ops import DecodeConfig
from blendtorch.transport import shm, zmq

pytestmark = pytest.mark.gpu

H, W = 40, 192
NCOL = W // 64
OUTS = (('float32', 'nchw'), ('bfloat16', 'nhwc'), ('uint8', 'nchw'))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    ops.hip_ext()  # must load: no silent fallback
    return torch.device('cuda', 0)


def _vcfg(channels, dtype, layout):
    if dtype == 'uint8':
        return DecodeConfig(channels=channels, gamma=2.2, dtype='uint8', layout=layout)
    return DecodeConfig.densityopt(channels=channels, gamma=2.2, dtype=dtype, layout=layout)


def _masks(band_rows):
    """Named masks: one uint16 word per band, bit c = column block c."""
    nb = -(-H // band_rows)
    full = (1 << NCOL) - 1
    rng = np.random.default_rng(900 + band_rows)
    corner = lambda k, c: [(1 << c) if i == k else 0 for i in range(nb)]   # noqa: E731
    return {
        'empty': [0] * nb,
        'full': [full] * nb,
        'checkerboard': [0b101 if k % 2 == 0 else 0b010 for k in range(nb)],
        'top left': corner(0, 0),
        'top right': corner(0, NCOL - 1),
        'bottom left': corner(nb - 1, 0),        # band_rows 16: the partial band
        'bottom right': corner(nb - 1, NCOL - 1),
        'random': [int(v) for v in rng.integers(0, full + 1, nb)],
    }


def _inside(mask, band_rows, Cin):
    m = np.zeros((H, W, Cin), bool)
    for k, word in enumerate(mask):
        for c in range(NCOL):
            if (word >> c) & 1:
                m[k * band_rows:(k + 1) * band_rows, 64 * c:64 * c + 64] = True
    return m


class _Blocks:
    """One decode_delta_blocks launch; image 0 has no mirror, images 1.. use ``masks``."""

    def __init__(self, dev, store, cfg, band_rows, masks, flip_bits):
        self.dev, self.store, self.cfg, self.flip_bits, self.band_rows = dev, store, cfg, flip_bits, band_rows
        self.B, _, _, self.Cin = store.shape
        self.masks = [[0] * len(masks[0])] + [list(m) for m in masks]
        self.fb = H * W * self.Cin
        self.img_bytes = H * W * cfg.cout * ELEM[cfg.dtype]
        self.bufs, self.dst = scattered_dst([(b % 2, b // 2) for b in range(self.B)], self.img_bytes, nbufs=2)
        ext = ops.hip_ext()
        # host frames: true inside the set blocks, poison outside (image 0: all true)
        host = np.empty((self.B, self.fb), np.uint8)
        mir = np.full(GUARD + (self.B - 1) * (self.fb + GUARD), SENTINEL, np.uint8)
        self.mir_off = [None] + [GUARD + (b - 1) * (self.fb + GUARD) for b in range(1, self.B)]
        self.ins = []
        for b in range(self.B):
            true = store[b]
            ins = np.ones_like(true, bool) if b == 0 else _inside(self.masks[b], band_rows, self.Cin)
            self.ins.append(ins)
            host[b] = np.where(ins, true, true ^ 0xFF).reshape(-1)
            if b:
                mir[self.mir_off[b]:self.mir_off[b] + self.fb] = np.where(ins, true ^ 0xFF, true).reshape(-1)
        self.host, self.host_dev = ext.host_mapped_alloc(host.size)
        ctypes.memmove(self.host, host.ctypes.data, host.size)
        self.mir = torch.from_numpy(mir).to(dev)
        self.outs = [torch.full((n,), SENTINEL, dtype=torch.uint8, device=dev) for n in self.bufs]

    def close(self):
        ops.hip_ext().host_mapped_free(self.host)

    def launch(self, B=None, band_rows=None, masks=None, W_=None):
        masks = self.masks if masks is None else masks
        B = self.B if B is None else B
        last = self.B - 1
        ops.hip_ext().decode_delta_blocks(
            [self.host_dev + min(b, last) * self.fb for b in range(B)],
            [0 if b == 0 else self.mir.data_ptr() + self.mir_off[min(b, last)] for b in range(B)],
            self.band_rows if band_rows is None else band_rows,
            [masks[min(b, last)] for b in range(B)], 0, ops.device_lut(self.cfg, self.dev).data_ptr(),
            B, H, W if W_ is None else W_, self.Cin, self.cfg.cout, list(self.cfg.cmap), 0,
            ops.OUT_DTYPES[self.cfg.dtype], ops.LAYOUTS[self.cfg.layout], ops._stream(self.dev),
            dsts=[self.outs[self.dst[min(b, last)][0]].data_ptr() + self.dst[min(b, last)][1] for b in range(B)],
            flip_bits=[self.flip_bits])
        torch.cuda.synchronize()

    def untouched(self):
        """Nothing was launched: outputs and mirrors are what they were."""
        assert all(bool((o == SENTINEL).all()) for o in self.outs)
        m = self.mir.cpu().numpy()
        for b in range(1, self.B):
            assert np.array_equal(m[self.mir_off[b]:self.mir_off[b] + self.fb],
                                  np.where(self.ins[b], self.store[b] ^ 0xFF, self.store[b]).reshape(-1))

    def check(self, what, ref):
        exp = [np.full(n, SENTINEL, np.uint8) for n in self.bufs]
        for b, (k, off) in enumerate(self.dst):
            exp[k][off:off + self.img_bytes] = ref[b]
        for k, (o, e) in enumerate(zip(self.outs, exp)):
            g = o.cpu().numpy()
            if not np.array_equal(g, e):
                bad = np.flatnonzero(g != e)
                where = [b for b, (kk, off) in enumerate(self.dst) if kk == k and off <= bad[0] < off + self.img_bytes]
                raise AssertionError(f'{what}: Cin {self.Cin} {self.cfg.channels} band_rows {self.band_rows} masks '
                                     f'{self.masks}: buffer {k}: {len(bad)} bytes differ, first at {bad[0]} '
                                     f'({"image %d" % where[0] if where else "GUARD"})')
        m = self.mir.cpu().numpy()
        want = np.full(m.size, SENTINEL, np.uint8)
        for b in range(1, self.B):
            want[self.mir_off[b]:self.mir_off[b] + self.fb] = self.store[b].reshape(-1)
        assert np.array_equal(m, want), f'{what}: the mirrors do not equal the true frames (or a guard was written)'


_ref_cache = {}


def _reference(store, cfg, flip_bits, key):
    """ops.reference_decode of the true frames, as bytes per image; computed once per (frames, config)."""
    if key not in _ref_cache:
        flags = [(flip_bits >> b) & 1 for b in range(store.shape[0])]
        ref = ops.reference_decode(torch.from_numpy(store), cfg, flip=flags)
        _ref_cache[key] = ref.contiguous().view(torch.uint8).reshape(store.shape[0], -1).numpy()
    return _ref_cache[key]


@pytest.mark.parametrize('band_rows', [8, 16])
@pytest.mark.parametrize('dtype,layout', OUTS)
def test_set_blocks_from_host_rest_from_mirror(dev, dtype, layout, band_rows):
    masks = _masks(band_rows)
    names = list(masks)
    # 9 images per launch: image 0 without a mirror, then every named mask; flipped and upright mixed
    flip_bits = 0b101101010
    for Cin, ch in ((3, 'bgr'), (4, 'rgb')):
        store = frames(1 + len(names), H, W, Cin, seed=700 + Cin)
        cfg = _vcfg(ch, dtype, layout)
        d = _Blocks(dev, store, cfg, band_rows, [masks[n] for n in names], flip_bits)
        try:
            d.launch()
            d.check('/'.join(names), _reference(store, cfg, flip_bits, (Cin, ch, dtype, layout)))
        finally:
            d.close()


def test_rejections_launch_nothing(dev):
    cfg = _vcfg('rgb', 'float32', 'nchw')
    store = frames(3, H, W, 4, seed=77)
    good = _masks(8)
    d = _Blocks(dev, store, cfg, 8, [good['checkerboard'], good['random']], 0b010)
    try:
        with pytest.raises((RuntimeError, ValueError)):
            d.launch(B=33)                                                         # more than 32 images: the library refuses
        d.untouched()
        for br in (12, 0, -8):                                                     # no power of two
            with pytest.raises((RuntimeError, ValueError)):
                d.launch(band_rows=br)
            d.untouched()
        with pytest.raises((RuntimeError, ValueError)):
            d.launch(band_rows=1, masks=[[0] * 30] * 3)                            # 40 bands of one row: more than 30
        d.untouched()
        with pytest.raises((RuntimeError, ValueError)):
            d.launch(masks=[[0] * 31] * 3)                                         # 31 words
        d.untouched()
        with pytest.raises((RuntimeError, ValueError)):
            d.launch(W_=200)                                                       # W % 64 != 0
        d.untouched()
        with pytest.raises((RuntimeError, ValueError)):
            d.launch(masks=[d.masks[0], [0b1000] + [0] * 4, d.masks[2]])           # column block 3 of 3
        d.untouched()
        with pytest.raises((RuntimeError, ValueError)):
            d.launch(masks=[d.masks[0], [0] * 5 + [1], d.masks[2]])                # band 5 of 5
        d.untouched()
        d.launch()
        d.check('after the rejections', _reference(store, cfg, 0b010, 'rejections'))
    finally:
        d.close()


# ---- loader -------------------------------------------------------------------------------------------------------

B, NBATCH = 4, 12
FH, FW = 64, 128
SEED = 11
_true = {}


def _args(*extra):
    return ['--mode', 'rgba', '--resolution', f'{FW}x{FH}', '--stamp', '--shm', '4', *extra]


PRODUCERS = [_args('--fps', '300'), _args('--fps', '300')]   # paced: both rings pass over their 4 slots several times
# one batch of more than 32 images: 24 slots per ring, so that 40 frames can be held at once, and enough
# batches that every slot is used about six times (its first uses carry no report: before the hints, at
# the layout flip, and the one that fills the mirror)
BIG_B, BIG_NBATCH = 40, 8
BIG_PRODUCERS = [_args('--shm', '24'), _args('--shm', '24')]


def _true_frames(port, producers=PRODUCERS, n=B * NBATCH):
    """{(btid, seq): H x W x 4 frame} of the first n frames of each producer, through the CPU path: random
    poses from the launcher's seeds, so a producer's frame ``seq`` is the same in every run."""
    key = (tuple(map(tuple, producers)), n)
    if key not in _true:
        out = _true[key] = {}
        with btt.BlenderLauncher(producer='cubesim', num_instances=2, named_sockets=['DATA'], start_port=port,
                                 proto='ipc', seed=SEED, instance_args=producers) as bl:
            for addr in bl.launch_info.addresses['DATA']:
                s = zmq.Context().socket(zmq.PULL)
                s.connect(addr)
                for _ in range(n):
                    assert s.poll(20000)
                    msg = shm.resolve(s.recv_pyobj(), strict=True)
                    out[(int(msg['btid']), int(msg['seq']))] = np.ascontiguousarray(msg['image'])
                s.close()
    return _true[key]


def _rgb():
    return DecodeConfig.unit(channels='rgb', gamma=2.2)


def _run(dev, port, cfg, producers=PRODUCERS, batch=B, nbatch=NBATCH):
    """{(btid, seq): decoded image (cpu)} of batch * nbatch frames, and the loader's stats."""
    out = {}
    with btt.BlenderLauncher(producer='cubesim', num_instances=2, named_sockets=['DATA'], start_port=port,
                             proto='ipc', seed=SEED, instance_args=producers) as bl:
        dl = DeviceLoader(bl.launch_info.addresses['DATA'], batch_size=batch, max_items=batch * nbatch, device=dev,
                          decode=cfg, slot_mirror=True)
        for b in dl:
            img = b['image'].cpu()
            for k in range(batch):
                out[(int(b['btid'][k]), int(b['seq'][k]))] = img[k]
        st = dict(dl.stats)
    assert len(out) == batch * nbatch and st['bad'] == 0 and st['batches'] == nbatch and st['shm_torn'] == 0
    return out, st


def _check(got, true, cfg):
    keys = sorted(got)
    ref = ops.reference_decode(torch.from_numpy(np.stack([true[k] for k in keys])), cfg, flip=[0] * len(keys))
    for i, key in enumerate(keys):
        assert torch.equal(got[key], ref[i]), key


def test_stream_over_two_block_producers_matches_the_oracle(dev, free_port, monkeypatch):
    true = _true_frames(free_port)
    assert len({f.tobytes()[16:] for f in true.values()}) > B * NBATCH         # the poses do differ
    got, st = _run(dev, free_port + 5, _rgb())
    _check(got, true, _rgb())
    assert st['block_frames'] > 0 and st['delta_frames'] >= st['block_frames'], st
    assert st['direct_batches'] == st['batches'], st
    # the rectangle path over the same producers (the switch is read when a loader is made): same
    # images, and more bytes over the link for as many frames
    monkeypatch.setenv('BT_SLOT_BLOCKS', '0')
    rgot, rst = _run(dev, free_port + 10, _rgb())
    _check(rgot, true, _rgb())
    assert rst['block_frames'] == 0 and rst['delta_frames'] > 0, rst
    assert rst['frames'] == st['frames'] == B * NBATCH
    assert st['image_bytes'] < rst['image_bytes'], (st, rst)


@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
def test_a_batch_of_more_than_32_images_is_split_in_two_launches(dev, free_port, layout):
    """One dense batch of 40 mirrored images: the block launch holds 32, so the batch takes two, the second
    writing output images 32..39 -- every image of every batch equals the oracle of its own frame."""
    cfg = DecodeConfig.unit(channels='rgb', gamma=2.2, layout=layout)
    n = BIG_B * BIG_NBATCH
    true = _true_frames(free_port, BIG_PRODUCERS, n)                            # either producer may supply up to all
    got, st = _run(dev, free_port + 5, cfg, BIG_PRODUCERS, BIG_B, BIG_NBATCH)
    _check(got, true, cfg)
    assert len({v.numpy().tobytes() for v in got.values()}) == n                # no image stands in for another
    assert st['block_frames'] > 0 and st['direct_batches'] == st['batches'] == BIG_NBATCH, st
