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
import numpy as np
import pytest
import torch

from decode_oracle import MirrorLaunch, frames
from test_gpu_slot_delta import _Delta
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


def _inside(mask, band_rows, Cin, H=H, W=W):
    m = np.zeros((H, W, Cin), bool)
    for k, word in enumerate(mask):
        for c in range(W // 64):
            if (word >> c) & 1:
                m[k * band_rows:(k + 1) * band_rows, 64 * c:64 * c + 64] = True
    return m


def _launch(d, B=None, band_rows=None, masks=None, W_=None):
    masks = d.masks if masks is None else masks
    B = d.B if B is None else B
    last = d.B - 1
    ops.hip_ext().decode_delta_blocks(
        [d.host_dev + min(b, last) * d.fb for b in range(B)],
        [0 if b == 0 else d.mir.data_ptr() + d.mir_off[min(b, last)] for b in range(B)],
        d.band_rows if band_rows is None else band_rows,
        [masks[min(b, last)] for b in range(B)], 0, ops.device_lut(d.cfg, d.dev).data_ptr(),
        B, d.H, d.W if W_ is None else W_, d.Cin, d.cfg.cout, list(d.cfg.cmap), 0,
        ops.OUT_DTYPES[d.cfg.dtype], ops.LAYOUTS[d.cfg.layout], ops._stream(d.dev),
        dsts=[d.outs[d.dst[min(b, last)][0]].data_ptr() + d.dst[min(b, last)][1] for b in range(B)],
        flip_bits=[d.flip_bits])


def _Blocks(dev, store, cfg, band_rows, masks, flip_bits):
    """One decode_delta_blocks launch; image 0 has no mirror, images 1.. use ``masks``."""
    _, h, w, Cin = store.shape
    d = MirrorLaunch(dev, store, cfg, [_inside(m, band_rows, Cin, h, w) for m in masks], _launch, flip_bits)
    d.band_rows = band_rows
    d.masks = [[0] * len(masks[0])] + [list(m) for m in masks]
    d.label = f'band_rows {band_rows} masks {d.masks}'
    return d


_ref_cache = {}


def _reference(d, key):
    """The launch's reference bytes per image; computed once per (frames, config)."""
    if key not in _ref_cache:
        _ref_cache[key] = d.reference()
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
            d.check('/'.join(names), _reference(d, (Cin, ch, dtype, layout)))
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
        d.check('after the rejections', _reference(d, 'rejections'))
    finally:
        d.close()


def _rect_blocks(region, nb, band_rows):
    """slot_mirror.h rect_blocks on a grid of ``band_rows``: the blocks a (widened) region touches."""
    y0, y1, x0, x1 = region
    bits = (2 << (x1 // 64)) - (1 << (x0 // 64)) if y1 >= y0 else 0
    return [bits if y0 // band_rows <= k <= y1 // band_rows else 0 for k in range(nb)]


@pytest.mark.parametrize('dtype,layout', [('float32', 'nchw'), ('uint8', 'nhwc')])
@pytest.mark.parametrize('Cin,ch', [(3, 'bgr'), (4, 'rgb')])
def test_a_rectangle_read_and_its_block_read_agree(dev, Cin, ch, dtype, layout):
    """The loader hands a rectangle-only producer's frames to the block read (rect_blocks): both reads of
    one rectangle on band and 64-column boundaries, over identical poisoned inputs, leave identical
    output and mirror bytes, equal to the reference.  Image 0 has no mirror, image 1 is flipped."""
    RH, RW, band_rows, flip_bits = 24, 128, 8, 0b010
    store = frames(3, RH, RW, Cin, seed=1200 + Cin)
    cfg = _vcfg(ch, dtype, layout)
    for regions in ([(8, 15, 64, 127), (0, -1, 0, -1)], [(0, RH - 1, 0, RW - 1), (8, 15, 64, 127)]):
        r = _Delta(dev, store, cfg, regions, flip_bits)
        b = _Blocks(dev, store, cfg, band_rows, [_rect_blocks(g, RH // band_rows, band_rows) for g in regions], flip_bits)
        try:
            assert np.array_equal(r.mir0, b.mir0) and np.array_equal(r.host0, b.host0)
            r.launch()
            b.launch()
            ref = r.reference()
            r.check('rectangle read', ref)
            b.check('block read', ref)
            assert all(torch.equal(x, y) for x, y in zip(r.outs, b.outs)) and torch.equal(r.mir, b.mir)
        finally:
            r.close()
            b.close()


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
