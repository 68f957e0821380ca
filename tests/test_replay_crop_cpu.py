"""Crop, mirror and random shift (replicate pad) on the replay path, without a GPU:
the numpy reference of the kernel's window draw (``ops.philox_windows``), the
CPU ``DeviceReplayBuffer`` with crop configs, ``reference_decode`` with a pad
against an independent ``np.pad`` formulation, and the argument checks."""
import dataclasses

import numpy as np
import pytest
import torch

from blendtorch import ops
from blendtorch.btt.gpu import DeviceLoader
from blendtorch.btt.replay import DeviceReplayBuffer
from blendtorch.ops import Crop, DecodeConfig

H, W = 7, 32
SEED = 20240


def _legal(win, crop, H, W):
    h, w = crop.size
    p = crop.pad
    return bool(((win[:, 0] >= -p) & (win[:, 0] <= H + p - h) & (win[:, 1] >= -p) & (win[:, 1] <= W + p - w)
                 & ((win[:, 2] == 0) | (win[:, 2] == 1))).all())


# ---- philox_windows -----------------------------------------------------------------------------------------------

def test_philox_windows_deterministic_and_legal():
    crop = Crop((4, 16), mirror=0.5, seed=3)
    a = ops.philox_windows(SEED, 17, 64, crop, H, W)
    b = ops.philox_windows(SEED, 17, 64, crop, H, W)
    assert a.dtype == np.int32 and a.shape == (64, 3) and np.array_equal(a, b)
    assert _legal(a, crop, H, W)
    # every legal origin and both mirror values occur in 64 draws of 4 x 17 origins? not required: a spread is
    assert len({tuple(r) for r in a}) > 32 and 0 < a[:, 2].sum() < 64
    # images of one launch differ, and so do consecutive counters
    assert not np.array_equal(a[:32], a[32:])
    assert not np.array_equal(a, ops.philox_windows(SEED, 18, 64, crop, H, W))
    # a prefix of a longer launch is the shorter launch (image b depends on (b, counter) only)
    assert np.array_equal(ops.philox_windows(SEED, 17, 9, crop, H, W), a[:9])


def test_crop_seed_changes_windows_not_indices():
    a = ops.philox_windows(SEED, 5, 32, Crop((4, 16), mirror=0.5, seed=0), H, W)
    b = ops.philox_windows(SEED, 5, 32, Crop((4, 16), mirror=0.5, seed=1), H, W)
    assert not np.array_equal(a, b)
    # the key is (buffer seed + crop seed) mod 2**64
    assert np.array_equal(b, ops.philox_windows(SEED + 1, 5, 32, Crop((4, 16), mirror=0.5, seed=0), H, W))
    assert np.array_equal(ops.philox_windows(2 ** 64 - 1, 5, 8, Crop((4, 16), seed=3), H, W),
                          ops.philox_windows(2, 5, 8, Crop((4, 16), seed=0), H, W))
    # the index draw has no crop in it: same function, same arguments, and word 3 of its counter stays 0
    idx = ops.philox_indices(SEED, 5, 32, 1000)
    assert np.array_equal(idx, ops.philox_indices(SEED, 5, 32, 1000))
    assert np.array_equal(ops._philox_blocks(SEED, 5, 32, 0)[0] * np.uint64(1000) >> np.uint64(32), idx.astype(np.uint64))
    assert not np.array_equal(ops._philox_blocks(SEED, 5, 32, 1)[0], ops._philox_blocks(SEED, 5, 32, 0)[0])


def test_mirror_probabilities_and_alignment():
    assert ops.philox_windows(SEED, 0, 128, Crop((4, 16), mirror=0.0), H, W)[:, 2].sum() == 0
    assert ops.philox_windows(SEED, 0, 128, Crop((4, 16), mirror=1.0), H, W)[:, 2].sum() == 128
    a = ops.philox_windows(SEED, 0, 128, Crop((4, 16), mirror=0.5, x_align=4), H, W)
    assert (a[:, 1] % 4 == 0).all() and set(a[:, 1]) == {0, 4, 8, 12, 16} and _legal(a, Crop((4, 16)), H, W)


def test_philox_formula_word_for_word():
    crop = Crop((3, 12), mirror=0.25, seed=9, x_align=4)
    o0, o1, o2, _ = ops._philox_blocks((SEED + 9) & (2 ** 64 - 1), (7 << 32) | 11, 16, 1)
    win = ops.philox_windows(SEED, (7 << 32) | 11, 16, crop, H, W)
    for b in range(16):
        assert win[b, 0] == (int(o0[b]) * (H - 3 + 1)) >> 32
        assert win[b, 1] == ((int(o1[b]) * ((W - 12) // 4 + 1)) >> 32) * 4
        assert win[b, 2] == ((int(o2[b]) >> 8) < int(0.25 * 2 ** 24))


def test_pad_shift_covers_all_offsets():
    """pad = 2 on the full-size window: origins in [-2, 2]^2, and 256 images of this seed hold all 25."""
    crop = Crop((H, W), pad=2)
    a = ops.philox_windows(SEED, 0, 256, crop, H, W)
    assert _legal(a, crop, H, W) and a[:, :2].min() == -2 and a[:, :2].max() == 2 and a[:, 2].sum() == 0
    assert len({(int(y), int(x)) for y, x, _ in a}) == 25


def test_replay_windows_center_and_fixed_are_the_stream_windows():
    for crop in (Crop((4, 16), mode='center', x_align=4), Crop((3, 5), origin=(2, 9))):
        assert np.array_equal(ops.replay_windows(crop, H, W, 5, seed=SEED, counter=3), ops.crop_windows(crop, H, W, 5))
    with pytest.raises(ValueError):
        ops.philox_windows(SEED, 0, 4, Crop((4, 16), mode='center'), H, W)


# ---- the CPU DeviceReplayBuffer ------------------------------------------------------------------------------------

def _buffer(seed=77, C=4):
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, size=(6, H, W, C), dtype=np.uint8)
    rb = DeviceReplayBuffer(6, device='cpu', seed=seed)
    rb.extend(frames, frameid=np.arange(6) * 10, xy=rng.normal(size=(6, 2)).astype(np.float32))
    return rb, frames


CFGS = [
    DecodeConfig.unit(channels='rgb', gamma=2.2, crop=Crop((4, 16), mirror=0.5, seed=4)),
    DecodeConfig.densityopt(channels='bgr', dtype='bfloat16', layout='nhwc', crop=Crop((H, W), pad=3, mirror=0.5)),
    DecodeConfig.raw(channels='rgba', crop=Crop((5, 30), pad=2, seed=1), flip=True),
]


def _check_batch(rb, b, cfg, want_win):
    idx = b['index']
    assert b['crop'].dtype == torch.int32 and tuple(b['crop'].shape) == (len(idx), 3)
    assert np.array_equal(b['crop'].numpy(), want_win)
    ref = ops.reference_decode(rb.store[idx], cfg, crop=b['crop'])
    assert b['image'].shape == ref.shape and b['image'].dtype == ref.dtype
    assert torch.equal(b['image'].view(torch.uint8), ref.view(torch.uint8))
    assert torch.equal(b['frameid'], rb.meta['frameid'][idx]) and torch.equal(b['xy'], rb.meta['xy'][idx])


@pytest.mark.parametrize('cfg', CFGS, ids=['f32-crop', 'bf16-shift', 'u8-pad-flip'])
def test_cpu_buffer_sample_gather_batches(cfg):
    rb, _ = _buffer()
    c0 = rb._ctr
    b = rb.sample(5, cfg)
    assert np.array_equal(b['index'].numpy(), ops.philox_indices(rb.seed, c0, 5, 6))
    _check_batch(rb, b, cfg, ops.philox_windows(rb.seed, c0, 5, cfg.crop, H, W))
    assert rb._ctr == c0 + 5
    b = rb.gather(torch.tensor([5, 0, 5]), cfg)
    assert b['index'].tolist() == [5, 0, 5]
    _check_batch(rb, b, cfg, ops.philox_windows(rb.seed, c0 + 5, 3, cfg.crop, H, W))
    assert rb._ctr == c0 + 8
    g = torch.Generator().manual_seed(1)
    seen = []
    for k, b in enumerate(rb.batches(4, cfg, generator=g, drop_last=False)):
        n = len(b['index'])
        _check_batch(rb, b, cfg, ops.philox_windows(rb.seed, c0 + 8 + 4 * k, n, cfg.crop, H, W))
        seen += b['index'].tolist()
    assert sorted(seen) == list(range(6)) and rb._ctr == c0 + 8 + 6
    # a torch.Generator gives the indices as without a crop; the windows stay the buffer's Philox draw
    g1, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    b = rb.sample(4, cfg, generator=g1)
    assert torch.equal(b['index'], torch.randint(0, 6, (4,), generator=g2))
    _check_batch(rb, b, cfg, ops.philox_windows(rb.seed, c0 + 14, 4, cfg.crop, H, W))


def test_same_seed_same_batches_and_graphed_sampler_on_cpu():
    cfg = CFGS[0]
    a, _ = _buffer(seed=9)
    b, _ = _buffer(seed=9)
    fa = a.graphed_sampler(3, cfg)
    for _ in range(3):
        x, y = fa(), b.sample(3, cfg)
        assert torch.equal(x['image'], y['image']) and torch.equal(x['crop'], y['crop'])
        assert torch.equal(x['index'], y['index'])
    c, _ = _buffer(seed=10)
    assert not torch.equal(c.sample(6, cfg)['crop'], _buffer(seed=9)[0].sample(6, cfg)['crop'])


def test_gather_without_a_random_crop_leaves_the_counter():
    rb, _ = _buffer()
    idx = torch.tensor([1, 4, 4, 2])
    for crop in (Crop((4, 16), mode='center', x_align=4), Crop((3, 5), origin=(2, 9))):
        cfg = DecodeConfig.unit(channels='rgb', crop=crop)
        c0 = rb._ctr
        b = rb.gather(idx, cfg)
        assert rb._ctr == c0
        _check_batch(rb, b, cfg, ops.crop_windows(crop, H, W, 4))
        assert (b['crop'][:, 2] == 0).all()
    c0 = rb._ctr
    rb.gather(idx, DecodeConfig.unit(channels='rgb'))
    assert rb._ctr == c0
    # sample advances by the batch as the fused sample does, crop or not
    rb.sample(4, DecodeConfig.unit(channels='rgb', crop=Crop((4, 16), mode='center')))
    assert rb._ctr == c0 + 4


def test_given_windows_are_used_verbatim_and_checked():
    rb, _ = _buffer()
    cfg = DecodeConfig.unit(channels='rgb', gamma=2.2, crop=Crop((H, W), pad=3))
    win = np.array([[-3, -3, 0], [3, 3, 1], [0, -1, 1], [-2, 2, 0]], np.int32)
    idx = torch.tensor([0, 5, 2, 2])
    c0 = rb._ctr
    for given in (win, torch.from_numpy(win), win.tolist()):
        b = rb.gather(idx, cfg, windows=given)
        _check_batch(rb, b, cfg, win)
    assert rb._ctr == c0                                   # nothing was drawn
    for bad in ([-4, 0, 0], [0, 4, 0], [4, 0, 1], [0, 0, 2], [0, -4, 0]):
        w = win.copy()
        w[2] = bad
        with pytest.raises(ValueError):
            rb.gather(idx, cfg, windows=w)
    with pytest.raises(ValueError):
        rb.gather(idx, cfg, windows=win[:3])
    with pytest.raises(ValueError):
        rb.gather(idx, cfg, windows=win.astype(np.float32))
    with pytest.raises(ValueError):
        rb.gather(idx, DecodeConfig.unit(channels='rgb'), windows=win)
    # without a pad the legal range is the frame
    small = DecodeConfig.unit(channels='rgb', crop=Crop((4, 16), mode='center'))
    b = rb.gather(idx, small, windows=[[3, 16, 1], [0, 0, 0], [1, 7, 1], [2, 9, 0]])
    assert b['crop'].tolist() == [[3, 16, 1], [0, 0, 0], [1, 7, 1], [2, 9, 0]]
    with pytest.raises(ValueError):
        rb.gather(idx, small, windows=[[4, 16, 1], [0, 0, 0], [1, 7, 1], [2, 9, 0]])
    with pytest.raises(ValueError):
        rb.gather(idx, small, windows=[[3, -1, 0], [0, 0, 0], [1, 7, 1], [2, 9, 0]])


def test_crop_points_follow_the_shifted_window():
    """A pixel of the frame that lies inside the window lands where crop_points says."""
    rb, frames = _buffer()
    cfg = DecodeConfig(channels='rgba', dtype='uint8', layout='nchw', crop=Crop((H, W), pad=2, mirror=0.5, seed=6))
    b = rb.sample(6, cfg)
    assert 0 < int(b['crop'][:, 2].sum()) < 6
    pts = np.tile(np.array([[[10.0, 3.0]]]), (6, 1, 1))           # (x, y) = (10, 3): inside every shifted window
    out = ops.crop_points(pts, b['crop'], cfg.crop.size)
    for k in range(6):
        x, y = int(out[k, 0, 0]), int(out[k, 0, 1])
        assert np.array_equal(b['image'][k][:, y, x].numpy(), frames[int(b['index'][k])][3, 10])


# ---- reference_decode with a pad against np.pad -------------------------------------------------------------------

@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('dtype', ['float32', 'bfloat16', 'uint8'])
def test_pad_reference_against_np_pad(dtype, layout):
    rng = np.random.default_rng(8)
    x = torch.from_numpy(rng.integers(0, 256, size=(6, H, W, 3), dtype=np.uint8))
    pad = 3
    kw = dict(channels='bgr', gamma=2.2, dtype=dtype, layout=layout)
    cfg = DecodeConfig(**kw, crop=Crop((5, 20), pad=pad)) if dtype == 'uint8' else \
        DecodeConfig.densityopt(**kw, crop=Crop((5, 20), pad=pad))
    # leaves the frame at the top, bottom, left, right, a corner (mirrored), and not at all
    win = [(-3, 4, 0), (H + pad - 5, 6, 1), (1, -2, 1), (0, W + pad - 20, 0), (-2, -3, 1), (1, 5, 1)]
    got = ops.reference_decode(x, cfg, crop=win)
    full = ops.reference_decode(x, dataclasses.replace(cfg, crop=None))
    raw = full.view(torch.int16).numpy() if dtype == 'bfloat16' else full.numpy()
    widths = ((0, 0), (0, 0), (pad, pad), (pad, pad)) if layout == 'nchw' else ((0, 0), (pad, pad), (pad, pad), (0, 0))
    padded = np.pad(raw, widths, mode='edge')
    g = got.view(torch.int16).numpy() if dtype == 'bfloat16' else got.numpy()
    for b, (y0, x0, m) in enumerate(win):
        ys, xs = slice(y0 + pad, y0 + pad + 5), slice(x0 + pad, x0 + pad + 20)
        want = padded[b][:, ys, xs] if layout == 'nchw' else padded[b][ys, xs]
        if m:
            want = want[:, :, ::-1] if layout == 'nchw' else want[:, ::-1]
        assert np.array_equal(g[b], want), (b, y0, x0, m)
    with pytest.raises(ValueError):
        ops.reference_decode(x, cfg, crop=[(-4, 0, 0)] + win[1:])
    with pytest.raises(ValueError):
        ops.reference_decode(x, cfg, crop=[(0, W + pad - 19, 0)] + win[1:])


def test_pad_zero_reference_is_untouched():
    x = torch.from_numpy(np.random.default_rng(2).integers(0, 256, size=(2, H, W, 4), dtype=np.uint8))
    cfg = DecodeConfig.unit(channels='rgb', crop=Crop((4, 16)))
    out = ops.reference_decode(x, cfg, crop=[(3, 16, 1), (0, 0, 0)])
    full = ops.reference_decode(x, DecodeConfig.unit(channels='rgb'))
    assert torch.equal(out[0], torch.flip(full[0][:, 3:7, 16:32], dims=[2])) and torch.equal(out[1], full[1][:, :4, :16])
    with pytest.raises(ValueError):
        ops.reference_decode(x, cfg, crop=[(-1, 0, 0), (0, 0, 0)])


# ---- validation ---------------------------------------------------------------------------------------------------

def test_crop_pad_validation():
    assert Crop((4, 16)).pad == 0 and Crop((4, 16), pad=2).pad == 2
    for kw in (dict(pad=-1), dict(pad=1, x_align=4), dict(pad=1, origin=(0, 0)), dict(pad=1, mode='center'),
               dict(pad=1.5), dict(pad=16384)):
        with pytest.raises(ValueError):
            Crop((4, 16), **kw)
    c = Crop((H + 4, W + 4), pad=2)
    c.check_frame(H, W)
    assert DecodeConfig.unit(channels='rgb', crop=c).out_shape(3, H, W) == (3, 3, H + 4, W + 4)
    with pytest.raises(ValueError):
        Crop((H + 5, W), pad=2).check_frame(H, W)
    with pytest.raises(ValueError):
        Crop((H, W + 5), pad=2).check_frame(H, W)
    with pytest.raises(ValueError):
        Crop((4, 16), pad=2).check_frame(32764, 64)          # H + 2 * pad > 32767
    Crop((4, 16), pad=2).check_frame(32763, 64)


def test_the_stream_side_rejects_a_pad():
    crop = Crop((4, 16), pad=1)
    cfg = DecodeConfig.unit(channels='rgb', crop=crop)
    with pytest.raises(ValueError, match='replay path only'):
        ops.crop_windows(crop, H, W, 4)
    with pytest.raises(ValueError, match='replay path only'):
        DeviceLoader(['ipc:///tmp/never-opened'], batch_size=4, device='cpu', decode=cfg)
    # ops.decode: the argument check comes first, before the extension or the tensor is looked at
    with pytest.raises(ValueError, match='replay path only'):
        ops.decode(torch.zeros(2, H, W, 4, dtype=torch.uint8), cfg, crop=[(0, 0, 0)] * 2)
