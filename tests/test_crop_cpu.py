"""Crop + mirror on the CPU: the ``ops.Crop`` / ``DecodeConfig(crop=)``
validation, the window draw (``ops.crop_windows`` against the native
``_native.crop_draw`` the stream loader shares, csrc/common/crop_draw.h), the
reference decode through a window, and ``ops.crop_points``."""
import dataclasses

import numpy as np
import pytest
import torch

from blendtorch import _native, ops
from blendtorch.ops import Crop, DecodeConfig

H, W = 48, 64
SMALL, FULL = (16, 32), (48, 64)
# Picked with the pure-Python draw (ops.crop_windows, the reference draw): the
# first five seeds, none a shifted copy of another, whose 200 windows of the
# 16x32 crop hit BOTH extreme origins -- (0, 0) and (H - h, W - w rounded down
# to x_align) -- for every x_align, and mirror between 35 % and 65 % of the
# images at mirror = 0.5.  Few seeds do: one corner is one of 33 x 33 origins,
# and the streams of seeds s and s + 1 are one draw apart (the state is
# seed * golden + constant, advanced by golden per draw), so qualifying seeds
# come in runs.  The native draw is then held to the same windows.
SEEDS = (2795, 8853, 15149, 17437, 17930)
N = 200


def _native_draw(c, H, W, n):
    return _native.crop_draw(c.seed, H, W, c.size[0], c.size[1], c.mirror, c.x_align, c.kind, n,
                             origin=c.origin or (0, 0))


# ---- validation ---------------------------------------------------------------------------------------------------

def test_crop_is_a_frozen_validated_dataclass():
    c = Crop(size=[16, 32], mirror=0.5, seed=3, x_align=4)
    assert c.size == (16, 32) and c.kind == 'random' and hash(c) == hash(Crop((16, 32), mirror=0.5, seed=3, x_align=4))
    with pytest.raises(dataclasses.FrozenInstanceError):
        c.mirror = 0.1
    assert Crop((4, 4), origin=[2, 3]).kind == 'fixed' and Crop((4, 4), origin=[2, 3]).origin == (2, 3)
    assert Crop((4, 4), mode='center').kind == 'center'
    for bad in (dict(size=(0, 4)), dict(size=(4, -1)), dict(size=(4,)), dict(size=4), dict(size=(4, 40000)),
                dict(size=(4, 4), mode='corner'), dict(size=(4, 4), mirror=-0.1), dict(size=(4, 4), mirror=1.5),
                dict(size=(4, 4), x_align=2), dict(size=(4, 4), x_align=0), dict(size=(4, 4), x_align=8),
                dict(size=(4, 4), origin=(-1, 0)), dict(size=(4, 4), origin=(1,)),
                dict(size=(4, 4), mode='center', mirror=0.5), dict(size=(4, 4), origin=(0, 0), mirror=0.5)):
        with pytest.raises(ValueError):
            Crop(**bad)
    for ok in (dict(mirror=0.0), dict(mirror=1.0), dict(x_align=1), dict(x_align=4), dict(x_align=16)):
        Crop((4, 4), **ok)


def test_decode_config_with_a_crop():
    crop = Crop((16, 32), mirror=0.5)
    cfg = DecodeConfig.unit(channels='rgb', gamma=2.2, crop=crop)
    assert cfg.out_shape(8, H, W) == (8, 3, 16, 32)
    assert DecodeConfig(channels='rgba', layout='nhwc', dtype='uint8', crop=crop).out_shape(2, H, W) == (2, 16, 32, 4)
    assert DecodeConfig().out_shape(8, H, W) == (8, 3, H, W)                 # unchanged without one
    assert cfg.out_shape(1, 16, 32) == (1, 3, 16, 32)                        # the window may be the frame
    assert hash(cfg) == hash(DecodeConfig.unit(channels='rgb', gamma=2.2, crop=Crop((16, 32), mirror=0.5)))
    with pytest.raises(TypeError):
        DecodeConfig(crop=(16, 32))
    eye = np.eye(4).tolist()
    for colour in (dict(color_matrix=eye), dict(color_matrices=[eye, eye]),
                   dict(channels='rgb', color_jitter=ops.ColorJitter(brightness=0.1))):
        with pytest.raises(ValueError, match='crop'):
            DecodeConfig(crop=crop, **colour)
    # a window larger than the frame: raised where the frame size is first known
    for shape in ((15, 64), (48, 31)):
        with pytest.raises(ValueError, match=r'16x32.*does not fit.*' + f'{shape[0]}x{shape[1]}'):
            cfg.out_shape(8, *shape)
        with pytest.raises(ValueError, match='does not fit'):
            ops.crop_windows(crop, *shape, 4)
    with pytest.raises(ValueError, match='does not fit'):
        DecodeConfig(crop=Crop((16, 32), origin=(33, 0))).out_shape(1, H, W)
    with pytest.raises(ValueError):
        _native.crop_draw(0, 15, 64, 16, 32, 0.5, 1, 'random', 4)
    with pytest.raises(ValueError):
        _native.crop_draw(0, H, W, 16, 32, 0.5, 1, 'fixed', 4, origin=(33, 0))
    # kernels without a crop path refuse the config instead of writing whole frames into a window-sized tensor
    with pytest.raises(ValueError, match='crop'):
        ops.decode_lut_bf16(DecodeConfig(channels='rgba', crop=crop), 'cpu')


# ---- the draw -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('x_align', [1, 4, 16])
@pytest.mark.parametrize('seed', SEEDS)
def test_random_windows(seed, x_align):
    for size in (SMALL, FULL):
        c = Crop(size, mirror=0.5, seed=seed, x_align=x_align)
        win = ops.crop_windows(c, H, W, N)
        assert win.dtype == np.int32 and win.shape == (N, 3)
        nat = _native_draw(c, H, W, N)
        assert nat.dtype == np.int32 and np.array_equal(win, nat)
        h, w = size
        y0, x0, m = win.T
        assert (y0 >= 0).all() and (y0 + h <= H).all() and (x0 >= 0).all() and (x0 + w <= W).all()
        assert (x0 % x_align == 0).all() and set(np.unique(m)) <= {0, 1}
        assert 0.35 <= m.mean() <= 0.65
        if size == FULL:
            assert not y0.any() and not x0.any()
        else:
            xmax = (W - w) // x_align * x_align
            assert ((y0 == 0) & (x0 == 0)).any() and ((y0 == H - h) & (x0 == xmax)).any()


@pytest.mark.parametrize('seed', SEEDS)
def test_the_stream_is_its_own_and_a_prefix_is_a_prefix(seed):
    c = Crop(SMALL, mirror=0.5, seed=seed)
    win = ops.crop_windows(c, H, W, N)
    assert np.array_equal(ops.crop_windows(c, H, W, 7), win[:7])            # arrival order: three draws per image
    assert not np.array_equal(ops.crop_windows(dataclasses.replace(c, seed=seed + 1), H, W, N), win)
    # mirror = 0 and 1 are certain, and the mirror draw does not shift the origins
    for p, want in ((0.0, 0), (1.0, 1)):
        w2 = ops.crop_windows(dataclasses.replace(c, mirror=p), H, W, N)
        assert (w2[:, 2] == want).all() and np.array_equal(w2[:, :2], win[:, :2])
        assert np.array_equal(_native_draw(dataclasses.replace(c, mirror=p), H, W, N), w2)


@pytest.mark.parametrize('x_align', [1, 4, 16])
@pytest.mark.parametrize('seed', SEEDS)
def test_center_and_fixed_windows(seed, x_align):
    for size in (SMALL, FULL, (15, 21)):
        h, w = size
        c = Crop(size, mode='center', seed=seed, x_align=x_align)
        win = ops.crop_windows(c, H, W, N)
        assert np.array_equal(win, _native_draw(c, H, W, N))
        assert (win == [(H - h) // 2, (W - w) // 2 // x_align * x_align, 0]).all()
        for origin in ((0, 0), (H - h, W - w), (min(3, H - h), min(5, W - w))):
            c = Crop(size, origin=origin, seed=seed, x_align=x_align)
            win = ops.crop_windows(c, H, W, N)
            assert np.array_equal(win, _native_draw(c, H, W, N))
            assert (win == [origin[0], origin[1], 0]).all()


# ---- the reference decode through a window ------------------------------------------------------------------------

@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('dtype', ['float32', 'bfloat16', 'uint8'])
def test_reference_decode_crop_is_slice_and_mirror(dtype, layout):
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.integers(0, 256, size=(4, 9, 12, 4), dtype=np.uint8))
    norm = {} if dtype == 'uint8' else dict(mean=(127.5,) * 4, std=(127.5,) * 4)
    base = DecodeConfig(channels='bgr', gamma=2.2, dtype=dtype, layout=layout, **norm)
    cfg = dataclasses.replace(base, crop=Crop((5, 6)))
    flip = [1, 0, 1, 0]
    win = [(4, 6, 1), (0, 0, 0), (2, 3, 0), (1, 5, 1)]                         # image 0: flipped AND mirrored
    full = ops.reference_decode(x, base, flip=flip)
    got = ops.reference_decode(x, cfg, flip=flip, crop=win)
    assert got.shape == cfg.out_shape(4, 9, 12) and got.dtype == cfg.torch_dtype()
    for b, (y0, x0, m) in enumerate(win):
        ref = full[b][:, y0:y0 + 5, x0:x0 + 6] if layout == 'nchw' else full[b][y0:y0 + 5, x0:x0 + 6]
        if m:
            ref = torch.flip(ref, dims=[2 if layout == 'nchw' else 1])
        assert torch.equal(got[b], ref), b
    # the flipped source: window row i is stored frame row H - 1 - (y0 + i)
    b, (y0, x0, _) = 0, win[0]
    rows = x[b, [9 - 1 - (y0 + i) for i in range(5)]][:, x0:x0 + 6].flip(1)
    again = ops.reference_decode(rows[None], base)[0]
    assert torch.equal(got[b], again)
    # tensors and arrays are windows too; wrong shapes, windows outside the frame and stray windows are errors
    assert torch.equal(ops.reference_decode(x, cfg, flip=flip, crop=torch.tensor(win)), got)
    assert torch.equal(ops.reference_decode(x, cfg, flip=flip, crop=np.asarray(win, np.int32)), got)
    for bad in (None, win[:3], [(5, 0, 0)] * 4, [(0, 7, 0)] * 4, [(-1, 0, 0)] * 4):
        with pytest.raises(ValueError):
            ops.reference_decode(x, cfg, flip=flip, crop=bad)
    with pytest.raises(ValueError):
        ops.reference_decode(x, base, crop=win)


# ---- crop_points --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['numpy', 'torch'])
def test_crop_points_follow_a_marked_pixel(kind):
    Hh, Ww, h, w = 9, 12, 5, 6
    win = np.array([(4, 6, 1), (0, 0, 0), (2, 3, 0), (1, 5, 1)], np.int32)
    marks = np.array([[(8, 5), (11, 8)], [(0, 0), (5, 4)], [(3, 2), (8, 6)], [(5, 1), (10, 5)]])   # (x, y), inside
    x = np.zeros((4, Hh, Ww, 1), np.uint8)
    for b in range(4):
        for k, (px, py) in enumerate(marks[b]):
            x[b, py, px, 0] = 100 + k
    cfg = DecodeConfig(channels=(0,), dtype='uint8', layout='nhwc', crop=Crop((h, w)))
    out = ops.reference_decode(torch.from_numpy(x), cfg, crop=win)[..., 0].numpy()
    xy = marks.astype(np.float32) if kind == 'numpy' else torch.from_numpy(marks.astype(np.float32))
    got = ops.crop_points(xy, win if kind == 'numpy' else torch.from_numpy(win), (h, w))
    assert type(got) is type(xy) and got.dtype == xy.dtype and tuple(got.shape) == (4, 2, 2)
    got = np.asarray(got)
    for b in range(4):
        for k in range(2):
            cx, cy = (int(v) for v in got[b, k])
            assert 0 <= cx < w and 0 <= cy < h
            assert out[b, cy, cx] == 100 + k, (b, k)
        assert (out[b] != 0).sum() == 2
    # integer coordinates, a flat [B, 2] list of points, windows as a plain list
    gi = ops.crop_points(marks[:, 0], win.tolist(), (h, w))
    assert np.array_equal(gi, got[:, 0].astype(gi.dtype)) and gi.dtype == marks.dtype
    # and back: mapping is its own inverse up to the origin (mirror twice = identity)
    back = np.asarray(got).copy()
    back[..., 0] = np.where(win[:, 2, None] != 0, w - 1 - back[..., 0], back[..., 0]) + win[:, 1, None]
    back[..., 1] += win[:, 0, None]
    assert np.array_equal(back, marks.astype(np.float32))
    with pytest.raises(ValueError):
        ops.crop_points(marks[:3], win, (h, w))
