"""Resized crop, the host side: ``ops.ResizedCrop`` / ``DecodeConfig.resize``
validation, the window draw (pure Python against ``_native.resized_crop_draw``),
``ops.reference_decode(..., window=)`` against the crop reference and against
``F.interpolate``, and ``ops.resized_crop_points``.  No GPU.
"""
import dataclasses
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from blendtorch import _native, ops
from blendtorch.ops import Crop, DecodeConfig, ResizedCrop

M64 = (1 << 64) - 1


# ---- validation -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kw', [
    dict(size=5), dict(size=(4,)), dict(size=(0, 4)), dict(size=(4, 32768)),
    dict(size=(4, 4), scale=(0.0, 1.0)), dict(size=(4, 4), scale=(0.5, 0.4)), dict(size=(4, 4), scale=(0.5, 1.5)),
    dict(size=(4, 4), scale=(0.5,)), dict(size=(4, 4), scale=0.5),
    dict(size=(4, 4), ratio=(1.1, 2.0)), dict(size=(4, 4), ratio=(0.5, 0.9)), dict(size=(4, 4), ratio=(0.0, 1.0)),
    dict(size=(4, 4), ratio=(1.0,)),
    dict(size=(4, 4), mode='fixed'), dict(size=(4, 4), mode='centre'),
    dict(size=(4, 4), window=(0, 0, 4)), dict(size=(4, 4), window=(-1, 0, 4, 4)), dict(size=(4, 4), window=(0, 0, 0, 4)),
    dict(size=(4, 4), window=(0, 0, 4, 0)), dict(size=(4, 4), window=(30000, 0, 4000, 4)), dict(size=(4, 4), window=7),
    dict(size=(4, 4), mirror=-0.1), dict(size=(4, 4), mirror=1.5),
    dict(size=(4, 4), mirror=0.5, mode='center'), dict(size=(4, 4), mirror=0.5, mode='full'),
    dict(size=(4, 4), mirror=0.5, window=(0, 0, 4, 4)),
])
def test_resized_crop_rejects(kw):
    with pytest.raises(ValueError):
        ResizedCrop(**kw)


def test_resized_crop_defaults_and_normalisation():
    rc = ResizedCrop([8, 6])
    assert rc.size == (8, 6) and rc.scale == (0.08, 1.0) and rc.ratio == (3 / 4, 4 / 3)
    assert rc.mode == 'random' and rc.kind == 'random' and rc.window is None and rc.mirror == 0.0 and rc.seed == 0
    assert ResizedCrop((8, 6), window=[1, 2, 3, 4]).kind == 'fixed'
    assert hash(DecodeConfig(resize=rc)) == hash(DecodeConfig(resize=ResizedCrop((8, 6))))
    assert [f.name for f in dataclasses.fields(DecodeConfig)][-1] == 'resize'


def test_decode_config_resize_is_exclusive():
    rc = ResizedCrop((8, 6))
    with pytest.raises(TypeError):
        DecodeConfig(resize=(8, 6))
    with pytest.raises(ValueError, match='crop'):
        DecodeConfig(resize=rc, crop=Crop((4, 4)))
    eye = np.eye(4).tolist()
    with pytest.raises(ValueError, match='color'):
        DecodeConfig(channels='rgba', resize=rc, color_matrix=eye)
    with pytest.raises(ValueError, match='color'):
        DecodeConfig(channels='rgba', resize=rc, color_matrices=[eye])
    with pytest.raises(ValueError, match='color'):
        DecodeConfig(resize=rc, color_jitter=ops.ColorJitter(brightness=0.1))
    with pytest.raises(ValueError):
        DecodeConfig.unit(dtype='uint8', resize=rc)            # uint8 only where it is legal today
    assert DecodeConfig(resize=rc).out_shape(3, 20, 30) == (3, 3, 8, 6)
    assert DecodeConfig(resize=rc, layout='nhwc', channels='rgba').out_shape(3, 20, 30) == (3, 8, 6, 4)
    fixed = DecodeConfig(resize=ResizedCrop((8, 6), window=(0, 0, 21, 30)))
    with pytest.raises(ValueError, match=r'21x30.*20x30'):
        fixed.out_shape(3, 20, 30)
    with pytest.raises(ValueError):
        ops.resized_windows(fixed.resize, 20, 30, 1)


def test_replay_and_gather_reject_a_resize_config():
    from blendtorch.btt.replay import DeviceReplayBuffer
    cfg = DecodeConfig(channels='rgb', resize=ResizedCrop((4, 4)))
    buf = DeviceReplayBuffer(8, device='cpu')
    buf.extend(torch.zeros(2, 6, 8, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match='resize'):
        buf.sample(2, cfg)
    with pytest.raises(ValueError, match='resize'):
        buf.gather(torch.tensor([0, 1]), cfg)


# ---- the draw ---------------------------------------------------------------------------------------------------

SEEDS = (0, 1, 8853, 1 << 63)
FRAMES = ((7, 32), (32, 64), (480, 640), (1, 1))
SPREADS = (((0.08, 1.0), (3 / 4, 4 / 3)), ((1.0, 1.0), (1.0, 1.0)), ((0.3, 0.31), (0.25, 3.0)))


def _native_windows(rc, H, W, n):
    return _native.resized_crop_draw(rc.seed & M64, H, W, rc.size[0], rc.size[1], rc.scale, rc.ratio, rc.mirror,
                                     rc.kind, n, list(rc.window or ()))


def _specs(seed, scale, ratio):
    yield ResizedCrop((16, 24), scale=scale, ratio=ratio, mirror=0.5, seed=seed)
    yield ResizedCrop((224, 224), scale=scale, ratio=ratio, mirror=0.0, seed=seed)
    yield ResizedCrop((16, 24), scale=scale, ratio=ratio, mode='center', seed=seed)
    yield ResizedCrop((3, 100), scale=scale, ratio=ratio, mode='center', seed=seed)
    yield ResizedCrop((100, 3), scale=scale, ratio=ratio, mode='center', seed=seed)
    yield ResizedCrop((16, 24), scale=scale, ratio=ratio, mode='full', seed=seed)


@pytest.mark.parametrize('H,W', FRAMES)
def test_python_draw_equals_the_native_draw(H, W):
    n = 200
    for seed, (scale, ratio) in itertools.product(SEEDS, SPREADS):
        for rc in _specs(seed, scale, ratio):
            py, nat = ops.resized_windows(rc, H, W, n), _native_windows(rc, H, W, n)
            assert py.dtype == np.int32 and py.shape == (n, 5) and nat.shape == (n, 5)
            assert np.array_equal(py, nat), (rc, H, W, np.flatnonzero((py != nat).any(1))[:5])
            y0, x0, h, w, m = py.T.astype(np.int64)
            assert (y0 >= 0).all() and (x0 >= 0).all() and (h >= 1).all() and (w >= 1).all()
            assert (y0 + h <= H).all() and (x0 + w <= W).all() and set(m) <= {0, 1}
            if rc.kind != 'random':
                assert (py == py[0]).all() and py[0, 4] == 0
            if rc.kind == 'full' or (rc.kind == 'random' and scale == (1.0, 1.0) and H == W):
                assert (h == H).all() and (w == W).all()
    fixed = ResizedCrop((5, 5), window=(0, 0, H, W))
    assert np.array_equal(ops.resized_windows(fixed, H, W, 3), _native_windows(fixed, H, W, 3))
    assert ops.resized_windows(fixed, H, W, 3).tolist() == [[0, 0, H, W, 0]] * 3


def test_center_mode_is_the_largest_window_of_the_output_aspect():
    H, W = 480, 640
    assert ops.resized_windows(ResizedCrop((224, 224), mode='center'), H, W, 1).tolist() == [[0, 80, 480, 480, 0]]
    assert ops.resized_windows(ResizedCrop((100, 400), mode='center'), H, W, 1).tolist() == [[160, 0, 160, 640, 0]]
    assert ops.resized_windows(ResizedCrop((3, 4), mode='center'), H, W, 1).tolist() == [[0, 0, 480, 640, 0]]
    assert ops.resized_windows(ResizedCrop((1000, 1), mode='center'), H, W, 1).tolist() == [[0, 319, 480, 1, 0]]


def test_default_stream_statistics():
    H, W, n = 480, 640, 4000
    win = ops.resized_windows(ResizedCrop((224, 224), mirror=0.5, seed=1), H, W, n).astype(np.int64)
    frac = win[:, 2] * win[:, 3] / (H * W)
    assert frac.min() >= 0.08 - 0.01 and frac.max() <= 1.0
    assert abs(win[:, 4].mean() - 0.5) <= 0.05
    assert len({(h, w) for h, w in win[:, 2:4]}) > 1000


def test_seeds_one_apart_are_streams_one_image_apart():
    for s in (0, 8853, (1 << 63) - 1):
        a = ops.resized_windows(ResizedCrop((8, 8), mirror=0.5, seed=s), 32, 64, 50)
        b = ops.resized_windows(ResizedCrop((8, 8), mirror=0.5, seed=s + 1), 32, 64, 50)
        # the state advances by the seed multiplier per word: seed + 1 starts one WORD later, so five
        # seeds on is one image (five words) on
        c = ops.resized_windows(ResizedCrop((8, 8), mirror=0.5, seed=s + 5), 32, 64, 50)
        assert np.array_equal(a[1:], c[:-1])
        assert not np.array_equal(a, b)


def test_crop_and_resize_streams_differ():
    for s in SEEDS:
        crop = ops.crop_windows(Crop((16, 32), mirror=0.5, seed=s), 32, 64, 50)
        rc = ops.resized_windows(ResizedCrop((16, 32), scale=(0.25, 0.25), ratio=(1.0, 1.0), mirror=0.5, seed=s), 32, 64, 50)
        # the resize draws y0, x0, m as its 3rd..5th words with the crop's formulas: sharing a state would
        # show as the crop's stream two words on
        assert not np.array_equal(crop[1:, 0], rc[:-1, 0]) and not np.array_equal(crop[:, 0], rc[:, 0])
        assert not np.array_equal(crop[:, 2], rc[:, 4])


# ---- the reference ----------------------------------------------------------------------------------------------

def _frames(B, H, W, C, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (B, H, W, C), dtype=np.uint8))


@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('dtype', ['float32', 'bfloat16', 'float16', 'uint8'])
def test_identity_resize_is_the_crop_reference(dtype, layout):
    x = _frames(3, 20, 36, 4, 5)
    win = [(3, 5, 9, 16, 0), (0, 0, 9, 16, 1), (11, 20, 9, 16, 1)]
    mk = [DecodeConfig.unit, DecodeConfig.densityopt] if dtype != 'uint8' else [DecodeConfig]
    for make in mk:
        for ch in ('rgb', 'bgr', 'rgba'):
            rcfg = make(channels=ch, dtype=dtype, layout=layout, resize=ResizedCrop((9, 16)))
            ccfg = make(channels=ch, dtype=dtype, layout=layout, crop=Crop((9, 16)))
            got = ops.reference_decode(x, rcfg, flip=[0, 1, 0], window=win)
            want = ops.reference_decode(x, ccfg, flip=[0, 1, 0], crop=[(y, xx, m) for y, xx, _, _, m in win])
            assert got.dtype == want.dtype and got.shape == want.shape
            assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))


def _ulp32(x):
    return float(np.spacing(np.float32(x)))


@pytest.mark.parametrize('H,W,win,size', [
    (32, 64, (4, 9, 17, 23, 0), (16, 16)),          # down, odd extents
    (32, 64, (13, 30, 5, 7, 0), (16, 16)),          # up
    (32, 64, (0, 0, 32, 64, 1), (16, 16)),          # down by 2 and 4, mirrored
    (20, 96, (7, 50, 1, 1, 0), (8, 8)),             # a 1 x 1 window
    (20, 96, (3, 0, 13, 96, 1), (8, 32)),           # down, mirrored
    (7, 32, (0, 0, 7, 32, 0), (9, 40)),             # up, non-integer
    (480, 640, (0, 0, 480, 640, 0), (224, 224)),    # the benchmark's Resize
    (480, 640, (100, 200, 137, 301, 1), (224, 224)),
    (480, 640, (70, 300, 331, 97, 0), (84, 84)),
])
def test_reference_against_interpolate(H, W, win, size):
    x = _frames(2, H, W, 4, 11)
    cfg = DecodeConfig.densityopt(channels='rgb', resize=ResizedCrop(size))
    full = ops.reference_decode(x, dataclasses.replace(cfg, resize=None))
    y0, x0, h, w, m = win
    want = F.interpolate(full[:, :, y0:y0 + h, x0:x0 + w].contiguous(), size=size, mode='bilinear', align_corners=False)
    if m:
        want = torch.flip(want, dims=[3])
    got = ops.reference_decode(x, cfg, window=[win, win])
    assert got.shape == want.shape == (2, 3) + tuple(size)
    vmax = float(full.abs().max())
    # one ulp of source coordinate per axis in each implementation, plus at most 16 roundings of
    # magnitude <= max|full| in each
    atol = (4 * _ulp32(max(h, w)) + 32 * 2.0 ** -24) * vmax
    err = float((got - want).abs().max())
    print(f'{H}x{W} {win} -> {size}: max |diff| = {err / (vmax * 2.0 ** -24):.1f} x 2^-24 max|v|, '
          f'atol {atol / (vmax * 2.0 ** -24):.1f}')
    assert err <= atol
    # nhwc is the same values permuted; a single window serves every image
    nhwc = ops.reference_decode(x, dataclasses.replace(cfg, layout='nhwc'), window=win)
    assert torch.equal(nhwc.permute(0, 3, 1, 2), got)


def test_reference_uint8_rounds_half_to_even_and_other_errors():
    # a 1 x 2 window of values (0, 1), (2, 3), ... resized to 1 x 4: taps at 0.25 / 0.75 and, at the ends, the pixels
    x = torch.zeros(1, 1, 2, 4, dtype=torch.uint8)
    x[0, 0, :, 0] = torch.tensor([2, 3])
    cfg = DecodeConfig(channels=(0,), dtype='uint8', resize=ResizedCrop((1, 1)))
    assert ops.reference_decode(x, cfg, window=[(0, 0, 1, 2, 0)]).reshape(-1).tolist() == [2]     # 2.5 -> 2
    x[0, 0, :, 0] = torch.tensor([3, 4])
    assert ops.reference_decode(x, cfg, window=[(0, 0, 1, 2, 0)]).reshape(-1).tolist() == [4]     # 3.5 -> 4
    with pytest.raises(ValueError):
        ops.reference_decode(x, cfg)                                      # a resize config needs its windows
    with pytest.raises(ValueError):
        ops.reference_decode(x, cfg, window=[(0, 0, 2, 2, 0)])            # leaves the frame
    with pytest.raises(ValueError):
        ops.reference_decode(x, cfg, window=[(0, 0, 1, 2, 0)] * 2)        # one window per image
    with pytest.raises(ValueError):
        ops.reference_decode(x, DecodeConfig(channels=(0,)), window=[(0, 0, 1, 2, 0)])


# ---- points -----------------------------------------------------------------------------------------------------

def test_resized_crop_points():
    size = (16, 24)
    win = np.array([[3, 5, 9, 13, 0], [0, 0, 32, 64, 1], [10, 20, 1, 1, 0]], np.int32)
    oh, ow = size
    for be in ('numpy', 'torch'):
        pts = []
        for y0, x0, h, w, m in win:
            # the window's corner pixels' outer corners: (x0 - 0.5, y0 - 0.5) .. (x0 + w - 0.5, y0 + h - 0.5)
            pts.append([[x0 - 0.5, y0 - 0.5], [x0 + w - 0.5, y0 - 0.5], [x0 - 0.5, y0 + h - 0.5],
                        [x0 + w - 0.5, y0 + h - 0.5], [x0 + (w - 1) / 2, y0 + (h - 1) / 2]])
        pts = np.array(pts, np.float64)
        got = ops.resized_crop_points(pts if be == 'numpy' else torch.from_numpy(pts),
                                      win if be == 'numpy' else torch.from_numpy(win), size)
        assert isinstance(got, np.ndarray if be == 'numpy' else torch.Tensor)
        got = np.asarray(got)
        # the output's outer corners and its centre; mirrored: x reflected
        want = np.array([[-0.5, -0.5], [ow - 0.5, -0.5], [-0.5, oh - 0.5], [ow - 0.5, oh - 0.5],
                         [(ow - 1) / 2, (oh - 1) / 2]])
        for b in range(3):
            e = want.copy()
            if win[b, 4]:
                e[:, 0] = ow - 1 - e[:, 0]
            assert np.allclose(got[b], e, atol=1e-9), (be, b, got[b], e)
    # the four corner pixels' centres under the half-pixel formula, and an identity window is a translation
    y0, x0, h, w = 3, 5, 9, 13
    cen = np.array([[[x0, y0], [x0 + w - 1, y0], [x0, y0 + h - 1], [x0 + w - 1, y0 + h - 1]]], np.float64)
    got = ops.resized_crop_points(cen, [[y0, x0, h, w, 0]], size)[0]
    sx, sy = ow / w, oh / h
    assert np.allclose(got, [[0.5 * sx - 0.5, 0.5 * sy - 0.5], [ow - 0.5 * sx - 0.5, 0.5 * sy - 0.5],
                             [0.5 * sx - 0.5, oh - 0.5 * sy - 0.5], [ow - 0.5 * sx - 0.5, oh - 0.5 * sy - 0.5]])
    ident = ops.resized_crop_points(cen, [[y0, x0, h, w, 0]], (h, w))[0]
    assert np.allclose(ident, [[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]])
    mirrored = ops.resized_crop_points(cen, [[y0, x0, h, w, 1]], (h, w))[0]
    assert np.allclose(mirrored, [[w - 1, 0], [0, 0], [w - 1, h - 1], [0, h - 1]])
    t = ops.resized_crop_points(torch.from_numpy(cen), torch.tensor([[y0, x0, h, w, 1]]), (h, w))
    assert np.allclose(t.numpy()[0], mirrored)
    with pytest.raises(ValueError):
        ops.resized_crop_points(cen, win, size)
