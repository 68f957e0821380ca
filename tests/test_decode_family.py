"""The decode kernel family (csrc/gpu/kernels.hip: ``decode``, ``decode_tiles``,
``replay_sample``, ``color4x4``) driven directly at every branch its launchers
dispatch on, each launch held to the addressing oracle of tests/decode_oracle.py
(docs/DECODE_ORACLE.md).

Every launch is described once, as a ``decode_oracle.Launch`` in :func:`cases`.
The unmarked tests check the oracle itself on the CPU: its codec against
``transport.shm``, its dense case against ``ops.reference_decode``, and that every
named mutation of it changes what it expects for every one of those launches.
The ``gpu`` tests run the launches: all decode / tile / replay comparisons are
bit-exact over the WHOLE output buffers, guards included (bf16 / f16 as raw
bits); color4x4 is held to ``reference_color4x4`` at the tolerance
tests/test_gpu_kernels.py uses and, bit for bit, to the dense per-image call.

Deliberately left out:

* the 64-bit branch of ``split_group``: it needs about 2^31 pixel groups;
* ``BT_REPLAY_UNI`` (TBL = 2): read once per process, off by default, measured slower;
* that a host-read RGBA u8 frame with ``W % 4 == 0`` but ``W % 16 != 0`` goes
  scalar: a performance matter, not a correctness one.
"""
import ctypes
import functools
import os
import time

import numpy as np
import pytest
import torch

import decode_oracle as do
from blendtorch import ops
from blendtorch.ops import DecodeConfig
from blendtorch.transport import shm

DTYPES = ('float32', 'bfloat16', 'float16', 'uint8')
LAYOUTS = ('nchw', 'nhwc')


def _vcfg(channels, dtype, layout):
    """Gamma + normalisation (u8: gamma only): a table with 256 distinct rows per channel kind."""
    if dtype == 'uint8':
        return DecodeConfig(channels=channels, gamma=2.2, dtype='uint8', layout=layout)
    return DecodeConfig.densityopt(channels=channels, gamma=2.2, dtype=dtype, layout=layout)


def _img_bytes(H, W, cfg):
    return H * W * cfg.cout * do.ELEM[cfg.dtype]


# ---- the launches -----------------------------------------------------------------------------------------------

CMAPS = {3: [(2, 0), 'rgb', 'bgr'], 4: [(3,), (2, 0), (1, 1, 3), 'rgb', 'bgr', 'rgba']}


def _matrix(dtype, layout):
    """decode's dispatch matrix: B = 3, H = 5, W in {16, 48, 12}, Cin in {3, 4}, every channel map.
    Which of them go vector depends on dtype (W % PPT) and on H*W*Cin % 16 (5x12x3 never does)."""
    out = []
    for W in (16, 48, 12):
        for Cin in (3, 4):
            for i, ch in enumerate(CMAPS[Cin]):
                cfg = _vcfg(ch, dtype, layout)
                bufs, dst = do.dense_dst(3, _img_bytes(5, W, cfg))
                fl = [dict(flip_bits=0b010), dict(flip=[1, 0, 1]), dict(flip_bits=0b100, flip=[0, 1, 0])][i % 3]
                out.append(do.Launch('decode', cfg, do.frames(3, 5, W, Cin, seed=10 * W + Cin + i), [0, 1, 2], bufs, dst,
                                     name=f'matrix-{dtype}-{layout}-W{W}-C{Cin}-{ch}', **fl))
    return out


ALIGN_VARIANTS = ('src_base+4', 'dst_base+1elem', 'one_src_misaligned', 'one_dst_misaligned', 'offsets_permuted_promised',
                  'offsets_permuted', 'offsets_odd_stride')


def _alignment(variant):
    """5x16x4 goes vector for every dtype -- unless one pointer is off: the scalar kernel must take it."""
    out = []
    H, W, Cin, fb = 5, 16, 4, 5 * 16 * 4
    for dtype, layout in zip(DTYPES, ('nchw', 'nhwc', 'nchw', 'nhwc')):
        cfg = _vcfg('rgba', dtype, layout)
        ib, es = _img_bytes(H, W, cfg), do.ELEM[dtype]
        kw = dict(flip_bits=0b101)
        store, src = do.frames(4, H, W, Cin, seed=77), [0, 1, 2]
        bufs, dst = do.dense_dst(3, ib)
        if variant == 'src_base+4':
            kw.update(src_pos=[4 + n * fb for n in range(4)])
        elif variant == 'dst_base+1elem':
            bufs, dst = do.dense_dst(3, ib, shift=es)
        elif variant == 'one_src_misaligned':
            kw.update(src_mode='srcs', src_pos=[n * (fb + 64) + (4 if n == 1 else 0) for n in range(4)])
        elif variant == 'one_dst_misaligned':
            bufs, dst = do.scattered_dst([(0, 0), (0, 1), (0, 2)], ib, shift=[0, es, 0])
            kw.update(dst_mode='dsts')
        elif variant == 'offsets_permuted_promised':
            src = [2, 0, 3]
            kw.update(src_mode='offsets_aligned')
        elif variant == 'offsets_permuted':
            src = [2, 0, 3]
            kw.update(src_mode='offsets')
        elif variant == 'offsets_odd_stride':
            src = [3, 1, 0]
            kw.update(src_mode='offsets', src_pos=[n * (fb + 4) for n in range(4)])
        else:
            raise ValueError(variant)
        out.append(do.Launch('decode', cfg, store, src, bufs, dst, name=f'align-{variant}-{dtype}', **kw))
    return out


STRIDE_FORMS = (('float32', 'nchw', 'rgb'), ('bfloat16', 'nhwc', 'rgba'), ('uint8', 'nchw', 'rgba'))


def _grid_stride():
    """One or two blocks over hundreds of pixel groups: the grid-stride loop, and with unroll = 2 a pass whose
    second group is past the end (B = 3 of 16x64 f32: 768 groups = one full pass of 2 x 256 and one half pass)."""
    out = []
    for dtype, layout, ch in STRIDE_FORMS:
        cfg = _vcfg(ch, dtype, layout)
        for B, grid, unroll in ((3, 1, 1), (3, 1, 2), (5, 2, 2)):
            bufs, dst = do.dense_dst(B, _img_bytes(16, 64, cfg))
            out.append(do.Launch('decode', cfg, do.frames(B, 16, 64, 4, seed=5 + B), list(range(B)), bufs, dst,
                                 flip_bits=0b10, max_grid=grid, unroll=unroll,
                                 name=f'stride-{dtype}-B{B}-grid{grid}-u{unroll}'))
    return out


POINTER_FORMS = (('float32', 'nchw', 4, 'rgb'), ('bfloat16', 'nhwc', 3, 'bgr'), ('uint8', 'nhwc', 4, 'rgba'),
                 ('float16', 'nchw', 4, (3, 0)))


def _pointers():
    """srcs[] in permuted order out of a larger store, dsts[] over two batch tensors in non-monotonic order,
    and the OR of flip_bits with flip[] and with flip_all."""
    out = []
    H, W = 6, 32
    for dtype, layout, Cin, ch in POINTER_FORMS:
        cfg = _vcfg(ch, dtype, layout)
        store = do.frames(8, H, W, Cin, seed=31 + Cin)
        fb = H * W * Cin
        bufs, dst = do.scattered_dst([(1, 1), (0, 2), (1, 0), (0, 0), (0, 1)], _img_bytes(H, W, cfg), nbufs=2)
        for tag, fl in (('bits_or_array', dict(flip_bits=0b10110, flip=[1, 1, 0, 0, 0])),
                        ('bits_or_all', dict(flip_bits=0b10110, flip_all=True))):
            out.append(do.Launch('decode', cfg, store, [6, 2, 7, 0, 3], bufs, dst, src_mode='srcs', dst_mode='dsts',
                                 src_pos=[n * (fb + 256) for n in range(8)], name=f'pointers-{dtype}-{tag}', **fl))
    return out


def _host():
    """Sources in host-mapped memory; RGBA -> RGBA u8 NHWC at W = 16 takes the 4-pixel host-read shape."""
    out = []
    for dtype, layout, ch in (('uint8', 'nhwc', 'rgba'), ('float32', 'nchw', 'rgb')):
        cfg = DecodeConfig.raw(channels=ch) if dtype == 'uint8' else _vcfg(ch, dtype, layout)
        bufs, dst = do.dense_dst(3, _img_bytes(5, 16, cfg))
        out.append(do.Launch('decode', cfg, do.frames(4, 5, 16, 4, seed=90), [3, 0, 2], bufs, dst, src_mode='host',
                             flip_bits=0b011, name=f'host-{dtype}'))
    return out


def _mixed(dtype, layout):
    """The loader's mixed-layout split: one output batch of 5, images 1 and 4 arrive as packed RGB (Cin = 3, the
    head of an rgb_a slot), the others as RGBA; one launch per kind with compacted srcs / dsts / flip_bits."""
    H, W = 6, 32
    cfg = _vcfg('rgb', dtype, layout)
    ib = _img_bytes(H, W, cfg)
    bufs, dst = do.scattered_dst([(0, k) for k in range(5)], ib)
    flip = [1, 1, 0, 0, 1]
    rgba = do.frames(5, H, W, 4, seed=55)
    out = []
    for Cin, members in ((4, [0, 2, 3]), (3, [1, 4])):
        bits = sum(1 << n for n, k in enumerate(members) if flip[k])
        out.append(do.Launch('decode', cfg, np.ascontiguousarray(rgba[..., :Cin]), members, bufs, [dst[k] for k in members],
                             src_mode='srcs', dst_mode='dsts', flip_bits=bits,
                             src_pos=[n * (H * W * Cin + 256) for n in range(5)], name=f'mixed-{dtype}-C{Cin}'))
    return out


TILE_COUNTS = ((0, 1, 6, 2), (3, 0, 0, 6))
TILE_CMAPS = {(3, 1): (1,), (3, 3): 'bgr', (3, 4): (2, 0, 1, 0), (4, 1): (1,), (4, 3): 'bgr', (4, 4): 'rgba'}


def _tiles(dtype, layout):
    """decode_tiles at 32x48 (2 x 3 tiles): B = 4 with empty images at the head, in the middle and never at
    the tail; Cin 3 / 4, Cout 1 / 3 / 4; shuffled positions, flip_bits or flip_all, one block, per-image dsts."""
    out = []
    H, W, nt = 32, 48, 6
    for Cin in (3, 4):
        for cout in (1, 3, 4):
            for ci, counts in enumerate(TILE_COUNTS):
                cfg = _vcfg(TILE_CMAPS[(Cin, cout)], dtype, layout)
                ib = _img_bytes(H, W, cfg)
                rng = np.random.default_rng(100 * Cin + 10 * cout + ci)
                keys = do.frames(4, H, W, Cin, seed=200 + Cin + cout, ramp=False)
                shown = keys.copy()
                enc = []
                for b, n in enumerate(counts):
                    pos = sorted(rng.permutation(nt)[:n].tolist())
                    if ci == 0:                                   # shuffled, distinct
                        pos = rng.permutation(pos).tolist() if n != 2 else [4, 1]
                    new = do.ramp_frame(H, W, Cin, k=b) if n == nt else \
                        rng.integers(0, 256, size=(H, W, Cin), dtype=np.uint8)
                    for p in pos:
                        ty, tx = divmod(p, W // 16)
                        sl = (slice(ty * 16, ty * 16 + 16), slice(tx * 16, tx * 16 + 16))
                        shown[b][sl] = new[sl]
                    enc.append(do.encode_tiles(shown[b], pos))
                if cout == 3:
                    bufs, dst = do.scattered_dst([(0, 2), (1, 0), (0, 0), (1, 1)], ib, nbufs=2)
                    mode = 'dsts'
                else:
                    bufs, dst = do.dense_dst(4, ib)
                    mode = 'dense'
                fl = dict(flip_bits=0b0110) if ci == 0 else dict(flip_all=True)
                out.append(do.Launch('tiles', cfg, shown, [0, 1, 2, 3], bufs, dst, enc=enc, keys=list(keys),
                                     fills=[do.sentinel_fill(ib, b, seed=Cin + cout) for b in range(4)],
                                     dst_mode=mode, max_grid=1 if cout == 1 else 0,
                                     name=f'tiles-{dtype}-{layout}-C{Cin}-o{cout}-{"".join(map(str, counts))}', **fl))
    return out


REPLAY_SHAPES = ((48, 64, 3), (16, 64, 4))
REPLAY_GIVEN = [8, 0, 3, 3, 5, 1]
REPLAY_SEED, REPLAY_CTR = 1234, 77


def _replay(dtype, shape):
    """A 9-frame store sampled by ONE block: past its first group every lane takes its frame from sh.idx.
    Drawn indices (Philox) and given ones; flip_all on the given ones of the 16x64x4 store."""
    H, W, Cin = shape
    layout = 'nchw' if (DTYPES.index(dtype) + Cin) % 2 else 'nhwc'
    cfg = _vcfg('rgb' if Cin == 3 else 'rgba', dtype, layout)
    store = do.frames(9, H, W, Cin, seed=3 * Cin)
    bufs, dst = do.dense_dst(6, _img_bytes(H, W, cfg))
    drawn = ops.philox_indices(REPLAY_SEED, REPLAY_CTR, 6, 9).tolist()
    return [do.Launch('replay', cfg, store, drawn, bufs, dst, max_grid=1, name=f'replay-{dtype}-{H}x{W}x{Cin}-drawn'),
            do.Launch('replay', cfg, store, REPLAY_GIVEN, bufs, dst, max_grid=1, flip_all=Cin == 4,
                      name=f'replay-{dtype}-{H}x{W}x{Cin}-given')]


def _replay_wide():
    """B = 300 > one block of lanes: the fill of sh.idx runs its b += 256 step."""
    out = []
    for dtype, layout in (('float32', 'nchw'), ('uint8', 'nhwc')):
        cfg = _vcfg('rgba', dtype, layout)
        store = do.frames(9, 2, 16, 4, seed=41)
        bufs, dst = do.dense_dst(300, _img_bytes(2, 16, cfg))
        drawn = ops.philox_indices(REPLAY_SEED, REPLAY_CTR, 300, 9).tolist()
        for grid in (0, 1):
            out.append(do.Launch('replay', cfg, store, drawn, bufs, dst, max_grid=grid,
                                 name=f'replay-wide-{dtype}-grid{grid}'))
    return out


COLOR_SHAPES = ((4, 64), (8, 96))


def _color(shape):
    """color4x4 through srcs[] / dsts[] / flip_bits / mat_pos[] (kColorPos): 4x64 is one wave segment per image."""
    H, W = shape
    rng = np.random.default_rng(H)
    bufs, dst = do.scattered_dst([(1, 0), (0, 1), (0, 2), (1, 1), (0, 0)], H * W * 4 * 4, nbufs=2)
    return [do.Launch('color', None, do.frames(7, H, W, 4, seed=H + W), [5, 1, 6, 0, 2], bufs, dst,
                      flip_bits=0b01101, mats=rng.uniform(-1, 1, size=(3, 4, 4)).astype(np.float32),
                      biases=rng.normal(size=(3, 4)).astype(np.float32), mat_pos=[2, 0, 1, 1, 2], gamma=2.2,
                      src_mode='srcs', dst_mode='dsts', src_pos=[n * (H * W * 4 + 256) for n in range(7)],
                      name=f'color-{H}x{W}')]


@functools.lru_cache(maxsize=None)
def cases():
    """Every launch the GPU tests run, by group."""
    g = {}
    for dtype in DTYPES:
        for layout in LAYOUTS:
            g[('matrix', dtype, layout)] = _matrix(dtype, layout)
            g[('tiles', dtype, layout)] = _tiles(dtype, layout)
            g[('mixed', dtype, layout)] = _mixed(dtype, layout)
        for shape in REPLAY_SHAPES:
            g[('replay', dtype, shape)] = _replay(dtype, shape)
    for v in ALIGN_VARIANTS:
        g[('align', v)] = _alignment(v)
    g[('stride',)] = _grid_stride()
    g[('pointers',)] = _pointers()
    g[('host',)] = _host()
    g[('replay_wide',)] = _replay_wide()
    for shape in COLOR_SHAPES:
        g[('color', shape)] = _color(shape)
    return g


def _teeth_kind(l):
    return 'replay_flipped' if l.kind == 'replay' and l.flip_all else l.kind


# ---- the oracle, on the CPU -------------------------------------------------------------------------------------

def test_encoder_matches_shm_ring_and_expansion():
    """The oracle's codec was written from the comment of csrc/codec/tiledelta.h; the Python producer
    (ShmRing.put_tile16) and consumer (shm._expand_tiled) were not consulted -- they must agree byte for byte."""
    H, W = 32, 48
    for C in (3, 4):
        rng = np.random.default_rng(C)
        key = rng.integers(0, 256, size=(H, W, C), dtype=np.uint8)
        frame = key.copy()
        frame[3, 40] ^= 1                  # tile (0, 2): one byte differs
        frame[16:32, 0:16] = rng.integers(0, 256, size=(16, 16, C), dtype=np.uint8)      # tile (1, 0)
        frame[31, 31, C - 1] ^= 0x80       # tile (1, 1): its last byte
        enc = do.encode_tile16(frame, key)
        assert do.changed_tiles(frame, key) == [2, 3, 4]
        assert do.payload_offset(H, W) == shm.tile16_payload_offset(H, W) == 256
        assert do.payload_offset(480, 640) == shm.tile16_payload_offset(480, 640)
        stamp = f'blendtorch-{os.getpid()}-oracle-{C}-{time.monotonic_ns()}'
        kring = shm.ShmRing(stamp + '-key', 1, key.nbytes)
        ring = shm.ShmRing(stamp, 2, shm.tile16_max_bytes(H, W, C))
        try:
            kring.put(key)
            slot, off, h, w, c, gen, n = ring.put_tile16(frame, key)
            assert (h, w, c, n) == (H, W, C, 3)
            assert bytes(ring.seg.mm[off:off + len(enc)]) == enc.tobytes()
            got = shm._expand_tiled(ring.seg, off, h, w, c, ('tile16', kring.name, 1)).reshape(H, W, C)
            assert np.array_equal(do.expand_tile16(enc, key), got)
            assert np.array_equal(got, frame)
        finally:
            ring.close()
            kring.close()
        # positions in any order show the same frame
        assert np.array_equal(do.expand_tile16(do.encode_tiles(frame, [4, 2, 3]), key), frame)
        with pytest.raises(ValueError):
            do.encode_tiles(frame, [1, 1])
        with pytest.raises(ValueError):
            do.encode_tiles(frame, [6])


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('layout', LAYOUTS)
def test_dense_oracle_is_reference_decode(dtype, layout):
    """No pointers, one dense output: the oracle is ``reference_decode(..., flip=)`` between two guards."""
    cfg = _vcfg('rgb', dtype, layout)
    x = do.frames(4, 6, 32, 4, seed=1)
    for fl in (dict(flip=[1, 0, 0, 1]), dict(flip_bits=0b1001), dict(flip_bits=0b1000, flip=[1, 0, 0, 0])):
        bufs, dst = do.dense_dst(4, _img_bytes(6, 32, cfg))
        got = do.expected(do.Launch('decode', cfg, x, [0, 1, 2, 3], bufs, dst, **fl))[0]
        ref = ops.reference_decode(torch.from_numpy(x), cfg, flip=[1, 0, 0, 1]).contiguous()
        body = ref.view(torch.uint8).numpy().reshape(-1)
        assert np.array_equal(got[do.GUARD:-do.GUARD], body)
        assert (got[:do.GUARD] == do.SENTINEL).all() and (got[-do.GUARD:] == do.SENTINEL).all()
    assert do.flips(do.Launch('decode', cfg, x, [0, 1, 2, 3], bufs, dst, flip_all=True)) == [True] * 4


def test_ramp_holds_every_value():
    for C in (3, 4):
        f = do.ramp_frame(16, 64, C)
        for c in range(C):
            assert len(np.unique(f[..., c])) == 256
        assert len(np.unique(do.frames(3, 16, 64, C, seed=9)[0].reshape(-1, C), axis=0)) >= 256


@pytest.mark.parametrize('group', sorted(cases(), key=str), ids=lambda g: '-'.join(map(str, g)))
def test_oracle_has_teeth(group):
    """Every named mutation of the oracle must change what it expects, for every launch the GPU tests run:
    else a kernel with that slip would pass them.  (A mutation a kind cannot suffer -- do.APPLIES -- must say so.)"""
    for l in cases()[group]:
        base = do.expected(l)
        assert any((b != do.SENTINEL).any() for b in base), l.name
        for m in do.MUTATIONS:
            if m not in do.APPLIES[_teeth_kind(l)]:
                if m in ('ignore_one_flip', 'flip_about_H'):
                    with pytest.raises(do.Inapplicable):
                        do.expected(l, mutate=m)
                continue
            mut = do.expected(l, mutate=m)
            assert any(not np.array_equal(a, b) for a, b in zip(base, mut)), (l.name, m)


def test_bindings_reject_lists_beyond_kmaxsrcs():
    """The pointer lists are copied into kMaxSrcs-sized kernel arguments: a longer list is an error of the
    binding itself, raised before any HIP call (so this runs without a GPU)."""
    ext = ops.hip_ext()
    long, ok = [256] * 65, [256] * 64
    dec = (0, 0, 0, 0, 0, 64, 5, 16, 4, 3, [0, 1, 2], 0, 0, 0, 0)
    for kw in (dict(srcs=long), dict(dsts=long), dict(srcs=ok, flip_bits=[0] * 5)):
        with pytest.raises(ValueError):
            ext.decode(*dec, **kw)
    col = (0, 0, 0, 0, 0, 0, 4, 4, 64, 4, 0, 0)
    for kw in (dict(srcs=long), dict(dsts=long), dict(mat_mode=1, Ms=256, mat_pos=[0, 1, 2]),
               dict(mat_mode=1, Ms=256, mat_pos=[0, 1, 2, 256]), dict(mat_pos=[0, 0, 0, 0])):
        with pytest.raises(ValueError):
            ext.color4x4(*col, **kw)
    til = dict(srcs=ok, fills=ok, tile_start=[0] * 65, dst=0, lut=0, flip=0, B=64, H=32, W=48, Cin=4, Cout=3,
               cmap=[0, 1, 2], flip_all=0, out_dtype=0, layout=0, stream=0)
    for kw in (dict(srcs=long), dict(fills=long), dict(tile_start=[0] * 66), dict(dsts=long), dict(H=0)):
        with pytest.raises(ValueError):
            ext.decode_tiles(**{**til, **kw})


# ---- the kernels ------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    ops.hip_ext()  # must load: no silent fallback
    return torch.device('cuda', 0)


class _Sources:
    """The store's frames at their byte positions in one source buffer the test owns (device or host-mapped)."""

    def __init__(self, dev, l, host=False):
        H, W, C = l.shape
        fb = H * W * C
        self.pos = list(l.src_pos) if l.src_pos is not None else [n * fb for n in range(len(l.store))]
        flat = np.zeros(max(self.pos) + fb + 64, np.uint8)
        for n, p in enumerate(self.pos):
            flat[p:p + fb] = l.store[n].reshape(-1)
        self.host = None
        if host:
            self.host, self.base = ops.hip_ext().host_mapped_alloc(len(flat))
            ctypes.memmove(self.host, flat.ctypes.data, len(flat))
        else:
            self.t = torch.from_numpy(flat).to(dev)
            self.base = self.t.data_ptr()
        assert self.base % 256 == 0

    def close(self):
        if self.host is not None:
            ops.hip_ext().host_mapped_free(self.host)
            self.host = None


def _outputs(dev, l):
    outs = [torch.full((n,), do.SENTINEL, dtype=torch.uint8, device=dev) for n in l.bufs]
    assert all(o.data_ptr() % 256 == 0 for o in outs)
    return outs


def _dst_args(l, outs):
    """``(dst, dsts)`` of the launch: one dense base, or one pointer per image."""
    if l.dst_mode == 'dense':
        k0, off0 = l.dst[0]
        assert all(tuple(d) == (k0, off0 + b * l.img_bytes) for b, d in enumerate(l.dst))
        return outs[k0].data_ptr() + off0, []
    return 0, [outs[k].data_ptr() + off for k, off in l.dst]


def _flip_args(dev, l):
    ft = torch.tensor(list(l.flip), dtype=torch.uint8, device=dev) if l.flip is not None else None
    return ft, (ft.data_ptr() if ft is not None else 0), ([l.flip_bits] if l.flip_bits else [])


def _check(l, outs, exp=None):
    exp = do.expected(l) if exp is None else exp
    for k, (o, e) in enumerate(zip(outs, exp)):
        got = o.cpu().numpy()
        if not np.array_equal(got, e):
            bad = np.flatnonzero(got != e)
            inside = [(kk, off) for kk, off, n in do.regions(l) if kk == k and off <= bad[0] < off + n]
            raise AssertionError(f'{l.name}: buffer {k}: {len(bad)} bytes differ, first at {bad[0]} '
                                 f'({"image at " + str(inside[0][1]) if inside else "GUARD / unused slot"}): '
                                 f'got {got[bad[0]]:#x}, expected {e[bad[0]]:#x}')


def run_decode(dev, l, outs=None):
    ext = ops.hip_ext()
    H, W, Cin = l.shape
    src = _Sources(dev, l, host=l.src_mode == 'host')
    try:
        outs = _outputs(dev, l) if outs is None else outs
        dst, dsts = _dst_args(l, outs)
        ft, flip, bits = _flip_args(dev, l)
        base, offs, offs_t, srcs = 0, 0, None, []
        if l.src_mode == 'dense':
            assert list(l.src) == list(range(l.B))
            assert all(src.pos[b] == src.pos[0] + b * H * W * Cin for b in range(l.B))
            base = src.base + src.pos[0]
        elif l.src_mode in ('offsets', 'offsets_aligned'):
            base = src.base
            offs_t = torch.tensor([src.pos[s] for s in l.src], dtype=torch.int64, device=dev)
            offs = offs_t.data_ptr()
            assert l.src_mode == 'offsets' or all(src.pos[s] % 16 == 0 for s in l.src)
        else:
            srcs = [src.base + src.pos[s] for s in l.src]
        lut = ops.device_lut(l.cfg, dev)
        ext.decode(base, offs, dst, lut.data_ptr(), flip, l.B, H, W, Cin, l.cfg.cout, l.cfg.cmap, int(l.flip_all),
                   ops.OUT_DTYPES[l.cfg.dtype], ops.LAYOUTS[l.cfg.layout], ops._stream(dev),
                   l.src_mode == 'offsets_aligned', srcs=srcs, dsts=dsts, flip_bits=bits, max_grid=l.max_grid,
                   unroll=l.unroll)
        torch.cuda.synchronize()
    finally:
        src.close()
    return outs


def _decode_group(dev, group):
    for l in cases()[group]:
        _check(l, run_decode(dev, l))


@pytest.mark.gpu
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_decode_dispatch_matrix(dev, dtype, layout):
    _decode_group(dev, ('matrix', dtype, layout))


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,layout', [('bfloat16', 'nhwc')])
def test_decode_dispatch_matrix_arithmetic_table(dev, monkeypatch, dtype, layout):
    """The same slice with the value table in its arithmetic form (lane-private gamma copies, reciprocal + fma)."""
    monkeypatch.setenv('BLENDTORCH_DECODE_XFORM', '1')
    monkeypatch.setattr(ops, '_lut_cache', {})
    for l in cases()[('matrix', dtype, layout)]:
        assert ops.build_table(l.cfg)[ops.XF_HEADER] == 1.0, l.name
    _decode_group(dev, ('matrix', dtype, layout))


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ALIGN_VARIANTS)
def test_decode_alignment_fallbacks(dev, variant):
    _decode_group(dev, ('align', variant))


@pytest.mark.gpu
def test_decode_grid_stride_and_unroll(dev):
    _decode_group(dev, ('stride',))


@pytest.mark.gpu
def test_decode_per_image_pointers_and_flip_or(dev):
    _decode_group(dev, ('pointers',))


@pytest.mark.gpu
def test_decode_host_mapped_sources(dev):
    _decode_group(dev, ('host',))


@pytest.mark.gpu
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_decode_mixed_layout_split(dev, dtype, layout):
    """Two launches into one batch; the assembled batch is the oracle of both."""
    rgba, rgb = cases()[('mixed', dtype, layout)]
    outs = run_decode(dev, rgb, run_decode(dev, rgba))
    exp = do.expected(rgba)
    for e, e2 in zip(exp, do.expected(rgb)):
        m = e2 != do.SENTINEL
        assert not (m & (e != do.SENTINEL)).any()        # the two launches' images do not overlap
        e[m] = e2[m]
    _check(rgba, outs, exp)
    # every slot of the batch was written by exactly one of the two
    ib = rgba.img_bytes
    assert sorted(off for _, off in list(rgba.dst) + list(rgb.dst)) == [off for _, off in do.scattered_dst(
        [(0, k) for k in range(5)], ib)[1]]


def run_tiles(dev, l, outs=None, **override):
    """decode_tiles of the launch; ``override`` replaces binding arguments (the rejection cases)."""
    ext = ops.hip_ext()
    H, W, Cin = l.shape
    pos, p = [], 0
    for e in l.enc:
        pos.append(p)
        p += -(-len(e) // 256) * 256
    flat = np.zeros(p + 256, np.uint8)
    for q, e in zip(pos, l.enc):
        flat[q:q + len(e)] = e
    enc_t = torch.from_numpy(flat).to(dev)
    fills_t = torch.from_numpy(np.concatenate([np.concatenate([f, np.zeros(256, np.uint8)]) for f in l.fills])).to(dev)
    fstride = l.img_bytes + 256
    assert enc_t.data_ptr() % 256 == 0 and fills_t.data_ptr() % 256 == 0 and fstride % 16 == 0
    counts = [len(do.parse_tiles(e, H, W, Cin)[0]) for e in l.enc]
    outs = _outputs(dev, l) if outs is None else outs
    dst, dsts = _dst_args(l, outs)
    ft, flip, bits = _flip_args(dev, l)
    lut = ops.device_lut(l.cfg, dev)
    kw = dict(srcs=[enc_t.data_ptr() + q for q in pos], fills=[fills_t.data_ptr() + b * fstride for b in range(l.B)],
              tile_start=np.concatenate([[0], np.cumsum(counts)]).astype(int).tolist(), dst=dst, lut=lut.data_ptr(),
              flip=flip, B=l.B, H=H, W=W, Cin=Cin, Cout=l.cfg.cout, cmap=l.cfg.cmap, flip_all=int(l.flip_all),
              out_dtype=ops.OUT_DTYPES[l.cfg.dtype], layout=ops.LAYOUTS[l.cfg.layout], stream=ops._stream(dev),
              dsts=dsts, flip_bits=bits, max_grid=l.max_grid)
    for k, v in override.items():
        kw[k] = v(kw[k]) if callable(v) else v
    try:
        ext.decode_tiles(**kw)
    finally:
        torch.cuda.synchronize()
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_decode_tiles(dev, dtype, layout):
    for l in cases()[('tiles', dtype, layout)]:
        _check(l, run_tiles(dev, l))


TILE_REJECTS = {
    'H=24': dict(H=24),
    'misaligned_fill': dict(fills=lambda f: [f[0], f[1] + 4] + f[2:]),
    'descending_tile_start': dict(tile_start=lambda t: [t[0], t[2], t[1]] + t[3:]),
    'more_tiles_than_frame': dict(tile_start=lambda t: [0, 7, 8, 9, 9]),
    'nsrcs!=B': dict(srcs=lambda s: s[:3]),
}


@pytest.mark.gpu
@pytest.mark.parametrize('what', sorted(TILE_REJECTS))
def test_decode_tiles_rejects_before_launch(dev, what):
    """decode_tiles returns hipErrorInvalidValue for each of these from its argument checks, ahead of the fill
    launch (kernels.hip: the checks precede ``tile_fill_kernel<<<>>>``): it raises and nothing is written."""
    l = [c for c in cases()[('tiles', 'float32', 'nchw')] if c.name.endswith('C4-o3-0162')][0]
    outs = _outputs(dev, l)
    with pytest.raises(RuntimeError, match='decode_tiles'):
        run_tiles(dev, l, outs, **TILE_REJECTS[what])
    for o in outs:
        assert bool((o == do.SENTINEL).all())
    _check(l, run_tiles(dev, l, outs))      # and the same buffers take the well-formed launch


def test_decode_tiles_reject_case_is_real():
    l = [c for c in cases()[('tiles', 'float32', 'nchw')] if c.name.endswith('C4-o3-0162')]
    assert len(l) == 1 and [len(do.parse_tiles(e, 32, 48, 4)[0]) for e in l[0].enc] == [0, 1, 6, 2]


def run_replay(dev, l, given):
    """replay_sample into a guarded buffer, with one metadata column of each width class (12 bytes: 4-byte
    words; 5 bytes: single bytes), each between guards too.  Returns (outs, indices, meta outs, meta stores)."""
    ext = ops.hip_ext()
    H, W, Cin = l.shape
    N = len(l.store)
    store = torch.from_numpy(l.store).to(dev)
    outs = _outputs(dev, l)
    dst, _ = _dst_args(l, outs)
    rng = np.random.default_rng(N + l.B)
    metas = [rng.normal(size=(N, 3)).astype(np.float32), rng.integers(0, 256, size=(N, 5), dtype=np.uint8)]
    msrc = [torch.from_numpy(m).to(dev) for m in metas]
    nbytes = [12, 5]
    mdst = [torch.full((2 * do.GUARD + l.B * nb,), do.SENTINEL, dtype=torch.uint8, device=dev) for nb in nbytes]
    idx_out = torch.full((l.B + 64,), -1, dtype=torch.int64, device=dev)
    idx_in = torch.tensor(list(l.src), dtype=torch.int64, device=dev) if given else None
    lut = ops.device_lut(l.cfg, dev)
    ext.replay_sample(store.data_ptr(), N, dst, lut.data_ptr(), l.B, H, W, Cin, l.cfg.cout, l.cfg.cmap,
                      int(l.flip_all), ops.OUT_DTYPES[l.cfg.dtype], ops.LAYOUTS[l.cfg.layout], REPLAY_SEED, 0,
                      REPLAY_CTR, idx_in.data_ptr() if given else 0, idx_out.data_ptr(),
                      [m.data_ptr() for m in msrc], [m.data_ptr() + do.GUARD for m in mdst], nbytes, ops._stream(dev),
                      ops.table_only(l.cfg, dev), max_grid=l.max_grid)
    torch.cuda.synchronize()
    return outs, idx_out.cpu().numpy(), [m.cpu().numpy() for m in mdst], metas


def _check_replay(dev, l, given):
    outs, idx, mdst, metas = run_replay(dev, l, given)
    want = np.asarray(l.src if given else ops.philox_indices(REPLAY_SEED, REPLAY_CTR, l.B, len(l.store)))
    assert np.array_equal(idx[:l.B], want), l.name
    assert (idx[l.B:] == -1).all(), l.name
    _check(l, outs)          # images: reference_decode(store[idx]) between untouched guards
    for got, m in zip(mdst, metas):
        row = m[want].reshape(l.B, -1).view(np.uint8).reshape(-1)
        assert np.array_equal(got[do.GUARD:-do.GUARD], row), l.name
        assert (got[:do.GUARD] == do.SENTINEL).all() and (got[-do.GUARD:] == do.SENTINEL).all(), l.name


@pytest.mark.gpu
@pytest.mark.parametrize('shape', REPLAY_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('dtype', DTYPES)
def test_replay_sample_one_block(dev, dtype, shape):
    drawn, given = cases()[('replay', dtype, shape)]
    _check_replay(dev, drawn, False)
    _check_replay(dev, given, True)


@pytest.mark.gpu
def test_replay_sample_more_images_than_lanes(dev):
    for l in cases()[('replay_wide',)]:
        _check_replay(dev, l, False)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', COLOR_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_color4x4_per_image_pointers(dev, shape):
    (l,) = cases()[('color', shape)]
    ext = ops.hip_ext()
    H, W, _ = l.shape
    src = _Sources(dev, l)
    outs = _outputs(dev, l)
    _, dsts = _dst_args(l, outs)
    rows = torch.from_numpy(np.concatenate([l.mats.reshape(3, 16), l.biases], axis=1)).contiguous().to(dev)
    lut = ops.device_lut(DecodeConfig(channels='rgba', gamma=l.gamma, color_matrix=np.eye(4)), dev)
    ext.color4x4(0, 0, lut.data_ptr(), 0, 0, 0, l.B, H, W, 4, 0, ops._stream(dev), 1, rows.data_ptr(),
                 srcs=[src.base + src.pos[s] for s in l.src], dsts=dsts, flip_bits=[l.flip_bits],
                 mat_pos=list(l.mat_pos))
    torch.cuda.synchronize()
    exp = do.expected(l)
    # the same images (flipped on the host) through the dense per-image call: the same arithmetic per pixel
    fl = do.flips(l)
    x = np.stack([l.store[s][::-1] if f else l.store[s] for s, f in zip(l.src, fl)])
    dense = ops.color4x4(torch.from_numpy(x.copy()).to(dev), l.mats[list(l.mat_pos)], l.biases[list(l.mat_pos)],
                         gamma=l.gamma).cpu()
    for k, (o, e) in enumerate(zip(outs, exp)):
        got = o.cpu().numpy()
        mask = np.zeros(len(got), bool)
        for b, (kk, off, n) in enumerate(do.regions(l)):
            if kk != k:
                continue
            mask[off:off + n] = True
            g = torch.from_numpy(got[off:off + n].copy()).view(torch.float32).reshape(4, H, W)
            r = torch.from_numpy(e[off:off + n].copy()).view(torch.float32).reshape(4, H, W)
            torch.testing.assert_close(g, r, rtol=1e-5, atol=1e-3, msg=lambda m: f'{l.name} image {b}: {m}')
            assert torch.equal(g.view(torch.int32), dense[b].view(torch.int32)), (l.name, b)
        assert (got[~mask] == do.SENTINEL).all(), l.name
