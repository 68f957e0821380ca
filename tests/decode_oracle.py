"""An addressing oracle of the decode kernel family (``decode``,
``decode_tiles``, ``replay_sample``, ``color4x4``; docs/DECODE_ORACLE.md).

The value of a pixel stays ``ops.reference_decode`` / ``ops.reference_color4x4``
(validated against the numpy formulas elsewhere).  What this file defines is
everything around it, on the CPU and with no code of the kernels' launchers:

* which stored frame image ``b`` of a launch reads (``Launch.src``);
* which rows are read upside down: ``flip_all OR flip[b] OR bit b of flip_bits``;
* where image ``b`` lands: a byte offset in one of several output buffers, every
  other byte of which must keep its sentinel (:data:`SENTINEL`);
* for key-frame delta frames the codec layout, written from the comment of
  ``csrc/codec/tiledelta.h``: ``u32 n | u32 pos[n] | pad to 256 B | n tiles``,
  tile ``pos = ty * (W / 16) + tx``, a tile stored as 16 rows of ``16 * C`` bytes.

:func:`expected` returns the launch's output buffers as bytes, so one
``array_equal`` per buffer checks the images bit for bit AND the guards.
``mutate=`` alters exactly one rule (:data:`MUTATIONS`): the tests use it to prove
that their inputs would expose that slip.
"""
import ctypes
import dataclasses
from typing import Optional, Sequence

import numpy as np
import torch

from blendtorch import ops
from blendtorch.ops import DecodeConfig, reference_color4x4, reference_decode

TILE = 16
SENTINEL = 0xA5            # every output byte before a launch
GUARD = 256                # bytes kept free before, after and between destinations
ELEM = {'float32': 4, 'bfloat16': 2, 'float16': 2, 'uint8': 1}
PPT = {'float32': 4, 'bfloat16': 8, 'float16': 8, 'uint8': 16}   # pixels per lane of the vector kernels

MUTATIONS = ('ignore_one_flip', 'flip_about_H', 'swap_tile_ty_tx', 'rotate_cmap', 'swap_two_dsts',
             'drop_last_group', 'key_for_fill')
# what each kind of launch can suffer: the tile mutations need tiles, and a flip
# mutation needs a flipped image (replay has flip_all only, on one case)
APPLIES = {
    'decode': ('ignore_one_flip', 'flip_about_H', 'rotate_cmap', 'swap_two_dsts', 'drop_last_group'),
    'color': ('ignore_one_flip', 'flip_about_H', 'rotate_cmap', 'swap_two_dsts', 'drop_last_group'),
    'tiles': MUTATIONS,
    'replay': ('rotate_cmap', 'swap_two_dsts', 'drop_last_group'),
    'replay_flipped': ('ignore_one_flip', 'flip_about_H', 'rotate_cmap', 'swap_two_dsts', 'drop_last_group'),
}


class Inapplicable(ValueError):
    """The launch has nothing this mutation could change (no flipped image, one image, ...)."""


@dataclasses.dataclass
class Launch:
    """One kernel launch as the oracle sees it.

    kind      'decode' | 'replay' | 'tiles' | 'color'
    store     u8 [N, H, W, Cin]: the frames the sources point into.  For 'tiles' the
              frame image b shows (its encoded form is ``enc[b]``).
    src       image b reads ``store[src[b]]`` (replay: the drawn / given frame indices)
    bufs      byte size of every output buffer
    dst       image b's first output byte: (buffer, byte offset)
    The rest of the fields say how the GPU test hands the launch to the binding
    (they do not change what is expected), see tests/test_decode_family.py.
    """
    kind: str
    cfg: DecodeConfig
    store: np.ndarray
    src: Sequence[int]
    bufs: Sequence[int]
    dst: Sequence[tuple]
    flip_all: bool = False
    flip: Optional[Sequence[int]] = None
    flip_bits: int = 0
    # tiles: encoded frames, the per-image fills (u8 [out_img_bytes]) and the keys they were encoded against
    enc: Optional[Sequence[np.ndarray]] = None
    fills: Optional[Sequence[np.ndarray]] = None
    keys: Optional[Sequence[np.ndarray]] = None
    # color: matrices [K, 4, 4], biases [K, 4], image b uses mat_pos[b]; gamma
    mats: Optional[np.ndarray] = None
    biases: Optional[np.ndarray] = None
    mat_pos: Optional[Sequence[int]] = None
    gamma: Optional[float] = None
    # how the GPU test launches it
    src_mode: str = 'dense'          # dense | offsets | offsets_aligned | srcs | host
    src_pos: Optional[Sequence[int]] = None   # byte position of every store frame in the source buffer
    dst_mode: str = 'dense'          # dense | dsts
    max_grid: int = 0
    unroll: int = 0
    name: str = ''

    @property
    def B(self):
        return len(self.src)

    @property
    def shape(self):
        return tuple(self.store.shape[1:])

    @property
    def cout(self):
        return 4 if self.kind == 'color' else self.cfg.cout

    @property
    def dtype(self):
        return 'float32' if self.kind == 'color' else self.cfg.dtype

    @property
    def layout(self):
        return 'nchw' if self.kind == 'color' else self.cfg.layout

    @property
    def img_bytes(self):
        H, W, _ = self.shape
        return H * W * self.cout * ELEM[self.dtype]


# ---- inputs -----------------------------------------------------------------------------------------------------

def ramp_frame(H, W, C, k=0):
    """A frame holding every byte value 0..255 in every channel (H * W >= 256):
    pixel i of channel c is ``(i * m_c + 7 c + k) mod 256`` with odd multipliers
    m_c, so no two channels and no two rows agree."""
    if H * W < 256:
        raise ValueError('a ramp needs at least 256 pixels')
    i = np.arange(H * W, dtype=np.int64)
    mult = (1, 3, 5, 7)
    f = np.stack([(i * mult[c] + 7 * c + k) % 256 for c in range(C)], axis=-1).astype(np.uint8)
    return f.reshape(H, W, C)


def frames(N, H, W, C, seed, ramp=True):
    """Seeded random u8 [N, H, W, C]; frame 0 is a ramp when it has room for one,
    else the ramp runs on over the following frames (a 5 x 16 frame has 80
    pixels: the batch then holds as much of the ramp as it has pixels)."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, size=(N, H, W, C), dtype=np.uint8)
    if ramp:
        if H * W >= 256:
            f[0] = ramp_frame(H, W, C, k=seed % 251)
        else:
            flat = f.reshape(-1, C)
            n = min(256, len(flat))
            i = np.arange(n)
            for c in range(C):
                flat[:n, c] = (i * (1, 3, 5, 7)[c] + seed) % 256
    return f


def sentinel_fill(nbytes, b, seed=0):
    """Image b's fill for a tile launch: seeded random BYTES, so it is the decode
    of nothing (for a float dtype most of it is not even a table value), and
    distinct per image."""
    return np.random.default_rng(1000 * seed + 17 * b + 5).integers(0, 256, size=nbytes, dtype=np.uint8)


def dense_dst(B, img_bytes, shift=0):
    """One output buffer: guard, B images back to back from byte ``GUARD + shift``, guard."""
    return [GUARD + shift + B * img_bytes + GUARD], [(0, GUARD + shift + b * img_bytes) for b in range(B)]


def scattered_dst(slots, img_bytes, nbufs=1, shift=None):
    """Per-image destinations: image b goes to slot ``slots[b] = (buffer, slot)``;
    a buffer is guard, slot, guard, slot, ..., guard.  ``shift[b]`` moves image
    b's destination by that many bytes into its trailing guard."""
    per = [1 + max([s for bb, s in slots if bb == k], default=-1) for k in range(nbufs)]
    stride = -(-(img_bytes + GUARD) // GUARD) * GUARD       # slots stay 256-byte aligned
    bufs = [GUARD + n * stride for n in per]
    dst = [(k, GUARD + s * stride + (shift[b] if shift else 0)) for b, (k, s) in enumerate(slots)]
    return bufs, dst


# ---- the codec, from the comment of csrc/codec/tiledelta.h ------------------------------------------------------

def payload_offset(H, W):
    """Count + position list, rounded up to 256 bytes."""
    nt = (H // TILE) * (W // TILE)
    return -(-((nt + 1) * 4) // 256) * 256


def changed_tiles(frame, key):
    """Raster-order indices ``ty * (W / 16) + tx`` of the tiles where frame != key."""
    H, W, _ = frame.shape
    out = []
    for ty in range(H // TILE):
        for tx in range(W // TILE):
            sl = (slice(ty * TILE, (ty + 1) * TILE), slice(tx * TILE, (tx + 1) * TILE))
            if not np.array_equal(frame[sl], key[sl]):
                out.append(ty * (W // TILE) + tx)
    return out


def encode_tiles(frame, positions):
    """The encoded bytes of ``frame`` with the listed tiles in the payload, in
    that order: ``[u32 n | u32 pos[n] | zero pad to 256 B | tile 0 | tile 1 ...]``,
    a tile = 16 rows of 16 * C contiguous bytes."""
    H, W, C = frame.shape
    if H % TILE or W % TILE:
        raise ValueError('tile16 needs H and W multiples of 16')
    ntx, nt = W // TILE, (H // TILE) * (W // TILE)
    if len(positions) > nt or len(set(positions)) != len(positions) or any(not 0 <= p < nt for p in positions):
        raise ValueError('positions must be distinct tiles of the frame')
    off = payload_offset(H, W)
    out = np.zeros(off + len(positions) * TILE * TILE * C, np.uint8)
    out[:4] = np.frombuffer(np.uint32(len(positions)).tobytes(), np.uint8)
    for k, p in enumerate(positions):
        out[4 + 4 * k:8 + 4 * k] = np.frombuffer(np.uint32(p).tobytes(), np.uint8)
        ty, tx = divmod(int(p), ntx)
        tile = frame[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE]          # [16, 16, C]
        out[off + k * TILE * TILE * C:off + (k + 1) * TILE * TILE * C] = tile.reshape(-1)
    return out


def encode_tile16(frame, key):
    """``frame`` as a key-frame delta against ``key``: the changed tiles in raster order."""
    return encode_tiles(frame, changed_tiles(frame, key))


def parse_tiles(enc, H, W, C):
    """``(positions, tiles u8 [n, 16, 16, C])`` of an encoded frame."""
    n = int(np.frombuffer(enc[:4].tobytes(), np.uint32)[0])
    pos = np.frombuffer(enc[4:4 + 4 * n].tobytes(), np.uint32).astype(np.int64)
    off = payload_offset(H, W)
    tiles = enc[off:off + n * TILE * TILE * C].reshape(n, TILE, TILE, C)
    return pos, tiles


def expand_tile16(enc, key):
    """The frame an encoded frame shows: the key, overwritten by the payload tiles."""
    H, W, C = key.shape
    out = key.copy()
    ntx = W // TILE
    pos, tiles = parse_tiles(enc, H, W, C)
    for p, t in zip(pos, tiles):
        ty, tx = divmod(int(p), ntx)
        out[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE] = t
    return out


# ---- what a launch must write -----------------------------------------------------------------------------------

def flips(l: Launch):
    """The OR rule: ``flip_all OR flip[b] OR flip_bits[b]``."""
    return [bool(l.flip_all or (l.flip is not None and l.flip[b]) or (l.flip_bits >> b) & 1) for b in range(l.B)]


def _bytes_of(t):
    """A tensor's elements as u8 [..., element size] (raw bits: bf16 / f16 are never compared as numbers)."""
    t = t.contiguous()
    return t.view(torch.uint8).numpy().reshape(tuple(t.shape) + (t.element_size(),)).copy()


def _src_rows(H, flipped, mutate):
    """Source row read for every output row."""
    y = np.arange(H)
    if not flipped:
        return y
    return (H - y) % H if mutate == 'flip_about_H' else H - 1 - y


def _cfg(l, mutate):
    if mutate != 'rotate_cmap' or l.kind == 'color':
        return l.cfg
    cin = l.shape[2]
    return dataclasses.replace(l.cfg, channels=tuple((c + 1) % cin for c in l.cfg.cmap))


def _decode(l, x, mutate):
    """Values of u8 frames x [n, h, w, Cin] (rows already in output order) as bytes [n, ..., elem]."""
    return _bytes_of(reference_decode(torch.from_numpy(np.ascontiguousarray(x)), _cfg(l, mutate)))


def _last_group(l):
    """Index of the last pixel group of an image, for its [C, H, W] / [H, W, C] byte array."""
    H, W, _ = l.shape
    n = min(PPT[l.dtype] if l.kind != 'color' else 4, W)
    return (slice(None), H - 1, slice(W - n, W)) if l.layout == 'nchw' else (H - 1, slice(W - n, W))


def images(l: Launch, mutate=None):
    """``(bytes, keep)`` per image: u8 [C, H, W, elem] / [H, W, C, elem] and the mask
    of the bytes the launch writes (all of them, short of a mutation)."""
    if mutate is not None and mutate not in MUTATIONS:
        raise ValueError(mutate)
    if l.cfg is not None and l.cfg.flip:
        raise ValueError('give flip_all to the launch, not to the config')
    H, W, Cin = l.shape
    fl = flips(l)
    if mutate in ('ignore_one_flip', 'flip_about_H'):
        cand = [b for b in range(l.B) if fl[b] and (l.kind != 'tiles' or len(parse_tiles(l.enc[b], H, W, Cin)[0]))]
        if not cand:
            raise Inapplicable('no flipped image')
        if mutate == 'ignore_one_flip':
            fl[cand[-1]] = False
    out = []
    if l.kind in ('decode', 'replay'):
        x = np.stack([l.store[l.src[b]][_src_rows(H, fl[b], mutate)] for b in range(l.B)])
        vals = _decode(l, x, mutate)
        out = [(vals[b], np.ones(vals[b].shape, bool)) for b in range(l.B)]
    elif l.kind == 'color':
        x = np.stack([l.store[l.src[b]][_src_rows(H, fl[b], mutate)] for b in range(l.B)])
        if mutate == 'rotate_cmap':
            x = np.roll(x, -1, axis=-1)
        M = np.asarray(l.mats, np.float32)[list(l.mat_pos)]
        bias = np.asarray(l.biases, np.float32)[list(l.mat_pos)]
        vals = _bytes_of(reference_color4x4(torch.from_numpy(np.ascontiguousarray(x)), M, bias, gamma=l.gamma))
        out = [(vals[b], np.ones(vals[b].shape, bool)) for b in range(l.B)]
    elif l.kind == 'tiles':
        ntx, nty = W // TILE, H // TILE
        shape = (l.cout, H, W) if l.layout == 'nchw' else (H, W, l.cout)
        es = ELEM[l.dtype]
        if mutate == 'swap_tile_ty_tx' and not any(
                divmod(int(p), ntx) != (int(p) % nty, int(p) // nty)
                for b in range(l.B) for p in parse_tiles(l.enc[b], H, W, Cin)[0]):
            raise Inapplicable('no tile whose row and column differ')
        if mutate == 'key_for_fill' and all(len(parse_tiles(e, H, W, Cin)[0]) == nty * ntx for e in l.enc):
            raise Inapplicable('no image with a tile outside its payload')
        for b in range(l.B):
            if mutate == 'key_for_fill':
                img = _decode(l, l.keys[b][None][:, _src_rows(H, fl[b], None)], None)[0]
            else:
                img = l.fills[b].reshape(shape + (es,)).copy()
            pos, tiles = parse_tiles(l.enc[b], H, W, Cin)
            if len(pos):
                vals = _decode(l, tiles, mutate)                     # [n, C, 16, 16, es] / [n, 16, 16, C, es]
                for k, p in enumerate(pos):
                    ty, tx = divmod(int(p), ntx)
                    if mutate == 'swap_tile_ty_tx':
                        ty, tx = int(p) % nty, int(p) // nty
                    sy = ty * TILE + np.arange(TILE)                 # stored rows of the tile
                    oy = sy
                    if fl[b]:
                        oy = (H - sy) % H if mutate == 'flip_about_H' else H - 1 - sy
                    xs = slice(tx * TILE, (tx + 1) * TILE)
                    if l.layout == 'nchw':
                        img[:, oy, xs] = vals[k]
                    else:
                        img[oy, xs] = vals[k]
            out.append((img, np.ones(img.shape, bool)))
    else:
        raise ValueError(l.kind)
    if mutate == 'drop_last_group':
        if l.kind == 'tiles':
            # the last lane of the last payload tile writes nothing: that run keeps the fill
            cand = [b for b in range(l.B) if len(parse_tiles(l.enc[b], H, W, Cin)[0])]
            if not cand:
                raise Inapplicable('no payload tile')
            b = cand[-1]
            p = int(parse_tiles(l.enc[b], H, W, Cin)[0][-1])
            ty, tx = divmod(p, W // TILE)
            sy = ty * TILE + TILE - 1
            oy = H - 1 - sy if fl[b] else sy
            n = PPT[l.dtype]
            xs = slice((tx + 1) * TILE - n, (tx + 1) * TILE)
            img = out[b][0]
            fill = l.fills[b].reshape(img.shape)
            if l.layout == 'nchw':
                img[:, oy, xs] = fill[:, oy, xs]
            else:
                img[oy, xs] = fill[oy, xs]
        else:
            out[-1][1][_last_group(l)] = False
    return out


def expected(l: Launch, mutate=None):
    """The launch's output buffers, u8, after it ran on buffers full of SENTINEL."""
    imgs = images(l, mutate)
    dst = list(l.dst)
    if mutate == 'swap_two_dsts':
        if l.B < 2:
            raise Inapplicable('one image')
        dst[0], dst[-1] = dst[-1], dst[0]
    bufs = [np.full(n, SENTINEL, np.uint8) for n in l.bufs]
    for (val, keep), (k, off) in zip(imgs, dst):
        flat, m = val.reshape(-1), keep.reshape(-1)
        if off < GUARD // 2 or off + flat.size > len(bufs[k]) - GUARD // 2:
            raise ValueError('a destination leaves less than half a guard free')
        region = bufs[k][off:off + flat.size]
        region[m] = flat[m]
    return bufs


def regions(l: Launch):
    """``[(buffer, offset, nbytes)]`` of the images, for tests that compare them as numbers."""
    return [(k, off, l.img_bytes) for k, off in l.dst]


class MirrorLaunch:
    """The buffers of one slot-mirror launch (``decode_delta``, ``decode_delta_blocks``) and what it must leave.

    ``inside[b]`` (bool H x W x Cin, b >= 1) says which bytes of image b the kernel has to take from the
    host; image 0 has no mirror and is read whole.  The host frames (pinned, device-mapped) hold the true
    bytes inside and POISON outside, the mirrors the true bytes outside and poison inside; outputs and
    the space around the mirrors are guard-filled.  ``launch(self, **kw)`` hands the buffers to a binding.
    """

    def __init__(self, dev, store, cfg, inside, launch, flip_bits, label=''):
        self.dev, self.store, self.cfg, self.flip_bits, self.label, self._launch = dev, store, cfg, flip_bits, label, launch
        self.B, self.H, self.W, self.Cin = store.shape
        self.fb = self.H * self.W * self.Cin
        self.img_bytes = self.H * self.W * cfg.cout * ELEM[cfg.dtype]
        self.bufs, self.dst = scattered_dst([(b % 2, b // 2) for b in range(self.B)], self.img_bytes, nbufs=2)
        self.ins = [np.ones_like(store[0], bool)] + list(inside)
        host = np.stack([np.where(i, t, t ^ 0xFF).reshape(-1) for i, t in zip(self.ins, store)])
        mir = np.full(GUARD + (self.B - 1) * (self.fb + GUARD), SENTINEL, np.uint8)
        self.mir_off = [None] + [GUARD + (b - 1) * (self.fb + GUARD) for b in range(1, self.B)]
        for b in range(1, self.B):
            mir[self.mir_off[b]:self.mir_off[b] + self.fb] = np.where(self.ins[b], store[b] ^ 0xFF, store[b]).reshape(-1)
        self.host0, self.mir0 = host, mir.copy()
        self.host, self.host_dev = ops.hip_ext().host_mapped_alloc(host.size)
        ctypes.memmove(self.host, host.ctypes.data, host.size)
        self.mir = torch.from_numpy(mir).to(dev)
        self.outs = [torch.full((n,), SENTINEL, dtype=torch.uint8, device=dev) for n in self.bufs]

    def close(self):
        ops.hip_ext().host_mapped_free(self.host)

    def launch(self, **kw):
        self._launch(self, **kw)
        torch.cuda.synchronize()

    def untouched(self):
        """Nothing was launched: outputs and mirrors are what they were."""
        assert all(bool((o == SENTINEL).all()) for o in self.outs)
        assert np.array_equal(self.mir.cpu().numpy(), self.mir0)

    def reference(self):
        """``ops.reference_decode`` of the true frames, as bytes per image."""
        flags = [(self.flip_bits >> b) & 1 for b in range(self.B)]
        ref = reference_decode(torch.from_numpy(self.store), self.cfg, flip=flags)
        return ref.contiguous().view(torch.uint8).reshape(self.B, -1).numpy()

    def check(self, what, ref=None):
        """Every output buffer, guards included, equals the reference; every mirror its true frame."""
        ref = self.reference() if ref is None else ref
        exp = [np.full(n, SENTINEL, np.uint8) for n in self.bufs]
        for b, (k, off) in enumerate(self.dst):
            exp[k][off:off + self.img_bytes] = ref[b]
        for k, (o, e) in enumerate(zip(self.outs, exp)):
            g = o.cpu().numpy()
            if not np.array_equal(g, e):
                bad = np.flatnonzero(g != e)
                where = [b for b, (kk, off) in enumerate(self.dst) if kk == k and off <= bad[0] < off + self.img_bytes]
                raise AssertionError(f'{what}: W {self.W} Cin {self.Cin} {self.cfg.channels} {self.label}: '
                                     f'buffer {k}: {len(bad)} bytes differ, first at {bad[0]} '
                                     f'({"image %d" % where[0] if where else "GUARD"})')
        m = self.mir.cpu().numpy()
        want = np.full(m.size, SENTINEL, np.uint8)
        for b in range(1, self.B):
            want[self.mir_off[b]:self.mir_off[b] + self.fb] = self.store[b].reshape(-1)
        assert np.array_equal(m, want), f'{what}: the mirrors do not equal the true frames (or a guard was written)'
