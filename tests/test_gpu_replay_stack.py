"""Frame-stacked transitions in one fused launch (csrc/gpu/kernels.hip
``replay_sample_stack``) and through ``DeviceReplayBuffer``.

Kernel launches go through the binding into SENTINEL-filled buffers
(tests/decode_oracle.py); the WHOLE image buffer -- 256-byte guards included -- is
compared bit for bit with the CPU buffer's batch (``ops.philox_transitions`` +
``ops.reference_decode``) at the same seed and counter, and the index, validity,
window and metadata outputs sit between guards too.  k = 3, S = 2 throughout
unless a test says otherwise."""
import dataclasses
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from decode_oracle import ELEM, GUARD, SENTINEL, frames
from blendtorch import ops
from blendtorch.btt.replay import DeviceReplayBuffer
from blendtorch.ops import Crop, DecodeConfig

pytestmark = pytest.mark.gpu

DTYPES = ('float32', 'bfloat16', 'float16', 'uint8')
SEED, CTR = 0x9E3779B97F4A7C15, (3 << 32) | 77
K, S = 3, 2


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    ops.hip_ext()  # must load: no silent fallback
    return torch.device('cuda', 0)


def _cfg(channels, dtype, crop):
    """Gamma + normalisation (u8: gamma only), as test_gpu_replay_crop._vcfg."""
    if dtype == 'uint8':
        return DecodeConfig(channels=channels, gamma=2.2, dtype='uint8', crop=crop)
    return DecodeConfig.densityopt(channels=channels, gamma=2.2, dtype=dtype, crop=crop)


def _cpu_buffer(n, cap, H, W, C, seed, first=None, every=4):
    """n frames of a 2-environment loop (one extend per step) in a ring of `cap`; an episode starts every
    `every` steps unless `first` gives the flags; a 12-byte and a 5-byte metadata column."""
    f = frames(n, H, W, C, seed=seed)
    rng = np.random.default_rng(seed)
    if first is None:
        first = ((np.arange(n) // S) % every == 0).astype(np.uint8)
    meta = dict(first=np.asarray(first, np.uint8), action=rng.normal(size=(n, 3)).astype(np.float32),
                tag=rng.integers(0, 256, size=(n, 5), dtype=np.uint8))
    rb = DeviceReplayBuffer(cap, device='cpu', seed=SEED)
    for s in range(0, n, S):
        rb.extend(f[s:s + S], **{k: v[s:s + S] for k, v in meta.items()})
    return rb


@pytest.fixture(scope='module')
def stores():
    """A wrapped ring of 24 slots (30 frames of 48 x 64 x 3) and a partly filled one (10 of 16 slots, 16 x 64 x 4)."""
    return {'rgb': _cpu_buffer(30, 24, 48, 64, 3, seed=11), 'rgba': _cpu_buffer(10, 16, 16, 64, 4, seed=12)}


def _bytes(t):
    return t.contiguous().view(torch.uint8).reshape(-1).numpy()


def _launch(dev, cpu, cfg, B, idx=None, k=K, stride=S, ctr=CTR, max_grid=0, shared=False, shift=0, what='', over=None):
    """One replay_transitions launch through the binding on guard-filled buffers, compared with the CPU
    buffer's batch at the same counter.  over: arguments replaced for the rejection tests (then no compare)."""
    ext = ops.hip_ext()
    N, H, W, C = cpu.store.shape
    crop = cfg.crop
    h, w = (H, W) if crop is None else crop.size
    side_bytes = B * k * cfg.cout * h * w * ELEM[cfg.dtype]
    out = torch.full((GUARD + shift + 2 * side_bytes + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    store, first = cpu.store.to(dev), cpu.meta['first'].to(dev)
    cols = [cpu.meta['action'].to(dev), cpu.meta['tag'].to(dev)]
    nbytes = [12, 5]
    mdst = [torch.full((2 * GUARD + B * nb,), SENTINEL, dtype=torch.uint8, device=dev) for nb in nbytes]
    ndst = [torch.full((2 * GUARD + B * nb,), SENTINEL, dtype=torch.uint8, device=dev) for nb in nbytes]
    idx_out = torch.full((B + 64,), -1, dtype=torch.int64, device=dev)
    nidx_out = torch.full((B + 64,), -1, dtype=torch.int64, device=dev)
    valid = torch.full((2 * GUARD + B,), SENTINEL, dtype=torch.uint8, device=dev)
    crop_out = torch.full((3 * B + 64,), -7, dtype=torch.int32, device=dev)
    ncrop_out = torch.full((3 * B + 64,), -7, dtype=torch.int32, device=dev)
    idx_in = None if idx is None else torch.tensor(idx, dtype=torch.int64, device=dev)
    ckw = {}
    if crop is not None:
        ckw = dict(crop_size=list(crop.size), crop_mode=crop.mode, crop_origin=list(crop.origin or ()),
                   crop_pad=crop.pad, mirror=crop.mirror, x_align=crop.x_align,
                   window_key=(SEED + crop.seed) & (2 ** 64 - 1), shared_window=int(shared),
                   crop_out=crop_out.data_ptr(), next_crop_out=ncrop_out.data_ptr())
    a = dict(store=store.data_ptr(), capacity=N, head=cpu._next, size=len(cpu), state=0, first=first.data_ptr(),
             stack=k, stride=stride, dst=out.data_ptr() + GUARD + shift, lut=ops.device_lut(cfg, dev).data_ptr(), B=B,
             H=H, W=W, Cin=C, Cout=cfg.cout, cmap=cfg.cmap, flip_all=int(cfg.flip), out_dtype=ops.OUT_DTYPES[cfg.dtype],
             layout=ops.LAYOUTS[cfg.layout], seed=SEED, counter=0, ctr_value=ctr,
             index_in=0 if idx_in is None else idx_in.data_ptr(), index_out=idx_out.data_ptr(),
             next_index_out=nidx_out.data_ptr(), valid_out=valid.data_ptr() + GUARD,
             meta_src=[c.data_ptr() for c in cols], meta_dst=[m.data_ptr() + GUARD for m in mdst], meta_bytes=nbytes,
             next_src=[c.data_ptr() for c in cols], next_dst=[m.data_ptr() + GUARD for m in ndst], next_bytes=nbytes,
             stream=ops._stream(dev), xf_table_only=ops.table_only(cfg, dev), max_grid=max_grid, **ckw)
    a.update(over or {})
    try:
        if over:
            with pytest.raises(RuntimeError, match='invalid'):
                ext.replay_transitions(**a)
        else:
            ext.replay_transitions(**a)
    finally:
        torch.cuda.synchronize()
    got = dict(out=out.cpu().numpy(), index=idx_out.cpu().numpy(), next_index=nidx_out.cpu().numpy(),
               valid=valid.cpu().numpy(), crop=crop_out.cpu().numpy(), next_crop=ncrop_out.cpu().numpy(),
               meta=[m.cpu().numpy() for m in mdst], next_meta=[m.cpu().numpy() for m in ndst])
    if over:
        return got
    kw = dict(stack=k, stride=stride, next_keys=('action', 'tag'), shared_window=shared, _counter=ctr)
    c0 = cpu._ctr
    want = cpu.sample_transitions(B, cfg, **kw) if idx is None else cpu.gather_transitions(torch.tensor(idx), cfg, **kw)
    assert cpu._ctr == c0                                             # a given counter leaves the buffer's alone
    where = f'{what} {cfg.channels} Cin {C} {cfg.dtype} crop {crop} index {want["index"].tolist()}'
    assert np.array_equal(got['index'][:B], want['index'].numpy()) and (got['index'][B:] == -1).all(), where
    assert np.array_equal(got['next_index'][:B], want['next_index'].numpy()) and (got['next_index'][B:] == -1).all(), where
    assert np.array_equal(got['valid'][GUARD:-GUARD], want['valid'].numpy().astype(np.uint8)), where
    assert (got['valid'][:GUARD] == SENTINEL).all() and (got['valid'][-GUARD:] == SENTINEL).all(), where
    for key in ('crop', 'next_crop'):
        if crop is not None:
            assert np.array_equal(got[key][:3 * B].reshape(-1, 3), want[key].numpy()), (where, key)
            assert (got[key][3 * B:] == -7).all(), where
        else:
            assert (got[key] == -7).all(), where
    exp = np.full(len(got['out']), SENTINEL, np.uint8)
    exp[GUARD + shift:GUARD + shift + side_bytes] = _bytes(want['obs'])
    exp[GUARD + shift + side_bytes:GUARD + shift + 2 * side_bytes] = _bytes(want['next_obs'])
    if not np.array_equal(got['out'], exp):
        bad = np.flatnonzero(got['out'] != exp)
        p = bad[0] - GUARD - shift
        raise AssertionError(f'{where}: {len(bad)} bytes differ, first at byte {p} of the images '
                             f'(image bytes {side_bytes // B}): got {got["out"][bad[0]]:#x}, expected {exp[bad[0]]:#x}')
    for m, nm, key in zip(got['meta'], got['next_meta'], ('action', 'tag')):
        for g, wkey in ((m, key), (nm, 'next_' + key)):
            assert np.array_equal(g[GUARD:-GUARD], _bytes(want[wkey])), (where, wkey)
            assert (g[:GUARD] == SENTINEL).all() and (g[-GUARD:] == SENTINEL).all(), (where, wkey)
    return want


CROPS = {'none': lambda H, W: None,
         'crop': lambda H, W: Crop((32, 48) if H >= 32 else (8, 48), mirror=0.5, seed=3),
         'shift': lambda H, W: Crop((H, W), pad=4)}
# given anchors: valid ones, a repeat, the newest step (no successor yet), and on the rgba store an empty slot
GIVEN = {'rgb': [7, 8, 3, 4, 5, 23, 7], 'rgba': [3, 2, 8, 9, 12, 5, 5]}


@pytest.mark.parametrize('kind', list(CROPS))
@pytest.mark.parametrize('given', (False, True), ids=['drawn', 'given'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_launch_equals_cpu_buffer(dev, stores, dtype, given, kind):
    for name, cpu in stores.items():
        H, W = cpu.frame_shape[:2]
        cfg = _cfg('bgr' if name == 'rgb' else 'rgba', dtype, CROPS[kind](H, W))
        want = _launch(dev, cpu, cfg, 7, idx=GIVEN[name] if given else None, what=f'{name} {kind}')
        if given:
            assert want['valid'].any() and not want['valid'].all()
        if kind != 'none':
            assert not torch.equal(want['crop'], want['next_crop'])
            if kind == 'crop':
                assert set(want['crop'][:, 2].tolist()) | set(want['next_crop'][:, 2].tolist()) == {0, 1}
    # one window for both stacks; a table-mode value table (the kernels' table-only instantiations)
    cpu = stores['rgb']
    crop = CROPS['crop'](48, 64)
    want = _launch(dev, cpu, _cfg('rgb', dtype, crop), 5, shared=True, idx=[7, 9] * 2 + [11] if given else None)
    assert torch.equal(want['crop'], want['next_crop'])
    tab = DecodeConfig(channels='rgb', gamma=2.2, dtype=dtype, crop=crop) if dtype == 'uint8' else \
        DecodeConfig.unit(channels='rgb', gamma=2.2, dtype=dtype, crop=crop)
    _launch(dev, cpu, tab, 5, idx=[7, 9] * 2 + [11] if given else None, what='table mode')


@pytest.mark.parametrize('dtype', DTYPES)
def test_grid_stride_loop_and_scalar_fallback(dev, stores, dtype):
    """One block (max_grid = 1) walks every group; window width 30 and Cin = 1 take the one-pixel kernel."""
    cpu = stores['rgba']
    _launch(dev, cpu, _cfg('rgb', dtype, Crop((8, 48), mirror=0.5, pad=2)), 4, max_grid=1, what='grid 1')
    _launch(dev, cpu, _cfg('rgba', dtype, None), 3, idx=[3, 2, 8], max_grid=1, what='grid 1 given')
    _launch(dev, cpu, _cfg('rgb', dtype, Crop((8, 30), mirror=0.5, pad=3)), 4, what='width 30')
    _launch(dev, cpu, _cfg('rgb', dtype, Crop((8, 30), mirror=0.5)), 4, max_grid=1, what='width 30 grid 1')
    _launch(dev, cpu, _cfg('rgb', dtype, Crop((16, 64), pad=4)), 4, shift=ELEM[dtype], what='dst + 1 element')
    gray = _cpu_buffer(12, 16, 16, 64, 1, seed=13)
    _launch(dev, gray, _cfg('gray', dtype, None), 5, what='Cin 1')
    _launch(dev, gray, _cfg('gray', dtype, Crop((16, 64), pad=4)), 5, idx=[1, 4, 6, 7, 0], what='Cin 1 shift')


def test_more_images_than_lanes(dev):
    """B = 300 of 2 x 16 x 4 frames: the table fill strides past the block's 256 lanes (300 * 4 entries)."""
    cpu = _cpu_buffer(40, 32, 2, 16, 4, seed=31)
    for dtype in ('float32', 'uint8'):
        want = _launch(dev, cpu, _cfg('rgba', dtype, None), 300, what='B 300')
        assert len(set(want['index'][256:].tolist())) > 8
        _launch(dev, cpu, _cfg('rgba', dtype, Crop((2, 16), pad=1, mirror=0.5)), 300, max_grid=1, what='B 300 one block')


def test_episode_boundaries_and_wrapped_ring(dev):
    """The hand-made patterns of tests/test_replay_stack_cpu.py, on the device (S = 1 and S = 2, k = 3 and 4)."""
    cfg = _cfg('rgb', 'float32', None)

    def ring(n, cap, first_slots):
        slot_first = np.zeros(cap, np.uint8)
        slot_first[first_slots] = 1
        first = np.zeros(n, np.uint8)
        for i in range(max(0, n - cap), n):                           # frame i lands in slot i % cap
            first[i] = slot_first[i % cap]
        return _cpu_buffer(n, cap, 4, 16, 3, seed=n, first=first)

    part = ring(20, 24, [0, 10])                                      # head 20, slots 0..19 stored
    want = _launch(dev, part, cfg, 5, idx=[11, 12, 10, 15, 9], stride=1)
    assert want['next_index'].tolist() == [12, 13, 11, 16, 9] and want['valid'].tolist() == [1, 1, 1, 1, 0]
    ref = part.gather(torch.tensor([10, 10, 11, 12]), cfg)['image']   # anchor 11: the episode's first frame repeats
    assert torch.equal(want['obs'][0], ref[:3].reshape(9, 4, 16)) and torch.equal(want['next_obs'][0], ref[1:].reshape(9, 4, 16))
    two = ring(20, 24, [0, 1, 11])
    want = _launch(dev, two, cfg, 2, idx=[13, 12], stride=2)
    ref = two.gather(torch.tensor([11, 11, 13, 15, 8, 10, 12, 14]), cfg)['image']
    assert torch.equal(want['obs'][0], ref[:3].reshape(9, 4, 16)) and torch.equal(want['next_obs'][1], ref[5:].reshape(9, 4, 16))
    wrapped = ring(24 + 6, 24, [12])                                  # head 6: the oldest slots are 6 and 7
    assert wrapped._next == 6 and len(wrapped) == 24
    want = _launch(dev, wrapped, cfg, 3, idx=[9, 8, 5], k=4, stride=2)
    assert want['valid'].tolist() == [1, 1, 0]                        # slot 5 is the newest step
    ref = wrapped.gather(torch.tensor([7, 7, 7, 9, 11]), cfg)['image']
    assert torch.equal(want['obs'][0], ref[:4].reshape(12, 4, 16)) and torch.equal(want['next_obs'][0], ref[1:].reshape(12, 4, 16))
    _launch(dev, wrapped, cfg, 64, k=4, stride=2, what='wrapped drawn')
    _launch(dev, wrapped, cfg, 64, k=1, stride=1, what='wrapped k 1')
    # every frame first: no valid transition, every stack a repeated frame
    allfirst = ring(20, 24, list(range(24)))
    want = _launch(dev, allfirst, cfg, 16, stride=2)
    assert not want['valid'].any() and torch.equal(want['index'], want['next_index'])
    assert torch.equal(want['obs'], want['next_obs']) and torch.equal(want['obs'][:, :3], want['obs'][:, 6:])


@pytest.mark.parametrize('what', ['k = 17', 'B * (k + 1) > 8192', 'stride >= capacity', 'NHWC', 'size <= stride',
                                  'no first column'])
def test_rejected_on_the_host_before_any_launch(dev, stores, what):
    cpu = stores['rgba']
    cfg = _cfg('rgb', 'float32', Crop((8, 48), pad=2))
    over = {'k = 17': dict(stack=17),
            # (no buffer of that size exists: a launch would write far past the guards)
            'B * (k + 1) > 8192': dict(B=1000, stack=8),
            'stride >= capacity': dict(stride=16),
            'NHWC': dict(layout=ops.LAYOUTS['nhwc']),
            'size <= stride': dict(size=2),
            'no first column': dict(first=0)}[what]
    got = _launch(dev, cpu, cfg, 4, over=over)                          # raises 'invalid' inside; nothing was written
    assert (got['out'] == SENTINEL).all() and (got['index'] == -1).all() and (got['next_index'] == -1).all()
    assert (got['valid'] == SENTINEL).all() and (got['crop'] == -7).all() and (got['next_crop'] == -7).all()
    assert all((m == SENTINEL).all() for m in got['meta'] + got['next_meta'])
    _launch(dev, cpu, cfg, 4, what='legal')                           # and the well-formed launch runs


# ---- ops.replay_transitions and DeviceReplayBuffer ----------------------------------------------------------------

def _gpu_twin(cpu, dev):
    gpu = DeviceReplayBuffer(cpu.capacity, device=dev, seed=cpu.seed)
    gpu.store = cpu.store.to(dev)
    gpu.meta = {k: v.to(dev) for k, v in cpu.meta.items()}
    gpu._next, gpu._size, gpu._ctr = cpu._next, cpu._size, cpu._ctr
    return gpu


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert torch.equal(a[k].contiguous().view(torch.uint8), b[k].cpu().contiguous().view(torch.uint8)), k


BUF_CFGS = [DecodeConfig.unit(channels='rgb', gamma=2.2),
            DecodeConfig.densityopt(channels='bgr', dtype='bfloat16', crop=Crop((32, 48), mirror=0.5, seed=4)),
            DecodeConfig(channels='rgb', dtype='uint8', crop=Crop((48, 64), pad=4))]


@pytest.mark.parametrize('cfg', BUF_CFGS, ids=['f32-plain', 'bf16-crop', 'u8-shift'])
def test_gpu_buffer_equals_cpu_buffer(dev, cfg):
    cpu = _cpu_buffer(30, 24, 48, 64, 3, seed=21)
    gpu = _gpu_twin(cpu, dev)
    kw = dict(stack=K, stride=S, next_keys=('action', 'first'))
    for _ in range(2):
        a, b = cpu.sample_transitions(6, cfg, **kw), gpu.sample_transitions(6, cfg, **kw)
        _same(a, b)
        assert b['obs'].is_cuda and b['obs'].shape == (6, K * 3) + (cfg.crop.size if cfg.crop else (48, 64))
    idx = torch.tensor([7, 8, 4, 23])
    _same(cpu.gather_transitions(idx, cfg, **kw), gpu.gather_transitions(idx.to(dev), cfg, **kw))
    assert cpu._ctr == gpu._ctr == 12 + (4 if cfg.crop is not None else 0)
    _same(cpu.sample_transitions(5, cfg, shared_window=True, **kw), gpu.sample_transitions(5, cfg, shared_window=True, **kw))
    # the existing entry points keep their stream: same counter, same sample as a buffer that never drew a transition
    fresh = _gpu_twin(_cpu_buffer(30, 24, 48, 64, 3, seed=21), dev)
    fresh._ctr = gpu._ctr
    x, y = gpu.sample(4, cfg), fresh.sample(4, cfg)
    assert torch.equal(x['index'], y['index']) and torch.equal(x['image'], y['image'])
    for bad in (dataclasses.replace(BUF_CFGS[0], layout='nhwc'),
                DecodeConfig.unit(channels='rgb', resize=ops.ResizedCrop((4, 8)))):
        with pytest.raises(ValueError):
            gpu.sample_transitions(4, bad, **kw)
    with pytest.raises(ValueError):
        gpu.sample_transitions(4, cfg, first_key='action', **kw)
    with pytest.raises(RuntimeError, match='invalid'):                # the kernel's own check, through ops
        ops.replay_transitions(gpu.store, gpu._next, gpu._size, 4, cfg, stack=17, stride=S, first=gpu.meta['first'],
                               counter=0)


def test_graphed_transition_sampler_follows_a_growing_store(dev):
    cfg = BUF_CFGS[1]
    H, W = 48, 64
    f = frames(8, H, W, 3, seed=5)
    meta = lambda n, first: dict(first=np.full(n, first, np.uint8), action=np.zeros((n, 3), np.float32),
                                 tag=np.zeros((n, 5), np.uint8))
    gpu = DeviceReplayBuffer(24, device=dev, seed=77)
    gpu.extend(f[:2], **meta(2, 1))
    for s in range(2, 8, 2):
        gpu.extend(f[s:s + 2], **meta(2, 0))
    kw = dict(stack=K, stride=S, next_keys=('action',))
    sampler = gpu.graphed_transition_sampler(8, cfg, warmup=2, **kw)
    seen = []
    for _ in range(2):
        c = int(sampler.counter)
        b = {k: v.clone() for k, v in sampler().items()}
        assert int(sampler.counter) == c + 8                          # the graph advances its own counter
        eager = gpu.sample_transitions(8, cfg, _counter=c, **kw)
        _same({k: v.cpu() for k, v in eager.items()}, b)
        assert int(b['index'].max()) < 6 and bool(b['valid'].all())   # anchors are never the newest step
        seen.append((b['index'].tolist(), b['crop'].tolist()))
    assert seen[0][0] != seen[1][0] and seen[0][1] != seen[1][1]
    # the store grows: 12 frames of one recognisable value; the SAME graph now draws among them
    const = np.full((12, H, W, 3), 200, np.uint8)
    for s in range(0, 12, 2):
        gpu.extend(const[s:s + 2], **meta(2, 0))
    value = ops.reference_decode(torch.from_numpy(const[:1]), dataclasses.replace(cfg, crop=None))[0, 0, 0, 0]
    new = 0
    for _ in range(3):
        c = int(sampler.counter)
        b = {k: v.clone() for k, v in sampler().items()}
        _same({k: v.cpu() for k, v in gpu.sample_transitions(8, cfg, _counter=c, **kw).items()}, b)
        assert int(b['index'].max()) < 18
        for i in torch.nonzero(b['index'] >= 8).flatten().tolist():
            new += 1
            assert bool((b['obs'][i, -3:].cpu() == value).all())      # the anchor's frame is one of the new ones
    assert new >= 4                                                   # 10 of the 18 anchors' slots are new


def test_bench_replay_stack_runs(dev):
    root = Path(__file__).resolve().parents[1]
    r = subprocess.run([sys.executable, str(root / 'benchmarks' / 'bench_replay.py'), '--stack', '3', '--frames', '64',
                        '--steps', '3', '--warmup', '1'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for row in ('fused transitions', 'composed gathers', 'equal-bytes sample'):
        assert row in r.stdout, r.stdout
