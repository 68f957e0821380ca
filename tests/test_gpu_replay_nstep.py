"""n-step transitions in the fused replay launch (csrc/gpu/kernels.hip ``replay_sample_stack`` with
``nstep``) and through ``DeviceReplayBuffer``.

As in tests/test_gpu_replay_stack.py the launches go through the binding into SENTINEL-filled buffers and every
output byte -- images, indices, validity, windows, the metadata at both ends and the three n-step outputs, guards
included -- is compared with the CPU buffer's batch at the same seed and counter.  The stores are that file's
small ones (30 frames of 48 x 64 x 3 in 24 slots, 10 of 16 slots of 16 x 64 x 4; S = 2) with the episode layouts,
reward and done columns of tests/nstep_cases.py, which tests/test_replay_nstep_cpu.py checks against a
brute-force simulation."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from decode_oracle import ELEM, GUARD, SENTINEL, frames
from nstep_cases import SEED, bits, classes, cpu_buffer
from blendtorch import ops
from blendtorch.btt.replay import DeviceReplayBuffer
from blendtorch.ops import Crop, DecodeConfig

pytestmark = pytest.mark.gpu

DTYPES = ('float32', 'bfloat16', 'float16', 'uint8')
CTR = (3 << 32) | 77
K, S, GAMMA = 3, 2, 0.99
NSTEPS = (1, 3, 5)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    ops.hip_ext()  # must load: no silent fallback
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def stores():
    """A wrapped ring of 24 slots (30 frames of 48 x 64 x 3) and a partly filled one (10 of 16 slots, 16 x 64 x 4)."""
    return {'rgb': cpu_buffer(30, 24, 48, 64, 3, S, seed=11)[0], 'rgba': cpu_buffer(10, 16, 16, 64, 4, S, seed=12)[0]}


def _cfg(channels, dtype, crop):
    if dtype == 'uint8':
        return DecodeConfig(channels=channels, gamma=2.2, dtype='uint8', crop=crop)
    return DecodeConfig.densityopt(channels=channels, gamma=2.2, dtype=dtype, crop=crop)


def _guarded(nbytes, dev):
    return torch.full((2 * GUARD + nbytes,), SENTINEL, dtype=torch.uint8, device=dev)


def _launch(dev, cpu, cfg, B, n, idx=None, k=K, stride=S, ctr=CTR, max_grid=0, shift=0, use_done=True, gamma=GAMMA,
            what='', over=None):
    """One n-step replay_transitions launch through the binding on guard-filled buffers, compared with the CPU
    buffer's batch at the same counter.  over: arguments replaced for the rejection tests (then no compare)."""
    ext = ops.hip_ext()
    N, H, W, C = cpu.store.shape
    crop = cfg.crop
    h, w = (H, W) if crop is None else crop.size
    side_bytes = B * k * cfg.cout * h * w * ELEM[cfg.dtype]
    out = torch.full((GUARD + shift + 2 * side_bytes + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    store, first = cpu.store.to(dev), cpu.meta['first'].to(dev)
    reward, done = cpu.meta['reward'].to(dev), cpu.meta['done'].to(dev)
    cols = [cpu.meta['action'].to(dev), cpu.meta['tag'].to(dev)]
    nbytes = [12, 5]
    mdst = [_guarded(B * nb, dev) for nb in nbytes]
    ndst = [_guarded(B * nb, dev) for nb in nbytes]
    idx_out = torch.full((B + 64,), -1, dtype=torch.int64, device=dev)
    nidx_out = torch.full((B + 64,), -1, dtype=torch.int64, device=dev)
    valid = _guarded(B, dev)
    ret, disc, steps = _guarded(4 * B, dev), _guarded(4 * B, dev), _guarded(4 * B, dev)
    crop_out = torch.full((3 * B + 64,), -7, dtype=torch.int32, device=dev)
    ncrop_out = torch.full((3 * B + 64,), -7, dtype=torch.int32, device=dev)
    idx_in = None if idx is None else torch.tensor(idx, dtype=torch.int64, device=dev)
    ckw = {}
    if crop is not None:
        ckw = dict(crop_size=list(crop.size), crop_mode=crop.mode, crop_origin=list(crop.origin or ()),
                   crop_pad=crop.pad, mirror=crop.mirror, x_align=crop.x_align,
                   window_key=(SEED + crop.seed) & (2 ** 64 - 1), shared_window=0,
                   crop_out=crop_out.data_ptr(), next_crop_out=ncrop_out.data_ptr())
    a = dict(store=store.data_ptr(), capacity=N, head=cpu._next, size=len(cpu), state=0, first=first.data_ptr(),
             stack=k, stride=stride, dst=out.data_ptr() + GUARD + shift, lut=ops.device_lut(cfg, dev).data_ptr(), B=B,
             H=H, W=W, Cin=C, Cout=cfg.cout, cmap=cfg.cmap, flip_all=int(cfg.flip), out_dtype=ops.OUT_DTYPES[cfg.dtype],
             layout=ops.LAYOUTS[cfg.layout], seed=SEED, counter=0, ctr_value=ctr,
             index_in=0 if idx_in is None else idx_in.data_ptr(), index_out=idx_out.data_ptr(),
             next_index_out=nidx_out.data_ptr(), valid_out=valid.data_ptr() + GUARD,
             meta_src=[c.data_ptr() for c in cols], meta_dst=[m.data_ptr() + GUARD for m in mdst], meta_bytes=nbytes,
             next_src=[c.data_ptr() for c in cols], next_dst=[m.data_ptr() + GUARD for m in ndst], next_bytes=nbytes,
             stream=ops._stream(dev), xf_table_only=ops.table_only(cfg, dev), max_grid=max_grid,
             nstep=n, gamma=gamma, reward=reward.data_ptr(), done=done.data_ptr() if use_done else 0,
             return_out=ret.data_ptr() + GUARD, discount_out=disc.data_ptr() + GUARD, steps_out=steps.data_ptr() + GUARD,
             **ckw)
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
               meta=[m.cpu().numpy() for m in mdst], next_meta=[m.cpu().numpy() for m in ndst],
               nstep_return=ret.cpu().numpy(), nstep_discount=disc.cpu().numpy(), nstep_steps=steps.cpu().numpy())
    if over:
        return got
    kw = dict(stack=k, stride=stride, next_keys=('action', 'tag'), _counter=ctr, nstep=n, gamma=gamma,
              done_key='done' if use_done else None)
    c0 = cpu._ctr
    want = cpu.sample_transitions(B, cfg, **kw) if idx is None else cpu.gather_transitions(torch.tensor(idx), cfg, **kw)
    assert cpu._ctr == c0
    where = f'{what} n {n} k {k} {cfg.channels} Cin {C} {cfg.dtype} crop {crop} index {want["index"].tolist()}'
    assert np.array_equal(got['index'][:B], want['index'].numpy()) and (got['index'][B:] == -1).all(), where
    assert np.array_equal(got['next_index'][:B], want['next_index'].numpy()) and (got['next_index'][B:] == -1).all(), where
    assert np.array_equal(got['valid'][GUARD:-GUARD], want['valid'].numpy().astype(np.uint8)), where
    assert (got['valid'][:GUARD] == SENTINEL).all() and (got['valid'][-GUARD:] == SENTINEL).all(), where
    for key in ('nstep_steps', 'nstep_return', 'nstep_discount'):     # bit for bit, sentinels intact around each
        g = got[key]
        assert np.array_equal(g[GUARD:-GUARD], bits(want[key])), (where, key, g[GUARD:-GUARD].view(
            np.int32 if key == 'nstep_steps' else np.float32).tolist(), want[key].tolist())
        assert (g[:GUARD] == SENTINEL).all() and (g[-GUARD:] == SENTINEL).all(), (where, key)
    for key in ('crop', 'next_crop'):
        if crop is not None:
            assert np.array_equal(got[key][:3 * B].reshape(-1, 3), want[key].numpy()), (where, key)
            assert (got[key][3 * B:] == -7).all(), where
        else:
            assert (got[key] == -7).all(), where
    exp = np.full(len(got['out']), SENTINEL, np.uint8)
    exp[GUARD + shift:GUARD + shift + side_bytes] = bits(want['obs'])
    exp[GUARD + shift + side_bytes:GUARD + shift + 2 * side_bytes] = bits(want['next_obs'])
    if not np.array_equal(got['out'], exp):
        bad = np.flatnonzero(got['out'] != exp)
        p = bad[0] - GUARD - shift
        raise AssertionError(f'{where}: {len(bad)} bytes differ, first at byte {p} of the images '
                             f'(image bytes {side_bytes // B}): got {got["out"][bad[0]]:#x}, expected {exp[bad[0]]:#x}')
    for m, nm, key in zip(got['meta'], got['next_meta'], ('action', 'tag')):
        for g, wkey in ((m, key), (nm, 'next_' + key)):
            assert np.array_equal(g[GUARD:-GUARD], bits(want[wkey])), (where, wkey)
            assert (g[:GUARD] == SENTINEL).all() and (g[-GUARD:] == SENTINEL).all(), (where, wkey)
    return want


CROPS = {'none': lambda H, W: None,
         'crop': lambda H, W: Crop((32, 48) if H >= 32 else (8, 48), mirror=0.5, seed=3),
         'shift': lambda H, W: Crop((H, W), pad=4)}


def _channels(name):
    return 'bgr' if name == 'rgb' else 'rgba'


def test_stores_cover_every_class(stores):
    """From the reference alone: every slot as an anchor meets a full walk, one cut by a first frame, one cut by
    the newest stored step, a termination and invalid anchors (the newest step, an empty slot)."""
    for n in (3, 5):
        got = set()
        for cpu in stores.values():
            head, size, cap = cpu._next, len(cpu), cpu.capacity
            first, done, reward = (cpu.meta[c].numpy() for c in ('first', 'done', 'reward'))
            anchor = np.arange(cap)
            valid = ops.given_transitions(anchor, head, size, cap, S, 1, first)[3]
            _, steps, _, disc = ops.nstep_transitions(anchor, valid, head, size, cap, S, n, GAMMA, reward, first, done)
            got |= classes(steps, valid, disc, anchor, head, size, cap, S, n, first, True)
        assert got == {'full', 'first', 'newest', 'terminated', 'invalid'}, (n, got)
    assert len(stores['rgba']) < stores['rgba'].capacity              # arange(capacity) holds empty slots


@pytest.mark.parametrize('given', (False, True), ids=['drawn', 'given'])
@pytest.mark.parametrize('k', (1, 3))
@pytest.mark.parametrize('n', NSTEPS)
def test_launch_equals_cpu_buffer(dev, stores, n, k, given):
    """fp32 random shift; given anchors: every slot of the ring (the newest step, empty slots, every class)."""
    for name, cpu in stores.items():
        H, W = cpu.frame_shape[:2]
        cfg = _cfg(_channels(name), 'float32', CROPS['shift'](H, W))
        idx = list(range(cpu.capacity)) if given else None
        for use_done in (True, False):
            want = _launch(dev, cpu, cfg, cpu.capacity if given else 16, n, idx=idx, k=k, use_done=use_done,
                           what=f'{name} done {use_done}')
            steps = want['nstep_steps']
            if given:
                assert want['valid'].any() and not want['valid'].all() and int(steps.min()) == 0
                if n > 1:
                    assert len(set(steps.tolist())) >= 3
                if use_done and n > 1:
                    assert bool(((want['nstep_discount'] == 0) & want['valid']).any())


@pytest.mark.parametrize('dtype', DTYPES)
def test_output_dtypes(dev, stores, dtype):
    for name, cpu in stores.items():
        H, W = cpu.frame_shape[:2]
        _launch(dev, cpu, _cfg(_channels(name), dtype, CROPS['crop'](H, W)), 9, 3, what=f'{name} drawn')
        _launch(dev, cpu, _cfg(_channels(name), dtype, CROPS['crop'](H, W)), cpu.capacity, 3,
                idx=list(range(cpu.capacity)), what=f'{name} given')


@pytest.mark.parametrize('kind', list(CROPS))
def test_crop_kinds(dev, stores, kind):
    for name, cpu in stores.items():
        H, W = cpu.frame_shape[:2]
        cfg = _cfg(_channels(name), 'float32', CROPS[kind](H, W))
        _launch(dev, cpu, cfg, 9, 3, what=f'{name} {kind} drawn')
        want = _launch(dev, cpu, cfg, cpu.capacity, 5, idx=list(range(cpu.capacity)), what=f'{name} {kind} given')
        if kind != 'none':
            assert not torch.equal(want['crop'], want['next_crop'])
    # a table-mode value table (the kernels' table-only instantiations)
    tab = DecodeConfig.unit(channels='rgb', gamma=2.2, crop=CROPS['crop'](48, 64))
    _launch(dev, stores['rgb'], tab, 24, 3, idx=list(range(24)), what='table mode')


def test_grid_stride_loop_and_scalar_fallback(dev, stores):
    """One block (max_grid = 1) walks every group; a destination shifted by one element and a window width of 30
    take the one-pixel kernel."""
    cpu = stores['rgba']
    every = list(range(cpu.capacity))
    for dtype in ('float32', 'uint8'):
        _launch(dev, cpu, _cfg('rgb', dtype, Crop((8, 48), mirror=0.5, pad=2)), 16, 3, idx=every, max_grid=1, what='grid 1')
        _launch(dev, cpu, _cfg('rgba', dtype, None), 5, 5, max_grid=1, what='grid 1 drawn')
        _launch(dev, cpu, _cfg('rgb', dtype, Crop((16, 64), pad=4)), 16, 3, idx=every, shift=ELEM[dtype], what='dst + 1 element')
        _launch(dev, cpu, _cfg('rgb', dtype, Crop((8, 30), mirror=0.5, pad=3)), 16, 5, idx=every, max_grid=1, what='width 30 grid 1')


def test_more_images_than_lanes(dev):
    """B = 300 of 2 x 16 x 4 frames: the table fill strides past the block's 256 lanes (300 * (3 + n) entries)."""
    cpu = cpu_buffer(40, 32, 2, 16, 4, S, seed=31)[0]
    want = _launch(dev, cpu, _cfg('rgba', 'float32', None), 300, 3, what='B 300')
    assert len(set(want['index'][256:].tolist())) > 8 and len(set(want['nstep_steps'][256:].tolist())) >= 2
    _launch(dev, cpu, _cfg('rgba', 'uint8', Crop((2, 16), pad=1, mirror=0.5)), 300, 5, max_grid=1, what='B 300 one block')
    _launch(dev, cpu, _cfg('rgba', 'float32', None), 300, 16, k=1, idx=[i % 32 for i in range(300)], what='B 300 n 16')


@pytest.mark.parametrize('what', ['n = 17', 'B * (k + n) > 8192', 'no reward column', 'misaligned reward', 'gamma = 1.5',
                                  'gamma NaN', 'n = -1', 'misaligned return'])
def test_rejected_on_the_host_before_any_launch(dev, stores, what):
    cpu = stores['rgba']
    cfg = _cfg('rgb', 'float32', Crop((8, 48), pad=2))
    reward = cpu.meta['reward'].to(dev)
    spare = torch.zeros(64, dtype=torch.float32, device=dev)
    over = {'n = 17': dict(nstep=17),
            # B * (k + 1) = 4000 passes the 1-step limit; (no buffer of that size exists: a launch would write
            # far past the guards)
            'B * (k + n) > 8192': dict(B=1000, stack=3, nstep=6),
            'no reward column': dict(reward=0),
            'misaligned reward': dict(reward=reward.data_ptr() + 2),
            'gamma = 1.5': dict(gamma=1.5),
            'gamma NaN': dict(gamma=float('nan')),
            'n = -1': dict(nstep=-1),
            'misaligned return': dict(return_out=spare.data_ptr() + 1)}[what]
    got = _launch(dev, cpu, cfg, 4, 3, over=over)                     # raises 'invalid' inside; nothing was written
    assert (got['out'] == SENTINEL).all() and (got['index'] == -1).all() and (got['next_index'] == -1).all()
    assert (got['valid'] == SENTINEL).all() and (got['crop'] == -7).all() and (got['next_crop'] == -7).all()
    assert all((m == SENTINEL).all() for m in got['meta'] + got['next_meta'])
    assert all((got[key] == SENTINEL).all() for key in ('nstep_return', 'nstep_discount', 'nstep_steps'))
    assert not spare.any()
    _launch(dev, cpu, cfg, 4, 3, what='legal')                        # and the well-formed launch runs


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
    cpu = cpu_buffer(30, 24, 48, 64, 3, S, seed=21)[0]
    gpu = _gpu_twin(cpu, dev)
    kw = dict(stack=K, stride=S, next_keys=('action', 'first'))
    keys = set(gpu.sample_transitions(6, cfg, **kw))
    cpu._ctr = gpu._ctr
    for n, done_key in ((3, 'done'), (5, None), (1, 'done')):
        nkw = dict(nstep=n, gamma=GAMMA, done_key=done_key)
        a, b = cpu.sample_transitions(6, cfg, **kw, **nkw), gpu.sample_transitions(6, cfg, **kw, **nkw)
        _same(a, b)
        assert set(b) == keys | {'nstep_return', 'nstep_discount', 'nstep_steps'} and b['nstep_return'].is_cuda
        idx = torch.arange(24)
        _same(cpu.gather_transitions(idx, cfg, **kw, **nkw), gpu.gather_transitions(idx.to(dev), cfg, **kw, **nkw))
        assert cpu._ctr == gpu._ctr
    # nstep = None draws what a buffer that never saw the keyword draws
    fresh = _gpu_twin(cpu, dev)
    _same({k: v.cpu() for k, v in fresh.sample_transitions(5, cfg, **kw).items()}, gpu.sample_transitions(5, cfg, **kw))
    first, reward, done = gpu.meta['first'], gpu.meta['reward'], gpu.meta['done']
    call = lambda **o: ops.replay_transitions(gpu.store, gpu._next, gpu._size, 4, cfg, stack=K, stride=S, first=first,
                                              counter=0, **{**dict(nstep=3, reward=reward, done=done), **o})
    for bad in (dict(reward=None), dict(reward=reward.double()), dict(reward=reward[:-1]), dict(reward=reward.cpu()),
                dict(reward=torch.zeros(48, device=dev)[::2]), dict(done=done.to(torch.int32)), dict(done=done[:-1]),
                dict(nstep=17), dict(gamma=1.5)):
        with pytest.raises(ValueError):
            call(**bad)
    out, info = call()
    assert info['nstep_steps'].dtype == torch.int32 and out.shape[:2] == (2, 4)


def test_graphed_sampler_follows_a_growing_store(dev):
    """n = 3 from one captured graph on the device's (head, size): the walk's newest-step cut moves with the store."""
    cfg = BUF_CFGS[1]
    H, W = 48, 64
    f = frames(24, H, W, 3, seed=5)
    rng = np.random.default_rng(5)
    meta = lambda n, first: dict(first=np.full(n, first, np.uint8), action=np.zeros((n, 3), np.float32),
                                 reward=rng.normal(size=n).astype(np.float32), done=np.zeros(n, np.uint8))
    gpu = DeviceReplayBuffer(24, device=dev, seed=77)
    gpu.extend(f[:2], **meta(2, 1))
    for s in range(2, 8, 2):
        gpu.extend(f[s:s + 2], **meta(2, 0))
    kw = dict(stack=K, stride=S, next_keys=('action',), nstep=3, gamma=GAMMA, done_key='done')
    sampler = gpu.graphed_transition_sampler(8, cfg, warmup=2, **kw)
    seen = set()
    for grow in range(4):
        for _ in range(2):
            c = int(sampler.counter)
            b = {k: v.clone() for k, v in sampler().items()}
            assert int(sampler.counter) == c + 8                      # the graph advances its own counter
            _same({k: v.cpu() for k, v in gpu.sample_transitions(8, cfg, _counter=c, **kw).items()}, b)
            assert bool(b['valid'].all()) and int(b['index'].max()) < len(gpu) - 2
            # one episode so far: the walk is cut by the newest stored step alone
            age = (len(gpu) - 1 - b['index']) // 2
            assert torch.equal(b['nstep_steps'].long(), age.clamp(max=3)), (b['index'], b['nstep_steps'])
            seen |= set(b['nstep_steps'].tolist())
        s = 8 + 4 * grow
        gpu.extend(f[s:s + 2], **meta(2, 0))
        gpu.extend(f[s + 2:s + 4], **meta(2, 0))
    assert seen == {1, 2, 3}


def test_bench_replay_nstep_runs(dev):
    root = Path(__file__).resolve().parents[1]
    r = subprocess.run([sys.executable, str(root / 'benchmarks' / 'bench_replay.py'), '--stack', '3', '--nstep', '3',
                        '--frame', '16', '64', '4', '--frames', '64', '--steps', '3', '--warmup', '1'],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for row in ('fused 3-step', 'fused 1-step', 'composed 3-step', 'n-step / 1-step', 'n-step / composed'):
        assert row in r.stdout, r.stdout
