"""Frame-stacked transition sampling without a GPU: the numpy reference of the
kernel's draw (``ops.philox_transitions`` / ``ops.given_transitions``) against a
plain-Python loop of the documented rule, hand-made episode patterns, the 16-try
rejection cap, the window streams, and the CPU ``DeviceReplayBuffer``."""
import dataclasses

import numpy as np
import pytest
import torch

from blendtorch import ops
from blendtorch.btt.replay import DeviceReplayBuffer
from blendtorch.ops import Crop, DecodeConfig

SEEDS = (0, 1, 1 << 63)
M32 = 0xFFFFFFFF


# ---- the rule, in plain Python ------------------------------------------------------------------------------------

def philox4x32(key, b, ctr, c3):
    """Philox4x32-10 (Salmon et al., SC'11): the four output words of counter (b, ctr lo, ctr hi, c3)."""
    c = [b & M32, ctr & M32, (ctr >> 32) & M32, c3 & M32]
    k0, k1 = key & M32, (key >> 32) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def table_py(anchor, succ, head, size, cap, S, k, first):
    e = [0] * (k + 1)
    e[k], e[k - 1] = succ, anchor
    for j in range(k - 2, -1, -1):
        nxt = e[j + 1]
        age = (head - 1 - nxt) % cap
        e[j] = nxt if (first[nxt] != 0 or age + S >= size) else (nxt - S) % cap
    return e


def transitions_py(seed, ctr, B, head, size, cap, S, k, first):
    anchors, succs, tables, valids = [], [], [], []
    for b in range(B):
        chosen = None
        for t in range(16):
            c3 = 0 if t < 4 else 1 + (t >> 2)
            w = philox4x32(seed, b, ctr, c3)[t & 3]
            a = S + ((w * (size - S)) >> 32)
            s = (head - 1 - a) % cap
            n = (s + S) % cap
            if first[n] == 0:
                chosen = (s, n)
                break
        valid = chosen is not None
        if not valid:
            chosen = (s, s)
        anchors.append(chosen[0]), succs.append(chosen[1]), valids.append(valid)
        tables.append(table_py(chosen[0], chosen[1], head, size, cap, S, k, first))
    return np.array(anchors), np.array(succs), np.array(tables), np.array(valids)


# (capacity, size, head, S): a partly filled ring (head == size) and rings extended past capacity
RINGS = [(24, 17, 17, 1), (24, 18, 18, 3), (24, 24, 7, 1), (24, 24, 9, 3), (23, 23, 0, 1)]


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('k', (1, 3, 4))
def test_philox_transitions_equals_the_plain_loop(seed, k):
    seen = set()
    for ri, (cap, size, head, S) in enumerate(RINGS):
        rng = np.random.default_rng(100 + ri)
        for density in (0.0, 0.3, 0.9):
            first = (rng.random(cap) < density).astype(np.uint8)
            for ctr in (0, 77, (3 << 32) | 5):
                got = ops.philox_transitions(seed, ctr, 40, head, size, cap, S, k, first)
                want = transitions_py(seed, ctr, 40, head, size, cap, S, k, first)
                for g, w, name in zip(got, want, ('anchor', 'successor', 'table', 'valid')):
                    assert np.array_equal(g, w), (name, cap, size, head, S, density, ctr)
                anchor, succ, table, valid = got
                assert table.shape == (40, k + 1) and valid.dtype == bool
                assert ((table >= 0) & (table < cap)).all()
                age = (head - 1 - table) % cap
                assert (age[:, :k] < size).all()                      # only stored frames
                assert np.array_equal(succ[~valid], anchor[~valid])
                seen |= {bool(v) for v in valid}
    assert seen == {True, False}                                      # the cap of 16 tries is reached somewhere


def test_first_candidate_is_the_index_draws_word():
    """Candidate 0 is word 0 of block 0: philox_indices' word."""
    cap = size = 1000
    first = np.zeros(cap, np.uint8)
    for seed in SEEDS:
        anchor, succ, _, valid = ops.philox_transitions(seed, 9, 64, 0, size, cap, 1, 1, first)
        assert valid.all()
        idx = ops.philox_indices(seed, 9, 64, size - 1)               # (word * (size - S)) >> 32
        assert np.array_equal(anchor, (0 - 1 - (1 + idx)) % cap)
        for b in (0, 5, 63):
            assert philox4x32(seed, b, 9, 0)[0] * (size - 1) >> 32 == idx[b]


# ---- hand-made episodes, capacity 24 ------------------------------------------------------------------------------

def test_stack_repeats_the_episodes_first_frame():
    cap, size, head = 24, 20, 20
    first = np.zeros(cap, np.uint8)
    first[[0, 10]] = 1
    a, s, tbl, valid = ops.given_transitions([11, 12, 10, 15], head, size, cap, 1, 3, first)
    assert tbl.tolist() == [[10, 10, 11, 12], [10, 11, 12, 13], [10, 10, 10, 11], [13, 14, 15, 16]]
    assert valid.all() and s.tolist() == [12, 13, 11, 16]
    # the step before a reset has no successor in its episode
    a, s, tbl, valid = ops.given_transitions([9], head, size, cap, 1, 3, first)
    assert not valid[0] and s[0] == 9 and tbl.tolist() == [[7, 8, 9, 9]]
    # two environments in lockstep: env 1 resets at slot 11, env 0 does not
    first = np.zeros(cap, np.uint8)
    first[[0, 1, 11]] = 1
    _, _, tbl, valid = ops.given_transitions([13, 12], head, size, cap, 2, 3, first)
    assert tbl.tolist() == [[11, 11, 13, 15], [8, 10, 12, 14]] and valid.all()


def test_stack_repeats_the_oldest_stored_frame():
    cap = size = 24
    first = np.zeros(cap, np.uint8)
    first[12] = 1
    _, _, tbl, valid = ops.given_transitions([6], 5, size, cap, 1, 4, first)       # oldest slot: 5
    assert tbl.tolist() == [[5, 5, 5, 6, 7]] and valid.all()
    _, _, tbl, valid = ops.given_transitions([9, 8], 6, size, cap, 2, 4, first)    # oldest slots: 6, 7
    assert tbl.tolist() == [[7, 7, 7, 9, 11], [6, 6, 6, 8, 10]] and valid.all()
    # a partly filled ring: nothing before slot 0
    _, _, tbl, _ = ops.given_transitions([1], 10, 10, cap, 1, 4, first)
    assert tbl.tolist() == [[0, 0, 0, 1, 2]]
    # given anchors that are no transition: among the newest S frames, or not stored
    _, s, _, valid = ops.given_transitions([9, 8, 15, 33], 10, 10, cap, 1, 2, first)
    assert valid.tolist() == [False, True, False, False] and s.tolist() == [9, 9, 15, 9]


@pytest.mark.parametrize('seed', SEEDS)
def test_valid_transitions_cross_no_reset_and_are_not_the_newest(seed):
    for cap, size, head, S in RINGS:
        first = (np.random.default_rng(cap + S).random(cap) < 0.3).astype(np.uint8)
        anchor, succ, table, valid = ops.philox_transitions(seed, 3, 256, head, size, cap, S, 3, first)
        assert valid.any()
        assert (first[succ[valid]] == 0).all()
        age = (head - 1 - anchor) % cap
        assert (age[valid] >= S).all() and (age < size).all()
        assert np.array_equal(succ[valid], (anchor[valid] + S) % cap)
        assert np.array_equal(table[:, -1], succ) and np.array_equal(table[:, -2], anchor)


def test_every_frame_first_gives_no_valid_transition():
    first = np.ones(24, np.uint8)
    for seed in SEEDS:
        anchor, succ, table, valid = ops.philox_transitions(seed, 0, 64, 7, 24, 24, 1, 3, first)
        assert not valid.any() and np.array_equal(succ, anchor)
        assert (table == anchor[:, None]).all()                       # the walk stays on a first frame


def test_rejection_cap_is_not_reached_with_one_first_frame_in_three():
    """At most one first frame in three: all 16 candidates fail with probability <= 3^-16 per image."""
    cap = size = 2997                                                 # a multiple of 9
    first = (np.arange(cap) % 3 == 0).astype(np.uint8)
    for seed in SEEDS:
        for S in (1, 3):
            f = first if S == 1 else (np.arange(cap) % 9 < 3).astype(np.uint8)
            assert f.mean() <= 1 / 3 + 1e-9
            _, succ, _, valid = ops.philox_transitions(seed, 0, 4096, 0, size, cap, S, 3, f)
            assert valid.all() and (f[succ] == 0).all()


def test_argument_checks():
    first = np.zeros(24, np.uint8)
    ok = dict(head=5, size=24, capacity=24, stride=1, stack=3, first=first)
    ops.philox_transitions(0, 0, 4, **ok)
    for bad in (dict(stack=0), dict(stack=17), dict(stride=0), dict(stride=24), dict(size=1), dict(size=25),
                dict(head=24), dict(head=-1), dict(first=first[:5]), dict(size=2, stride=2)):
        with pytest.raises(ValueError):
            ops.philox_transitions(0, 0, 4, **{**ok, **bad})


# ---- windows ------------------------------------------------------------------------------------------------------

def test_window_streams():
    H, W = 20, 96
    crop = Crop((8, 32), mirror=0.5, pad=4, seed=5)
    for seed in SEEDS:
        w = ops.transition_windows(crop, H, W, 64, seed=seed, counter=11)
        assert w.shape == (2, 64, 3) and w.dtype == np.int32
        assert np.array_equal(w[0], ops.philox_windows(seed, 11, 64, crop, H, W))
        assert np.array_equal(w[1], ops.philox_windows(seed, 11, 64, crop, H, W, block=5))
        assert not np.array_equal(w[0], w[1])
        ops._check_windows(w[1].astype(np.int64), crop, H, W)
        sh = ops.transition_windows(crop, H, W, 64, seed=seed, counter=11, shared_window=True)
        assert np.array_equal(sh[0], w[0]) and np.array_equal(sh[1], w[0])
    # block= defaults to the block replay_sample draws from
    assert np.array_equal(ops.philox_windows(3, 4, 8, crop, H, W), ops.philox_windows(3, 4, 8, crop, H, W, block=1))
    # the window blocks (1, 5) are none of the candidate blocks (0, 2, 3, 4), also with crop.seed == 0
    assert {0 if t < 4 else 1 + (t >> 2) for t in range(16)} == {0, 2, 3, 4}
    for mode in (Crop((8, 32), mode='center'), Crop((8, 32), origin=(3, 9))):
        w = ops.transition_windows(mode, H, W, 5)
        assert np.array_equal(w[0], ops.crop_windows(mode, H, W, 5)) and np.array_equal(w[0], w[1])


# ---- the CPU buffer -----------------------------------------------------------------------------------------------

CAP, FH, FW = 24, 8, 32


def _buffer(n=30, stride=2, seed=5, every=7):
    """n frames of a 2-environment loop in a ring of 24 (wrapped for n > 24); an episode starts every 7 steps."""
    rng = np.random.default_rng(1)
    frames = rng.integers(0, 256, size=(n, FH, FW, 4), dtype=np.uint8)
    step = np.arange(n) // stride
    meta = dict(first=(step % every == 0).astype(np.uint8), action=rng.normal(size=(n, 3)).astype(np.float32),
                reward=np.arange(n, dtype=np.float32), tag=rng.integers(0, 256, size=(n, 5), dtype=np.uint8))
    rb = DeviceReplayBuffer(CAP, device='cpu', seed=seed)
    for s in range(0, n, stride):                                     # one extend per environment step
        rb.extend(frames[s:s + stride], **{k: v[s:s + stride] for k, v in meta.items()})
    return rb


CFGS = [DecodeConfig.unit(channels='rgb', gamma=2.2),
        DecodeConfig.unit(channels='rgba', dtype='bfloat16', crop=Crop((6, 16), mirror=0.5, seed=2)),
        DecodeConfig(channels='rgb', dtype='uint8', crop=Crop((FH, FW), pad=4))]


@pytest.mark.parametrize('cfg', CFGS, ids=['plain', 'crop-mirror', 'shift'])
@pytest.mark.parametrize('given', (False, True), ids=['drawn', 'given'])
def test_cpu_buffer_stacks_the_tables_frames(cfg, given):
    rb = _buffer()
    assert rb._next == 6 and len(rb) == CAP
    B, k, S = 7, 3, 2
    first = rb.meta['first'].numpy()
    c0 = rb._ctr
    if given:
        idx = torch.tensor([7, 8, 3, 4, 5, 23, 0])
        batch = rb.gather_transitions(idx, cfg, stack=k, stride=S, next_keys=('reward', 'first'))
        anchor, succ, table, valid = ops.given_transitions(idx.numpy(), rb._next, CAP, CAP, S, k, first)
        assert not valid.all() and valid.any()                        # slots 4, 5 are the newest step
        assert rb._ctr == c0 + (B if cfg.crop is not None else 0)
    else:
        batch = rb.sample_transitions(B, cfg, stack=k, stride=S, next_keys=('reward', 'first'))
        anchor, succ, table, valid = ops.philox_transitions(rb.seed, c0, B, rb._next, CAP, CAP, S, k, first)
        assert rb._ctr == c0 + B
    want_keys = {'obs', 'next_obs', 'first', 'action', 'reward', 'tag', 'next_reward', 'next_first', 'index',
                 'next_index', 'valid'} | ({'crop', 'next_crop'} if cfg.crop is not None else set())
    assert set(batch) == want_keys
    assert np.array_equal(batch['index'].numpy(), anchor) and np.array_equal(batch['next_index'].numpy(), succ)
    assert batch['valid'].dtype == torch.bool and np.array_equal(batch['valid'].numpy(), valid)
    h, w = (FH, FW) if cfg.crop is None else cfg.crop.size
    assert batch['obs'].shape == batch['next_obs'].shape == (B, k * cfg.cout, h, w)
    assert batch['obs'].dtype == cfg.torch_dtype()
    if cfg.crop is not None:
        wins = ops.transition_windows(cfg.crop, FH, FW, B, seed=rb.seed, counter=c0)
        assert np.array_equal(batch['crop'].numpy(), wins[0]) and np.array_equal(batch['next_crop'].numpy(), wins[1])
        assert not np.array_equal(wins[0], wins[1])
    for d, key in enumerate(('obs', 'next_obs')):
        for f in range(k):
            slots = torch.from_numpy(table[:, f + d])
            kw = {} if cfg.crop is None else dict(windows=batch['crop' if d == 0 else 'next_crop'])
            ref = rb.gather(slots, cfg, **kw)['image']
            got = batch[key][:, f * cfg.cout:(f + 1) * cfg.cout]
            assert torch.equal(got.contiguous().view(torch.uint8), ref.contiguous().view(torch.uint8)), (key, f)
    ia, isucc = torch.from_numpy(anchor), torch.from_numpy(succ)
    for key in ('first', 'action', 'reward', 'tag'):
        assert torch.equal(batch[key], rb.meta[key][ia]), key
    assert torch.equal(batch['next_reward'], rb.meta['reward'][isucc])
    assert torch.equal(batch['next_first'], rb.meta['first'][isucc])
    assert not batch['next_first'][batch['valid']].any()


def test_cpu_buffer_shared_window_and_sequence():
    cfg = CFGS[1]
    a, b = _buffer(), _buffer()
    x = a.sample_transitions(5, cfg, stack=2, stride=2, shared_window=True)
    assert torch.equal(x['crop'], x['next_crop'])
    y = b.sample_transitions(5, cfg, stack=2, stride=2)
    assert torch.equal(x['crop'], y['crop']) and not torch.equal(y['crop'], y['next_crop'])
    assert torch.equal(x['index'], y['index']) and torch.equal(x['obs'], y['obs'])
    # the same seed and call sequence give the same batches; the next call draws others
    x2, y2 = a.sample_transitions(5, cfg, stack=2, stride=2), b.sample_transitions(5, cfg, stack=2, stride=2)
    assert torch.equal(x2['index'], y2['index']) and torch.equal(x2['next_obs'], y2['next_obs'])
    assert not torch.equal(x2['index'], x['index'])
    # the graphed sampler of a CPU buffer is the eager call
    s = a.graphed_transition_sampler(5, cfg, stack=2, stride=2)
    assert torch.equal(s()['index'], b.sample_transitions(5, cfg, stack=2, stride=2)['index'])
    # next_obs of a valid transition one step on: its newest frame is the successor
    plain = CFGS[0]
    z = a.sample_transitions(6, plain, stack=3, stride=2)
    nxt = a.gather(z['next_index'], plain)['image']
    assert torch.equal(z['next_obs'][:, 6:9], nxt) and torch.equal(z['next_obs'][:, 3:6], z['obs'][:, 6:9])


def test_cpu_buffer_rejections():
    rb = _buffer()
    ok = dict(stack=3, stride=2)
    for bad in (dataclasses.replace(CFGS[0], layout='nhwc'),
                DecodeConfig.unit(channels='rgb', resize=ops.ResizedCrop((4, 8))),
                DecodeConfig.unit(channels='rgb', color_matrix=np.eye(4, dtype=np.float32).tolist())):
        with pytest.raises(ValueError):
            rb.sample_transitions(4, bad, **ok)
        with pytest.raises(ValueError):
            rb.gather_transitions(torch.tensor([1, 2]), bad, **ok)
    with pytest.raises(ValueError, match='nofirst'):
        rb.sample_transitions(4, CFGS[0], first_key='nofirst', **ok)
    with pytest.raises(ValueError, match='action'):
        rb.sample_transitions(4, CFGS[0], first_key='action', **ok)   # not a one-byte flag column
    with pytest.raises(ValueError, match='next_keys'):
        rb.sample_transitions(4, CFGS[0], next_keys=('nope',), **ok)
    for bad in (dict(stack=0), dict(stack=17), dict(stride=0), dict(stride=CAP)):
        with pytest.raises(ValueError):
            rb.sample_transitions(4, CFGS[0], **{**ok, **bad})
    with pytest.raises(ValueError, match='batch'):
        rb.sample_transitions(1000, CFGS[0], stack=16, stride=2)      # 1000 * 17 > 8192
    small = DeviceReplayBuffer(CAP, device='cpu', seed=1)
    with pytest.raises(IndexError):
        small.sample_transitions(2, CFGS[0])
    small.extend(np.zeros((2, FH, FW, 4), np.uint8), first=np.ones(2, np.uint8))
    with pytest.raises(ValueError, match='stride'):
        small.sample_transitions(2, CFGS[0], stack=2, stride=2)       # size <= stride
    assert rb._ctr == 0 and small._ctr == 0                           # a rejected call draws nothing
