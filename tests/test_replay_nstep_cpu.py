"""n-step transitions without a GPU: the numpy reference (``ops.nstep_transitions``, the ``nstep=`` tables of
``ops.given_transitions`` / ``ops.philox_transitions``) and the CPU ``DeviceReplayBuffer`` against a brute-force
simulation that knows only the episodes (tests/nstep_cases.py: per-environment Python lists, one transition at
a time, its own float32 accumulation)."""
import numpy as np
import pytest
import torch

from nstep_cases import SEED, classes, cpu_buffer, simulate
from blendtorch import ops
from blendtorch.ops import Crop, DecodeConfig

GAMMA = 0.99
# name -> (frames, capacity): a ring that wrapped, and one that is partly filled
RINGS = {'wrapped': (60, 48), 'partial': (22, 32)}
NSTEPS = (1, 3, 5)


def _buffer(ring, S):
    n, cap = RINGS[ring]
    return cpu_buffer(n, cap, 4, 16, 3, S, seed=7 + S)


def _ring(rb):
    return rb._next, len(rb), rb.capacity


def _columns(rb, use_done):
    m = rb.meta
    return m['reward'].numpy(), m['first'].numpy(), m['done'].numpy() if use_done else None


@pytest.mark.parametrize('use_done', (True, False), ids=['done', 'nodone'])
@pytest.mark.parametrize('n', NSTEPS)
@pytest.mark.parametrize('S', (1, 2))
@pytest.mark.parametrize('ring', list(RINGS))
def test_reference_equals_simulation(ring, S, n, use_done):
    """Every slot of the ring as an anchor (stored or not): steps, return and discount bit for bit, the successor,
    and for k = 1 and 3 the next stack's frames."""
    rb, episodes = _buffer(ring, S)
    head, size, cap = _ring(rb)
    reward, first, done = _columns(rb, use_done)
    anchor = np.arange(cap)
    a, succ1, table1, valid = ops.given_transitions(anchor, head, size, cap, S, 3, first)
    succ, steps, ret, disc = ops.nstep_transitions(anchor, valid, head, size, cap, S, n, GAMMA, reward, first, done)
    assert steps.dtype == np.int32 and ret.dtype == np.float32 and disc.dtype == np.float32
    sims = [simulate(s, episodes, rb.total, cap, S, n, GAMMA, 3, use_done) for s in anchor]
    for s, sim in zip(anchor, sims):
        where = f'{ring} S {S} n {n} slot {s}: {sim}'
        assert bool(valid[s]) == sim['valid'] and steps[s] == sim['steps'], where
        assert ret[s].tobytes() == sim['ret'].tobytes() and disc[s].tobytes() == sim['discount'].tobytes(), where
        assert succ[s] == (sim['succ_frame'] % cap if sim['valid'] else s), where
    if n == 1:                                                        # one step: the 1-step successor, reward, gamma
        assert np.array_equal(succ, succ1)
        assert np.array_equal(ret[valid], reward[anchor[valid]])
    for k in (1, 3):                                                  # n < k and n > k both occur over NSTEPS
        _, s1, t1, v1 = ops.given_transitions(anchor, head, size, cap, S, k, first)
        a2, s2, (obs_t, next_t), v2 = ops.given_transitions(anchor, head, size, cap, S, k, first, nstep=n, done=done)
        assert np.array_equal(a2, anchor) and np.array_equal(v2, v1) and np.array_equal(s2, succ)
        assert obs_t.shape == next_t.shape == (cap, k) and np.array_equal(obs_t, t1[:, :k])
        for s in anchor:
            if v1[s]:
                sim = simulate(s, episodes, rb.total, cap, S, n, GAMMA, k, use_done)
                assert next_t[s].tolist() == [f % cap for f in sim['next_frames']], (ring, S, n, k, s)
            else:                                                     # today's layout: e[1 .. k], e[k] the anchor
                assert next_t[s].tolist() == t1[s, 1:].tolist() and t1[s, k] == s
    # anchors drawn on the device's rule see the same walk
    a3, s3, (o3, n3), v3 = ops.philox_transitions(SEED, 5, 64, head, size, cap, S, 3, first, nstep=n, done=done)
    a4, s4, t4, v4 = ops.philox_transitions(SEED, 5, 64, head, size, cap, S, 3, first)
    assert np.array_equal(a3, a4) and np.array_equal(v3, v4) and np.array_equal(o3, t4[:, :3])
    assert np.array_equal(s3, succ[a3]) and np.array_equal(n3[v3], next_table_of(a3[v3], episodes, rb, S, n, use_done))


def next_table_of(anchors, episodes, rb, S, n, use_done, k=3):
    return np.array([[f % rb.capacity for f in simulate(s, episodes, rb.total, rb.capacity, S, n, GAMMA, k,
                                                        use_done)['next_frames']] for s in anchors]).reshape(-1, k)


@pytest.mark.parametrize('S', (1, 2))
def test_inputs_cover_every_class(S):
    """From the reference alone: the stores of these tests hold an image of every class, so a comparison with
    the device cannot pass on full-length walks only."""
    for n in (3, 5):
        for use_done in (True, False):
            got = set()
            for ring in RINGS:
                rb, _ = _buffer(ring, S)
                head, size, cap = _ring(rb)
                reward, first, done = _columns(rb, use_done)
                anchor = np.arange(cap)
                valid = ops.given_transitions(anchor, head, size, cap, S, 1, first)[3]
                _, steps, _, disc = ops.nstep_transitions(anchor, valid, head, size, cap, S, n, GAMMA, reward, first, done)
                got |= classes(steps, valid, disc, anchor, head, size, cap, S, n, first, use_done)
            want = {'full', 'first', 'newest', 'invalid'} | ({'terminated'} if use_done else set())
            assert got == want, (S, n, use_done, got)


CFGS = [DecodeConfig.unit(channels='rgb', gamma=2.2), DecodeConfig(channels='rgb', dtype='uint8', crop=Crop((4, 16), pad=2))]


@pytest.mark.parametrize('use_done', (True, False), ids=['done', 'nodone'])
@pytest.mark.parametrize('k', (1, 3))
@pytest.mark.parametrize('S', (1, 2))
@pytest.mark.parametrize('ring', list(RINGS))
def test_cpu_buffer_equals_simulation(ring, S, k, use_done):
    rb, episodes = _buffer(ring, S)
    cap = rb.capacity
    base_keys = None
    for cfg in CFGS:
        kw = dict(stack=k, stride=S, next_keys=('action', 'tag'))
        rb._ctr = 40
        base = rb.sample_transitions(16, cfg, **kw)
        assert 'nstep_return' not in base and 'nstep_steps' not in base and 'nstep_discount' not in base
        base_keys = set(base)
        assert base_keys == {'obs', 'next_obs', 'reward', 'done', 'first', 'action', 'tag', 'next_action', 'next_tag',
                             'index', 'next_index', 'valid'} | ({'crop', 'next_crop'} if cfg.crop else set())
        for n in NSTEPS:
            rb._ctr = 40
            nkw = dict(nstep=n, gamma=GAMMA, done_key='done' if use_done else None)
            got = rb.sample_transitions(16, cfg, **kw, **nkw)
            assert rb._ctr == 56
            assert set(got) == base_keys | {'nstep_return', 'nstep_discount', 'nstep_steps'}
            # the draw does not depend on n; neither do the anchor's outputs
            for key in ('index', 'valid', 'obs', 'reward', 'action', 'tag') + (('crop', 'next_crop') if cfg.crop else ()):
                assert torch.equal(got[key], base[key]), (key, n)
            _check(rb, episodes, got, cfg, S, k, n, use_done)
            if n == 1:                                                # one step: today's batch plus the three outputs
                for key in base_keys:
                    assert torch.equal(got[key], base[key]), key
            idx = torch.arange(cap)
            _check(rb, episodes, rb.gather_transitions(idx, cfg, **kw, **nkw), cfg, S, k, n, use_done)


def _check(rb, episodes, got, cfg, S, k, n, use_done):
    cap = rb.capacity
    assert got['nstep_return'].dtype == torch.float32 and got['nstep_discount'].dtype == torch.float32
    assert got['nstep_steps'].dtype == torch.int32
    plain = cfg if cfg.crop is None else None
    for b, s in enumerate(got['index'].tolist()):
        sim = simulate(s, episodes, rb.total, cap, S, n, GAMMA, k, use_done)
        where = f'image {b} slot {s}: {sim}'
        assert bool(got['valid'][b]) == sim['valid'] and int(got['nstep_steps'][b]) == sim['steps'], where
        assert got['nstep_return'][b].numpy().tobytes() == sim['ret'].tobytes(), where
        assert got['nstep_discount'][b].numpy().tobytes() == sim['discount'].tobytes(), where
        c_m = sim['succ_frame'] % cap if sim['valid'] else s
        assert int(got['next_index'][b]) == c_m, where
        assert torch.equal(got['next_action'][b], rb.meta['action'][c_m]) and torch.equal(got['next_tag'][b], rb.meta['tag'][c_m])
        if sim['valid'] and plain is not None:                        # whole frames: the stack is the decoded frames
            slots = torch.tensor([f % cap for f in sim['next_frames']])
            want = ops.reference_decode(rb.store.index_select(0, slots), plain).reshape(got['next_obs'][b].shape)
            assert torch.equal(got['next_obs'][b], want), where
        elif sim['valid']:                                            # a shift: the anchor's frame closes obs, c_m's next_obs
            win = got['next_crop'][b:b + 1].numpy()
            want = ops.reference_decode(rb.store[c_m:c_m + 1], cfg, crop=win)[0]
            assert torch.equal(got['next_obs'][b, -3:], want), where


def test_arguments_are_checked():
    rb, _ = _buffer('partial', 2)
    head, size, cap = _ring(rb)
    reward, first, done = _columns(rb, True)
    anchor, valid = np.arange(4), np.ones(4, bool)
    args = (anchor, valid, head, size, cap, 2)
    for bad in (dict(nstep=0), dict(nstep=17), dict(gamma=1.5), dict(gamma=-0.1), dict(gamma=float('nan')),
                dict(reward=reward.astype(np.float64)), dict(reward=reward[:-1]), dict(done=done.astype(np.int32)),
                dict(done=done[:-1])):
        a = dict(nstep=3, gamma=GAMMA, reward=reward, first=first, done=done)
        a.update(bad)
        with pytest.raises(ValueError):
            ops.nstep_transitions(*args, **a)
    cfg = CFGS[0]
    kw = dict(stack=3, stride=2)
    for bad in (dict(nstep=0), dict(nstep=17), dict(nstep=3, gamma=1.5), dict(nstep=3, reward_key='action'),
                dict(nstep=3, reward_key='missing'), dict(nstep=3, done_key='reward'), dict(nstep=3, done_key='missing')):
        with pytest.raises(ValueError):
            rb.sample_transitions(4, cfg, **kw, **bad)
    with pytest.raises(ValueError):                                   # 1024 * (3 + 6) > 8192
        rb.sample_transitions(1024, cfg, nstep=6, **kw)
    assert rb._ctr == 0                                               # nothing was drawn by a refused call
