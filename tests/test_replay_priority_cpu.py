"""Prioritized replay without a GPU: the numpy references of the priority kernels
(csrc/gpu/priority.hip) against brute force, and ``DeviceReplayBuffer(priority_alpha=...)``
on the CPU.  tests/test_gpu_replay_priority.py holds the kernels to these references."""
import numpy as np
import pytest
import torch

from nstep_cases import SEED, layout
from priority_cases import CAPACITIES, TOP, Eligible, buffer, mass_patterns, rebuilt, same_tree, search_draw
from blendtorch import ops
from blendtorch.btt.replay import DeviceReplayBuffer
from blendtorch.ops import Crop, DecodeConfig

CTR = (5 << 32) | 1234


def test_tree_levels():
    """50 slots: one level; 200: two, the leaves padded; 5000: three, padded at two levels; 2^31: six."""
    assert ops.priority_level_counts(50) == [64]
    assert ops.priority_level_counts(200) == [256, 4]
    assert ops.priority_level_counts(5000) == [5056, 128, 2]
    assert ops.priority_level_counts(64 * 64 * 64) == [262144, 4096, 64]
    assert len(ops.priority_level_counts(2 ** 31)) == 6 and ops.priority_level_counts(2 ** 31)[-1] == 2
    with pytest.raises(ValueError):
        ops.priority_level_counts(2 ** 31 + 1)
    levels = ops.priority_tree(np.arange(5000, dtype=np.uint32))
    assert [lev.dtype for lev in levels] == [np.uint32, np.uint64, np.uint64]
    assert int(levels[1][1]) == sum(range(64, 128)) and int(levels[1][79:].sum()) == 0
    assert int(levels[2].sum()) == sum(range(5000))


@pytest.mark.parametrize('cap', CAPACITIES)
def test_reference_draw_equals_cumsum_search(cap):
    """Every mass pattern (spread with holes, a single mass, T < B, 2^32 - 1 among ones, every mass 2^32 - 1,
    T == 0) at B = 1, 8, 256: the descent finds the slot np.searchsorted finds on the exact cumulative sum."""
    for name, masses in mass_patterns(cap, seed=cap).items():
        levels = ops.priority_tree(masses)
        for B in (1, 8, 256):
            want = search_draw(masses, SEED, CTR + B, B)
            got = ops.reference_priority_draw(levels, SEED, CTR + B, B)
            for g, w, key in zip(got, want, ('index', 'mass', 'prob')):
                assert g.dtype == w.dtype and np.array_equal(g, w), (name, cap, B, key, g[:8], w[:8])
            if name == 'empty':
                assert not got[0].any() and not got[1].any() and not got[2].any()
            else:
                assert (got[1] > 0).all() and (got[0] < cap).all(), (name, cap, B)
            if name == 'single':
                assert (got[0] == cap * 2 // 3).all()
            if name == 'few' and B > 3:
                assert set(got[0].tolist()) == {1, cap // 2, cap - 1}


def test_reference_draw_is_stratified():
    """Image b draws inside the b-th B-th of the total mass: with equal masses, inside its own run of slots."""
    levels = ops.priority_tree(np.full(256, 7, np.uint32))
    idx = ops.reference_priority_draw(levels, SEED, 3, 8)[0]
    assert (idx // 32 == np.arange(8)).all(), idx


def test_proportionality():
    """4096 draws of B = 64 over 200 slots whose masses span three decades: every slot's count lies within 5
    standard deviations (binomial: stratification only lowers the variance) of draws * B * mass / T."""
    rng = np.random.default_rng(7)
    masses = np.rint(65536 * 10.0 ** rng.uniform(-1.5, 1.5, 200)).astype(np.uint32)
    assert masses.max() / masses.min() > 500
    levels = ops.priority_tree(masses)
    draws, B = 4096, 64
    count = np.zeros(200, np.int64)
    for i in range(draws):
        count += np.bincount(ops.reference_priority_draw(levels, SEED, i * B, B)[0], minlength=200)
    p = masses.astype(np.float64) / masses.astype(np.float64).sum()
    n = draws * B
    dev = np.abs(count - n * p) / np.sqrt(n * p * (1 - p))
    assert dev.max() < 5, (dev.max(), int(dev.argmax()))


def test_reference_mass():
    p = np.array([1.0, 0.5, 0.0, -3.0, np.nan, np.inf, 1e-9, 70000.0, 65535.99, 2.5 / 65536], np.float32)
    m = ops.reference_priority_mass(p, 1.0)
    assert m.dtype == np.uint32
    assert m.tolist() == [65536, 32768, 1, 1, 1, TOP, 1, TOP, 2 ** 32 - 768, 2]   # float32(65535.99) = 65536 - 3 / 256; 2.5 rounds to even
    m6 = ops.reference_priority_mass(p, 0.6)
    assert m6[0] == 65536 and m6[2] == 1 and m6[4] == 1 and m6[5] == TOP
    assert m6[1] == int(np.rint(0.5 ** 0.6 * 65536))


@pytest.mark.parametrize('cap', CAPACITIES)
def test_updates_keep_the_tree_exact(cap):
    """Duplicates in a batch (the last entry wins), a priority for an ineligible slot (stays 0), an index outside
    the store (ignored), max_mass growing: the incrementally updated tree is the tree rebuilt from its leaves."""
    masses = mass_patterns(cap, seed=3)['spread']
    levels = ops.priority_tree(masses)
    live, dead = np.flatnonzero(masses != 0), np.flatnonzero(masses == 0)
    index = np.array([live[0], live[1], live[0], dead[0], live[-1], live[0], cap, -1, live[1]], np.int64)
    prio = np.array([3.0, 0.25, 7.0, 9.0, 0.0, 2.0, 5.0, 5.0, 0.5], np.float32)
    mx = ops.reference_priority_update(levels, ops.PRIORITY_ONE, index, prio, 1.0)
    assert same_tree(levels, rebuilt(levels))
    assert levels[0][live[0]] == 2 * 65536 and levels[0][live[1]] == 32768     # the last entry of each duplicate
    assert levels[0][dead[0]] == 0 and levels[0][live[-1]] == 1
    assert mx == 2 * 65536                         # 3.0 and 7.0 lost to the later 2.0; 9.0 went to an ineligible slot
    untouched = np.setdiff1d(np.arange(cap), index[(index >= 0) & (index < cap)])
    assert np.array_equal(levels[0][untouched], masses[untouched])
    mx = ops.reference_priority_update(levels, mx, live[:3], np.array([1e9, 0.1, 0.1], np.float32), 1.0)
    assert mx == TOP and levels[0][live[0]] == TOP and same_tree(levels, rebuilt(levels))
    assert ops.reference_priority_update(levels, mx, live[:1], np.array([0.1], np.float32), 1.0) == TOP   # never shrinks


@pytest.mark.parametrize('per_extend', (2, 6, 5, 1), ids=['n=stride', 'three-steps', 'odd-n', 'half-step'])
def test_reference_extend_equals_eligibility_scan(per_extend):
    """The episode layouts of tests/nstep_cases.py into a 24-slot ring, S = 2, `per_extend` frames per append (one
    step, three steps, 5 and 1: no multiples of the stride) until the ring has wrapped twice; a priority written
    late in the run raises max_mass.  After every append the leaves are what the frame-by-frame scan leaves, and the
    tree is the tree rebuilt from them."""
    cap, S, n = 24, 2, 60
    first_all = layout(n, S, seed=11)[0]['first']
    levels = ops.priority_tree(np.zeros(cap, np.uint32))
    scan, first, max_mass, head, size = Eligible(cap, S, first_all), np.zeros(cap, np.uint8), ops.PRIORITY_ONE, 0, 0
    wrote = False
    for s in range(0, n, per_extend):
        k = min(per_extend, n - s)
        for i in range(s, s + k):
            first[i % cap] = first_all[i]
        start, head, size = head, (head + k) % cap, min(cap, size + k)
        ops.reference_priority_extend(levels, max_mass, cap, start, k, head, size, S, first)
        scan.append(k)
        assert np.array_equal(levels[0][:cap], scan.leaves()), (s, levels[0][:cap], scan.leaves())
        assert same_tree(levels, rebuilt(levels)), s
        if s >= 44 and not wrote:        # late: frames that entered before it are still stored at the end
            slot = int(np.flatnonzero(levels[0])[0])
            max_mass = ops.reference_priority_update(levels, max_mass, [slot, (head - 1) % cap], [4.0, 8.0], 1.0)
            scan.write(slot, 4 * 65536)
            assert max_mass == 4 * 65536             # the newest frame is not drawable: its 8.0 is ignored
            wrote = True
    eligible = levels[0][:cap] != 0
    assert eligible.any() and not eligible.all() and len(set(levels[0][:cap].tolist())) == 3   # 0, 65536, 4 * 65536
    # the ring state agrees with the transition sampler's own notion of a valid anchor
    valid = ops.given_transitions(np.arange(cap), head, size, cap, S, 1, first)[3]
    assert np.array_equal(valid, eligible)


# ---- DeviceReplayBuffer on the CPU -------------------------------------------------------------------------------

SHIFT = Crop((8, 16), pad=4)


def _cfg(crop):
    return DecodeConfig.densityopt(channels='bgr', gamma=2.2, dtype='float32', crop=crop)


def test_buffer_keeps_masses_through_extend():
    rb, _ = buffer(30, 24, 2, seed=11)
    mass = rb.priority_mass
    assert mass.dtype == torch.uint32 and tuple(mass.shape) == (24,)
    first = rb.meta['first'].numpy()
    valid = ops.given_transitions(np.arange(24), rb._next, len(rb), 24, 2, 1, first)[3]
    assert np.array_equal(mass.numpy() != 0, valid) and set(mass.numpy().tolist()) == {0, 65536}
    assert same_tree([lev.numpy() for lev in rb._levels], rebuilt([lev.numpy() for lev in rb._levels]))
    rb3, _ = buffer(30, 24, 2, seed=11, steps=3)          # three env steps per extend: the same store, the same masses
    assert np.array_equal(rb3.priority_mass.numpy(), mass.numpy())


@pytest.mark.parametrize('crop', (SHIFT, None), ids=['shift', 'nocrop'])
def test_prioritized_sample_on_the_cpu(crop):
    """The anchors are the reference draw's, the rest is gather_transitions at the same counter; the counter
    moves on by B per sample, with and without drawn windows; update_priorities steers the next draw."""
    rb, _ = buffer(30, 24, 2, seed=11)
    twin, _ = buffer(30, 24, 2, seed=11)
    kw = dict(stack=3, stride=2, next_keys=('action',), nstep=3, gamma=0.99, done_key='done')
    c0 = rb._ctr
    batch = rb.sample_transitions(16, _cfg(crop), prioritized=True, beta=0.5, **kw)
    assert rb._ctr == c0 + 16
    levels = [lev.numpy() for lev in twin._levels]
    idx, mass, prob = ops.reference_priority_draw(levels, SEED, c0, 16)
    want = twin.gather_transitions(torch.from_numpy(idx), _cfg(crop), _counter=c0, **kw)
    assert set(batch) == set(want) | {'prob', 'weight'}
    for k, v in want.items():
        assert torch.equal(batch[k], v), k
    assert bool(batch['valid'].all())
    assert np.array_equal(batch['prob'].numpy(), prob) and batch['prob'].dtype == torch.float32
    assert np.array_equal(batch['weight'].numpy(), np.ones(16, np.float32))       # equal masses: equal weights
    # one anchor takes ten times the mass of any other: several strata land on it, and it has the smallest weight
    hot = int(batch['index'][5])
    rb.update_priorities(batch['index'], torch.where(batch['index'] == hot, 10.0, 1.0))
    assert int(rb.priority_mass[hot]) == 10 * 65536 and int(rb._max_mass[0]) == 10 * 65536
    b2 = rb.sample_transitions(16, _cfg(crop), prioritized=True, beta=0.5, **kw)
    assert rb._ctr == c0 + 32
    on_hot = (b2['index'] == hot).numpy()
    assert 4 <= int(on_hot.sum()) < 16
    w = b2['weight'].numpy()
    assert np.array_equal(w[on_hot], np.full(int(on_hot.sum()), 0.1 ** 0.5).astype(np.float32))
    assert np.array_equal(w[~on_hot], np.ones(int((~on_hot).sum()), np.float32))
    # a frame appended now enters with the largest mass so far
    f, meta = buffer(32, 24, 2, seed=11)[1]
    rb.extend(torch.from_numpy(f[30:32]), **{k: v[30:32] for k, v in meta.items()})
    assert 10 * 65536 in rb.priority_mass[[(rb._next - 3) % 24, (rb._next - 4) % 24]].tolist()


def test_buffer_without_priorities_is_unchanged():
    plain, _ = buffer(30, 24, 2, seed=11, priority_alpha=None)
    prio, _ = buffer(30, 24, 2, seed=11)
    assert plain._levels is None and plain._max_mass is None
    kw = dict(stack=3, stride=2, nstep=3)
    with pytest.raises(ValueError, match='priority_alpha'):
        plain.sample_transitions(8, _cfg(SHIFT), prioritized=True, **kw)
    with pytest.raises(ValueError, match='priority_alpha'):
        plain.update_priorities(torch.zeros(1, dtype=torch.int64), torch.ones(1))
    with pytest.raises(ValueError, match='priority_alpha'):
        plain.priority_mass
    a, b = plain.sample_transitions(8, _cfg(SHIFT), **kw), prio.sample_transitions(8, _cfg(SHIFT), **kw)
    assert set(a) == set(b) and 'weight' not in a
    for k in a:
        assert torch.equal(a[k], b[k]), k
    with pytest.raises(ValueError, match='stride'):
        prio.sample_transitions(8, _cfg(SHIFT), prioritized=True, stack=3, stride=1)
    with pytest.raises(ValueError, match='first'):
        DeviceReplayBuffer(8, device='cpu', priority_alpha=0.6).extend(np.zeros((2, 8, 16, 3), np.uint8))


def test_no_eligible_transition():
    """T == 0 (every stored frame is a first frame): index 0, prob 0, weight 0, valid False."""
    rb = DeviceReplayBuffer(8, device='cpu', seed=SEED, priority_alpha=1.0)
    rb.extend(np.zeros((4, 8, 16, 3), np.uint8), first=np.ones(4, np.uint8))
    b = rb.sample_transitions(4, _cfg(None), prioritized=True)
    assert not b['valid'].any() and not b['index'].any() and not b['prob'].any() and not b['weight'].any()
