"""The priority kernels (csrc/gpu/priority.hip: ``priority_draw``, ``priority_update``,
``priority_extend``) and prioritized sampling through ``DeviceReplayBuffer``.

The launches go through the bindings on SENTINEL-guarded buffers -- the tree's levels and ``max_mass``
included, they are written by two of the kernels -- and are compared with the numpy references of
``blendtorch.ops``, which tests/test_replay_priority_cpu.py checks against brute force.  Every number in
the tree is an integer, so everything but the importance weights is compared bit for bit."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from decode_oracle import GUARD, SENTINEL
from nstep_cases import SEED, layout
from priority_cases import CAPACITIES, buffer, mass_patterns, rebuilt, same_tree
from blendtorch import ops
from blendtorch.ops import Crop, DecodeConfig

pytestmark = pytest.mark.gpu

CTR = (3 << 32) | 77
# weight = expf(beta * (logf(min) - logf(mass))) against (min / mass)^beta in float64, for beta <= 1 and masses
# < 2^32 (logarithms < 32, one ulp there is 2^-19).  Absolute error of the exponent: two logf of 3 ulp each (the
# OpenCL bound for log) plus 2^-24 each for the mass's conversion to float32, half an ulp for the difference,
# 32 * 2^-24 = 2^-19 for the product with beta: 7.5 * 2^-19 + 2^-23.  An absolute error of the exponent is a
# relative error of the result, to which expf adds its 3 ulp (the OpenCL bound for exp) = 3 * 2^-23.
WEIGHT_RTOL = 7.5 * 2.0 ** -19 + 4 * 2.0 ** -23


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    ops.hip_ext()  # must load: no silent fallback
    return torch.device('cuda', 0)


class Guarded:
    """nbytes of device memory between two guards of SENTINEL bytes."""

    def __init__(self, nbytes, dev, init=None):
        self.buf = torch.full((2 * GUARD + nbytes,), SENTINEL, dtype=torch.uint8, device=dev)
        self.nbytes = nbytes
        if init is not None:
            self.buf[GUARD:GUARD + nbytes] = torch.from_numpy(np.ascontiguousarray(init).view(np.uint8).reshape(-1)).to(dev)

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD

    def read(self, dtype):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == SENTINEL).all() and (b[GUARD + self.nbytes:] == SENTINEL).all(), 'guard overwritten'
        return b[GUARD:GUARD + self.nbytes].copy().view(dtype)


class DeviceTree:
    """A priority tree in guarded device buffers."""

    def __init__(self, levels, capacity, dev, max_mass=ops.PRIORITY_ONE):
        self.capacity = capacity
        self.levels = [Guarded(lev.nbytes, dev, lev) for lev in levels]
        self.dtypes = [lev.dtype for lev in levels]
        self.counts = [int(lev.shape[0]) for lev in levels]
        self.max = Guarded(4, dev, np.array([max_mass], np.uint32))

    def args(self):
        return dict(levels=[g.ptr for g in self.levels], counts=self.counts, capacity=self.capacity, max_mass=self.max.ptr)

    def read(self):
        return [g.read(dt) for g, dt in zip(self.levels, self.dtypes)], int(self.max.read(np.uint32)[0])


def _draw(dev, tree, B, beta, counter=None, ctr_value=0, advance=0, over=None):
    """One priority_draw launch on guarded outputs: (index, mass, prob, weight) as numpy."""
    ext = ops.hip_ext()
    out = dict(index=Guarded(8 * B, dev), mass=Guarded(4 * B, dev), prob=Guarded(4 * B, dev), weight=Guarded(4 * B, dev))
    beta_t = torch.tensor([beta], dtype=torch.float32, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    a = dict(tree.args(), B=B, seed=SEED, counter=0 if counter is None else counter.data_ptr(), ctr_value=ctr_value,
             advance=advance, beta=beta_t.data_ptr(), ticket=ticket.data_ptr(), index_out=out['index'].ptr,
             mass_out=out['mass'].ptr, prob_out=out['prob'].ptr, weight_out=out['weight'].ptr, stream=ops._stream(dev))
    a.update(over or {})
    try:
        if over:
            with pytest.raises(RuntimeError, match='invalid'):
                ext.priority_draw(**a)
        else:
            ext.priority_draw(**a)
    finally:
        torch.cuda.synchronize()
    assert int(ticket[0]) == 0                          # the last wave leaves the ticket as it found it
    got = [out[k].read(dt) for k, dt in (('index', np.int64), ('mass', np.uint32), ('prob', np.float32),
                                         ('weight', np.float32))]
    if over:                                            # refused before anything ran: nothing was written
        assert all((g.view(np.uint8) == SENTINEL).all() for g in got)
    return got


@pytest.mark.parametrize('B', (1, 8, 256, 1024))
@pytest.mark.parametrize('cap', CAPACITIES)
def test_draw_equals_reference(dev, cap, B):
    """index, mass and prob bit for bit, for every mass pattern, with the counter given by value and read from
    the device (which the launch advances by B only when asked to).  The weights lie within WEIGHT_RTOL (see
    above: 1.5e-5, from the 3-ulp bounds of logf and expf) of the float64 reference, and are exactly 1 for the
    smallest mass of the batch."""
    for name, masses in mass_patterns(cap, seed=cap).items():
        levels = ops.priority_tree(masses)
        tree = DeviceTree(levels, cap, dev)
        want = ops.reference_priority_draw(levels, SEED, CTR, B)
        counter = torch.tensor([CTR], dtype=torch.int64, device=dev)
        for how, beta in (('value', 0.4), ('device', 1.0), ('advance', 0.4)):
            where = (name, cap, B, how)
            if how == 'value':
                got = _draw(dev, tree, B, beta, ctr_value=CTR)
            else:
                got = _draw(dev, tree, B, beta, counter=counter, ctr_value=12345, advance=int(how == 'advance'))
                assert int(counter[0]) == (CTR + B if how == 'advance' else CTR), where
            for g, w, key in zip(got, want, ('index', 'mass', 'prob')):
                assert np.array_equal(g, w), (where, key, g[:8], w[:8])
            wref = ops.reference_priority_weights(want[1], np.float32(beta))
            print(where, 'weight rel err', float(np.max(np.abs(got[3] - wref) / np.maximum(wref, 1e-300), initial=0)))
            assert np.all(np.abs(got[3] - wref) <= WEIGHT_RTOL * wref), (where, got[3][:8], wref[:8])
            if name != 'empty':
                assert np.array_equal(got[3][want[1] == want[1].min()], np.ones(int((want[1] == want[1].min()).sum()), np.float32))
        assert same_tree(tree.read()[0], levels) and tree.read()[1] == ops.PRIORITY_ONE   # a draw writes nothing to the tree


def test_draw_rejected_arguments(dev):
    levels = ops.priority_tree(mass_patterns(200, seed=1)['spread'])
    tree = DeviceTree(levels, 200, dev)
    ok = tree.args()
    _draw(dev, tree, 8, 0.4, over=dict(B=1025))
    _draw(dev, tree, 8, 0.4, over=dict(levels=[0, ok['levels'][1]]))                      # a null tree
    _draw(dev, tree, 8, 0.4, over=dict(levels=[]))
    _draw(dev, tree, 8, 0.4, over=dict(capacity=2 ** 31 + 1))
    _draw(dev, tree, 8, 0.4, over=dict(levels=[ok['levels'][0], ok['levels'][1] + 4]))    # uint64 sums at 4 mod 8
    _draw(dev, tree, 8, 0.4, over=dict(levels=[ok['levels'][0] + 2, ok['levels'][1]]))
    _draw(dev, tree, 8, 0.4, over=dict(counts=[256, 5]))                                  # not this capacity's tree
    _draw(dev, tree, 8, 0.4, over=dict(max_mass=0))
    _draw(dev, tree, 8, 0.4, over=dict(weight_out=0))
    ext = ops.hip_ext()
    idx = torch.zeros(8, dtype=torch.int64, device=dev)
    pr = torch.ones(8, dtype=torch.float32, device=dev)
    first = torch.zeros(200, dtype=torch.uint8, device=dev)
    s = ops._stream(dev)
    for bad in (dict(B=1025), dict(levels=[0, ok['levels'][1]]), dict(capacity=2 ** 31 + 1), dict(alpha=-1.0),
                dict(alpha=float('nan')), dict(index=0), dict(levels=[ok['levels'][0], ok['levels'][1] + 4])):
        a = dict(ok, index=idx.data_ptr(), priority=pr.data_ptr(), B=8, alpha=1.0, stream=s)
        a.update(bad)
        with pytest.raises(RuntimeError, match='invalid'):
            ext.priority_update(**a)
    for bad in (dict(n=201), dict(n=-1), dict(start=200), dict(stride=0), dict(stride=200), dict(first=0), dict(head=200),
                dict(size=201), dict(levels=[0, ok['levels'][1]]), dict(capacity=2 ** 31 + 1)):
        a = dict(ok, start=0, n=4, head=4, size=4, stride=2, first=first.data_ptr(), stream=s)
        a.update(bad)
        with pytest.raises(RuntimeError, match='invalid'):
            ext.priority_extend(**a)
    torch.cuda.synchronize()
    assert same_tree(tree.read()[0], levels)


def _update_case(cap, B, seed):
    """B (index, priority) pairs over a spread tree: duplicates, ineligible slots, indices outside the store,
    NaN / negative / infinite / huge / tiny priorities."""
    rng = np.random.default_rng(seed)
    masses = mass_patterns(cap, seed=3)['spread']
    index = rng.integers(0, cap, B).astype(np.int64)
    index[rng.random(B) < 0.3] = index[0]                        # one slot many times over
    if B >= 8:
        index[3], index[5] = cap, -1
        index[6] = int(np.flatnonzero(masses == 0)[0])
    prio = (10.0 ** rng.uniform(-3, 3, B)).astype(np.float32)
    prio[::7] = np.array([np.nan, -1.0, np.inf, 1e30, 0.0, 1e-30, 65535.99], np.float32)[np.arange(len(prio[::7])) % 7]
    return masses, index, prio


@pytest.mark.parametrize('B', (1, 9, 300, 1024))
@pytest.mark.parametrize('cap', CAPACITIES)
def test_update_alpha_one_is_exact(dev, cap, B):
    """alpha = 1: the leaves, every level and max_mass equal the reference bit for bit; two updates in a row."""
    ext = ops.hip_ext()
    masses, index, prio = _update_case(cap, B, seed=B)
    levels = ops.priority_tree(masses)
    tree = DeviceTree(levels, cap, dev)
    mx = ops.PRIORITY_ONE
    for rnd in range(2):
        idx_t, pr_t = torch.from_numpy(index).to(dev), torch.from_numpy(prio).to(dev)
        ext.priority_update(**tree.args(), index=idx_t.data_ptr(), priority=pr_t.data_ptr(), B=B, alpha=1.0,
                            stream=ops._stream(dev))
        torch.cuda.synchronize()
        mx = ops.reference_priority_update(levels, mx, index, prio, 1.0)
        got, gmx = tree.read()
        assert same_tree(got, levels) and gmx == mx, (cap, B, rnd, gmx, mx)
        index, prio = index[::-1].copy(), np.roll(prio, 1)
    assert same_tree(levels, rebuilt(levels))


@pytest.mark.parametrize('cap', CAPACITIES)
def test_update_alpha_fractional(dev, cap):
    """alpha = 0.6: every leaf within max(1, ref * 16 * 2^-23) of the float64 reference (the 16 ulp OpenCL allows
    pow, plus the unit of the final rounding); the levels are the exact sums of the leaves read back."""
    ext = ops.hip_ext()
    B = 300
    masses, index, prio = _update_case(cap, B, seed=5)
    levels = ops.priority_tree(masses)
    tree = DeviceTree(levels, cap, dev)
    idx_t, pr_t = torch.from_numpy(index).to(dev), torch.from_numpy(prio).to(dev)
    ext.priority_update(**tree.args(), index=idx_t.data_ptr(), priority=pr_t.data_ptr(), B=B, alpha=0.6,
                        stream=ops._stream(dev))
    torch.cuda.synchronize()
    ops.reference_priority_update(levels, ops.PRIORITY_ONE, index, prio, 0.6)
    got, gmx = tree.read()
    ref, leaf = levels[0].astype(np.float64), got[0].astype(np.float64)
    err = np.abs(leaf - ref)
    print(cap, 'largest leaf error in units of the bound', float(np.max(err / np.maximum(1.0, ref * 16 * 2.0 ** -23))))
    assert np.all(err <= np.maximum(1.0, ref * 16 * 2.0 ** -23)), (cap, got[0][err > 1][:8], levels[0][err > 1][:8])
    assert np.array_equal(got[0] == 0, levels[0] == 0)
    assert same_tree(got, rebuilt(got))
    written = [int(i) for i in set(index.tolist()) if 0 <= i < cap and masses[i] != 0]
    assert gmx == max(ops.PRIORITY_ONE, int(got[0][written].max()))


def test_extend_equals_reference(dev):
    """A 24-slot ring, stride 2, appended to 2, 6, 5, 1, ... 24 frames at a time until it has wrapped twice,
    with a priority update on the way that raises max_mass: leaves, tree and max_mass after every append."""
    ext = ops.hip_ext()
    cap, S, n = 24, 2, 60
    first_all = layout(n, S, seed=11)[0]['first']
    levels = ops.priority_tree(np.zeros(cap, np.uint32))
    tree = DeviceTree(levels, cap, dev)
    first, mx, head, size, s = np.zeros(cap, np.uint8), ops.PRIORITY_ONE, 0, 0, 0
    first_t = torch.zeros(cap, dtype=torch.uint8, device=dev)
    sizes = [2, 2, 6, 5, 1, 2, 24, 2, 4, 2, 3, 3, 2, 2]      # the update below: late enough for older masses to stay
    assert sum(sizes) <= n
    for step, k in enumerate(sizes):
        for i in range(s, s + k):
            first[i % cap] = first_all[i]
        first_t.copy_(torch.from_numpy(first))
        start, head, size, s = head, (head + k) % cap, min(cap, size + k), s + k
        ext.priority_extend(**tree.args(), start=start, n=k, head=head, size=size, stride=S, first=first_t.data_ptr(),
                            stream=ops._stream(dev))
        torch.cuda.synchronize()
        ops.reference_priority_extend(levels, mx, cap, start, k, head, size, S, first)
        got, gmx = tree.read()
        assert same_tree(got, levels) and gmx == mx, (step, k, got[0], levels[0])
        if step == 8:
            index = np.array([int(np.flatnonzero(levels[0])[0]), (head - 1) % cap], np.int64)
            prio = np.array([4.0, 8.0], np.float32)
            idx_t, pr_t = torch.from_numpy(index).to(dev), torch.from_numpy(prio).to(dev)
            ext.priority_update(**tree.args(), index=idx_t.data_ptr(), priority=pr_t.data_ptr(), B=2, alpha=1.0,
                                stream=ops._stream(dev))
            mx = ops.reference_priority_update(levels, mx, index, prio, 1.0)
            assert mx == 4 * 65536
    assert len(set(levels[0][:cap].tolist())) == 3 and same_tree(levels, rebuilt(levels))


def test_extend_large_wrapped_range(dev):
    """5000 slots (three levels), 1300 frames appended across the wrap, stride 3: more than one block, every
    level touched, atomic adds from many lanes into the same parents."""
    ext = ops.hip_ext()
    cap, S = 5000, 3
    rng = np.random.default_rng(4)
    levels = ops.priority_tree(mass_patterns(cap, seed=9)['spread'])
    tree = DeviceTree(levels, cap, dev, max_mass=3 * 65536)
    first = (rng.random(cap) < 0.05).astype(np.uint8)
    first_t = torch.from_numpy(first).to(dev)
    start, k = 4400, 1300
    head = (start + k) % cap
    ext.priority_extend(**tree.args(), start=start, n=k, head=head, size=cap, stride=S, first=first_t.data_ptr(),
                        stream=ops._stream(dev))
    torch.cuda.synchronize()
    ops.reference_priority_extend(levels, 3 * 65536, cap, start, k, head, cap, S, first)
    got, gmx = tree.read()
    assert same_tree(got, levels) and gmx == 3 * 65536 and same_tree(levels, rebuilt(levels))


# ---- DeviceReplayBuffer ----------------------------------------------------------------------------------------

def _cfg(crop):
    return DecodeConfig.densityopt(channels='bgr', gamma=2.2, dtype='float32', crop=crop)


def _same(gpu_batch, cpu_batch, what):
    assert set(gpu_batch) == set(cpu_batch), what
    for k, v in cpu_batch.items():
        g = gpu_batch[k].cpu()
        if k == 'weight':
            w = v.double().numpy()
            assert np.all(np.abs(g.double().numpy() - w) <= (WEIGHT_RTOL + 2.0 ** -24) * w), (what, k)   # + the CPU's rounding
        else:
            assert g.dtype == v.dtype and torch.equal(g, v), (what, k, g.reshape(-1)[:8], v.reshape(-1)[:8])


def _priorities(index):
    return ((index % 7).float() + 0.5) * 0.37


@pytest.mark.parametrize('crop', (Crop((8, 16), pad=4), None), ids=['shift', 'nocrop'])
def test_buffer_equals_cpu_buffer(dev, crop):
    """A GPU and a CPU buffer with the same seed through sample, update_priorities, extend, sample: every key
    of both batches is equal (weights: WEIGHT_RTOL); then a graphed sampler on a fresh GPU buffer replayed
    around the same update and extend gives the same two batches.  Without a crop nothing but the anchors is
    drawn: the counter still advances by B per sample, in the eager buffer and in the graph."""
    B, kw = 16, dict(stack=3, stride=2, next_keys=('action',), nstep=3, gamma=0.99, done_key='done')
    cfg = _cfg(crop)
    cpu, (f, meta) = buffer(30, 24, 2, seed=11)
    gpu, _ = buffer(30, 24, 2, seed=11, device=dev)
    graphed, _ = buffer(30, 24, 2, seed=11, device=dev)
    sampler = graphed.graphed_transition_sampler(B, cfg, warmup=2, prioritized=True, beta=0.4, **kw)
    sampler.counter.fill_(cpu._ctr)                       # the warm-up launches drew, too
    assert sampler.beta.dtype == torch.float32 and float(sampler.beta) == np.float32(0.4)
    want = []
    for rnd in range(2):
        c0 = cpu._ctr
        want.append(cpu.sample_transitions(B, cfg, prioritized=True, beta=0.4, **kw))
        assert cpu._ctr == c0 + B and bool(want[-1]['valid'].all())
        got = gpu.sample_transitions(B, cfg, prioritized=True, beta=0.4, **kw)
        assert gpu._ctr == cpu._ctr
        _same(got, want[-1], ('eager', rnd))
        replayed = {k: v.clone() for k, v in sampler().items()}
        assert int(sampler.counter) == c0 + B
        _same(replayed, want[-1], ('graph', rnd))
        if rnd == 0:
            prio = _priorities(want[0]['index'])
            for rb in (cpu, gpu, graphed):
                rb.update_priorities(want[0]['index'], prio)
                rb.extend(torch.from_numpy(f[:4]), **{k: v[:4] for k, v in meta.items()})
            for rb in (gpu, graphed):
                assert torch.equal(rb.priority_mass.cpu(), cpu.priority_mass)
                assert all(torch.equal(a.cpu(), b) for a, b in zip(rb._levels, cpu._levels))
                assert int(rb._max_mass.cpu()[0]) == int(cpu._max_mass[0])
    assert not torch.equal(want[0]['index'], want[1]['index'])
    assert len(set(want[1]['weight'].tolist())) > 2       # the update spread the masses
    # beta is read on the device: the same graph, annealed
    sampler.beta.fill_(1.0)
    sampler.counter.fill_(cpu._ctr)
    _same({k: v.clone() for k, v in sampler().items()}, cpu.sample_transitions(B, cfg, prioritized=True, beta=1.0, **kw),
          'beta 1')


def test_buffer_without_priorities(dev):
    plain, _ = buffer(30, 24, 2, seed=11, device=dev, priority_alpha=None)
    prio, _ = buffer(30, 24, 2, seed=11, device=dev)
    cpu, _ = buffer(30, 24, 2, seed=11, priority_alpha=None)
    cfg, kw = _cfg(Crop((8, 16), pad=4)), dict(stack=3, stride=2, nstep=3)
    with pytest.raises(ValueError, match='priority_alpha'):
        plain.sample_transitions(8, cfg, prioritized=True, **kw)
    with pytest.raises(ValueError, match='priority_alpha'):
        plain.graphed_transition_sampler(8, cfg, prioritized=True, **kw)
    assert plain._levels is None
    want = cpu.sample_transitions(8, cfg, **kw)
    for rb in (plain, prio):                              # the uniform sample does not see the priorities
        got = rb.sample_transitions(8, cfg, **kw)
        assert set(got) == set(want)
        for k, v in want.items():
            assert torch.equal(got[k].cpu(), v), k


def test_large_update_batches_and_alpha(dev):
    """update_priorities splits more than 1024 entries into launches in order (a later entry still wins), with
    the buffer's alpha."""
    cpu, _ = buffer(30, 24, 2, seed=11, priority_alpha=0.6)
    gpu, _ = buffer(30, 24, 2, seed=11, device=dev, priority_alpha=0.6)
    rng = np.random.default_rng(2)
    index = torch.from_numpy(rng.integers(0, 24, 2500))
    prio = torch.from_numpy((10.0 ** rng.uniform(-2, 2, 2500)).astype(np.float32))
    cpu.update_priorities(index, prio)
    gpu.update_priorities(index, prio)
    ref, got = cpu.priority_mass.numpy().astype(np.float64), gpu.priority_mass.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - ref) <= np.maximum(1.0, ref * 16 * 2.0 ** -23))
    levels = [lev.cpu().numpy() for lev in gpu._levels]
    assert same_tree(levels, rebuilt(levels))


def test_bench_replay_prioritized_runs(dev):
    root = Path(__file__).resolve().parents[1]
    r = subprocess.run([sys.executable, str(root / 'benchmarks' / 'bench_replay.py'), '--stack', '3', '--nstep', '3',
                        '--prioritized', '--graph', '--frame', '16', '64', '4', '--frames', '256', '--steps', '3',
                        '--warmup', '1'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(res['us_per_batch']) == {'prioritized sample', 'uniform sample', 'priority draw', 'update_priorities'}
    assert res['tree_levels'] == 2 and all(v > 0 for v in res['us_per_batch'].values())
