"""The discriminator training step against an oracle that shares no code with
it (tests/disc_oracle.py, docs/STEP_ORACLE.md): an fp64 autograd model that
rounds to bf16 where the kernels' contracts say they round.  The budgets come
from references alone -- the same model with fp32 accumulation in two memory
formats, and the library's autocast path -- so no tolerance is fixed here.

The CPU tests prove the oracle (it is the plain fp64 model when it does not
round) and the comparator (references pass it, six deliberate errors do not);
the GPU tests hold the fused path, eager and graphed, to it."""
import copy

import pytest
import torch

import disc_oracle as do
from blendtorch import ops
from blendtorch.models import Discriminator

DEC = ops.DecodeConfig.unit(channels='rgba', gamma=2.2, dtype='bfloat16', layout='nhwc')


def _model(seed, nc=3, adaptive=True, fused=False):
    torch.manual_seed(seed)
    net = Discriminator(nc=nc, ndf=32, adaptive=adaptive, fused=fused)
    do.perturb_bn_affine(net, seed + 100)
    return net


def _frames(seed, n, h, w):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, 4), dtype=torch.uint8, generator=g)


def _references(params, buffers, passes, adaptive=True, decode=DEC, device='cpu'):
    """(fp64 oracle, [fp32 contiguous, fp32 channels-last], library) of one step."""
    common = dict(passes=passes, adaptive=adaptive, decode=decode)
    ref64 = do.oracle_step(params, buffers, dtype=torch.float64, device=device, **common)
    noise = [do.oracle_step(params, buffers, dtype=torch.float32, channels_last=cl, device=device, **common)
             for cl in (False, True)]
    lib = do.library_step(params, buffers, **common)
    return ref64, noise, lib


# ---- CPU: the oracle is the plain model when it does not round ---------------------------------------------------

@pytest.mark.parametrize('adaptive,shape', [(True, (3, 96, 128)), (False, (3, 64, 64))], ids=['adaptive', 'dcgan64'])
def test_unrounded_oracle_is_the_fp64_module(adaptive, shape):
    net = _model(0, adaptive=adaptive).double()
    params, buffers = do.split_state(net)
    x = torch.rand(shape[0], 3, *shape[1:], generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    tgt = torch.tensor([1.0, 0.0, 1.0], dtype=torch.float64)
    r = do.oracle_step(params, buffers, x, tgt, dtype=torch.float64, round_bf16=False, adaptive=adaptive)
    net.train()
    out = net(x.double())
    loss = torch.nn.BCELoss()(out, tgt)
    loss.backward()

    def rel(a, b):
        return float((a - b).norm() / b.norm().clamp_min(1e-300))
    assert rel(r['loss'][0], loss.detach()) < 1e-10
    assert rel(torch.sigmoid(r['logits']), out.detach()) < 1e-10
    for n, p in net.named_parameters():
        assert rel(r['grads'][n], p.grad) < 1e-10, n
    for n, b in net.named_buffers():
        assert rel(r['buffers'][n], b.double()) < 1e-10, n
        if n.endswith('num_batches_tracked'):
            assert int(b) == 1


# ---- CPU: references stay inside the rule, mutations do not --------------------------------------------------------

def _two_pass_case(seed):
    """densityopt's D step shape: mixed labels on one batch, zeros on another."""
    params, buffers = do.split_state(_model(seed))
    passes = [(_frames(seed + 1, 3, 96, 128), torch.tensor([1.0, 0.0, 1.0])), (_frames(seed + 2, 3, 96, 128), 0.0)]
    return params, buffers, passes


@pytest.fixture(scope='module')
def base():
    params, buffers, passes = _two_pass_case(0)
    ref64, noise, lib = _references(params, buffers, passes)
    return dict(params=params, buffers=buffers, passes=passes, ref64=ref64, noise=noise, lib=lib)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_references_stay_inside_the_rule(seed, base):
    if seed == 0:
        ref64, noise, lib = base['ref64'], base['noise'], base['lib']
    else:
        ref64, noise, lib = _references(*_two_pass_case(10 * seed))
    # one accumulation variant as the implementation, budgets from the other and the library
    rows, bs = do.compare(noise[0], ref64, noise=[noise[1]], lib=lib)
    print(f'seed {seed}: fp32 contiguous as impl\n' + do.format_table(rows, bs))
    # the library as the implementation: inside budget_d by construction (its slopes: the record)
    rows, bs = do.compare(lib, ref64, noise=noise, lib=lib, check=False)
    print(f'seed {seed}: autocast as impl\n' + do.format_table(rows, bs))
    assert all(r['d_impl'] <= r['budget_d'] for r in rows)


def _scaled(res, pick, factor):
    out = copy.deepcopy(res)
    hit = [n for n in out['grads'] if pick(n, out['grads'][n])]
    assert hit
    for n in hit:
        out['grads'][n] = out['grads'][n] * factor
    return out


MUTATIONS = ['bn_weight_grad_x1.05', 'conv_weight_grads_x2', 'targets_flipped', 'biased_running_var',
             'second_pass_stats_dropped', 'last_conv_wgrad_tail16']


@pytest.mark.parametrize('mutation', MUTATIONS)
def test_comparator_has_teeth(mutation, base):
    """The rounding-matched fp32 oracle with exactly one thing altered must fail compare."""
    n0 = base['noise'][0]
    kw = dict(passes=base['passes'], dtype=torch.float32, decode=DEC)
    if mutation == 'bn_weight_grad_x1.05':
        m = _scaled(n0, lambda n, g: n == 'features.4.weight', 1.05)
    elif mutation == 'conv_weight_grads_x2':
        m = _scaled(n0, lambda n, g: g.dim() == 4, 2.0)
    elif mutation == 'targets_flipped':
        kw['passes'] = [(x, 1.0 - torch.as_tensor(t)) for x, t in base['passes']]
        m = do.oracle_step(base['params'], base['buffers'], **kw)
    else:
        m = do.oracle_step(base['params'], base['buffers'], mutate=(mutation,), **kw)
    rows, bs = do.compare(m, base['ref64'], noise=base['noise'], lib=base['lib'], check=False)
    print(f'{mutation}\n' + do.format_table(rows, bs))
    with pytest.raises(do.OverBudget):
        do.compare(m, base['ref64'], noise=base['noise'], lib=base['lib'])


# ---- GPU: the fused step against the oracle ------------------------------------------------------------------------

@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    ops.hip_ext()
    return torch.device('cuda', 0)


COUNTED = ('conv_fwd', 'conv_wgrad', 'conv_dgrad', 'head_forward', 'bn_forward_lazy', 'bn_backward_by_head',
           'bn_backward_deferred_fold')


def _fused_model(dev, seed, nc=3, adaptive=True):
    return _model(seed, nc=nc, adaptive=adaptive, fused=True).to(dev).to(memory_format=torch.channels_last)


def _run_case(dev, name, net, passes, run_pass, expect, adaptive=True, decode=None):
    """One eager fused step (``run_pass(x, target) -> (loss, logits)`` per pass,
    every loss backward into the same .grad) held to the oracle of the weights
    and buffers the model had before it; ``expect``: KERNEL_CALLS deltas."""
    params, buffers = do.split_state(net)
    before = {k: ops.KERNEL_CALLS.get(k, 0) for k in COUNTED}
    losses, logits = [], []
    for x, t in passes:
        loss, lg = run_pass(x, t)
        loss.backward()
        losses.append(loss)
        logits.append(lg)
    torch.cuda.synchronize()
    delta = {k: ops.KERNEL_CALLS.get(k, 0) - before[k] for k in COUNTED}
    impl = do.fused_result(net, losses, logits)
    ref64, noise, lib = _references(params, buffers, passes, adaptive=adaptive, decode=decode)
    rows, bs = do.compare(impl, ref64, noise=noise, lib=lib, check=False)
    print(f'\n{name}: kernel calls {delta}\n' + do.format_table(rows, bs))
    for k, v in expect.items():     # the fused kernels ran: no library fallback passes this test
        assert delta[k] == v, (k, delta)
    do.compare(impl, ref64, noise=noise, lib=lib)


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['bench-mixed', 'bench-zero'])
def test_fused_step_u8_frames(dev, case):
    """The benchmark's path: raw u8 RGBA frames decoded in the first convolution, optimizer
    shadows, class defaults.  bench-mixed: M = 144 at the last layer (a partial pixel tile),
    mixed labels; bench-zero: a 5x7 head input (overlapping pool windows), M = 70, the (1 - y) side."""
    n, h, w, tgt = (3, 96, 128, torch.tensor([1.0, 0.0, 1.0])) if case == 'bench-mixed' else (2, 80, 112, 0.0)
    net = _fused_model(dev, 0)
    opt = ops.FusedAdam(net.parameters(), lr=2e-4)
    net.use_optimizer_shadows(opt)
    frames = _frames(3, n, h, w).to(dev)
    _run_case(dev, case, net, [(frames, tgt)],
              lambda x, t: net.bce_bf16(x.permute(0, 3, 1, 2), t, decode=DEC, probs='logits'),
              dict(conv_fwd=4, conv_wgrad=4, conv_dgrad=3, head_forward=1, bn_forward_lazy=1, bn_backward_by_head=1,
                   bn_backward_deferred_fold=1), decode=DEC)


@pytest.mark.gpu
def test_fused_step_rgb_bf16(dev):
    """nc = 3 decoded input: the first layer on the library path feeds the MFMA layers; no
    shadows, so the weights take the cast / transpose launches.

    With the library's bf16 convolution as the first layer every tensor was over budget
    (docs/STEP_ORACLE.md): gradients d_impl 4.7e-2 .. 1.08e-1 against budgets 2.4e-2 ..
    3.6e-2, BN 1 running_mean 2.8e-3 against 2.9e-7; bce_bf16 now runs it in fp32."""
    net = _fused_model(dev, 1)
    x = torch.rand(3, 3, 96, 128, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16)
    x = x.to(dev).contiguous(memory_format=torch.channels_last)
    _run_case(dev, 'rgb-bf16', net, [(x, 1.0)], lambda x, t: net.bce_bf16(x, t, probs='logits'),
              dict(conv_fwd=3, conv_wgrad=3, conv_dgrad=3, head_forward=1, bn_forward_lazy=1, bn_backward_by_head=1))


@pytest.mark.gpu
def test_library_first_layer_rounds_once_to_nearest(dev):
    """The narrow case behind rgb-bf16's first miss: the 3-channel first layer (off the MFMA
    path) must give bf16 RNE of the exact convolution, as the MFMA layers do.  The library's
    bf16 convolution gave a mean 0.28 % low (slope 0.9972, what truncation gives).
    The library's bf16 call: 147362 of 294912 elements off, slope 0.997210; the step's fp32
    convolution rounded once: 9 elements off, slope 0.999995.

    Bounds, from the formats: 48 exact bf16 products added in fp32 are within 48 * 2^-24 = 3e-6
    (relative) of the exact sum, a bf16 ulp is 2^-8 .. 2^-7 of the value, so at most
    2 * 3e-6 / 2^-8 = 1.5e-3 of the elements can sit close enough to a tie to round the other
    way, each by one ulp; RNE has no bias, so over 1.5e5 elements the slope stays within
    2^-9 / sqrt(1.5e5) = 5e-6 of 1 -- 1e-4 asserted, truncation gives 2.8e-3."""
    import torch.nn.functional as F
    net = _fused_model(dev, 1)
    x = torch.rand(3, 3, 96, 128, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16)
    with torch.no_grad():
        y = net._run_bf16(x.to(dev).contiguous(memory_format=torch.channels_last), list(net.features)[:1], True,
                          round_once=True)
    w = net.features[0].weight.detach().cpu().to(torch.bfloat16)
    ref = F.conv2d(x.double(), w.double(), None, 2, 1)
    r16, y = ref.to(torch.bfloat16).double(), y.cpu().double()
    off = y != r16
    slope = float((y * ref).sum() / (ref * ref).sum())
    print(f'\nfirst layer: {int(off.sum())} of {off.numel()} elements off RNE(exact), slope {slope:.6f}')
    assert float(off.double().mean()) <= 1.5e-3
    assert float(((y - r16).abs() / r16.abs().clamp_min(1e-30))[off].max() if off.any() else 0.0) <= 2 ** -7
    assert abs(slope - 1) < 1e-4


@pytest.mark.gpu
def test_fused_step_lazy_all(dev):
    """Every BN apply moved into a consumer (forward) or the producing convolution's weight
    gradient (backward), on a 4-channel bf16 input with mixed labels."""
    net = _fused_model(dev, 2)
    net.lazy_conv_bn = net.defer_bn_bwd = net.lazy_head_bn = True
    x = torch.rand(2, 4, 96, 128, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16)
    x = x.to(dev).contiguous(memory_format=torch.channels_last)
    _run_case(dev, 'lazy-all', net, [(x, torch.tensor([0.0, 1.0]))], lambda x, t: net.bce_bf16(x, t, probs='logits'),
              dict(conv_fwd=4, conv_wgrad=4, conv_dgrad=3, head_forward=1, bn_forward_lazy=4,
                   bn_backward_deferred_fold=4))


@pytest.mark.gpu
def test_fused_step_dopt_two_pass(dev):
    """densityopt's D step: the 64x64 stack (identity-pool head), real against 1 then simulated
    against 0, both losses backward into the same .grad, two statistics updates.

    Over budget before rgb-bf16's fix (docs/STEP_ORACLE.md): gradients d_impl 5.3e-2 ..
    1.38e-1 against budgets 3.0e-2 .. 6.8e-2, BN 1 running_mean 4.0e-3 against 2.9e-6."""
    net = _fused_model(dev, 3, adaptive=False)
    g = torch.Generator().manual_seed(6)
    real, sim = [(2 * torch.rand(4, 3, 64, 64, generator=g) - 1).to(torch.bfloat16).to(dev)
                 .contiguous(memory_format=torch.channels_last) for _ in range(2)]
    _run_case(dev, 'dopt-two-pass', net, [(real, 1.0), (sim, 0.0)], lambda x, t: net.bce_bf16(x, t, probs='logits'),
              dict(conv_fwd=6, conv_wgrad=6, conv_dgrad=6, head_forward=2), adaptive=False)


@pytest.mark.gpu
def test_fused_graphed_steps(dev):
    """Three graphed steps (CapturedStep, FusedAdam with shadows, u8 frames, one graph per
    input and the copy path for the third) against the oracle trained the same way: the
    capture's warm-up steps train on the first input, so the oracle takes them too.  Losses,
    final BN buffers and num_batches_tracked by the same rule; parameters are not compared
    (Adam's first steps are +-lr whatever the gradient's size)."""
    from blendtorch.parallel.step import CapturedStep
    lr, warmup = 2e-4, 2
    net = _fused_model(dev, 4)
    params, buffers = do.split_state(net)
    opt = ops.FusedAdam(net.parameters(), lr=lr)
    net.use_optimizer_shadows(opt)
    bufs = [_frames(20 + k, 3, 96, 128).to(dev) for k in range(3)]
    tgt = torch.tensor([1.0, 0.0, 1.0], device=dev)
    step = CapturedStep(net, opt, lambda m, x: m.bce_loss_bf16(x.permute(0, 3, 1, 2), tgt, decode=DEC),
                        allreduce=False, graph=True, static_inputs=2, warmup=warmup)
    before = {k: ops.KERNEL_CALLS.get(k, 0) for k in COUNTED}
    losses = [step(b).clone() for b in bufs]
    torch.cuda.synchronize()
    assert step.state == 'graph', step.error
    delta = {k: ops.KERNEL_CALLS.get(k, 0) - before[k] for k in COUNTED}
    assert delta['conv_fwd'] >= 4 and delta['conv_wgrad'] >= 4 and delta['conv_dgrad'] >= 3 and delta['head_forward'] >= 1
    impl = do.fused_result(net, losses)
    impl['grads'] = {}
    seq = [bufs[0]] * warmup + bufs
    kw = dict(lr=lr, decode=DEC, report=range(warmup, len(seq)))
    tcpu = tgt.cpu()
    ref64 = do.oracle_train(params, buffers, seq, tcpu, dtype=torch.float64, **kw)
    noise = [do.oracle_train(params, buffers, seq, tcpu, dtype=torch.float32, channels_last=cl, **kw)
             for cl in (False, True)]
    lib = do.library_train(params, buffers, seq, tcpu, **kw)
    rows, bs = do.compare(impl, ref64, noise=noise, lib=lib, check=False)
    print(f'\ngraphed-steps: kernel calls {delta}\n' + do.format_table(rows, bs))
    for n, b in net.named_buffers():
        if n.endswith('num_batches_tracked'):
            assert int(b) == len(seq)
    do.compare(impl, ref64, noise=noise, lib=lib)
