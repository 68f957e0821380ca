"""An oracle of the discriminator training step that shares no code with the
fused path: plain PyTorch autograd in fp64 (or fp32), rounding to bf16 at
exactly the points where the kernels' contracts say they round, the same stack
on library kernels under autocast, and the comparator that turns them into a
budget (docs/STEP_ORACLE.md).

Only ``DecodeConfig`` and ``reference_decode`` come from ``blendtorch.ops``
(they turn u8 frames into values); ``library_step`` builds the unfused
``Discriminator``, which runs the library's kernels only.
"""
import torch
import torch.nn.functional as F

from blendtorch.ops import DecodeConfig, reference_decode

MOMENTUM, EPS, SLOPE = 0.1, 1e-5, 0.2


class _RoundBoth(torch.autograd.Function):
    """bf16 RNE and back, of the value AND of the gradient that reaches it: an
    activation the kernels store as bf16, whose gradient (dz / dx / gx) they
    store as bf16 too."""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


class _RoundFwd(torch.autograd.Function):
    """bf16 RNE and back of the value only: the bf16 copy of an fp32 master
    weight, whose gradient goes to the master unrounded."""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


def split_state(net):
    """``(params, buffers)`` of a Discriminator as detached clones by name."""
    return ({n: p.detach().clone() for n, p in net.named_parameters()},
            {n: b.detach().clone() for n, b in net.named_buffers()})


def perturb_bn_affine(net, seed):
    """BN weights / biases away from 1 / 0, so that neither drops out of a gradient."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if p.dim() == 1:
                r = torch.randn(p.shape, generator=g).to(p.device)
                p.copy_(1.0 + 0.3 * r if n.endswith('weight') else 0.2 * r)


def input_values(frames_or_x, decode=None):
    """fp32 NCHW RGB values of a step's input: raw u8 RGBA frames [N, H, W, 4]
    through ``decode``'s fp32 table, or decoded values [N, 3 or 4, H, W] as they
    are.  The alpha channel is dropped: an RGB weight ignores it (kernels.h
    ConvFwdParams::w_channels: "3 = an RGB weight, input channel 3 ignored")."""
    x = frames_or_x
    if x.dtype == torch.uint8:
        cfg = DecodeConfig(channels='rgb', gamma=decode.gamma, scale=decode.scale, mean=decode.mean,
                           std=decode.std, dtype='float32', layout='nchw')
        return reference_decode(x, cfg)
    return x[:, :3].float()


def _layers(params):
    convs = [n for n, p in params.items() if p.dim() == 4]
    bnw = [n for n, p in params.items() if p.dim() == 1 and n.endswith('.weight')]
    return convs[:-1], convs[-1], [n[:-len('.weight')] for n in bnw]


def oracle_step(params, buffers, frames_or_x=None, target=None, *, dtype=torch.float64, round_bf16=True,
                adaptive=True, passes=None, decode=None, channels_last=False, device='cpu', mutate=(),
                head_dz_bf16=True):
    """Forward and backward of the DCGAN discriminator's training step through
    autograd in ``dtype``.  ``passes``: ``[(input, target), ...]`` run one after
    the other on the same parameters -- gradients accumulate, the running
    statistics update once per pass (densityopt's D step); default: the one
    pass ``(frames_or_x, target)``.  A target is a scalar or [N].

    ``round_bf16`` rounds (RNE to bf16, back to ``dtype``) where the kernels do
    and nowhere else -- see the numbered comments.  ``channels_last`` only
    changes the memory format of the convolutions' operands (another
    accumulation order).  ``mutate`` names deliberate errors for the
    comparator's own tests: 'biased_running_var', 'second_pass_stats_dropped',
    'last_conv_wgrad_tail16'.

    Returns ``{'loss': [P], 'logits': [P * N], 'grads': {name: tensor},
    'buffers': {name: tensor}}``, fp64 on the CPU."""
    if passes is None:
        passes = [(frames_or_x, target)]
    rb = _RoundBoth.apply if round_bf16 else (lambda t: t)
    rf = _RoundFwd.apply if round_bf16 else (lambda t: t)
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    P = {n: p.detach().to(device=device, dtype=dtype).clone().requires_grad_(True) for n, p in params.items()}
    B = {n: b.detach().to(device).clone() for n, b in buffers.items()}
    for n in B:
        if B[n].is_floating_point():
            B[n] = B[n].to(dtype)
    convs, head, bns = _layers(P)
    losses, logits = [], []
    for k, (inp, tgt) in enumerate(passes):
        # 1. input: the bf16 RNE of the fp32 decode-table value (kernels.h ConvFwdParams::lut:
        #    "lut their decode table as bf16 [4][256] (RNE of the fp32 table)"); a bf16 input
        #    is its own rounding
        a = input_values(inp.to(device), decode).to(torch.bfloat16 if round_bf16 else torch.float32).to(dtype)
        for li, (cn, bn) in enumerate(zip(convs, bns)):
            # 2. weight: the bf16 RNE of the fp32 master, the gradient goes to the master
            #    unrounded (kernels.h AdamParams::shadow: "bf16 shadow copy of the new weights ...
            #    what a bf16 forward reads next step"; conv_wgrad writes fp32)
            w = rf(P[cn])
            if 'last_conv_wgrad_tail16' in mutate and li == len(convs) - 1:
                y = F.conv2d(a, w.detach(), None, 2, 1)
                yw = F.conv2d(a.detach(), w, None, 2, 1)
                keep = torch.ones(y.shape[0] * y.shape[2] * y.shape[3], dtype=dtype, device=y.device)
                keep[-16:] = 0       # the weight gradient misses the last 16 output pixels (NHW order)
                keep = keep.view(y.shape[0], 1, y.shape[2], y.shape[3])
                y = y + (yw - yw.detach()) * keep
            else:
                y = F.conv2d(a.contiguous(memory_format=fmt), w.contiguous(memory_format=fmt), None, 2, 1)
            # 3. conv output: ONE rounding after the full-precision accumulation, and its gradient
            #    dz is bf16 (kernels.h conv_fwd: "y [N][Ho][Wo][Cout] bf16")
            y = rb(y)
            # 4. batch statistics of the ROUNDED y (kernels.h conv_fwd: "sum / sum of squares of
            #    the rounded y"), biased variance to normalise, unbiased for running_var
            M = y.shape[0] * y.shape[2] * y.shape[3]
            mean = y.mean((0, 2, 3))
            var = ((y - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
            if not ('second_pass_stats_dropped' in mutate and k > 0):
                with torch.no_grad():
                    rv = var if 'biased_running_var' in mutate else var * (M / (M - 1))
                    B[bn + '.running_mean'].mul_(1 - MOMENTUM).add_(MOMENTUM * mean)
                    B[bn + '.running_var'].mul_(1 - MOMENTUM).add_(MOMENTUM * rv)
                    B[bn + '.num_batches_tracked'] += 1
            xhat = (y - mean.view(1, -1, 1, 1)) * torch.rsqrt(var + EPS).view(1, -1, 1, 1)
            z = xhat * P[bn + '.weight'].view(1, -1, 1, 1) + P[bn + '.bias'].view(1, -1, 1, 1)
            # 5. leaky_relu(bn(y)): ONE rounding, also where a consumer applies it as it reads y
            #    (kernels.h HeadParams::act: "the pooling reads leaky(bn(z)) rounded to bf16"), and
            #    the gradient that reaches it (conv_dgrad's dx, head_backward's dz) is bf16
            #    -- except the last activation's when the head applies that BN's backward itself
            #    (HeadParams::bn_sums: "write the BN's INPUT gradient gx (not dz) into dz": dz is
            #    never stored, only gx is rounded; ``head_dz_bf16=False``)
            last = li == len(convs) - 1
            a = (rb if head_dz_bf16 or not last else rf)(F.leaky_relu(z, SLOPE))
        # 6. pool -> head dot -> sigmoid -> mean BCE: unrounded (HeadParams::pooled is fp32), fp32
        #    head weight and gradient, the logs clamped at -100 (head.hip head_loss_wave:
        #    "fmaxf(logf(pr), -100.f)")
        if adaptive:
            a = F.adaptive_avg_pool2d(a, tuple(P[head].shape[2:]))
        logit = F.conv2d(a, P[head]).reshape(-1)
        t = torch.as_tensor(tgt, dtype=dtype, device=logit.device).expand_as(logit)
        p = torch.sigmoid(logit)
        loss = -(t * torch.log(p).clamp(min=-100) + (1 - t) * torch.log(1 - p).clamp(min=-100)).mean()
        loss.backward()
        losses.append(loss.detach())
        logits.append(logit.detach())
    return {'loss': torch.stack(losses).double().cpu(), 'logits': torch.cat(logits).double().cpu(),
            'grads': {n: p.grad.double().cpu() for n, p in P.items()},
            'buffers': {n: b.double().cpu() for n, b in B.items()}}


# The library reference runs on the CPU, also in the GPU tests: on the MI355X the library's
# BatchNorm under bf16 autocast ended the process (a host segmentation fault inside
# torch.batch_norm, channels-last, N = 2, 80x112) and its cause was not found.  The CPU
# autocast path rounds at the same places and sits CLOSER to the oracle than the GPU
# library did where both ran, so the budget it gives is the stricter one.

def _library_net(params, buffers, adaptive):
    from blendtorch.models import Discriminator
    cw = [p for p in params.values() if p.dim() == 4]
    net = Discriminator(nc=cw[0].shape[1], ndf=cw[0].shape[0], adaptive=adaptive, fused=False)
    net.load_state_dict({n: t.detach().cpu() for n, t in {**params, **buffers}.items()})
    return net.to(memory_format=torch.channels_last)


def _library_pass(net, inp, tgt, decode):
    seen = []
    hook = net.features[-2].register_forward_hook(lambda m, i, o: seen.append(o.detach()))
    x = input_values(inp.cpu(), decode).contiguous(memory_format=torch.channels_last)
    try:
        with torch.autocast('cpu', dtype=torch.bfloat16):
            out = net(x)
    finally:
        hook.remove()
    out = out.float()   # (binary_cross_entropy refuses to run under autocast)
    loss = F.binary_cross_entropy(out, torch.as_tensor(tgt, dtype=torch.float32).cpu().expand_as(out))
    return loss, seen[0].reshape(-1)


def library_step(params, buffers, frames_or_x=None, target=None, *, adaptive=True, passes=None, decode=None):
    """The same step as ``Discriminator(fused=False)`` under
    ``torch.autocast(bfloat16)``, channels-last, then ``F.binary_cross_entropy``:
    library kernels only.  Same arguments and result as :func:`oracle_step`."""
    if passes is None:
        passes = [(frames_or_x, target)]
    net = _library_net(params, buffers, adaptive).train()
    losses, logits = [], []
    for inp, tgt in passes:
        loss, lg = _library_pass(net, inp, tgt, decode)
        loss.backward()
        losses.append(loss.detach())
        logits.append(lg)
    return {'loss': torch.stack(losses).double().cpu(), 'logits': torch.cat(logits).double().cpu(),
            'grads': {n: p.grad.double().cpu() for n, p in net.named_parameters()},
            'buffers': {n: b.double().cpu() for n, b in net.named_buffers()}}


def oracle_train(params, buffers, inputs, target, *, lr, dtype=torch.float64, adaptive=True, decode=None,
                 channels_last=False, device='cpu', report=None):
    """One :func:`oracle_step` and one ``torch.optim.Adam`` update of masters
    kept in ``dtype`` per input (the weights are rounded again every step).
    Returns the losses of the steps listed in ``report`` (default: all), no
    gradients, and the final buffers."""
    masters = {n: p.detach().to(device='cpu', dtype=dtype).clone().requires_grad_(True) for n, p in params.items()}
    opt = torch.optim.Adam(list(masters.values()), lr=lr)
    bufs, losses = buffers, []
    for x in inputs:
        r = oracle_step(masters, bufs, x, target, dtype=dtype, adaptive=adaptive, decode=decode,
                        channels_last=channels_last, device=device)
        for n, p in masters.items():
            p.grad = r['grads'][n].to(dtype)
        opt.step()
        bufs = r['buffers']
        losses.append(r['loss'][0])
    losses = torch.stack(losses)
    return {'loss': losses if report is None else losses[list(report)], 'grads': {},
            'buffers': {n: b.double() for n, b in bufs.items()}}


def library_train(params, buffers, inputs, target, *, lr, adaptive=True, decode=None, report=None):
    """:func:`oracle_train` on library kernels: autocast and fp32 ``torch.optim.Adam``."""
    net = _library_net(params, buffers, adaptive).train()
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    losses = []
    for x in inputs:
        opt.zero_grad(set_to_none=True)
        loss, _ = _library_pass(net, x, target, decode)
        loss.backward()
        opt.step()
        losses.append(loss.detach().double().cpu())
    losses = torch.stack(losses)
    return {'loss': losses if report is None else losses[list(report)], 'grads': {},
            'buffers': {n: b.double().cpu() for n, b in net.named_buffers()}}


def fused_result(net, losses, logits=None):
    """The fused path's step in :func:`oracle_step`'s result form."""
    r = {'loss': torch.stack([l.detach().reshape(()) for l in losses]).double().cpu(),
         'grads': {n: p.grad.double().cpu() for n, p in net.named_parameters() if p.grad is not None},
         'buffers': {n: b.double().cpu() for n, b in net.named_buffers()}}
    if logits is not None:
        r['logits'] = torch.cat([l.detach().reshape(-1) for l in logits]).double().cpu()
    return r


def _flat(r):
    out = {}
    for n, g in r['grads'].items():
        out['grad:' + n] = g
    for n, b in r['buffers'].items():
        out['buf:' + n] = b
    if 'logits' in r:
        out['logits'] = r['logits']
    for k, l in enumerate(r['loss']):
        out[f'loss[{k}]'] = l
    return out


def _d_s(t, t64):
    t, t64 = t.double().reshape(-1), t64.double().reshape(-1)
    nn = float(t64 @ t64)
    if t64.numel() == 1 or nn == 0.0:      # scalars (and an all-zero reference): absolute difference
        return float((t - t64).norm()), None
    return float((t - t64).norm()) / nn ** 0.5, float(t @ t64) / nn


class OverBudget(AssertionError):
    pass


def format_table(rows, budget_s):
    def f(v):
        return '    -    ' if v is None else f'{v:9.3e}'
    lines = [f'{"tensor":34s} {"d_impl":>9s} {"d_lib":>9s} {"d_noise":>9s} {"budget_d":>9s} {"s_impl":>9s}  '
             f'(budget_s {budget_s:.3e})']
    for r in rows:
        s = '    -    ' if r['s_impl'] is None else f'{r["s_impl"]:9.5f}'
        lines.append(f'{r["tensor"]:34s} {f(r["d_impl"])} {f(r["d_lib"])} {f(r["d_noise"])} {f(r["budget_d"])} {s}'
                     + ('   OVER' if r['over'] else ''))
    return '\n'.join(lines)


def compare(impl, ref64, noise, lib, check=True):
    """Every tensor ``T`` of ``impl`` (each parameter gradient, each BN buffer,
    the logits, each loss) against the fp64 oracle's ``T64``:

      d(T) = |T - T64|_2 / |T64|_2   (absolute difference for scalars)
      s(T) = <T, T64> / <T64, T64>

    with budgets made in this call from references only (``noise``: the same
    rounding-matched oracle with another accumulation; ``lib``: library_step):

      budget_d(T) = max(d_lib(T), 2 max_k d_noise_k(T))
      budget_s    = 2 max over the gradient tensors and k of |s_noise_k - 1|

    Returns ``(rows, budget_s)``; raises :class:`OverBudget` with the table when
    any ``d_impl > budget_d`` or any gradient tensor's ``|s_impl - 1| > budget_s``."""
    T64, TI, TL = _flat(ref64), _flat(impl), _flat(lib)
    TN = [_flat(n) for n in noise]
    missing = [k for k in T64 if k not in TI]
    if missing:
        raise OverBudget(f'compare: the implementation has no {missing}')
    # the slope rule is the gradients' (their budget is pooled over them); for every tensor
    # |s - 1| <= d, so budget_d already bounds the other tensors' slopes
    sloped = [k for k in T64 if k.startswith('grad:')]
    budget_s = 2 * max([abs(_d_s(n[k], T64[k])[1] - 1) for n in TN for k in sloped
                        if _d_s(n[k], T64[k])[1] is not None] or [0.0])
    rows = []
    for k in T64:
        d, s = _d_s(TI[k], T64[k])
        dl = _d_s(TL[k], T64[k])[0]
        dn = max(_d_s(n[k], T64[k])[0] for n in TN)
        bd = max(dl, 2 * dn)
        over = d > bd or (k in sloped and s is not None and abs(s - 1) > budget_s)
        rows.append(dict(tensor=k, d_impl=d, d_lib=dl, d_noise=dn, budget_d=bd, s_impl=s, over=over))
    if check and any(r['over'] for r in rows):
        raise OverBudget('over budget:\n' + format_table(rows, budget_s))
    return rows, budget_s
