"""Mixture-of-softmaxes output head (misc/MixtureOfSoftmax.py; opts.py --use_mos / --num_expert) on the HIP path.

`MixtureOfSoftmax` has the reference's constructor, sub-module names and state_dict keys, so a reference checkpoint's
`mos.*` entries load as they are.  All arithmetic runs in librfn_hip.so (include/rfn.h, "mixture of softmaxes"): the three
linear maps on the f32 GEMM, the mix kernels in csrc/rfn_mos.hip.  There is no CPU path.

The head computes log(sum_k pi_k softmax(x_k)) in log-sum-exp form, which is the reference's function wherever that is finite
and stays finite where its linear f32 form underflows.
"""
import torch
import torch.nn as nn

from . import _native as N


class _ModuleGrads:
    """Gradient sink of a stand-alone module: fresh tensors, handed back through autograd."""

    def __init__(self, params):
        self.params = params

    def buffers(self, dev):
        self.grads = [torch.empty_like(p) for p in self.params]
        return self.grads

    def done(self):
        return tuple(self.grads)


class _MosFn(torch.autograd.Function):
    """The head as one autograd node over rfn_mos_fwd / _bwd, or -- spec['kind'] == 'loss' -- over rfn_mos_loss_fwd / _loss_bwd
    (the masked, label-smoothed NLL straight from the expert logits: neither log_prob nor its gradient is materialised).

    h: (rows, R) rows, any row stride.  spec: {'kind': 'logp', 'shape', 'inner', 's_inner', 's_outer'} -- the output tensor and
    the row remap of rfn_mos_fwd -- or {'kind': 'loss', 'B', 'T', 'target', 'mask', 'eps'} for time-major rows r = t * B + b.
    sink: where the parameter gradients go -- .buffers(dev) -> tensors in slot order, .done() -> what backward returns for the
    parameters (the gradients themselves, or Nones when the sink has handed them over itself)."""

    @staticmethod
    def _run_fwd(md, spec, h, params, ws, dev, train):
        if spec['kind'] == 'loss':
            B, T = spec['B'], spec['T']
            loss = torch.zeros(1, device=dev)
            scratch = torch.empty(B * T, device=dev)
            N.mos_loss_fwd(md, B, T, h, params, spec['target'], spec['mask'], spec['eps'], scratch, loss, ws)
            return loss[0]
        out = torch.empty(spec['shape'], device=dev)
        N.mos_fwd(md, h, params, out, ws, spec['inner'], spec['s_inner'], spec['s_outer'], train=train)
        return out

    @staticmethod
    def forward(ctx, md, spec, sink, save_bwd, h, *params):
        h = N.require_cuda_f32(h, 'h') if h.stride(-1) != 1 else h
        if not h.is_cuda or h.dtype != torch.float32 or h.dim() != 2 or h.size(1) != md.R:
            raise N.RfnError('the head takes float32 GPU rows (rows, %d), got %s %s' % (md.R, tuple(h.shape), h.dtype))
        for p in params:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise N.RfnError('the head\'s parameters must be contiguous float32 GPU tensors')
        dev = h.device
        train = bool(save_bwd) or spec['kind'] == 'loss'
        ws = N.mos_workspace(md, h.size(0), train, dev)
        out = _MosFn._run_fwd(md, spec, h, params, ws, dev, train)
        if save_bwd:
            ctx.md, ctx.spec, ctx.sink, ctx.params, ctx.consumed = md, spec, sink, params, False
            ctx.save_for_backward(h, ws)          # ws: freed with the graph
        return out

    @staticmethod
    def backward(ctx, g):
        md, spec, params = ctx.md, ctx.spec, ctx.params
        h, ws = ctx.saved_tensors
        dev = h.device
        if ctx.consumed:      # the first backward wrote d x over x: a second one over the same graph recomputes the pass
            _MosFn._run_fwd(md, spec, h, params, ws, dev, True)
        ctx.consumed = True
        d_h = torch.empty(h.size(0), md.R, device=dev)
        grads = ctx.sink.buffers(dev)
        if spec['kind'] == 'loss':
            N.mos_loss_bwd(md, spec['B'], spec['T'], h, params, spec['target'], spec['mask'], spec['eps'], 1.0,
                           g.contiguous().float(), d_h, grads, ws)
        else:
            N.mos_bwd(md, h, params, g.contiguous(), d_h, grads, ws, spec['inner'], spec['s_inner'], spec['s_outer'])
        return (None, None, None, None, d_h) + tuple(ctx.sink.done())


class MixtureOfSoftmax(nn.Module):
    """misc/MixtureOfSoftmax.py:10-34: n_experts experts tanh(Linear(h)) share one vocabulary projection `decoder`; a softmax
    over `prior(h)` mixes their softmaxes.  `forward(h)` returns probabilities as the reference does; `log_prob(h)` is what the
    decoder uses (the reference takes torch.log of forward's output, misc/ReviewNetModel.py:122-125)."""

    def __init__(self, rnn_size, emb_size, n_experts, dict_size):
        super().__init__()
        if not 1 <= int(n_experts) <= N.MOS_MAXK:
            raise ValueError('num_expert = %d: the head takes 1 <= num_expert <= %d experts' % (n_experts, N.MOS_MAXK))
        self.rnn_size, self.emb_size, self.n_experts, self.dict_size = rnn_size, emb_size, int(n_experts), dict_size
        self.prior = nn.Linear(rnn_size, n_experts, bias=False)
        self.latent = nn.ModuleList([nn.Sequential(nn.Linear(rnn_size, emb_size), nn.Tanh()) for _ in range(self.n_experts)])
        self.decoder = nn.Linear(emb_size, dict_size)
        self.md = N.mos_dims(rnn_size, emb_size, self.n_experts, dict_size)
        self.slot_names = N.mos_param_names(self.md)
        if self.slot_names != [k for k, _ in self.named_parameters()]:
            raise N.RfnError('parameter schema mismatch between MixtureOfSoftmax and librfn_hip.so')

    def slot_params(self):
        """The parameters in the library's slot order (= state_dict order)."""
        return [p for _, p in self.named_parameters()]

    def log_prob(self, h):
        """h (..., rnn_size) on the GPU -> log-probs (..., dict_size)."""
        lead = h.shape[:-1]
        h2 = h.reshape(-1, self.rnn_size)
        params = self.slot_params()
        spec = {'kind': 'logp', 'shape': (h2.size(0), self.dict_size), 'inner': h2.size(0), 's_inner': self.dict_size, 's_outer': 0}
        out = _MosFn.apply(self.md, spec, _ModuleGrads(params), torch.is_grad_enabled(), h2, *params)
        return out.view(*lead, self.dict_size)

    def forward(self, output):
        return torch.exp(self.log_prob(output))
