"""RecurrentFusionModel: host-side mirror of the reference's module for the HIP path.

Same constructor argument (an ``opt`` Namespace), same ``forward(fc_feats, att_feats, seq)`` /
``sample(fc_feats, att_feats, opt)`` / ``sample_beam`` / ``get_init_state`` / ``get_thought_vectors`` /
``one_time_step`` surface and the same ``state_dict`` keys and shapes as the reference's
``misc/RecurrentFusionModel.py:117-658`` -- so ``models.setup(opt)``, ``train.py`` and ``eval.py`` drop in.
All arithmetic runs in librfn_hip.so (include/rfn.h); PyTorch only owns device memory, the stream and
the autograd graph edges between the two phases.  There is no CPU path: inputs must be on the GPU.

The sub-modules below (``_AttParams`` ...) hold parameters only; they exist to reproduce the reference's
parameter names (``review_steps_individual.{t}.lstm.{i}.att_model.att_2_att_h.weight`` ...).
"""
from __future__ import annotations

import ctypes as C
import re
import weakref

import numpy as np
import torch
import torch.nn as nn

from . import _native as N
from .distill import TopKTeacher
from .decode import (MAX_BEAM, MAX_STEPS, BeamBuffers, GreedyBuffers, _Consensus, _Constraints, _diverse_beams, _Diversity, _LazyList,
                     _length_penalty, _Lexical, _Sampling, _Scoring, _sorted_done_beams, _Stepper, ScoreBuffers, early_exit,
                     host_beam_loop, host_greedy_loop, keep_candidates_n, run_beam_loop, run_greedy_loop, _Stochastic,
                     StochasticBuffers)
from .mos import MixtureOfSoftmax, _MosFn

_INIT = 0.1


def _uniform(*tensors):
    for t in tensors:
        t.data.uniform_(-_INIT, _INIT)


class _AttParams(nn.Module):
    """Parameters of AttentionModelCore (misc/AttentionModelCore.py:16-29)."""

    def __init__(self, rnn_size, feat_size, att_hid):
        super().__init__()
        self.att_2_att_h = nn.Linear(feat_size, att_hid)
        self.h_2_att_h = nn.Linear(rnn_size, att_hid)
        self.att_h_2_out = nn.Linear(att_hid, 1)
        for lin in (self.att_2_att_h, self.h_2_att_h, self.att_h_2_out):
            _uniform(lin.weight, lin.bias)


class _FusionCellParams(nn.Module):
    """Parameters of LSTMFusionNoInputCore (misc/RecurrentFusionModel.py:30-45); biases keep nn.Linear's
    default init as in the reference."""

    def __init__(self, H_size, rnn_size, feat_size, att_hid):
        super().__init__()
        self.att_model = _AttParams(rnn_size, feat_size, att_hid)
        self.H2h = nn.Linear(H_size, 4 * rnn_size)
        self.z2h = nn.Linear(feat_size, 4 * rnn_size)
        _uniform(self.H2h.weight, self.z2h.weight)


class _FusionStepParams(nn.Module):
    """FeatArrayFusionNoInputCore (misc/RecurrentFusionModel.py:93-97)."""

    def __init__(self, M, rnn_size, feat_sizes, att_hid):
        super().__init__()
        self.lstm = nn.ModuleList([_FusionCellParams(M * rnn_size, rnn_size, feat_sizes[i], att_hid) for i in range(M)])


class _ReviewStepParams(nn.Module):
    """LSTMSoftMultiAttentionFeatArrayNoInputCore (misc/LSTMSoftMultiAttentionFeatArrayNoInputCore.py:24-38)."""

    def __init__(self, M, rnn_size, att_hid, maxout=0):
        super().__init__()
        gw = (5 if maxout else 4) * rnn_size
        self.h2h = nn.Linear(rnn_size, gw)
        self.z_2_h = nn.ModuleList([nn.Linear(rnn_size, gw) for _ in range(M)])
        self.att_model = nn.ModuleList([_AttParams(rnn_size, rnn_size, att_hid) for _ in range(M)])
        _uniform(self.h2h.weight, self.h2h.bias)


class _DecoderParams(nn.Module):
    """LSTMSoftAttentionCore (misc/LSTMSoftAttentionCore.py:24-58)."""

    def __init__(self, enc_size, rnn_size, att_hid, maxout=0):
        super().__init__()
        gw = (5 if maxout else 4) * rnn_size
        self.i2h = nn.Linear(enc_size, gw)
        self.h2h = nn.Linear(rnn_size, gw)
        self.z2h = nn.Linear(rnn_size, gw)
        self.att_2_att_h = nn.Linear(rnn_size, att_hid)
        self.h_2_att_h = nn.Linear(rnn_size, att_hid)
        self.att_h_2_out = nn.Linear(att_hid, 1)
        for lin in (self.i2h, self.h2h, self.z2h, self.att_2_att_h, self.h_2_att_h, self.att_h_2_out):
            _uniform(lin.weight, lin.bias)


# path_flags under which the decoder cell reads the thought vectors per row: rows cannot share them (_need_hoisted)
_NOT_HOISTED = N.PATH_OPT_DEC_UNHOISTED | N.PATH_OPT_PERSIST_DEC_FWD | N.PATH_OPT_PERSIST_DEC_BWD


def _fresh_seed() -> int:
    # dropout masks are Philox streams keyed by this seed; drawn from torch's CPU generator so that
    # torch.manual_seed(seed + rank) (train.py:23) makes runs reproducible
    return int(torch.randint(0, 2 ** 62, (1,)).item())


class _PrefixFn(torch.autograd.Function):
    """Phase 1 (fc2h + fusion stages I and II) as one autograd node: rfn_prefix_fwd / rfn_prefix_bwd."""

    @staticmethod
    def forward(ctx, model, save_bwd, drop, seed, M, lens, *tensors):
        # lens: None, or M entries (None | (B,) int32 device tensor): the valid rows of each stage-I map (N.att_lens_arg)
        fc = [N.require_cuda_f32(t, 'fc_feats') for t in tensors[:M]]
        att = [N.require_cuda_f32(t, 'att_feats') for t in tensors[M:2 * M]]
        params = tensors[2 * M:]
        train = bool(save_bwd)
        # a feature tensor that requires grad: the workspace keeps every stage-I step's d z (RFN_PATH_OPT_INPUT_GRADS) for
        # rfn_prefix_bwd_inputs; the forward launches and their results are the same either way
        input_grads = train and any(ctx.needs_input_grad[6:6 + 2 * M])
        d = model._dims_for(drop, input_grads)
        B = fc[0].shape[0]
        dev = fc[0].device
        R, T2, K = d.R, d.T2, d.K
        table = model._param_table(params, model._prefix_slots)
        ws_bytes = N.lib.rfn_prefix_ws_bytes(C.byref(d), B, int(train))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        comb = torch.empty(T2, B, R, device=dev)
        h = torch.empty(B, R, device=dev)
        c = torch.empty(B, R, device=dev)
        reason = torch.empty(M + 1, B, K, device=dev)
        len_ptrs = N.ptr_array(lens) if lens is not None else None
        model._check_ragged(N.lib.rfn_prefix_fwd_ex(C.byref(d), B, table, N.ptr_array(fc), N.ptr_array(att), comb.data_ptr(),
                                                    h.data_ptr(), c.data_ptr(), reason.data_ptr(), ws.data_ptr(), ws_bytes,
                                                    int(train), seed, len_ptrs, N.stream_ptr()), lens, 'rfn_prefix_fwd')
        if train:
            ctx.lens = lens
            ctx.model, ctx.seed, ctx.M, ctx.B, ctx.drop, ctx.input_grads = model, seed, M, B, drop, input_grads
            ctx.fc, ctx.att, ctx.params, ctx.consumed, ctx.snapshot = fc, att, params, False, None
            # the multi-GB workspace is a SAVED tensor, not an attribute: autograd frees it right after a non-retained
            # backward instead of keeping it for as long as anything references the graph (a trainer's `loss` variable)
            ctx.save_for_backward(ws)
        return comb, h, c, reason

    @staticmethod
    def backward(ctx, d_comb, d_h, d_c, d_reason):
        model, M, B = ctx.model, ctx.M, ctx.B
        ws, = ctx.saved_tensors
        d = model._dims_for(ctx.drop, ctx.input_grads)      # the forward's flags: the workspace layout (and the recompute's)
        dev = ctx.fc[0].device
        table = model._param_table(ctx.params, model._prefix_slots)
        flats, by_slot, gtable = model._grad_buffers(model._prefix_buckets, dev)
        cont = lambda t: None if t is None else t.contiguous()  # noqa: E731
        d_comb, d_h, d_c, d_reason = cont(d_comb), cont(d_h), cont(d_c), cont(d_reason)
        ws_bytes = ws.numel()
        att_ptrs = N.ptr_array(ctx.att)
        len_ptrs = N.ptr_array(ctx.lens) if ctx.lens is not None else None
        if ctx.consumed and ctx.snapshot is not None:
            # model.retain_activations: the activations of the ORIGINAL forward (see below).  Through .data: `ws` is a
            # saved tensor, and a versioned in-place write would make autograd refuse the NEXT backward over this graph
            # (ppo_k = 10 passes in the reference's loop, train_rl.py:190-201)
            ws.data.copy_(ctx.snapshot)
        elif ctx.consumed:
            # backward overwrites activations in place (projections -> their gradients, gates -> gate gradients), so a
            # second backward over the same graph (loss.backward(retain_graph=True) in the PPO loop, train_rl.py:190-201)
            # first recomputes phase 1 into the workspace: same inputs, same dropout seed, the weights AS THEY ARE NOW.
            # If optimizer.step() ran in between (it does in that loop) these are the activations of the updated weights:
            # a self-consistent gradient at the new weights.  The reference instead backpropagates the activations saved
            # at the original forward through the updated weights; set model.retain_activations = True for exactly that
            # (costs one copy of the workspace per retained graph).
            R, T2, K = d.R, d.T2, d.K
            scratch = torch.empty(T2 * B * R + 2 * B * R + (M + 1) * B * K, device=dev)
            o1, o2, o3 = T2 * B * R, T2 * B * R + B * R, T2 * B * R + 2 * B * R
            N.check(N.lib.rfn_prefix_fwd_ex(C.byref(d), B, table, N.ptr_array(ctx.fc), att_ptrs, scratch.data_ptr(),
                                            scratch[o1:].data_ptr(), scratch[o2:].data_ptr(), scratch[o3:].data_ptr(),
                                            ws.data_ptr(), ws_bytes, 1, ctx.seed, len_ptrs, N.stream_ptr()),
                    'rfn_prefix_fwd (recompute)')
        elif getattr(model, 'retain_activations', False):
            ctx.snapshot = ws.clone()
        ctx.consumed = True
        # everything except the per-encoder stage-I weight gradients ...
        model._check_ragged(N.lib.rfn_prefix_bwd_ex(C.byref(d), B, table, N.ptr_array(ctx.fc), att_ptrs, N.ptr(d_comb),
                                                    N.ptr(d_h), N.ptr(d_c), N.ptr(d_reason), gtable, ws.data_ptr(), ws_bytes,
                                                    ctx.seed, 1, len_ptrs, N.stream_ptr()), ctx.lens, 'rfn_prefix_bwd')
        model._bucket_done('core', flats['core'])
        # ... then the per-encoder stage-I weight gradients, the BIG buckets first: part a of every encoder (H2h, z2h,
        # h_2_att_h: 277 MB each at C3, short K = B GEMMs) is produced and handed over before the first long att_2_att_h
        # product (part b: 34 MB, the largest GEMMs of backward) starts, so a data-parallel host has 71 % of the gradient
        # bytes in flight under ALL of those GEMMs instead of encoder i's bucket under encoder i's GEMM only -- at a
        # 32-caption shard the b-products are 3.3 ms against 5+ ms of exchange
        todo = [(i, part, tag) for part, tag in ((1, 'a'), (2, 'b')) for i in range(M)]
        if getattr(model, '_wgrad_interleaved', False):      # tools A/B only: encoder by encoder (a0 b0 a1 b1 ...)
            todo = [(i, part, tag) for i in range(M) for part, tag in ((1, 'a'), (2, 'b'))]
        for i, part, tag in todo:
            N.check(N.lib.rfn_prefix_bwd_wgrad(C.byref(d), B, att_ptrs, gtable, ws.data_ptr(), ws_bytes, i,
                                               part, N.stream_ptr()), 'rfn_prefix_bwd_wgrad')
            model._bucket_done('enc%d%s' % (i, tag), flats['enc%d%s' % (i, tag)])
        # gradients of the features that asked for one (rfn_prefix_bwd_inputs reads dP1, the attention rows, the d z slices
        # and d h0 / d c0 out of the workspace; no buffer, no launch for the others)
        d_in = [None] * (2 * M)
        if ctx.input_grads:
            feats = ctx.fc + ctx.att
            for j, need in enumerate(ctx.needs_input_grad[6:6 + 2 * M]):
                if need:
                    d_in[j] = torch.empty_like(feats[j])
            N.check(N.lib.rfn_prefix_bwd_inputs(C.byref(d), B, table, N.ptr_array(d_in[:M]), N.ptr_array(d_in[M:]), ws.data_ptr(),
                                                ws_bytes, len_ptrs, N.stream_ptr()), 'rfn_prefix_bwd_inputs')
        return (None, None, None, None, None, None) + tuple(d_in) + (None,) * len(ctx.params)


class _DecoderFn(torch.autograd.Function):
    """Phase 2 (decoder + logit + log-softmax): rfn_decoder_fwd / rfn_decoder_bwd.

    ss_prob > 0 (scheduled sampling, misc/RecurrentFusionModel.py:260-270): the pass runs one step at a time
    (rfn_decoder_fwd_begin / rfn_decoder_fwd_step) and, between steps, replaces a row's next input token with
    probability ss_prob by a draw from the distribution the step just produced.  The step-wise pass leaves the
    workspace exactly as the batched pass on the final ids would (bit for bit), so backward is the same call: the pass
    that is sampled IS the pass that is differentiated -- dropout masks included -- and nothing is computed twice.  No
    host read-back: the draw is made for every row and kept where the row's coin says so.

    n > 1 (rfn.h "multi-sample self-critical"): the B rows are n draws per image, image-major; comb and its gradient are
    (T2, B / n, R), h0 / c0 stay per row.  n = 1 is the calls and the bits of the plain entry points, which forward to these."""

    @staticmethod
    def forward(ctx, model, save_bwd, drop, seed, ids, comb, h0, c0, ss_prob, inv_temp, n, *params):
        d = model._dims_for(drop)
        train = bool(save_bwd)
        B, S = ids.shape
        dev = comb.device
        n = int(n)
        if n < 1 or B % n or comb.size(1) * n != B or h0.size(0) != B or c0.size(0) != B:
            raise N.RfnError('%d decoder rows, %d rows per image: comb holds %d images, h0 / c0 %d / %d rows'
                             % (B, n, comb.size(1), h0.size(0), c0.size(0)))
        comb, h0, c0 = comb.contiguous(), h0.contiguous(), c0.contiguous()
        ids = ids.contiguous()
        table = model._param_table(params, model._decoder_slots)
        ws_bytes = N.lib.rfn_decoder_ws_bytes_ex(C.byref(d), B, S, int(train), n)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        log_prob = torch.empty(B, S, d.V1, device=dev)
        if ss_prob > 0.0 and S > 1:
            ids = ids.clone()
            # one call queues begin + S x (draw, step): the host is off the critical path (uniforms drawn up front)
            r = getattr(model, '_ss_uniforms', None)      # a captured step reads the buffer its owner refills (graphed.py)
            if r is None:
                r = torch.rand(2, S, B, device=dev)
            elif tuple(r.shape) != (2, S, B) or r.device != dev:
                raise N.RfnError('scheduled-sampling uniforms are %s, this pass needs %s' % (tuple(r.shape), (2, S, B)))
            N.check(N.lib.rfn_decoder_fwd_sampled_ex(C.byref(d), B, S, table, comb.data_ptr(), h0.data_ptr(), c0.data_ptr(),
                                                     ids.data_ptr(), ids.stride(0), float(ss_prob), float(inv_temp),
                                                     r[0].data_ptr(), r[1].data_ptr(), log_prob.data_ptr(), ws.data_ptr(),
                                                     ws_bytes, int(train), seed, n, N.stream_ptr()), 'rfn_decoder_fwd_sampled')
            if getattr(model, '_trace_ss', False):
                model._ss_ids = ids.clone()      # test hook: the token matrix the pass ended up feeding
        else:
            N.check(N.lib.rfn_decoder_fwd_ex(C.byref(d), B, S, table, comb.data_ptr(), h0.data_ptr(), c0.data_ptr(),
                                             ids.data_ptr(), ids.stride(0), log_prob.data_ptr(), ws.data_ptr(), ws_bytes,
                                             int(train), seed, n, N.stream_ptr()), 'rfn_decoder_fwd')
        if train:
            ctx.model, ctx.seed, ctx.B, ctx.S, ctx.drop, ctx.n = model, seed, B, S, drop, n
            ctx.ids, ctx.params, ctx.consumed, ctx.snapshot = ids, params, False, None
            ctx.save_for_backward(comb, h0, c0, log_prob, ws)     # ws: freed with the graph (see _PrefixFn.forward)
        ctx.mark_non_differentiable(ids)
        return log_prob, ids

    @staticmethod
    def backward(ctx, d_log_prob, _d_ids=None):
        model, B, S = ctx.model, ctx.B, ctx.S
        comb, h0, c0, log_prob, ws = ctx.saved_tensors
        d = model._dims_for(ctx.drop)
        dev = comb.device
        table = model._param_table(ctx.params, model._decoder_slots)
        flats, by_slot, gtable = model._grad_buffers(['decoder'], dev)
        d_log_prob = d_log_prob.contiguous()
        d_comb = torch.empty_like(comb)
        d_h0 = torch.empty_like(h0)
        d_c0 = torch.empty_like(c0)
        if ctx.consumed and ctx.snapshot is not None:
            ws.data.copy_(ctx.snapshot)          # .data: no version bump on a saved tensor (see _PrefixFn.backward)
        elif ctx.consumed:
            # second backward over the same graph: recompute phase 2 first (see _PrefixFn.backward), log-probs included,
            # so the pass differentiated is self-consistent at the current weights
            log_prob = torch.empty_like(log_prob)
            N.check(N.lib.rfn_decoder_fwd_ex(C.byref(d), B, S, table, comb.data_ptr(), h0.data_ptr(), c0.data_ptr(),
                                             ctx.ids.data_ptr(), ctx.ids.stride(0), log_prob.data_ptr(),
                                             ws.data_ptr(), ws.numel(), 1, ctx.seed, ctx.n, N.stream_ptr()),
                    'rfn_decoder_fwd (recompute)')
        elif getattr(model, 'retain_activations', False):
            ctx.snapshot = ws.clone()
        ctx.consumed = True
        N.check(N.lib.rfn_decoder_bwd_ex(C.byref(d), B, S, table, comb.data_ptr(), h0.data_ptr(), c0.data_ptr(),
                                         ctx.ids.data_ptr(), ctx.ids.stride(0), log_prob.data_ptr(),
                                         d_log_prob.data_ptr(), d_comb.data_ptr(), d_h0.data_ptr(), d_c0.data_ptr(),
                                         gtable, ws.data_ptr(), ws.numel(), ctx.seed, ctx.n, N.stream_ptr()),
                'rfn_decoder_bwd')
        model._bucket_done('decoder', flats['decoder'])
        return (None, None, None, None, None, d_comb, d_h0, d_c0, None, None, None) + (None,) * len(ctx.params)


class _DecoderLossFn(torch.autograd.Function):
    """Phase 2 + the language term of the XE criterion as ONE autograd node: rfn_decoder_fwd stops at the
    logits (time-major rows in the workspace), rfn_xe_logits_fwd turns them into the masked (label-smoothed) NLL and the rows'
    logsumexps; backward writes d logits over the logits (rfn_xe_logits_bwd, scaled by the upstream gradient read on the
    device) and rfn_decoder_bwd runs from there.  Neither log_prob (B, S, V+1) nor its gradient is ever materialised
    (misc/RecurrentFusionModel.py:276 + misc/utils.py:163-184).

    `kd` = None, or (teacher (B, >= S, V+1) f32 with unit stride in the last dimension, alpha, inv_temp) for distillation:
    rfn_kd_logits_fwd / _bwd take the place of the XE pair (rfn.h: loss = (1 - alpha) * xe + alpha * kd), the node keeps the
    rows' three logsumexps, and `terms` (2 floats, {xe, kd}) is filled for logging.  The teacher is a constant: it is held
    by the node as it is, outside autograd's saved tensors.  A distill.TopKTeacher in the teacher's place (K <= 32 (id, value)
    pairs per row) goes to rfn_kd_topk_fwd / _bwd, with the same statistics and terms."""

    @staticmethod
    def _criterion_fwd(d, B, S, logits, target, mask, eps, kd, stats, scratch, loss, terms, st):
        if kd is None:
            N.check(N.lib.rfn_xe_logits_fwd(logits, d.V1, B, S, d.V1, target.data_ptr(), target.stride(0), mask.data_ptr(),
                                            mask.stride(0), float(eps), stats.data_ptr(), scratch.data_ptr(), loss.data_ptr(), 0, st),
                    'rfn_xe_logits_fwd')
        else:
            z, alpha, it = kd
            if isinstance(z, TopKTeacher):
                N.check(N.lib.rfn_kd_topk_fwd(logits, d.V1, B, S, d.V1, target.data_ptr(), target.stride(0), mask.data_ptr(),
                                              mask.stride(0), float(eps), *z._abi(), alpha, it, stats.data_ptr(), scratch.data_ptr(),
                                              loss.data_ptr(), 0, N.ptr(terms), st), 'rfn_kd_topk_fwd')
                return
            N.check(N.lib.rfn_kd_logits_fwd(logits, d.V1, B, S, d.V1, target.data_ptr(), target.stride(0), mask.data_ptr(),
                                            mask.stride(0), float(eps), z.data_ptr(), z.stride(0), z.stride(1), alpha, it,
                                            stats.data_ptr(), scratch.data_ptr(), loss.data_ptr(), 0, N.ptr(terms), st),
                    'rfn_kd_logits_fwd')

    @staticmethod
    def forward(ctx, model, save_bwd, drop, seed, ids, target, mask, eps, kd, terms, comb, h0, c0, *params):
        d = model._dims_for(drop)
        B, S = ids.shape
        dev = comb.device
        comb, h0, c0, ids = comb.contiguous(), h0.contiguous(), c0.contiguous(), ids.contiguous()
        table = model._param_table(params, model._decoder_slots)
        train = bool(save_bwd)
        ws_bytes = N.lib.rfn_decoder_ws_bytes(C.byref(d), B, S, int(train))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        st = N.stream_ptr()
        N.check(N.lib.rfn_decoder_fwd(C.byref(d), B, S, table, comb.data_ptr(), h0.data_ptr(), c0.data_ptr(), ids.data_ptr(),
                                      ids.stride(0), None, ws.data_ptr(), ws_bytes, int(train), seed, st), 'rfn_decoder_fwd')
        logits = N.lib.rfn_decoder_logits(C.byref(d), B, S, int(train), ws.data_ptr())
        nk = 1 if kd is None else 3                  # row statistics / scratch arrays per row (rfn.h)
        lse = torch.empty(nk * S * B, device=dev)
        scratch = torch.empty(min(nk, 2) * B * S, device=dev)
        loss = torch.zeros(1, device=dev)
        _DecoderLossFn._criterion_fwd(d, B, S, logits, target, mask, eps, kd, lse, scratch, loss, terms, st)
        if train:
            ctx.model, ctx.seed, ctx.B, ctx.S, ctx.drop, ctx.eps = model, seed, B, S, drop, float(eps)
            ctx.ids, ctx.target, ctx.mask, ctx.params, ctx.consumed, ctx.kd = ids, target, mask, params, False, kd
            ctx.save_for_backward(comb, h0, c0, lse, ws)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        model, B, S, kd = ctx.model, ctx.B, ctx.S, ctx.kd
        comb, h0, c0, lse, ws = ctx.saved_tensors
        d = model._dims_for(ctx.drop)
        dev = comb.device
        st = N.stream_ptr()
        table = model._param_table(ctx.params, model._decoder_slots)
        flats, by_slot, gtable = model._grad_buffers(['decoder'], dev)
        if ctx.consumed:
            # the first backward turned the logits into their gradient and the activations into theirs: a second backward over
            # the same graph recomputes the pass first (same inputs, same dropout seed, the weights as they are now)
            N.check(N.lib.rfn_decoder_fwd(C.byref(d), B, S, table, comb.data_ptr(), h0.data_ptr(), c0.data_ptr(),
                                          ctx.ids.data_ptr(), ctx.ids.stride(0), None, ws.data_ptr(), ws.numel(), 1, ctx.seed, st),
                    'rfn_decoder_fwd (recompute)')
            lse = torch.empty_like(lse)
            tmp, junk = torch.empty((1 if kd is None else 2) * B * S, device=dev), torch.zeros(1, device=dev)
            _DecoderLossFn._criterion_fwd(d, B, S, N.lib.rfn_decoder_logits(C.byref(d), B, S, 1, ws.data_ptr()), ctx.target,
                                          ctx.mask, ctx.eps, kd, lse, tmp, junk, None, st)
        ctx.consumed = True
        g = g.contiguous().float()
        logits = N.lib.rfn_decoder_logits(C.byref(d), B, S, 1, ws.data_ptr())
        if kd is None:
            N.check(N.lib.rfn_xe_logits_bwd(logits, d.V1, B, S, d.V1, ctx.target.data_ptr(), ctx.target.stride(0),
                                            ctx.mask.data_ptr(), ctx.mask.stride(0), ctx.eps, lse.data_ptr(), 1.0, g.data_ptr(), st),
                    'rfn_xe_logits_bwd')
        else:
            z, alpha, it = kd
            if isinstance(z, TopKTeacher):
                N.check(N.lib.rfn_kd_topk_bwd(logits, d.V1, B, S, d.V1, ctx.target.data_ptr(), ctx.target.stride(0),
                                              ctx.mask.data_ptr(), ctx.mask.stride(0), ctx.eps, *z._abi(), alpha, it, lse.data_ptr(),
                                              1.0, g.data_ptr(), st), 'rfn_kd_topk_bwd')
            else:
                N.check(N.lib.rfn_kd_logits_bwd(logits, d.V1, B, S, d.V1, ctx.target.data_ptr(), ctx.target.stride(0),
                                                ctx.mask.data_ptr(), ctx.mask.stride(0), ctx.eps, z.data_ptr(), z.stride(0), z.stride(1),
                                                alpha, it, lse.data_ptr(), 1.0, g.data_ptr(), st), 'rfn_kd_logits_bwd')
        d_comb, d_h0, d_c0 = torch.empty_like(comb), torch.empty_like(h0), torch.empty_like(c0)
        N.check(N.lib.rfn_decoder_bwd(C.byref(d), B, S, table, comb.data_ptr(), h0.data_ptr(), c0.data_ptr(),
                                      ctx.ids.data_ptr(), ctx.ids.stride(0), None, None, d_comb.data_ptr(), d_h0.data_ptr(),
                                      d_c0.data_ptr(), gtable, ws.data_ptr(), ws.numel(), ctx.seed, st), 'rfn_decoder_bwd')
        model._bucket_done('decoder', flats['decoder'])
        return (None,) * 10 + (d_comb, d_h0, d_c0) + (None,) * len(ctx.params)


class _DecoderRLFn(torch.autograd.Function):
    """Phase 2 + the policy and entropy terms of the RL criterion as ONE autograd node, _DecoderLossFn's shape with n rows per
    image: rfn_decoder_logits_fwd stops at the time-major logits, rfn_rl_logits_fwd turns them into the loss, the rows' statistics
    and the tokens' log-probs; backward writes d logits over the logits (rfn_rl_logits_bwd, scaled by the upstream gradient read
    on the device) and rfn_decoder_logits_bwd runs from there.  Neither logprobs_all (rows, T, V+1) nor its gradient exists
    (misc/RecurrentFusionModel.py:623-658 replayed teacher-forced + misc/utils.py:50-72).

    `rl` = (seq (B, T) int64, reward (B, T) f32, old_logprobs (B, T) f32 or None, entropy_reg, ppo_clip): constants held by the
    node.  `out`: a dict that receives 'logprobs' (B, T) and 'terms' (2 floats: policy, entropy)."""

    @staticmethod
    def _criterion_fwd(d, B, T, logits, rl, stats, tok_lp, scratch, loss, terms, st):
        seq, reward, old, ent, clip = rl
        N.check(N.lib.rfn_rl_logits_fwd(logits, d.V1, B, T, d.V1, seq.data_ptr(), seq.stride(0), reward.data_ptr(), reward.stride(0),
                                        ent, N.ptr(old), 0 if old is None else old.stride(0), int(old is not None), clip,
                                        stats.data_ptr(), tok_lp.data_ptr(), tok_lp.stride(0), scratch.data_ptr(), loss.data_ptr(), 0,
                                        N.ptr(terms), st), 'rfn_rl_logits_fwd')

    @staticmethod
    def _decoder_fwd(d, B, T, n, table, comb, h0, c0, ids, ws, train, seed, st, what='rfn_decoder_logits_fwd'):
        N.check(N.lib.rfn_decoder_logits_fwd(C.byref(d), B, T, table, comb.data_ptr(), h0.data_ptr(), c0.data_ptr(), ids.data_ptr(),
                                             ids.stride(0), ws.data_ptr(), ws.numel(), int(train), seed, n, st), what)
        return N.lib.rfn_decoder_logits_ex(C.byref(d), B, T, int(train), n, ws.data_ptr())

    @staticmethod
    def forward(ctx, model, save_bwd, drop, seed, ids, rl, n, out, comb, h0, c0, *params):
        d = model._dims_for(drop)
        B, T = ids.shape
        dev = comb.device
        comb, h0, c0, ids = comb.contiguous(), h0.contiguous(), c0.contiguous(), ids.contiguous()
        table = model._param_table(params, model._decoder_slots)
        train = bool(save_bwd)
        ws = torch.empty(N.lib.rfn_decoder_ws_bytes_ex(C.byref(d), B, T, int(train), n), dtype=torch.uint8, device=dev)
        st = N.stream_ptr()
        logits = _DecoderRLFn._decoder_fwd(d, B, T, n, table, comb, h0, c0, ids, ws, train, seed, st)
        stats = torch.empty(3 * T * B, device=dev)
        tok_lp = torch.empty(B, T, device=dev)
        terms = torch.empty(2, device=dev)
        loss = torch.zeros(1, device=dev)
        _DecoderRLFn._criterion_fwd(d, B, T, logits, rl, stats, tok_lp, torch.empty(3 * B * T, device=dev), loss, terms, st)
        out['logprobs'], out['terms'] = tok_lp, terms
        if train:
            ctx.model, ctx.seed, ctx.B, ctx.T, ctx.drop, ctx.n = model, seed, B, T, drop, n
            ctx.ids, ctx.rl, ctx.params, ctx.consumed = ids, rl, params, False
            ctx.save_for_backward(comb, h0, c0, stats, ws)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        model, B, T, n = ctx.model, ctx.B, ctx.T, ctx.n
        comb, h0, c0, stats, ws = ctx.saved_tensors
        seq, reward, old, ent, clip = ctx.rl
        d = model._dims_for(ctx.drop)
        dev = comb.device
        st = N.stream_ptr()
        table = model._param_table(ctx.params, model._decoder_slots)
        flats, by_slot, gtable = model._grad_buffers(['decoder'], dev)
        if ctx.consumed:
            # the first backward turned the logits into their gradient and the activations into theirs: a second backward over
            # the same graph recomputes the pass first (same inputs, same dropout seed, the weights as they are now)
            logits = _DecoderRLFn._decoder_fwd(d, B, T, n, table, comb, h0, c0, ctx.ids, ws, True, ctx.seed, st,
                                               'rfn_decoder_logits_fwd (recompute)')
            stats = torch.empty_like(stats)
            _DecoderRLFn._criterion_fwd(d, B, T, logits, ctx.rl, stats, torch.empty(B, T, device=dev), torch.empty(B * T, device=dev),
                                        torch.zeros(1, device=dev), None, st)
        ctx.consumed = True
        g = g.contiguous().float()
        logits = N.lib.rfn_decoder_logits_ex(C.byref(d), B, T, 1, n, ws.data_ptr())
        N.check(N.lib.rfn_rl_logits_bwd(logits, d.V1, B, T, d.V1, seq.data_ptr(), seq.stride(0), reward.data_ptr(), reward.stride(0),
                                        ent, N.ptr(old), 0 if old is None else old.stride(0), int(old is not None), clip,
                                        stats.data_ptr(), 1.0, g.data_ptr(), st), 'rfn_rl_logits_bwd')
        d_comb, d_h0, d_c0 = torch.empty_like(comb), torch.empty_like(h0), torch.empty_like(c0)
        N.check(N.lib.rfn_decoder_logits_bwd(C.byref(d), B, T, table, comb.data_ptr(), ctx.ids.data_ptr(), ctx.ids.stride(0),
                                             d_comb.data_ptr(), d_h0.data_ptr(), d_c0.data_ptr(), gtable, ws.data_ptr(), ws.numel(),
                                             ctx.seed, n, st), 'rfn_decoder_logits_bwd')
        model._bucket_done('decoder', flats['decoder'])
        return (None,) * 8 + (d_comb, d_h0, d_c0) + (None,) * len(ctx.params)


class _HiddenFn(torch.autograd.Function):
    """Phase 2 without its output layer, for a model whose head is a mixture of softmaxes (rfn.h "mixture of softmaxes"):
    rfn_decoder_fwd_hidden -> the (S * B, R) time-major rows the logit layer would read (a copy: the head's node keeps them);
    backward runs rfn_decoder_bwd_hidden from the head's d hidden.  The logit.* gradient slots of the decoder bucket are
    zero-filled: `logit` stays in the model, unused, as in the reference (misc/ReviewNetModel.py:59-60)."""

    @staticmethod
    def _run(model, d, B, S, table, comb, h0, c0, ids, ws, train, seed):
        N.check(N.lib.rfn_decoder_fwd_hidden(C.byref(d), B, S, table, comb.data_ptr(), h0.data_ptr(), c0.data_ptr(),
                                             ids.data_ptr(), ids.stride(0), ws.data_ptr(), ws.numel(), int(train), seed,
                                             N.stream_ptr()), 'rfn_decoder_fwd_hidden')

    @staticmethod
    def forward(ctx, model, save_bwd, drop, seed, ids, comb, h0, c0, *params):
        d = model._dims_for(drop)
        train = bool(save_bwd)
        B, S = ids.shape
        dev = comb.device
        comb, h0, c0, ids = comb.contiguous(), h0.contiguous(), c0.contiguous(), ids.contiguous()
        table = model._param_table(params, model._decoder_slots)
        ws = torch.empty(N.lib.rfn_decoder_ws_bytes(C.byref(d), B, S, int(train)), dtype=torch.uint8, device=dev)
        _HiddenFn._run(model, d, B, S, table, comb, h0, c0, ids, ws, train, seed)
        off = N.lib.rfn_decoder_hidden(C.byref(d), B, S, int(train), ws.data_ptr()) - ws.data_ptr()
        hidden = ws[off:off + 4 * S * B * d.R].view(torch.float32).view(S * B, d.R).clone()
        if train:
            ctx.model, ctx.seed, ctx.B, ctx.S, ctx.drop = model, seed, B, S, drop
            ctx.ids, ctx.params, ctx.consumed = ids, params, False
            ctx.save_for_backward(comb, h0, c0, ws)
        return hidden

    @staticmethod
    def backward(ctx, d_hidden):
        model, B, S = ctx.model, ctx.B, ctx.S
        comb, h0, c0, ws = ctx.saved_tensors
        d = model._dims_for(ctx.drop)
        dev = comb.device
        table = model._param_table(ctx.params, model._decoder_slots)
        flats, by_slot, gtable = model._grad_buffers(['decoder'], dev)
        if ctx.consumed:      # a second backward over the same graph: recompute the pass first (see _PrefixFn.backward)
            _HiddenFn._run(model, d, B, S, table, comb, h0, c0, ctx.ids, ws, True, ctx.seed)
        ctx.consumed = True
        d_hidden = d_hidden.contiguous()
        d_comb, d_h0, d_c0 = torch.empty_like(comb), torch.empty_like(h0), torch.empty_like(c0)
        N.check(N.lib.rfn_decoder_bwd_hidden(C.byref(d), B, S, table, comb.data_ptr(), h0.data_ptr(), c0.data_ptr(),
                                             ctx.ids.data_ptr(), ctx.ids.stride(0), d_hidden.data_ptr(), d_comb.data_ptr(),
                                             d_h0.data_ptr(), d_c0.data_ptr(), gtable, ws.data_ptr(), ws.numel(), ctx.seed,
                                             N.stream_ptr()), 'rfn_decoder_bwd_hidden')
        model._bucket_done('decoder', flats['decoder'])
        return (None, None, None, None, None, d_comb, d_h0, d_c0) + (None,) * len(ctx.params)


class _MosBucketGrads:
    """Gradient sink of the model's head (mos._MosFn): the flat 'mos' bucket, handed over like every other bucket."""

    def __init__(self, model):
        self.model = model

    def buffers(self, dev):
        self.flats, by_slot, _ = self.model._grad_buffers(['mos'], dev)
        return [by_slot[s] for s in self.model._mos_slots]

    def done(self):
        self.model._bucket_done('mos', self.flats['mos'])
        return (None,) * len(self.model._mos_slots)


class RecurrentFusionModel(nn.Module):
    def __init__(self, opt):
        super().__init__()
        # the fields the reference reads (misc/RecurrentFusionModel.py:120-151)
        self.vocab_size = opt.vocab_size
        self.input_encoding_size = opt.input_encoding_size
        self.rnn_type = getattr(opt, 'rnn_type', 'lstm')
        self.rnn_size = opt.rnn_size
        self.num_layers = getattr(opt, 'num_layers', 1)
        self.drop_prob_lm = opt.drop_prob_lm
        self.drop_prob_reason = opt.drop_prob_reason
        self.drop_prob_fusion = opt.drop_prob_fusion
        self.seq_length = opt.seq_length
        self.num_review_steps = opt.num_review_steps
        self.num_review_steps_0 = opt.num_review_steps_0
        self.top_words_count = opt.top_words_count
        self.att_hid_size = opt.att_hid_size
        self.ss_prob = 0.0
        self.review_maxout = opt.review_maxout
        self.decoder_maxout = opt.maxout
        self.fusion_maxout = opt.fusion_maxout  # accepted and ignored, exactly like the reference (:94-96)
        self.use_cuda = getattr(opt, 'use_cuda', 1)
        self.feat_array_info = opt.feat_array_info
        M = self.num_feat_array = len(self.feat_array_info)
        self.fc_feat_size = [f['fc_feat_size'] for f in self.feat_array_info]
        self.att_feat_size = [f['att_feat_size'] for f in self.feat_array_info]
        self.att_num = [f['att_num'] for f in self.feat_array_info]
        R, A, E = self.rnn_size, self.att_hid_size, self.input_encoding_size

        self.fc2h = nn.ModuleList([nn.Linear(self.fc_feat_size[i], R) for i in range(M)])
        self.embed = nn.Embedding(self.vocab_size + 1, E)
        self.logit = nn.Linear(R, self.vocab_size + 1)
        self.review_steps_individual = nn.ModuleList(
            [_FusionStepParams(M, R, self.att_feat_size, A) for _ in range(self.num_review_steps_0)])
        self.reason_linear_individual = nn.ModuleList([nn.Linear(R, self.top_words_count) for _ in range(M)])
        self.review_steps = nn.ModuleList([_ReviewStepParams(M, R, A, self.review_maxout)
                                           for _ in range(self.num_review_steps)])
        self.reason_linear = nn.Linear(R, self.top_words_count)
        self.decoder = _DecoderParams(E, R, A, self.decoder_maxout)
        # opts.py --use_mos / --num_expert: a mixture-of-softmaxes head in place of log_softmax(logit(h)); `logit` stays,
        # unused, as in the reference (misc/ReviewNetModel.py:59-60,122-125)
        self.use_mos = int(getattr(opt, 'use_mos', 0) or 0)
        if self.use_mos:
            self.num_expert = int(getattr(opt, 'num_expert', 10))
            self.mos = MixtureOfSoftmax(R, R, self.num_expert, self.vocab_size + 1)
        self.init_weights()

        # RFN_GEMM_OPT_* bits handed to every GEMM of the path (rfn.h); a data-parallel host sets
        # N.GEMM_OPT_LDS_LEAN so RCCL's kernels can co-reside with the long weight-gradient GEMMs (parallel.GradSync does)
        self.gemm_flags = 0
        self.path_flags = 0              # RFN_PATH_OPT_* bits (rfn.h); 0 = defaults
        self._probe = None
        self._dims = {}
        self._param_cache = {}
        self._slot_names = N.param_names(self._dims_for(False))
        # the head's parameters follow the path's slots (the path's tables are indexed by slot and never read beyond their own)
        self._mos_slots = []
        if self.use_mos:
            self._mos_slots = list(range(len(self._slot_names), len(self._slot_names) + len(self.mos.slot_names)))
            self._slot_names = self._slot_names + ['mos.' + n for n in self.mos.slot_names]
        schema = dict(self.named_parameters())
        missing = [n for n in self._slot_names if n not in schema]
        if missing or len(schema) != len(self._slot_names):
            raise N.RfnError('parameter schema mismatch between module and librfn_hip.so: %s' % missing[:3])
        is_dec = lambda n: n.startswith(('embed.', 'logit.', 'decoder.'))  # noqa: E731
        self._prefix_slots = [i for i, n in enumerate(self._slot_names) if not is_dec(n) and not n.startswith('mos.')]
        self._decoder_slots = [i for i, n in enumerate(self._slot_names) if is_dec(n)]
        # gradient buckets, in the order their gradients become final during backward: the decoder, the
        # fusion "core" (everything of phase 1 except the per-encoder stage-I weights) and two buckets per
        # encoder (rfn_prefix_bwd_wgrad parts 1 and 2; all a-buckets are produced before the first b-bucket).  Each bucket is one flat buffer = one all-reduce = one Adam launch.
        enc_re = re.compile(r'^review_steps_individual\.\d+\.lstm\.(\d+)\.(att_model\.att_2_att_h|att_model\.h_2_att_h|H2h|z2h)\.')
        self._bucket_slots = {'decoder': list(self._decoder_slots), 'core': []}
        if self.use_mos:
            self._bucket_slots['mos'] = list(self._mos_slots)    # the head's bucket: final before the decoder's
        for i in range(M):
            self._bucket_slots['enc%da' % i] = []    # H2h, z2h, h_2_att_h of encoder i (rfn_prefix_bwd_wgrad part 1)
            self._bucket_slots['enc%db' % i] = []    # att_2_att_h of encoder i            (part 2)
        for idx in self._prefix_slots:
            m = enc_re.match(self._slot_names[idx])
            if not m:
                self._bucket_slots['core'].append(idx)
            else:
                self._bucket_slots['enc%s%s' % (m.group(1), 'b' if 'att_2_att_h' in m.group(2) else 'a')].append(idx)
        self._prefix_buckets = ['core'] + ['enc%da' % i for i in range(M)] + ['enc%db' % i for i in range(M)]   # production order
        self.grad_ready_hook = None      # callable(bucket_name, flat_grad_tensor), see parallel.GradSync
        # callable('prefix' | 'decoder'): called right before the parameters of that phase are handed to a kernel.  A
        # sharded optimizer (FusedClampAdam(shard=...)) waits there for the all-gather of the parameters it updated.
        self.param_wait_hook = None
        # state_dict() (the reference's checkpoint pattern right after optimizer.step(), train.py:226-233) must not read
        # parameters an asynchronous update is still writing: join first
        self.register_state_dict_pre_hook(_join_before_state_dict)
        # flat buckets (gradients, and the optimizer's parameter / moment buffers) are padded to a multiple of this many
        # elements: 4 * world_size under a sharded optimizer, so every rank's shard is the same 16-B aligned length
        self.flat_pad = 1
        # Opt-in: real batches hold each image's features `seq_per_img` times in a row (dataloader.py:251-252).
        # With this set to that count, stages I/II run once per image and their outputs are fanned out to the
        # caption rows (exactly the same numbers: rows are independent); only legal while drop_prob_fusion and
        # drop_prob_reason are 0, which forward() checks.
        self.dedup_seq_per_img = 0
        # Opt-in: the self-critical loop samples twice from the same batch (train_rl.py:160-166: a multinomial sample
        # with grad, then the greedy baseline under no_grad).  With this set, a no-grad call whose input tensors are
        # the very same objects (unchanged `_version`) as the previous call's, with unchanged weights and no active
        # dropout, reuses that call's stage-I/II outputs instead of recomputing them.
        self.reuse_prefix = False
        # Opt-in for loops that call loss.backward(retain_graph=True) repeatedly with optimizer steps in between (PPO,
        # train_rl.py:190-201): keep a copy of the activations backward consumes, so later passes differentiate the
        # ORIGINAL forward's activations through the current weights, as the reference does.  Off: they are recomputed
        # at the current weights.
        self.retain_activations = False
        self._prefix_cache = None
        self._weights_epoch = 0          # bumped by FusedClampAdam.step (it writes parameters behind autograd's back)
        self._last_flat_grads = {}
        self._steps_cache = None
        self.last_distill = None         # forward_loss with a teacher: {'xe', 'kd'}, the two loss terms as 0-dim device tensors
        self.last_rl = None              # rl_loss: {'logprobs' (rows, T), 'policy', 'entropy'} (device tensors)
        # set by graphed.GraphedTrainStep while it captures / warms up: run exactly this many decoder steps instead of
        # stopping at the first all-zero label column (the loader's masks are zero on the extra steps)
        self.fixed_decoder_steps = None
        # set by graphed.GraphedTrainStep(device_rng=True) while its step runs: a one-element int64 device tensor holding the
        # dropout seed (the kernels read it when they run: RFN_PATH_OPT_SEED_DEV, rfn.h) and the (2, S, B) scheduled-sampling
        # uniforms; None = a fresh seed and fresh uniforms per forward, drawn here
        self._seed_dev = None
        self._ss_uniforms = None
        self.done_beams = []
        self.diverse_beams = None       # sample_beam with group_size > 1: per image the G group bests
        self.consensus = None           # sample / sample_beam with opt['consensus']: {'index', 'scores'} of the pick (device)
        self.candidates = None          # sample_beam with opt['keep_candidates']: {'seq' (B, m, S), 'n_cand' (B,)} (device)
        self.lexical_met = None         # sample_beam with opt['require']: (B,) int32, the non-empty sets the caption satisfies (device)

    def init_weights(self):
        """misc/RecurrentFusionModel.py:188-196."""
        _uniform(self.embed.weight, self.logit.weight, self.reason_linear.weight)
        self.logit.bias.data.fill_(0)
        for i in range(self.num_feat_array):
            _uniform(self.reason_linear_individual[i].weight, self.fc2h[i].weight)

    # ---- plumbing -------------------------------------------------------------------------------
    def set_probe_events(self, events):
        """Measurement hook (rfn.h rfn_dims.probe_events): 4*M `torch.cuda.Event(enable_timing=True)` objects that the path
        records around its dominant launches -- [2i], [2i+1] encoder i's hoisted projection (forward), [2M+2i], [2M+2i+1] its
        att_2_att_h weight gradient (backward) -- or None to switch the hook off.  The events must have been recorded once
        (that is when PyTorch creates the HIP event behind them); the caller keeps them alive while the hook is set."""
        if events is None:
            self._probe = None
            return
        if len(events) != 4 * self.num_feat_array:
            raise N.RfnError('set_probe_events: expected %d events' % (4 * self.num_feat_array))
        arr = (C.c_void_p * len(events))(*[int(e.cuda_event) for e in events])
        self._probe = (arr, list(events))

    def _dims_for(self, train: bool, input_grads: bool = False) -> N.Dims:
        """`input_grads`: phase 1 of a pass whose fc_feats / att_feats require grad (RFN_PATH_OPT_INPUT_GRADS)."""
        d = self._dims_cached(train, input_grads)
        probe = getattr(self, '_probe', None)
        d.probe_events = C.cast(probe[0], C.c_void_p) if probe is not None else None
        return d

    def _dims_cached(self, train: bool, input_grads: bool = False) -> N.Dims:
        path_flags = int(self.path_flags) | (N.PATH_OPT_SEED_DEV if getattr(self, '_seed_dev', None) is not None else 0)
        if input_grads:
            path_flags |= N.PATH_OPT_INPUT_GRADS
        key = (bool(train), int(self.gemm_flags), path_flags)
        if key not in self._dims:
            self._dims[key] = N.make_dims(
                self.num_feat_array, self.rnn_size, self.att_hid_size, self.input_encoding_size,
                self.num_review_steps_0, self.num_review_steps, self.top_words_count, self.vocab_size + 1,
                self.att_num, self.att_feat_size, self.fc_feat_size,
                review_maxout=self.review_maxout, decoder_maxout=self.decoder_maxout,
                drop_fusion=self.drop_prob_fusion if train else 0.0,
                drop_reason=self.drop_prob_reason if train else 0.0,
                drop_lm=self.drop_prob_lm if train else 0.0, gemm_flags=self.gemm_flags, path_flags=path_flags)
        return self._dims[key]

    def _params_of(self, slots):
        """The parameters of a phase, about to be handed to its kernels: the one place the compute stream meets an
        asynchronous update of them again (`param_wait_hook`: a sharded optimizer's all-gathers, an overlapped update's side
        stream).  Forward entry points only -- bookkeeping that merely needs the parameter OBJECTS (bucket layouts, gradient
        views) uses `_params_lookup` and waits for nothing (the hook used to fire from inside backward)."""
        if self.param_wait_hook is not None:
            self.param_wait_hook('decoder' if slots is self._decoder_slots else 'prefix')
        return self._params_lookup(slots)

    def _params_lookup(self, slots):
        # Parameter objects are stable under .cuda()/.to() (their .data is swapped in place), so the
        # by-name lookup is done once per slot list
        key = id(slots)
        if key not in self._param_cache:
            named = dict(self.named_parameters())
            self._param_cache[key] = [named[self._slot_names[i]] for i in slots]
        return self._param_cache[key]

    def _param_table(self, params, slots):
        table = (C.c_void_p * len(self._slot_names))()
        for p, i in zip(params, slots):
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise N.RfnError('parameter %s must be a contiguous float32 GPU tensor' % self._slot_names[i])
            table[i] = p.data_ptr()
        return table

    def bucket_names(self):
        return (['mos'] if self.use_mos else []) + ['decoder'] + list(self._prefix_buckets)

    def bucket_layout(self, name):
        """(params, offsets, total) of one bucket: parameters back to back, each start 16-B aligned."""
        params = self._params_lookup(self._bucket_slots[name])
        offs, total = [], 0
        for p in params:
            offs.append(total)
            total += (p.numel() + 3) & ~3
        pad = max(1, int(self.flat_pad))
        return params, offs, -(-total // pad) * pad

    def _grad_buffers(self, buckets, dev):
        """One flat gradient buffer per bucket; returns ({name: flat}, {slot: view}, pointer table)."""
        flats, by_slot = {}, {}
        table = (C.c_void_p * len(self._slot_names))()
        for name in buckets:
            params, offs, total = self.bucket_layout(name)
            flat = torch.empty(total, device=dev, dtype=torch.float32)
            if self.flat_pad > 1:       # the shard padding behind the last parameter is exchanged and updated like data
                flat[offs[-1] + params[-1].numel():].zero_()
            flats[name] = flat
            for slot, p, o in zip(self._bucket_slots[name], params, offs):
                v = flat[o:o + p.numel()].view_as(p)
                by_slot[slot] = v
                table[slot] = v.data_ptr()
        return flats, by_slot, table

    def _bucket_done(self, name, flat):
        """Backward has queued every kernel that writes bucket `name`: hand its gradients over.

        `.grad` of the bucket's parameters become VIEWS of the flat buffer, so `.grad`, the all-reduce operand and the
        fused optimizer's operand are the same memory (returning the gradients through autograd instead makes
        AccumulateGrad clone most of them: hundreds of small D2D copies per step).  A second backward before
        zero_grad() accumulates into the buffer already registered -- as autograd would -- so the optimizer operand
        always equals `.grad`."""
        params, offs, _ = self.bucket_layout(name)
        live = self._last_flat_grads.get(name)
        first = next((i for i, p in enumerate(params) if p.requires_grad), None)
        if (live is not None and first is not None and params[first].grad is not None
                and params[first].grad.data_ptr() == live.data_ptr() + 4 * offs[first]):
            if self.grad_ready_hook is not None:
                raise N.RfnError('bucket %s was produced twice before zero_grad(): gradient accumulation over several '
                                 'backward passes cannot be combined with a grad_ready_hook (GradSync all-reduces each '
                                 'bucket once per step)' % name)
            live.add_(flat)
            return
        for p, o in zip(params, offs):
            if not p.requires_grad:
                continue
            v = flat[o:o + p.numel()].view_as(p)
            if p.grad is not None:      # a gradient that did not come from this path (or was never zeroed): fold it in
                v.add_(p.grad)
            p.grad = v
        self._last_flat_grads[name] = flat
        if self.grad_ready_hook is not None:
            self.grad_ready_hook(name, flat)

    def _check_inputs(self, fc_feats, att_feats):
        M = self.num_feat_array
        if len(fc_feats) != M or len(att_feats) != M:
            raise N.RfnError('expected %d fc / att feature tensors' % M)
        B = fc_feats[0].size(0)
        for i in range(M):
            if tuple(fc_feats[i].shape) != (B, self.fc_feat_size[i]):
                raise N.RfnError('fc_feats[%d] has shape %s, expected %s' % (
                    i, tuple(fc_feats[i].shape), (B, self.fc_feat_size[i])))
            if tuple(att_feats[i].shape) != (B, self.att_num[i], self.att_feat_size[i]):
                raise N.RfnError('att_feats[%d] has shape %s, expected %s' % (
                    i, tuple(att_feats[i].shape), (B, self.att_num[i], self.att_feat_size[i])))
        return B

    def _att_lens(self, att_lens, B, dev):
        """The `att_lens` keyword of the entry points (INTEGRATION.md "Ragged attention maps") as _PrefixFn takes it; the forms
        that were not taught lengths are refused by name before anything is launched."""
        lens = N.att_lens_arg(att_lens, self.att_num, B, dev)
        if lens is not None:
            for bit, name in ((N.PATH_OPT_PERSIST_S2_FWD, 'RFN_PATH_OPT_PERSIST_S2_FWD'),
                              (N.PATH_OPT_PERSIST_S2_BWD, 'RFN_PATH_OPT_PERSIST_S2_BWD')):
                if int(self.path_flags) & bit:
                    raise N.RfnError('att_lens: path_flags selects %s, a form that was not taught per-image lengths' % name)
        return lens

    def _check_ragged(self, rc, lens, what):
        if rc == -2 and lens is not None and int(self.gemm_flags) & N.GEMM_OPT_BF16X3:   # RFN_ERR_UNSUPPORTED
            raise N.RfnError('att_lens: gemm_flags selects RFN_GEMM_OPT_BF16X3, whose attention backward writes bf16 planes '
                             '(rfn_attn_bwd_grouped_ks) and was not taught per-image lengths')
        N.check(rc, what)

    def _prefix(self, fc_feats, att_feats, drop, seed, att_lens=None):
        """-> comb (T2,B,R) time-major, h, c (B,R), reason (M+1,B,K).  `drop`: apply dropout (training mode)."""
        B = self._check_inputs(fc_feats, att_feats)
        params = self._params_of(self._prefix_slots)
        lens = self._att_lens(att_lens, B, fc_feats[0].device)
        if (torch.is_grad_enabled() and int(self.gemm_flags) & N.GEMM_OPT_BF16X3
                and any(t.requires_grad for t in list(fc_feats) + list(att_feats))):
            raise N.RfnError('feature gradients: gemm_flags selects RFN_GEMM_OPT_BF16X3, whose attention backward may leave the '
                             'projection gradients as bf16 planes only (rfn_attn_bwd_grouped_ks); fc_feats / att_feats that '
                             'require grad need the exact-f32 path')
        cacheable = self.reuse_prefix and not (drop and (self.drop_prob_fusion > 0 or self.drop_prob_reason > 0)) and lens is None
        if cacheable:
            ins = list(fc_feats) + list(att_feats)
            stamp = (tuple(t._version for t in ins), sum(p._version for p in params), self._weights_epoch)
            hit = self._prefix_cache
            if (hit is not None and not torch.is_grad_enabled() and hit[1] == stamp and len(hit[0]) == len(ins)
                    and all(r() is t for r, t in zip(hit[0], ins))):
                return hit[2]
        out = _PrefixFn.apply(self, torch.is_grad_enabled(), bool(drop), seed, self.num_feat_array, lens, *fc_feats,
                              *att_feats, *params)
        if cacheable:
            # weak references: a dead input invalidates the entry, so a recycled address can never alias it
            self._prefix_cache = ([weakref.ref(t) for t in ins], stamp, tuple(o.detach() for o in out))
        return out

    # ---- mixture-of-softmaxes head (opt.use_mos) ---------------------------------------------------------------------
    def _mos_refuse(self, option, why):
        """What a mixture-of-softmaxes model does not do yet is refused by name, never silently run through the logit layer."""
        if self.use_mos:
            raise ValueError('use_mos: %s is not available for a mixture-of-softmaxes model (%s)' % (option, why))

    def _mos_refuse_path_flags(self):
        bad = int(self.path_flags) & (N.PATH_OPT_PERSIST_ALL | N.PATH_OPT_DEC_UNHOISTED)
        if self.use_mos and bad:
            raise N.RfnError('use_mos: path_flags selects RFN_PATH_OPT_PERSIST_* / RFN_PATH_OPT_DEC_UNHOISTED (bits %d); the '
                             'decoder pass without its output layer takes the hoisted cell only' % bad)

    def _decode_hidden(self, ids, comb, h, c, drop, seed):
        """-> the (S * B, R) time-major rows the output layer reads (rfn_decoder_fwd_hidden), one autograd node."""
        self._mos_refuse_path_flags()
        params = self._params_of(self._decoder_slots)
        return _HiddenFn.apply(self, torch.is_grad_enabled(), bool(drop), seed, ids, comb, h, c, *params)

    def _mos_head(self, hidden, spec):
        params = self._params_of(self._mos_slots)
        return _MosFn.apply(self.mos.md, spec, _MosBucketGrads(self), torch.is_grad_enabled(), hidden, *params)

    @torch.no_grad()
    def decoder_hidden(self, fc_feats, att_feats, seq, att_lens=None):
        """The decoder's outputs on the ground-truth prefix, before any output layer -> (B, S, R), S as forward finds it: the
        rows `logit` (or the mixture-of-softmaxes head) reads, under dropout the dropped-out ones.  A probing utility; runs
        under no_grad in the module's mode."""
        train = bool(self.training)
        seed = self._step_seed(train)
        S = self._decoder_steps(seq)
        comb, h, c, _ = self._prefix(fc_feats, att_feats, train, seed, att_lens)
        dev = comb.device
        hidden = _HiddenFn.apply(self, False, train, seed, seq[:, :S].to(dev).long(), comb, h, c, *self._params_of(self._decoder_slots))
        return hidden.view(S, seq.size(0), self.rnn_size).transpose(0, 1).contiguous()

    def _decode_teacher_forced(self, ids, comb, h, c, drop, seed, ss_prob=0.0, n=1):
        if self.use_mos:
            if ss_prob > 0:
                self._mos_refuse('ss_prob > 0', 'scheduled sampling steps through the logit layer')
            if n != 1:
                self._mos_refuse('n rows per image', 'the pass without its output layer carries one row per image')
            B, S, V1 = ids.size(0), ids.size(1), self.vocab_size + 1
            hidden = self._decode_hidden(ids, comb, h, c, drop, seed)
            return self._mos_head(hidden, {'kind': 'logp', 'shape': (B, S, V1), 'inner': B, 's_inner': S * V1, 's_outer': V1})
        params = self._params_of(self._decoder_slots)
        return _DecoderFn.apply(self, torch.is_grad_enabled(), bool(drop), seed, ids, comb, h, c, float(ss_prob), 1.0, n,
                                *params)[0]

    def _decode_sampled(self, comb, h, c, drop, seed, steps, inv_temp, n=1):
        """Free-running multinomial decode as ONE step-wise pass of the training decoder (every row's next token is
        drawn from the distribution the step just produced): -> (log_prob (B, steps, V+1), ids (B, steps) fed).
        n > 1: h, c hold n rows per image, comb one (rfn.h "multi-sample self-critical")."""
        params = self._params_of(self._decoder_slots)
        ids0 = torch.zeros(h.size(0), steps, dtype=torch.long, device=h.device)     # column 0 = BOS
        return _DecoderFn.apply(self, torch.is_grad_enabled(), bool(drop), seed, ids0, comb, h, c, 1.0, float(inv_temp), n,
                                *params)

    def _step_seed(self, train):
        """The `seed` argument of this forward's native calls (and of its backward): a fresh draw in training mode, or the
        address of the seed tensor a captured step's owner has installed (`_dims_for` then sets RFN_PATH_OPT_SEED_DEV)."""
        held = getattr(self, '_seed_dev', None)
        if held is not None:
            return held.data_ptr()
        return _fresh_seed() if train else 0

    # ---- reference API ----------------------------------------------------------------------------
    def forward(self, fc_feats, att_feats, seq, att_lens=None):
        """misc/RecurrentFusionModel.py:198-281 -> (log_prob (B,T,V+1), reason_pred list[M+1] of (B,K)).

        att_lens (here and on forward_loss, get_thought_vectors, sample, sample_beam, sample_group, sample_distinct, score):
        ragged attention maps -- per image, how many rows of att_feats[i] are real (INTEGRATION.md "Ragged attention maps").
        One (B,) integer tensor or sequence for all encoders, or a list of M such values with None for an encoder whose maps
        are full.  Stage I attends over those rows only; the padded rows must be finite.  fc_feats stays the caller's."""
        train = bool(self.training)
        seed = self._step_seed(train)
        S = self._decoder_steps(seq)          # may read `seq` back once: do it before queueing phase 1
        g = int(self.dedup_seq_per_img)
        if g > 1:
            self._mos_refuse('dedup_seq_per_img', 'the fan-out of one image\'s rows was not taught the head')
            if train and (self.drop_prob_fusion > 0 or self.drop_prob_reason > 0):
                raise N.RfnError('dedup_seq_per_img needs drop_prob_fusion = drop_prob_reason = 0')
            rows, n_feat = seq.size(0), fc_feats[0].size(0)
            lens_u = self._att_lens(att_lens, n_feat, fc_feats[0].device)
            if n_feat == rows and rows % g == 0:      # caption rows (the loader's layout): keep one row per image
                fc_u, att_u = [f[::g] for f in fc_feats], [a[::g] for a in att_feats]
                if lens_u is not None:
                    lens_u = [None if v is None else v[::g].contiguous() for v in lens_u]
            elif n_feat * g == rows:                  # unique images already (FeatureFeeder.batch(expand=False))
                fc_u, att_u = list(fc_feats), list(att_feats)
            else:
                raise N.RfnError('dedup_seq_per_img = %d: %d feature rows do not match %d caption rows' % (g, n_feat, rows))
            comb, h, c, reason = self._prefix(fc_u, att_u, train, seed, lens_u)
            comb = comb.repeat_interleave(g, dim=1)       # autograd sums the caption rows back onto the image
            h, c = h.repeat_interleave(g, dim=0), c.repeat_interleave(g, dim=0)
            reason = reason.repeat_interleave(g, dim=1)
        else:
            comb, h, c, reason = self._prefix(fc_feats, att_feats, train, seed, att_lens)
        log_prob = self._decode_teacher_forced(seq[:, :S], comb, h, c, train, seed, self.ss_prob)
        return log_prob, list(reason.unbind(0))

    def _check_teacher(self, teacher, B, S, dev):
        """The distillation teacher of forward_loss: a CUDA f32 tensor indexed (B, T_t >= S, V+1), unit stride in the last
        dimension, any strides in the first two (forward's batch-major log-probs, EnsembleDecoder.teacher_logits' view of a
        time-major buffer) -- or a distill.TopKTeacher (B, T_t >= S, K) on that device (its own constructor has checked dtype,
        K and strides).  Runs before any native call."""
        V1 = self.vocab_size + 1
        if isinstance(teacher, TopKTeacher):
            if teacher.size(0) != B or teacher.size(1) < S:
                raise N.RfnError('teacher has shape %s, this pass needs (%d, >= %d, K)' % (tuple(teacher.shape), B, S))
            if not teacher.ids.is_cuda:
                raise N.RfnError('teacher must live on the GPU: the HIP path has no CPU fallback')
            if teacher.device != dev:
                raise N.RfnError('teacher lives on %s, the features on %s' % (teacher.device, dev))
            return teacher
        if not torch.is_tensor(teacher):
            raise N.RfnError('teacher must be a tensor (B, T, V+1) of logits or log-probs, got %s' % type(teacher).__name__)
        if teacher.dim() != 3 or teacher.size(0) != B or teacher.size(1) < S or teacher.size(2) != V1:
            raise N.RfnError('teacher has shape %s, this pass needs (%d, >= %d, %d)' % (tuple(teacher.shape), B, S, V1))
        if teacher.dtype != torch.float32:
            raise N.RfnError('teacher must be float32, got %s' % teacher.dtype)
        if not teacher.is_cuda:
            raise N.RfnError('teacher must live on the GPU: the HIP path has no CPU fallback')
        if teacher.device != dev:
            raise N.RfnError('teacher lives on %s, the features on %s' % (teacher.device, dev))
        if teacher.stride(2) != 1 or abs(teacher.stride(0)) < V1 or abs(teacher.stride(1)) < V1:
            raise N.RfnError('teacher rows need unit stride and must not overlap: strides %s' % (tuple(teacher.stride()),))
        return teacher.detach()

    def forward_loss(self, fc_feats, att_feats, seq, masks, top_words, crit, reason_weight=1.0, teacher=None, kd_alpha=0.5,
                     kd_temperature=1.0, att_lens=None):
        """The XE train step's forward AND criterion in one call (opt-in) ->
        (loss, reason_pred): the value and the gradients of
            log_prob, reason_pred = model(fc_feats, att_feats, seq)
            loss = crit(log_prob, seq[:, 1:], masks[:, 1:], reason_pred, top_words, reason_weight)     (train.py:154-159)
        with `crit` a ReviewNetEnsembleCriterion (its label-smoothing setting is honoured), without the (B, T, V+1) log_prob
        tensor, its gradient and the four passes over them: the language term comes straight from the logits and its
        backward writes d logits in place (rfn_xe_logits_fwd / _bwd).  Equal to the two-call form to rounding (the row
        logsumexp is the same; the loss terms are summed in the same order).  Scheduled sampling needs the per-step
        distributions and takes the two-call form.

        Distillation (rfn.h rfn_kd_logits_fwd): with `teacher` -- (B, T_t >= S, V+1) f32 logits or log-probs on the device, unit
        stride in the last dimension; `teacher_model(fc, att, seq)[0]` under no_grad, or EnsembleDecoder.teacher_logits -- the
        language term becomes (1 - kd_alpha) * xe + kd_alpha * kd, kd = the masked KL(teacher || student) at temperature
        kd_temperature times its square, still one pass over the logits rows in each direction (one more read of the teacher
        row).  The teacher is a constant.  `self.last_distill` = {'xe', 'kd'}: the two terms as 0-dim device tensors (no
        read-back).  kd_alpha == 0 is the call without a teacher, bit for bit ('kd' is then None).  Scheduled sampling does not
        combine with a teacher: its rows are conditioned on the ground-truth prefix.

        A compact teacher (rfn.h rfn_kd_topk_fwd): `teacher` may be a distill.TopKTeacher -- the K <= 32 best (id, log-prob)
        pairs of every row, 8 * K bytes instead of 4 * (V+1), from TopKTeacher.from_dense, EnsembleDecoder.teacher_topk or a
        cache on disk.  Same arguments, same `last_distill`, same refusals; the meaning is the dense teacher's with -inf off
        the K ids (the K entries are renormalised; the tail mass is dropped)."""
        from .criteria import _MLMFn
        if self.use_mos:
            if teacher is not None:
                self._mos_refuse('teacher=', 'the distillation kernels read the logit layer\'s rows')
            if self.ss_prob > 0:
                self._mos_refuse('ss_prob > 0', 'scheduled sampling steps through the logit layer')
            if int(self.dedup_seq_per_img) > 1:
                self._mos_refuse('dedup_seq_per_img', 'the fan-out of one image\'s rows was not taught the head')
        if teacher is not None:
            if self.ss_prob > 0:
                raise N.RfnError('distillation does not combine with scheduled sampling (ss_prob = %g): the teacher\'s rows are '
                                 'conditioned on the ground-truth prefix' % self.ss_prob)
            kd_alpha, kd_temperature = float(kd_alpha), float(kd_temperature)
            if not 0.0 <= kd_alpha <= 1.0:
                raise N.RfnError('kd_alpha = %g is outside [0, 1]' % kd_alpha)
            if not (0.0 < kd_temperature < float('inf')):
                raise N.RfnError('kd_temperature = %g must be positive and finite' % kd_temperature)
        if self.ss_prob > 0:
            log_prob, reason = self.forward(fc_feats, att_feats, seq, att_lens=att_lens)
            return crit(log_prob, seq[:, 1:], masks[:, 1:], reason, top_words, reason_weight), reason
        train = bool(self.training)
        seed = self._step_seed(train)
        S = self._decoder_steps(seq)
        if seq.size(1) < S + 1 or masks.size(1) < S + 1:
            raise N.RfnError('labels / masks need %d columns for %d decoder steps' % (S + 1, S))
        if int(self.dedup_seq_per_img) > 1:
            raise N.RfnError('forward_loss does not combine with dedup_seq_per_img; use forward() + the criterion')
        dev = fc_feats[0].device
        kd = terms = None
        if teacher is not None:
            z = self._check_teacher(teacher, seq.size(0), S, dev)
            if kd_alpha > 0.0:
                kd, terms = (z, kd_alpha, 1.0 / kd_temperature), torch.empty(2, device=dev)
        comb, h, c, reason = self._prefix(fc_feats, att_feats, train, seed, att_lens)
        seq = seq.to(dev).long()
        masks = masks.to(dev).float()
        if seq.stride(1) != 1:
            seq = seq.contiguous()
        if masks.stride(1) != 1:
            masks = masks.contiguous()
        eps = float(crit.label_smoothing_epsilon) if crit.use_label_smoothing else 0.0
        if self.use_mos:      # hidden pass + the head's loss form: neither log_prob nor its gradient is materialised
            hidden = self._decode_hidden(seq[:, :S], comb, h, c, train, seed)
            lang = self._mos_head(hidden, {'kind': 'loss', 'B': seq.size(0), 'T': S, 'target': seq[:, 1:S + 1],
                                           'mask': masks[:, 1:S + 1], 'eps': eps})
        else:
            params = self._params_of(self._decoder_slots)
            lang = _DecoderLossFn.apply(self, torch.is_grad_enabled(), train, seed, seq[:, :S], seq[:, 1:S + 1], masks[:, 1:S + 1],
                                        eps, kd, terms, comb, h, c, *params)
        if teacher is not None:
            self.last_distill = {'xe': terms[0], 'kd': terms[1]} if kd is not None else {'xe': lang.detach(), 'kd': None}
        heads = list(reason.unbind(0))
        return lang + _MLMFn.apply(float(reason_weight) / len(heads), top_words, *heads), heads

    def rl_loss(self, fc_feats, att_feats, seq, reward, top_words, entropy_reg=0.0, reason_weight=1.0, n=1, old_logprobs=None,
                ppo_clip=0.2, att_lens=None):
        """The policy-gradient step's replay AND criterion in one call (INTEGRATION.md "Policy-gradient loss from the logits") ->
        (loss, reason_pred): the value and the gradients, to rounding, of
            seq_, lp, lp_all, reason_pred = model.sample_group(fc_feats, att_feats, n, {'force_ids': seq})
            loss = rl_crit(lp, seq_, reward, lp_all, entropy_reg, reason_pred, top_words, reason_weight, old_logprobs, opt)
        with `rl_crit` a ReviewNetRewardCriterion (train_rl.py:160-203, misc/utils.py:44-84), without logprobs_all (rows, T, V+1),
        its gradient and the passes over them: the policy and entropy terms come straight from the logits and their backward
        writes d logits in place (rfn_rl_logits_fwd / _bwd).  So captions from ANY decode can be trained on -- the fast no-grad
        loops (sample with sample_n / top_k / top_p), a beam search's candidates, sample_distinct -- not only the differentiated
        sampled pass.

        seq (rows, T) int64, 1 <= T <= seq_length: captions as sample / sample_group / sample_distinct hand them out (zeros from
        the END on), rows image-major, rows = images * n with features per image.  The decoder runs T steps, fed BOS and
        seq[:, :T-1], scored against seq[:, :T]; nothing is read back, so a caller who wants the reference's early-exit trim passes
        what sample returned.  reward (rows, T) or (rows, 1) f32.  PPO is on iff old_logprobs (rows, T) is given (ppo_clip as
        opt.ppo_clip).  Stages I / II run once per image; dropout follows the module's mode with a fresh seed (the replay draws its
        own masks, as the reference's PPO epochs do).  Feature tensors that require grad get their gradients; att_lens works.
        `self.last_rl` = {'logprobs': (rows, T) the tokens' log-probs, detached (what a PPO loop keeps as sample_logprobs_old),
        'policy', 'entropy': the two terms of the loss as 0-dim device tensors}."""
        from .criteria import _MLMFn
        self._mos_refuse('rl_loss', 'the policy-gradient kernels read the logit layer\'s rows')
        if self.fixed_decoder_steps is not None or getattr(self, '_seed_dev', None) is not None:
            raise N.RfnError('rl_loss: the model is owned by a running GraphedTrainStep; the RL step is not captured')
        n = int(n)
        if n < 1:
            raise ValueError('rl_loss takes n >= 1 rows per image (got %d)' % n)
        B = self._check_inputs(fc_feats, att_feats)
        if not torch.is_tensor(seq) or seq.dim() != 2 or seq.size(0) != B * n or seq.dtype != torch.long:
            raise N.RfnError('rl_loss: seq must be int64 (%d, T) for %d images and n = %d, got %s %s'
                             % (B * n, B, n, getattr(seq, 'dtype', type(seq).__name__), tuple(getattr(seq, 'shape', ()))))
        rows, T = seq.shape
        if not 1 <= T <= self.seq_length:
            raise N.RfnError('rl_loss: seq has T = %d columns, this model decodes 1 <= T <= seq_length = %d' % (T, self.seq_length))
        if not torch.is_tensor(reward) or reward.dim() != 2 or reward.size(0) != rows or reward.size(1) not in (1, T):
            raise N.RfnError('rl_loss: reward must be (%d, %d) or (%d, 1), got %s' % (rows, T, rows, tuple(getattr(reward, 'shape', ()))))
        if old_logprobs is not None and (not torch.is_tensor(old_logprobs) or tuple(old_logprobs.shape) != (rows, T)):
            raise N.RfnError('rl_loss: old_logprobs must be (%d, %d), got %s' % (rows, T, tuple(getattr(old_logprobs, 'shape', ()))))
        if n > 1:
            self._need_hoisted('rl_loss: n rows per image need')
        train = bool(self.training)
        seed = self._step_seed(train)
        dev = fc_feats[0].device
        comb, h, c, reason = self._prefix(fc_feats, att_feats, train, seed, att_lens)
        if n > 1:      # the state fans out to the rows (autograd sums it back); the thought vectors stay per image
            h, c = h.repeat_interleave(n, dim=0), c.repeat_interleave(n, dim=0)
        seq = seq.to(dev).contiguous()
        ids = torch.zeros(rows, T, dtype=torch.long, device=dev)      # column t = the token fed at step t; column 0 = BOS
        ids[:, 1:] = seq[:, :T - 1]
        reward = reward.detach().to(dev).float().expand(rows, T).contiguous()
        old = None if old_logprobs is None else old_logprobs.detach().to(dev).float().contiguous()
        out = {}
        params = self._params_of(self._decoder_slots)
        lang = _DecoderRLFn.apply(self, torch.is_grad_enabled(), train, seed, ids, (seq, reward, old, float(entropy_reg), float(ppo_clip)),
                                  n, out, comb, h, c, *params)
        self.last_rl = {'logprobs': out['logprobs'], 'policy': out['terms'][0], 'entropy': out['terms'][1]}
        heads = list(reason.unbind(0))
        return lang + _MLMFn.apply(float(reason_weight) / len(heads), top_words, *heads), heads

    def _decoder_steps(self, seq):
        """Number of decoder steps: the reference breaks at the first all-zero column i >= 1 (:274).  The
        answer for a given (tensor, version) is cached, so a caller that reuses one label tensor pays the
        device read-back once instead of the reference's 17 syncs per forward."""
        if self.fixed_decoder_steps is not None:      # a captured step runs a fixed count (graphed.GraphedTrainStep)
            if not 1 <= self.fixed_decoder_steps <= seq.size(1):
                raise N.RfnError('fixed_decoder_steps = %d does not fit labels of %d columns' % (self.fixed_decoder_steps, seq.size(1)))
            return int(self.fixed_decoder_steps)
        key = (seq.data_ptr(), seq._version, tuple(seq.shape))
        hit = self._steps_cache
        if hit is not None and hit[0] == key and hit[1] is seq:
            return hit[2]
        nz = (seq != 0).any(0).tolist()
        S = seq.size(1)
        for i in range(1, seq.size(1)):
            if not nz[i]:
                S = i
                break
        self._steps_cache = (key, seq, S)     # holds `seq` so its storage cannot be recycled under the key
        return S

    def saliency(self, fc_feats, att_feats, seq, masks=None, att_lens=None, mode='grad_x_input'):
        """Which regions does a caption rest on: the gradient of each caption's log-likelihood with respect to the attention
        maps (INTEGRATION.md "Input gradients").  Per caption s_b = sum_t mask[b, t] * log p(seq[b, t + 1] | seq[b, :t + 1])
        through `forward`, differentiated with backward(ones), so row b of every result belongs to caption b alone.
        -> a list of M tensors: (B, L_i) maps -- sum_d grad * att_feats ('grad_x_input') or the L2 norm of each region's
        gradient ('grad_norm') -- or the (B, L_i, D_i) gradients themselves ('raw').
        masks: (B, >= S + 1) as the criterion takes them (column t + 1 weighs target seq[:, t + 1]); None: every target up to and
        including the caption's first END (0).  The model runs in the mode it is in: call it under eval() unless the dropout
        masks are wanted in the gradient.
        The path's backward hands parameter gradients over by assigning `.grad` (not through autograd's return values), so this
        method SAVES every parameter's `.grad` (and the flat-buffer registry and the grad_ready_hook) before the pass and
        RESTORES them after it: `.grad` tensors are the same objects with the same values as before the call, None stays
        None, and no hook fires."""
        if mode not in ('grad_x_input', 'grad_norm', 'raw'):
            raise ValueError("saliency: mode must be 'grad_x_input', 'grad_norm' or 'raw', got %r" % (mode,))
        att = [a.detach().requires_grad_(True) for a in att_feats]
        fc = [f.detach() for f in fc_feats]
        params = list(self.parameters())
        kept = ([p.grad for p in params], dict(self._last_flat_grads), self.grad_ready_hook)
        self.grad_ready_hook, self._last_flat_grads = None, {}
        for p in params:      # the pass starts from no gradients: nothing it produces is added INTO a buffer the caller holds
            p.grad = None
        try:
            with torch.enable_grad():
                log_prob, _ = self.forward(fc, att, seq, att_lens=att_lens)
                S = min(log_prob.size(1), seq.size(1) - 1)
                tgt = seq[:, 1:S + 1].to(log_prob.device).long()
                lp = log_prob[:, :S].gather(2, tgt.unsqueeze(2)).squeeze(2)
                if masks is None:
                    ended = (tgt == 0).long()
                    m = ((ended.cumsum(1) - ended) == 0).to(lp.dtype)
                else:
                    if masks.size(1) < S + 1:
                        raise N.RfnError('saliency: masks need %d columns for %d decoder steps' % (S + 1, S))
                    m = masks[:, 1:S + 1].to(lp.device).to(lp.dtype)
                s = (lp * m).sum(1)
                grads = torch.autograd.grad(s, att, grad_outputs=torch.ones_like(s))
        finally:
            for p, g in zip(params, kept[0]):
                p.grad = g
            self._last_flat_grads = kept[1]
            self.grad_ready_hook = kept[2]
        if mode == 'raw':
            return list(grads)
        if mode == 'grad_norm':
            return [g.norm(dim=2) for g in grads]
        return [(g * a.detach()).sum(2) for g, a in zip(grads, att)]

    def get_init_state(self, fc_feats):
        """misc/RecurrentFusionModel.py:333-343 (inference helper, no autograd)."""
        out = []
        with torch.no_grad():
            for i in range(self.num_feat_array):
                h0 = N.linear(fc_feats[i], self.fc2h[i].weight, self.fc2h[i].bias).unsqueeze(0)
                out.append((h0, h0.clone()))
        return out

    def get_thought_vectors(self, fc_feats, att_feats, state_list=None, att_lens=None):
        """misc/RecurrentFusionModel.py:283-331 -> (thought_vectors_comb (B,T2,R), reason_pred, state_review).
        `state_list`: the M (h, c) pairs of shape (1,B,R) that get_init_state returns -- used as given, like the
        reference; None recomputes them from fc_feats."""
        with torch.no_grad():
            if state_list is None:
                comb, h, c, reason = self._prefix(fc_feats, att_feats, False, 0, att_lens)
            else:
                comb, h, c, reason = self._prefix_from_state(att_feats, state_list, att_lens)
        return (comb.transpose(0, 1).contiguous(), list(reason.unbind(0)),
                (h.unsqueeze(0), c.unsqueeze(0)))

    def _prefix_from_state(self, att_feats, state_list, att_lens=None):
        M, R = self.num_feat_array, self.rnn_size
        if len(state_list) != M or len(att_feats) != M:
            raise N.RfnError('expected %d (h, c) states and att feature tensors' % M)
        B = att_feats[0].size(0)
        hs = [N.require_cuda_f32(s_[0].reshape(-1, R), 'state h') for s_ in state_list]
        cs = [N.require_cuda_f32(s_[1].reshape(-1, R), 'state c') for s_ in state_list]
        att = [N.require_cuda_f32(a, 'att_feats') for a in att_feats]
        for i in range(M):
            if hs[i].size(0) != B or cs[i].size(0) != B:
                raise N.RfnError('state %d has batch %d, features have %d' % (i, hs[i].size(0), B))
            if tuple(att[i].shape) != (B, self.att_num[i], self.att_feat_size[i]):
                raise N.RfnError('att_feats[%d] has shape %s' % (i, tuple(att[i].shape)))
        d = self._dims_for(False)
        dev = att[0].device
        lens = self._att_lens(att_lens, B, dev)
        K = self.top_words_count
        table = self._param_table(self._params_of(self._prefix_slots), self._prefix_slots)
        ws_bytes = N.lib.rfn_prefix_ws_bytes(C.byref(d), B, 0)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        comb = torch.empty(d.T2, B, R, device=dev)
        h, c = torch.empty(B, R, device=dev), torch.empty(B, R, device=dev)
        reason = torch.empty(M + 1, B, K, device=dev)
        self._check_ragged(N.lib.rfn_prefix_fwd_from_state_ex(C.byref(d), B, table, N.ptr_array(hs), N.ptr_array(cs),
                                                              N.ptr_array(att), comb.data_ptr(), h.data_ptr(), c.data_ptr(),
                                                              reason.data_ptr(), ws.data_ptr(), ws_bytes,
                                                              N.ptr_array(lens) if lens is not None else None, N.stream_ptr()),
                           lens, 'rfn_prefix_fwd_from_state')
        return comb, h, c, reason

    def one_time_step(self, xt, fc_feats, thought_vectors_comb, state_decode):
        """misc/RecurrentFusionModel.py:345-350 -> (logit (B,V+1) pre-softmax, state).  `xt` is the embedded
        input (B, E) exactly as in the reference (its callers do xt = model.embed(it), eval_utils.py:368), or int64
        token ids (B,), in which case the embedding is fused into the step."""
        with torch.no_grad():
            comb = thought_vectors_comb.transpose(0, 1).contiguous()
            drop = bool(self.training)
            stepper = _Stepper(self, comb, state_decode[0][-1].clone(), state_decode[1][-1].clone(), drop,
                               _fresh_seed() if drop else 0)
            logits = stepper.step(xt.contiguous(), want='logits')
            return logits, (stepper.h.unsqueeze(0), stepper.c.unsqueeze(0))

    def sample(self, fc_feats, att_feats, opt={}, att_lens=None):
        """misc/RecurrentFusionModel.py:545-658.

        opt['consensus'] = a rewards.CiderD scorer, with sample_max = 0 and sample_n = n > 1 (rfn.h "consensus reranking"): the n
        draws of an image are reranked on the device and the call returns B rows -- seq, seqLogprobs and logprobs of the draw that
        agrees most with the image's other draws under CIDEr-D, cut at those rows' own early exit -- and `self.consensus` =
        {'index': (B,), 'scores': (B, n)} (device tensors).  With beam_size > 1 the key goes to sample_beam."""
        sample_max = opt.get('sample_max', 1)
        beam_size = opt.get('beam_size', 1)
        temperature = opt.get('temperature', 1.0)
        samp = _Sampling.parse(opt)
        if self.use_mos and beam_size <= 1:
            if not sample_max:
                self._mos_refuse('sample_max = 0', 'the sampled pass draws inside the step-wise decoder, logit layer included')
            if torch.is_grad_enabled():
                self._mos_refuse('sample under grad', 'greedy decoding is stepped from the host: call it under no_grad')
        if beam_size > 1:
            if samp is not None:
                raise ValueError('top_k / top_p / sample_n apply to multinomial sampling, not to beam search')
            return self.sample_beam(fc_feats, att_feats, opt, att_lens=att_lens)
        cons = _Constraints.parse(opt, self.vocab_size + 1, self.seq_length)
        if cons is not None and opt.get('force_ids', None) is not None:
            raise ValueError('force_ids replays given tokens: decoding constraints cannot be combined with it')
        if samp is not None and opt.get('force_ids', None) is not None:
            raise ValueError('force_ids replays given tokens: top_k / top_p / sample_n cannot be combined with it')
        cs = _Consensus.parse_sample(opt, self.vocab_size + 1, self.seq_length, samp, sample_max)
        self.consensus = None
        self.candidates = None          # a sample_n call's B * n rows are its candidates
        if samp is not None and sample_max:
            if samp.n > 1:
                raise ValueError('sample_n > 1 with sample_max=1 would return n identical captions: sample with sample_max=0')
            samp = None           # the argmax survives any truncation
        want_grad = torch.is_grad_enabled() and not sample_max
        if (cons is not None or samp is not None) and want_grad:
            raise N.RfnError('decoding constraints are not applied to the differentiated sampling pass: sample under no_grad')
        # dropout follows the module's mode, as the reference's nn.Dropout layers do (train_rl.py samples in train()
        # mode)
        train = bool(self.training)
        seed = self._step_seed(train)
        with torch.set_grad_enabled(want_grad):
            comb, h, c, reason = self._prefix(fc_feats, att_feats, train, seed, att_lens)
        reason_pred = list(reason.unbind(0))
        force = opt.get('force_ids', None)
        if (not sample_max and cons is None and samp is None) or force is not None:
            out = self._sample_replayed(comb, h, c, train, seed, want_grad, temperature, force)
        elif self.use_mos:       # greedy, stepped from the host: the loop EnsembleDecoder.sample runs (decode.host_greedy_loop)
            with torch.no_grad():
                stepper = _Stepper(self, comb.detach(), h.detach().clone(), c.detach().clone(), train, seed)
                bufs = host_greedy_loop(lambda ids, o: stepper.step(ids, out=o, want='logits'), h.size(0), self.seq_length,
                                        self.vocab_size + 1, comb.device, cons)
                out = bufs.read_back()
        else:
            out = self._sample_device_loop(comb, h, c, train, seed, sample_max, temperature, cons, samp, cs)
        return (*out, reason_pred)

    def _need_hoisted(self, what, flags=_NOT_HOISTED, error=N.RfnError):
        """Refuse a call whose rows share thought vectors when path_flags select a decoder form that reads them per row."""
        if int(self.path_flags) & flags:
            raise error('%s the hoisted decoder cell (path_flags select another form)' % what)

    def sample_group(self, fc_feats, att_feats, n, opt={}, att_lens=None):
        """The RL trainer's sampled pass (train_rl.py:160, misc/RecurrentFusionModel.py:623-631) with n draws per image ->
        (seq (B*n, <= S), seqLogprobs, logprobs_all, reason_pred) with rows image-major (row k * n + j is draw j of image k) and
        reason_pred per image.  Stages I and II run once per image; ONE decoder node carries the n rows of every image, reads
        the image's thought vectors and sums their gradient back (rfn.h "multi-sample self-critical").  Works under grad and
        under no_grad.  opt: 'temperature', and 'force_ids' (B*n, S) to replay given tokens teacher-forced; every other
        decoding key is refused.  n = 1 is sample(..., {'sample_max': 0}) bit for bit.  The uniforms hook `_ss_uniforms` is
        (2, S+1, B*n)."""
        self._mos_refuse('sample_group', 'the differentiated sampled pass steps through the logit layer')
        n = int(n)
        if n < 1:
            raise ValueError('sample_group draws n >= 1 captions per image (got %d)' % n)
        bad = sorted(k for k in opt if k not in ('temperature', 'force_ids'))
        if bad:
            raise ValueError('sample_group is the differentiated multinomial pass: it takes temperature and force_ids, not %s'
                             % ', '.join(map(repr, bad)))
        force = opt.get('force_ids', None)
        B = self._check_inputs(fc_feats, att_feats)
        if force is not None and (force.dim() != 2 or force.size(0) != B * n or force.size(1) < self.seq_length):
            raise ValueError('force_ids must be (%d, >= %d), got %s' % (B * n, self.seq_length, tuple(force.shape)))
        if n > 1:
            self._need_hoisted('n draws per image need')
        train = bool(self.training)
        seed = self._step_seed(train)
        want_grad = torch.is_grad_enabled()
        comb, h, c, reason = self._prefix(fc_feats, att_feats, train, seed, att_lens)
        if n > 1:      # the state fans out to the rows (autograd sums it back); the thought vectors stay per image
            h, c = h.repeat_interleave(n, dim=0), c.repeat_interleave(n, dim=0)
        out = self._sample_replayed(comb, h, c, train, seed, want_grad, opt.get('temperature', 1.0), force, n)
        return (*out, list(reason.unbind(0)))

    def sample_distinct(self, fc_feats, att_feats, n, opt={}, att_lens=None):
        """n DISTINCT sampled captions per image by stochastic beam search (rfn.h "stochastic beam search"; Kool et al. 2019; the
        reference has nothing of the kind): one beam search of width n on Gumbel-perturbed log-probabilities, an exact sample
        without replacement from the model's distribution over captions -> (seq (B*n, S) int64, seqLogprobs (B*n, S) f32,
        reason_pred), rows image-major in descending perturbed score (row k * n is an exact ordinary sample of image k), zeros
        after a caption's END and in dead rows (an image with fewer than n possible captions).  Nothing is read back: no early-exit
        trim, no synchronisation.  Sets
            self.stochastic_beams = {'logprob', 'gumbel', 'weight': (B, n) f64, 'n_live': (B,) int32}   device tensors: the
                caption's log-probability (the ascending fp64 sum of its seqLogprobs), its perturbed score G, and its importance
                weight -- sum_j weight[k, j] * f(caption j) estimates E f under the model (the last live row is the threshold and
                weighs 0); -inf / -inf / 0 for dead rows
            self.candidates = {'seq': (B, n, S), 'n_cand': n_live}   what rewards.consensus, rewards.diversity,
                evalcap.DiversityEval and decode.rescore take, as after sample_beam's keep_candidates.
        opt: 'seed' (the 64-bit key of the noise; default a fresh one from torch's generator, so torch.manual_seed reproduces a
        call) and the decoding constraints 'block_ngram', 'banned_ids', 'bad_endings' -- the weights are then relative: the
        restricted distribution is not renormalised.  Every other key raises ValueError by name.  Runs under no_grad only; dropout
        follows the module's mode, as in sample_beam.  n <= 32, seq_length <= 64; needs the hoisted decoder cell.  EnsembleDecoder
        has no such method.  To train on the set: rewards.get_self_critical_reward_distinct turns the weights into the normalised
        importance-weighted policy-gradient coefficients (with their built-in baseline) and rl_loss(..., n=n) replays the rows."""
        self._mos_refuse('sample_distinct', 'stochastic beam search is a device loop with the logit layer inside')
        B, S, V1 = self._check_inputs(fc_feats, att_feats), self.seq_length, self.vocab_size + 1
        sb = _Stochastic.parse(opt, n, S)
        if sb.n > V1:
            raise ValueError('sample_distinct draws n <= vocab_size + 1 = %d captions per image, got %d' % (V1, sb.n))
        cons = _Constraints.parse(opt, V1, S)
        if torch.is_grad_enabled():
            raise N.RfnError('stochastic beam search is not differentiated: call sample_distinct under no_grad')
        self._need_hoisted('n rows per image need')
        W = sb.n
        drop = bool(self.training)
        seed = _fresh_seed() if drop else 0
        noise_seed = sb.seed if sb.seed is not None else _fresh_seed()
        comb, h, c, reason = self._prefix(fc_feats, att_feats, drop, seed, att_lens)
        dev = comb.device
        stepper = _Stepper(self, comb, h.repeat_interleave(W, dim=0).contiguous(), c.repeat_interleave(W, dim=0).contiguous(),
                           drop, seed)
        bufs = StochasticBuffers(B, W, S, dev)
        run_beam_loop(stepper, bufs, cons, sbs_seed=noise_seed)
        cands = bufs.bs.permute(1, 2, 0).contiguous()                                # (B, n, S)
        self.stochastic_beams = {'logprob': bufs.phi, 'gumbel': bufs.gumbel, 'weight': bufs.weight, 'n_live': bufs.n_live}
        self.candidates = {'seq': cands, 'n_cand': bufs.n_live}
        self.consensus = None
        return cands.view(B * W, S), bufs.bl.permute(1, 2, 0).reshape(B * W, S), list(reason.unbind(0))

    def _sample_replayed(self, comb, h, c, train, seed, want_grad, temperature, force, n=1):
        """Multinomial (:623-631) or replayed ids -> (seq, seq_lp, logp).  ONE pass of the training decoder is both the pass
        that is sampled and, under grad, the pass that is differentiated (train_rl.py:160-166): step-wise with a device-side
        inverse-CDF draw between steps, or -- when the ids are given -- simply teacher-forced."""
        B, S, dev = h.size(0), self.seq_length, comb.device
        with torch.set_grad_enabled(want_grad):
            if force is not None:
                raw = torch.zeros(B, S + 1, dtype=torch.long, device=dev)      # column t = token fed at step t
                raw[:, 1:] = force[:, :S].to(dev)
            else:
                logp_full, raw = self._decode_sampled(comb, h, c, train, seed, S + 1, 1.0 / float(temperature), n)
            tok = raw[:, 1:]
            unf = torch.cumprod((tok > 0).long(), 1)                           # a row is finished after its first 0
            seq = tok * unf
            t_stop = early_exit(unf.sum(0).tolist(), S)                        # one read-back
            n_seq = t_stop - 1
            if force is not None:
                logp = self._decode_teacher_forced(raw[:, :t_stop].contiguous(), comb, h, c, train, seed, n=n)
            else:
                logp = logp_full[:, :t_stop]
            seq_lp = logp[:, :n_seq].gather(2, tok[:, :n_seq].unsqueeze(2)).squeeze(2)
        if getattr(self, '_trace_ss', False):
            self._sample_ids = raw[:, :t_stop].clone()       # test hook: the tokens the pass fed
        return seq[:, :n_seq], seq_lp, logp.contiguous()

    @torch.no_grad()
    def _sample_device_loop(self, comb, h, c, train, seed, sample_max, temperature, cons, samp=None, cs=None):
        """Greedy, or constrained / truncated multinomial: the whole free-running loop in one call -> (seq, seq_lp, logp).
        samp.n > 1: n rows per image, image-major, all reading the image's thought vectors (comb stays per image).
        cs (a parsed _Consensus): one row per image comes back, the draw that agrees most with the image's other draws, cut at
        the chosen rows' own early exit; the pick is queued behind the loop and rides on its one read-back."""
        S, dev = self.seq_length, comb.device
        n = samp.n if samp is not None else 1
        if n > 1:
            h, c = h.detach().repeat_interleave(n, dim=0), c.detach().repeat_interleave(n, dim=0)
        else:
            h, c = h.detach().clone(), c.detach().clone()
        B = h.size(0)
        stepper = _Stepper(self, comb.detach(), h, c, train, seed)
        bufs = GreedyBuffers(B, S, self.vocab_size + 1, dev)
        mode, inv_temp, u = 0, 1.0, None
        if not sample_max:     # the same loop drawing with the uniforms the sampled pass would use
            r = getattr(self, '_ss_uniforms', None)
            if r is None:
                r = torch.rand(2, S + 1, B, device=dev)
            elif tuple(r.shape) != (2, S + 1, B) or r.device != dev:
                raise N.RfnError('sampling uniforms are %s, this pass needs %s' % (tuple(r.shape), (2, S + 1, B)))
            mode, inv_temp, u = 1, 1.0 / float(temperature), r[0, 1:].contiguous()
        run_greedy_loop(stepper, bufs, mode, inv_temp, u, cons, samp)
        if cs is not None:
            best = cs.pick(bufs.seq.view(B // n, n, S))
            self.consensus = cs.result
            return bufs.read_back_picked(best, n)
        return bufs.read_back()        # waits for the loop: the call's one read-back

    @torch.no_grad()
    def score(self, fc_feats, att_feats, seq, opt={}, att_lens=None):
        """How likely the model finds the captions it is GIVEN (rfn.h "caption scoring"; the reference has nothing of the kind) ->
        a dict of device tensors over the caption rows (image-major):
            'token_logprobs' (rows, steps) f32   log-prob of each given token, 0 at positions that are not scored
            'logprob' (rows,) f64                their sum, ascending, in fp64
            'length' (rows,) int32               how many positions were scored
            'score' (rows,) f64                  logprob / length^alpha, alpha = opt['length_penalty'] (default 0)
            'rank' (rows, steps) int32, 'entropy' (rows, steps) f32   when opt['outputs'] names them: the given token's place in
                                                 the step's distribution (0 = the argmax, -1 where not scored) and that
                                                 distribution's entropy in nats
        seq: word ids as sample() returns them (no BOS column, zeros after the caption): (B, T), (B, n, T), or (B * n, T) with
        opt['n'], T <= seq_length + 1; the first min(T, seq_length) columns are read as words (labels[:, 1:] of the loader is a
        valid argument) and steps = min(T, seq_length) + 1 -- nothing is read back to trim them.  A caption's words and its END are
        scored (the XE criterion's mask); opt['include_end'] = False scores the words only (eval_utils' sum(seqLogprobs * (seq >
        0))).  Always runs under no_grad with dropout off, whatever the module's mode.  Stages I / II run once per image; with n > 1
        the n rows of an image read its thought vectors.  The (rows, steps, V+1) log-probs are never materialised: the logits of
        at most opt['max_rows'] rows (default: 1 GiB of them) exist at a time, and the chunking changes no bit."""
        so = _Scoring.parse(opt)
        B = self._check_inputs(fc_feats, att_feats)
        rows, n, T = so.layout(seq.shape, B, self.seq_length)
        if n > 1:
            self._need_hoisted('n captions per image need')
        comb, h, c, _ = self._prefix(fc_feats, att_feats, False, 0, att_lens)
        dev = comb.device
        if n > 1:
            h, c = h.repeat_interleave(n, dim=0), c.repeat_interleave(n, dim=0)
        h, c = h.contiguous(), c.contiguous()
        bufs = ScoreBuffers(so, seq, rows, T, self.seq_length, dev)
        S, V1 = bufs.steps, self.vocab_size + 1
        d = self._dims_for(False)
        table = self._param_table(self._params_of(self._decoder_slots), self._decoder_slots)
        per_call = so.rows_per_call(n, S, V1)
        if self.use_mos:      # the head's K expert rows per caption row: K times fewer rows per call
            per_call = max(n, per_call // self.num_expert // n * n)
            return self._score_mos(bufs, so, comb, h, c, rows, n, per_call)
        ws_bytes = N.lib.rfn_decoder_score_ws_bytes(C.byref(d), min(rows, per_call), S, n)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        for r0 in range(0, rows, per_call):
            r1 = min(rows, r0 + per_call)
            cb = comb if (r0 == 0 and r1 == rows) else comb[:, r0 // n:r1 // n].contiguous()
            sl = lambda t: N.ptr(None if t is None else t[r0:r1])  # noqa: E731
            N.check(N.lib.rfn_decoder_score(C.byref(d), r1 - r0, S, table, cb.data_ptr(), sl(h), sl(c), sl(bufs.feed),
                                            bufs.feed.stride(0), sl(bufs.target), bufs.target.stride(0), int(so.include_end),
                                            sl(bufs.tok_lp), sl(bufs.rank), sl(bufs.ent), bufs.tok_lp.stride(0), sl(bufs.cap_lp),
                                            sl(bufs.cap_len), ws.data_ptr(), ws_bytes, n, N.stream_ptr()), 'rfn_decoder_score')
        return bufs.result()

    def _score_mos(self, bufs, so, comb, h, c, rows, n, per_call):
        """score() of a mixture-of-softmaxes model: the hidden pass, the head's time-major log-prob rows in the place of the
        logits (their log-sum-exp is 0 up to rounding), then rfn_score_logits / rfn_score_captions as rfn_decoder_score runs
        them.  With n > 1 an image's thought vectors are repeated physically (the hidden pass carries one row per image)."""
        S, V1, st = bufs.steps, self.vocab_size + 1, N.stream_ptr()
        md, params = self.mos.md, self._params_of(self._mos_slots)
        for r0 in range(0, rows, per_call):
            r1 = min(rows, r0 + per_call)
            m = r1 - r0
            cb = comb[:, r0 // n:r1 // n]
            if n > 1:
                cb = cb.repeat_interleave(n, dim=1)
            hidden = self._decode_hidden(bufs.feed[r0:r1, :S], cb.contiguous(), h[r0:r1], c[r0:r1], False, 0)
            logp = torch.empty(S * m, V1, device=hidden.device)
            N.mos_fwd(md, hidden, params, logp, N.mos_workspace(md, S * m, False, hidden.device))
            sl = lambda t: N.ptr(None if t is None else t[r0:r1])  # noqa: E731
            N.check(N.lib.rfn_score_logits(logp.data_ptr(), V1, m, S, 0, V1, sl(bufs.target), bufs.target.stride(0),
                                           int(so.include_end), sl(bufs.tok_lp), sl(bufs.rank), sl(bufs.ent), bufs.tok_lp.stride(0), st),
                    'rfn_score_logits')
            N.check(N.lib.rfn_score_captions(sl(bufs.tok_lp), bufs.tok_lp.stride(0), sl(bufs.target), bufs.target.stride(0), m, S, V1,
                                             int(so.include_end), sl(bufs.cap_lp), sl(bufs.cap_len), st), 'rfn_score_captions')
        return bufs.result()

    def attention(self, fc_feats, att_feats, seq, opt={}, att_lens=None):
        """Where the model looked when it wrote each word of the captions it is GIVEN (rfn.h "attention maps", INTEGRATION.md
        "Attention maps"; the reference never returns its attention weights) -> a dict of device tensors, caption rows image-major:
            'encoder'  list of M (B, T1, L_i)      stage I: encoder i's review steps over its regions
            'fusion'   (B, T2, M, T1)              stage II: each fusion step over encoder i's thought vectors
            'decoder'  (rows, steps, T2)           the decoder over the fused thought vectors, zeros at dead steps
            'rollout'  list of M (rows, steps, L_i)  G_i[r, s, l] = sum_t2 decoder[r, s, t2] * (sum_t1 fusion[k, t2, i, t1] *
                                                   encoder_i[k, t1, l]), k = r // n: the three levels composed (rfn_attn_rollout)
            'length'   (rows,) int32               live steps per row: the caption's words and its END, at most steps
            'peak', 'entropy', 'mass'  lists of M (rows, steps), when opt['outputs'] names them: the first argmax region (-1 at
                                                   dead steps), the map's entropy in nats, and the weight inside
                                                   opt['region_mask'] (a list of M (rows, steps, L_i) bool / uint8 device tensors,
                                                   None entries allowed -- their 'mass' entry is None)
        seq, opt['n'] and steps = min(T, seq_length) + 1 exactly as score() takes them; opt['max_rows'] bounds the rows of one
        decoder call.  Always runs under no_grad with dropout off.  Stages I / II run once per image; the decoder runs the pass
        that stops before the output layer (no logits: a use_mos model works unchanged).  Rollout composes attention weights only
        -- it is not a gradient attribution (saliency() is).  Refused by name before any launch: path_flags that select another
        decoder form than the hoisted cell, a model owned by a running GraphedTrainStep, unknown opt keys, a bad region_mask."""
        from .attention_maps import attention
        return attention(self, fc_feats, att_feats, seq, opt, att_lens)

    def sample_beam(self, fc_feats, att_feats, opt={}, att_lens=None):
        """misc/RecurrentFusionModel.py:352-543, batched and device-resident.

        Stages I/II run ONCE for the batch (the reference recomputes them per image on beam_size identical rows),
        all images' beams share one decoder batch of B*beam rows, and rfn_beam_step does the reference's
        candidate / stable-sort / fork / done-beam bookkeeping on the device -- no per-step host read-back.  The
        done beams are sorted (stably, by -p, as :529) on the host once at the end.

        opt['group_size'] = G > 1 (with opt['diversity_lambda'], default 0.5): diverse beam search (rfn.h "diverse beam
        search") -- beam_size is still the total number of beams.  Every `done_beams` dict then carries its 'group', and
        `self.diverse_beams[k]` lists image k's G group bests under the call's ranking.  G = 1 is the plain search.

        opt['consensus'] = a rewards.CiderD scorer (rfn.h "consensus reranking"): the returned seq / seqLogprobs are, per image,
        the candidate that agrees most with the others under CIDEr-D -- among the first opt['consensus_n'] (default beam_size,
        at most 32) ranked done beams, or among the G group bests of a diverse search -- with opt['consensus_weights'] 'uniform'
        or 'prob'.  `self.consensus` = {'index': (B,) rank (or group) of the pick, 'scores': (B, n)}, device tensors; top_seq,
        top_prob, done_beams and diverse_beams are unchanged, and the call stays lazy.

        opt['keep_candidates'] = True leaves `self.candidates` = {'seq': (B, m, S) int64, 'n_cand': (B,) int32} on the device: the
        candidate set the consensus pick chooses from (with or without 'consensus'), for evalcap.DiversityEval.  Without the key
        `self.candidates` is None and the call issues the launches it always did.

        opt['require'] = per image up to 3 sets of token ids, a (B, C, K) tensor padded with -1 or nested lists (rfn.h "lexically
        constrained beam search"): the caption should hold one id of every set.  beam_size is then the beam of each of the 2^C
        states and the search runs beam_size * 2^C <= 32 rows per image.  The done beams are ranked by the number of satisfied sets
        first; every `done_beams` dict carries its 'state' (the bit mask of satisfied sets), and `self.lexical_met` is a (B,) int32
        device tensor: how many of the image's non-empty sets the returned caption satisfies.  Composes with block_ngram,
        banned_ids, bad_endings, length_penalty and keep_candidates; not with group_size > 1 or consensus.  With every set empty
        the call issues the launches it always did."""
        beam_size = opt.get('beam_size', 10)
        B, S, V1 = fc_feats[0].size(0), self.seq_length, self.vocab_size + 1
        assert beam_size <= V1, 'lets assume this for now'
        if beam_size > MAX_BEAM or S > MAX_STEPS:
            raise N.RfnError('beam search supports beam_size <= 32 and seq_length <= 64')
        lex = _Lexical.parse(opt, B, V1, beam_size)
        W = lex.W if lex is not None else beam_size
        cons, alpha, div = _Constraints.parse(opt, V1, S), _length_penalty(opt), _Diversity.parse(opt, beam_size)
        cs = _Consensus.parse(opt, V1, S, beam_size)
        if lex is not None and (div is not None or cs is not None):
            raise ValueError('require cannot be combined with group_size > 1 or consensus')
        if lex is not None:
            self._mos_refuse('require', 'lexically constrained beam search is a device loop with the logit layer inside')
            self._need_hoisted('require needs', N.PATH_OPT_DEC_UNHOISTED, ValueError)
        keep_n = keep_candidates_n(opt, beam_size)
        keep = None if keep_n is None else {'n': keep_n}
        if (cons is not None or alpha) and opt.get('force_ids', None) is not None:
            raise ValueError('force_ids replays given tokens: decoding constraints cannot be combined with it')
        with torch.no_grad():
            drop = bool(self.training)
            seed = _fresh_seed() if drop else 0
            comb_b, h_b, c_b, reason = self._prefix(fc_feats, att_feats, drop, seed, att_lens)
            dev = comb_b.device
            h_w, c_w = h_b.repeat_interleave(W, dim=0).contiguous(), c_b.repeat_interleave(W, dim=0).contiguous()
            if self.use_mos:     # stepped from the host: the loop EnsembleDecoder.sample_beam runs (decode.host_beam_loop); a
                # host-stepped stepper's rows do not share thought vectors, so they are repeated physically
                stepper = _Stepper(self, comb_b.repeat_interleave(W, dim=1), h_w, c_w, drop, seed)
                bufs = host_beam_loop(lambda ids, o: stepper.step(ids, out=o, want='logits'), stepper.reorder, B, W, S, V1, dev,
                                      cons, div)
            else:
                # the W beam rows of image k (rows k*W .. k*W+W-1) read the image's thought vectors: comb stays (T2, B, R)
                stepper = _Stepper(self, comb_b, h_w, c_w, drop, seed)
                bufs = BeamBuffers(B, W, S, dev, div.groups if div is not None else 1, lex.G if lex is not None else 1)
                run_beam_loop(stepper, bufs, cons, div, lex.bind(dev) if lex is not None else None)
            lex_out = {} if lex is not None else None
            seq, seq_lp, top_seq, top_prob, done_beams = _sorted_done_beams(bufs, alpha, cs, div.groups if div is not None else 1, keep,
                                                                            lex_out)
            heads = reason.unsqueeze(2).expand(-1, -1, W, -1)                       # (M+1, B, W, K) broadcast view
        self.done_beams = done_beams
        self.consensus = cs.result if cs is not None else None
        self.candidates = None if keep is None else {'seq': keep['seq'], 'n_cand': keep['n_cand']}
        self.diverse_beams = _diverse_beams(done_beams, div.groups) if div is not None else None
        self.lexical_met = lex.met(lex_out['state']) if lex is not None else None
        reason_batch = _LazyList(B, lambda: [list(t.unbind(0)) for t in heads.unbind(1)])
        return seq, seq_lp, top_seq, top_prob, reason_batch


def _join_before_state_dict(module, prefix, keep_vars):
    hook = getattr(module, 'param_wait_hook', None)
    if hook is not None:
        hook(None)
