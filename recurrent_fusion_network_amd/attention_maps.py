"""RecurrentFusionModel.attention: where the model looked when it wrote each word of a GIVEN caption (rfn.h "attention maps",
INTEGRATION.md "Attention maps").  The three families of attention weights the forward kernels leave in their workspaces are
handed out, and composed on the device into one word-to-region map per (caption row, encoder) -- rfn_attn_rollout -- with the
optional per-word statistics of rfn_attn_map_stats.  Nothing is read back to the host."""
from __future__ import annotations

import ctypes as C

import torch

from . import _native as N
from .decode import _Scoring, ScoreBuffers

KEYS = ('n', 'outputs', 'region_mask', 'max_rows')
OUTPUTS = ('peak', 'entropy', 'mass')


class _Attention:
    """The options of one attention() call: opt['n'] and opt['max_rows'] as score() takes them (_Scoring), opt['outputs'] (names
    among 'peak', 'entropy', 'mass': the optional per-word statistics) and opt['region_mask'] (a list of M entries, each None or a
    (rows, steps, L_i) bool / uint8 device tensor; 'mass' needs it).  Unknown keys and bad values raise ValueError; nothing here
    touches a device."""

    @classmethod
    def parse(cls, opt):
        bad = sorted(k for k in opt if k not in KEYS)
        if bad:
            raise ValueError('attention takes %s, not %s' % (', '.join(KEYS), ', '.join(map(repr, bad))))
        a = cls()
        a.so = _Scoring.parse({k: opt[k] for k in ('n', 'max_rows') if k in opt})
        outs = opt.get('outputs', None)
        outs = () if outs is None else ((outs,) if isinstance(outs, str) else tuple(outs))
        unknown = [o for o in outs if o not in OUTPUTS]
        if unknown:
            raise ValueError("outputs names 'peak', 'entropy' and / or 'mass', got %r" % (unknown,))
        a.outputs = tuple(o for o in OUTPUTS if o in outs)
        a.region_mask = opt.get('region_mask', None)
        if 'mass' in a.outputs and a.region_mask is None:
            raise ValueError("outputs names 'mass', which needs opt['region_mask']")
        return a

    def masks(self, att_num, rows, steps, dev):
        """opt['region_mask'] checked against the call -> a list of M entries, None or a contiguous uint8 tensor."""
        M = len(att_num)
        if self.region_mask is None:
            return [None] * M
        rm = list(self.region_mask) if isinstance(self.region_mask, (list, tuple)) else None
        if rm is None or len(rm) != M:
            raise ValueError('region_mask must be a list of %d entries (None, or a (rows, steps, L_i) bool / uint8 tensor)' % M)
        out = []
        for i, m in enumerate(rm):
            if m is None:
                out.append(None)
                continue
            want = (rows, steps, att_num[i])
            if not torch.is_tensor(m) or tuple(m.shape) != want:
                raise ValueError('region_mask[%d] must have shape %s, got %s' % (i, want, tuple(getattr(m, 'shape', ()))))
            if m.dtype not in (torch.bool, torch.uint8):
                raise ValueError('region_mask[%d] must be bool or uint8, got %s' % (i, m.dtype))
            if m.device != dev:
                raise ValueError('region_mask[%d] lives on %s, the features on %s' % (i, m.device, dev))
            m = m.contiguous()
            out.append(m.view(torch.uint8) if m.dtype == torch.bool else m)
        return out


def _floats(ws, addr, numel):
    """`numel` floats of the byte tensor `ws` at the device address `addr` (what a native accessor returned)."""
    if not addr:
        raise N.RfnError('the workspace accessor refused its arguments')
    off = addr - ws.data_ptr()
    return ws[off:off + 4 * numel].view(torch.float32)


@torch.no_grad()
def attention(model, fc_feats, att_feats, seq, opt={}, att_lens=None):
    ao = _Attention.parse(opt)
    if model.fixed_decoder_steps is not None or getattr(model, '_seed_dev', None) is not None:
        raise N.RfnError('attention: the model is owned by a running GraphedTrainStep; its passes are not captured')
    # the decoder pass that stops before the output layer (rfn_decoder_fwd_hidden) takes the hoisted cell only
    model._need_hoisted('attention: the decoder pass without its output layer needs')
    B = model._check_inputs(fc_feats, att_feats)
    rows, n, T = ao.so.layout(seq.shape, B, model.seq_length)
    fc = [N.require_cuda_f32(t, 'fc_feats') for t in fc_feats]
    att = [N.require_cuda_f32(t, 'att_feats') for t in att_feats]
    dev = fc[0].device
    M, T1, T2, R, K = model.num_feat_array, model.num_review_steps_0, model.num_review_steps, model.rnn_size, model.top_words_count
    Ls = [int(x) for x in model.att_num]
    S = min(T, model.seq_length) + 1
    masks = ao.masks(Ls, rows, S, dev)
    lens = model._att_lens(att_lens, B, dev)
    d = model._dims_for(False)                  # dropout off whatever the module's mode
    st = N.stream_ptr()

    # stages I / II, once per image, on a workspace this call keeps: the inference size holds every step's weights
    table = model._param_table(model._params_of(model._prefix_slots), model._prefix_slots)
    ws_bytes = N.lib.rfn_prefix_ws_bytes(C.byref(d), B, 0)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    comb = torch.empty(T2, B, R, device=dev)
    h, c = torch.empty(B, R, device=dev), torch.empty(B, R, device=dev)
    reason = torch.empty(M + 1, B, K, device=dev)
    model._check_ragged(N.lib.rfn_prefix_fwd_ex(C.byref(d), B, table, N.ptr_array(fc), N.ptr_array(att), comb.data_ptr(),
                                                h.data_ptr(), c.data_ptr(), reason.data_ptr(), ws.data_ptr(), ws_bytes, 0, 0,
                                                N.ptr_array(lens) if lens is not None else None, st), lens, 'rfn_prefix_fwd')
    a1 = [_floats(ws, N.lib.rfn_prefix_alpha1(C.byref(d), B, 0, i, ws.data_ptr()), T1 * B * Ls[i]).view(T1, B, Ls[i])
          for i in range(M)]
    a2 = _floats(ws, N.lib.rfn_prefix_alpha2(C.byref(d), B, 0, ws.data_ptr()), T2 * M * B * T1).view(T2, M, B, T1)
    # copies, never views: a returned tensor must not alias (and pin) the workspace, also where B or T1 is 1
    out = {'encoder': [a.transpose(0, 1).clone(memory_format=torch.contiguous_format) for a in a1],
           'fusion': a2.permute(2, 0, 1, 3).clone(memory_format=torch.contiguous_format)}

    # the captions as score() lays them out; a caption's words and its END are live
    bufs = ScoreBuffers(ao.so, seq, rows, T, model.seq_length, dev)
    assert bufs.steps == S
    V1 = model.vocab_size + 1
    tgt = bufs.target[:, :S]
    words = ((tgt > 0) & (tgt < V1)).to(torch.int32).cumprod(1).sum(1)
    length = (words + 1).clamp_(max=S).to(torch.int32)
    out['length'] = length

    # the decoder pass without its output layer; n rows of an image read its thought vectors, repeated physically
    if n > 1:
        comb = comb.repeat_interleave(n, dim=1)
        h, c = h.repeat_interleave(n, dim=0), c.repeat_interleave(n, dim=0)
    h, c = h.contiguous(), c.contiguous()
    dtable = model._param_table(model._params_of(model._decoder_slots), model._decoder_slots)
    # rfn_decoder_ws_bytes sizes the workspace of the full pass: its (S, rows, V+1) logits slab is allocated though this pass
    # never touches it, so the rows of one call are bounded as score() bounds them
    per_call = ao.so.rows_per_call(1, S, V1)
    dws_bytes = N.lib.rfn_decoder_ws_bytes(C.byref(d), min(rows, per_call), S, 0)
    dws = torch.empty(dws_bytes, dtype=torch.uint8, device=dev)
    dec = torch.empty(rows, S, T2, device=dev)
    for r0 in range(0, rows, per_call):
        r1 = min(rows, r0 + per_call)
        m = r1 - r0
        cb = comb if m == rows else comb[:, r0:r1].contiguous()
        N.check(N.lib.rfn_decoder_fwd_hidden(C.byref(d), m, S, dtable, cb.data_ptr(), h[r0:r1].data_ptr(), c[r0:r1].data_ptr(),
                                             bufs.feed[r0:r1].data_ptr(), bufs.feed.stride(0), dws.data_ptr(), dws_bytes, 0, 0, st),
                'rfn_decoder_fwd_hidden')
        aD = N.lib.rfn_decoder_alpha(C.byref(d), m, S, 0, 1, dws.data_ptr())
        if not aD:
            raise N.RfnError('rfn_decoder_alpha refused its arguments')
        N.check(N.lib.rfn_attn_decoder_copy(aD, m * T2, T2, length[r0:r1].data_ptr(), m, S, T2, dec[r0:r1].data_ptr(), S * T2, T2, st),
                'rfn_attn_decoder_copy')
    out['decoder'] = dec

    # the rollout, one launch per encoder, straight from the prefix workspace and the caption-major decoder weights
    rollout, stats = [], {k: [] for k in ao.outputs}
    for i in range(M):
        L = Ls[i]
        G = torch.empty(rows, S, L, device=dev)
        N.check(N.lib.rfn_attn_rollout(dec.data_ptr(), T2, S * T2, a2[:, i].data_ptr(), M * B * T1, T1, a1[i].data_ptr(), B * L, L,
                                       length.data_ptr(), N.ptr(lens[i]) if lens is not None else 0, rows, n, S, T1, T2, L,
                                       G.data_ptr(), S * L, L, st), 'rfn_attn_rollout')
        rollout.append(G)
        if ao.outputs:
            mask = masks[i] if 'mass' in ao.outputs else None
            peak = torch.empty(rows, S, dtype=torch.int32, device=dev)
            ent = torch.empty(rows, S, device=dev)
            mass = torch.empty(rows, S, device=dev) if mask is not None else None
            N.check(N.lib.rfn_attn_map_stats(G.data_ptr(), S * L, L, length.data_ptr(), N.ptr(mask), S * L, L, rows, S, L,
                                             peak.data_ptr(), ent.data_ptr(), N.ptr(mass), st), 'rfn_attn_map_stats')
            for k, v in (('peak', peak), ('entropy', ent), ('mass', mass)):
                if k in stats:
                    stats[k].append(v)
    out['rollout'] = rollout
    out.update(stats)
    return out
