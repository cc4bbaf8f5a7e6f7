"""Free-running decoding, shared by RecurrentFusionModel.sample / sample_beam / one_time_step and the EnsembleDecoder: the
decoder state, the decoding constraints, the loops' buffers, the two device-loop calls and the done-beam ranking -- and, for
captions that are given instead of decoded, the option parse and buffers of score() and n-best rescoring.  The model
is an argument (its `_dims_for`, `_param_table`, `_params_of` and `_decoder_slots` are used); it is never imported here."""
from __future__ import annotations

import collections.abc
import ctypes as C

import torch

from . import _native as N

MAX_BEAM = 32        # rows per image of a beam search, and entries of a row's top list (csrc: BEAM_MAX_W, LSM_TOPW)
MAX_STEPS = 64       # decode steps a beam-step block keeps the histories for (csrc: BEAM_MAX_S)


class _Stepper:
    """Free-running decoder state for sample / beam / one_time_step: rfn_decoder_prepare + rfn_decoder_step."""

    def __init__(self, model, comb, h, c, drop=False, seed=0):
        """drop / seed: apply the decoder dropout masks of (seed, step index) -- the ones rfn_decoder_fwd applies at
        the same steps -- so a free-running pass in training mode reproduces the teacher-forced pass bit for bit."""
        self.model = model
        self.d = model._dims_for(bool(drop))
        self.seed, self.t = int(seed), 0
        self.comb = comb.contiguous()
        self.h, self.c = h.contiguous(), c.contiguous()
        self.B = self.h.size(0)
        dev = self.h.device
        self.table = model._param_table(model._params_of(model._decoder_slots), model._decoder_slots)
        # the loop-invariant products of the thought vectors: att_2_att_h(comb) and U = comb . z2h.weight^T (rfn.h)
        self.Bc = self.comb.size(1)          # rows per thought vector: B, or the images of a beam search (B = Bc * beam)
        self.cproj = torch.empty(N.lib.rfn_decoder_cproj_floats(C.byref(self.d), self.Bc), device=dev)
        N.check(N.lib.rfn_decoder_prepare(C.byref(self.d), self.Bc, self.table, self.comb.data_ptr(),
                                          self.cproj.data_ptr(), N.stream_ptr()), 'rfn_decoder_prepare')
        self.ws_bytes = N.lib.rfn_decoder_step_ws_bytes(C.byref(self.d), self.B)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        # a mixture-of-softmaxes model (opt.use_mos): the cell runs with no logits and the head turns the new h into mixture
        # log-probs, handed out in the place of the logits -- their log-softmax is themselves up to rounding, so the
        # log-softmax / top-W / constraint kernels apply to them unchanged
        self.mos = getattr(model, 'mos', None) if getattr(model, 'use_mos', 0) else None
        if self.mos is not None:
            model._mos_refuse_path_flags()
            self.mos_params = model._params_of(model._mos_slots)
            self.mos_ws = N.mos_workspace(self.mos.md, self.B, False, dev)

    def _head(self, out):
        N.mos_fwd(self.mos.md, self.h, self.mos_params, out, self.mos_ws, self.B, out.stride(0), 0)

    def step(self, ids, out=None, want='logp'):
        """ids: int64 token ids (B,) -- or an already embedded float input (B, E), as the reference's one_time_step."""
        V1 = self.d.V1
        if self.Bc != self.B:
            raise N.RfnError('a stepper whose rows share thought vectors (beam search) is driven by rfn_beam_loop only')
        if out is None:
            out = torch.empty(self.B, V1, device=self.h.device)
        head = self.mos is not None
        logits_ptr = out.data_ptr() if want == 'logits' and not head else None
        logp_ptr = out.data_ptr() if want == 'logp' and not head else None
        if ids.is_floating_point():
            xt = N.require_cuda_f32(ids, 'xt')
            if tuple(xt.shape) != (self.B, self.d.E):
                raise N.RfnError('embedded xt must be (%d, %d), got %s' % (self.B, self.d.E, tuple(xt.shape)))
            N.check(N.lib.rfn_decoder_step_embedded(C.byref(self.d), self.B, self.table, self.comb.data_ptr(),
                                                    self.cproj.data_ptr(), xt.data_ptr(), xt.stride(0),
                                                    self.h.data_ptr(), self.c.data_ptr(), logits_ptr, logp_ptr,
                                                    out.stride(0), self.ws.data_ptr(), self.ws_bytes, self.seed,
                                                    self.t, N.stream_ptr()),
                    'rfn_decoder_step_embedded')
            self.t += 1
            if head:
                self._head(out)
            return out
        if ids.dtype != torch.long or not ids.is_contiguous():
            ids = ids.long().contiguous()
        N.check(N.lib.rfn_decoder_step(C.byref(self.d), self.B, self.table, self.comb.data_ptr(),
                                       self.cproj.data_ptr(), ids.data_ptr(), self.h.data_ptr(), self.c.data_ptr(),
                                       logits_ptr, logp_ptr, out.stride(0), self.ws.data_ptr(), self.ws_bytes,
                                       self.seed, self.t, N.stream_ptr()), 'rfn_decoder_step')
        self.t += 1
        if head:
            self._head(out)
        return out

    def reorder(self, order):
        """Row r continues from row order[r] (int32, device): rfn_gather_rows on h and c."""
        if order.dtype != torch.int32 or not order.is_contiguous():
            order = order.to(torch.int32).contiguous()
        h2, c2 = torch.empty_like(self.h), torch.empty_like(self.c)
        st = N.stream_ptr()
        N.check(N.lib.rfn_gather_rows(self.h.data_ptr(), h2.data_ptr(), order.data_ptr(), self.B, self.d.R, st), 'rfn_gather_rows')
        N.check(N.lib.rfn_gather_rows(self.c.data_ptr(), c2.data_ptr(), order.data_ptr(), self.B, self.d.R, st), 'rfn_gather_rows')
        self.h, self.c = h2, c2


def early_exit(alive, S):
    """The reference's early exit (misc/RecurrentFusionModel.py:645): the first t >= 1 with no unfinished row, S + 1 without
    one.  alive[t - 1]: the rows still unfinished after the t-th token (a host list)."""
    return next((t for t in range(1, S + 1) if alive[t - 1] == 0), S + 1)


class GreedyBuffers:
    """What a greedy / sampled loop over B rows writes.  `it` is the token fed next: rfn_decoder_loop sets it itself, a
    host-stepped loop feeds it at t = 0 and asks for `bos=True` (zeros)."""

    def __init__(self, B, S, V1, dev, bos=False):
        self.S = S
        self.logp_all = torch.empty(B, S + 1, V1, device=dev)
        self.seq = torch.zeros(B, S, dtype=torch.long, device=dev)
        self.seq_lp = torch.zeros(B, S, device=dev)
        self.unf = torch.zeros(S + 1, B, dtype=torch.int32, device=dev)
        self.it = (torch.zeros if bos else torch.empty)(B, dtype=torch.long, device=dev)

    def read_back(self):
        """The call's one synchronisation: the unfinished counts come to the host -> (seq, seq_lp, logp_all) cut there."""
        t_stop = early_exit(self.unf[1:].sum(1).tolist(), self.S)
        return self.seq[:, :t_stop - 1], self.seq_lp[:, :t_stop - 1], self.logp_all[:, :t_stop].contiguous()

    def read_back_picked(self, best, n):
        """read_back for one picked row per image (best (B / n,) int64, row best[k] of image k's n rows; a pick of -1 gives
        zeros): the rows are gathered on the device (one launch for seq and seq_lp) and cut at THEIR early exit, with the same
        single synchronisation."""
        from . import rewards as RW
        rows = torch.arange(best.numel(), device=best.device) * n + best.clamp(min=0)
        seq, seq_lp, _ = RW.consensus_gather(best, n, self.seq, self.seq_lp)
        logp, unf = self.logp_all.index_select(0, rows), self.unf.index_select(1, rows)
        t_stop = early_exit(unf[1:].sum(1).tolist(), self.S)
        return seq[:, :t_stop - 1], seq_lp[:, :t_stop - 1], logp[:, :t_stop].contiguous()


def _refuse_mos_device_loop(stepper, what):
    if getattr(stepper, 'mos', None) is not None:
        raise N.RfnError('use_mos: %s runs the logit layer inside the device loop; a mixture-of-softmaxes model decodes through '
                         'the host-stepped loops' % what)


def host_greedy_loop(step, B, S, V1, dev, cons=None):
    """The greedy free-running loop stepped from the host (the ensemble's, and a mixture-of-softmaxes model's): step(ids, out)
    runs one decoder step of every row on the tokens `ids` (B,) and leaves the rows' pre-softmax logits in out (B, V1); the
    log-softmax, the constraints and the pick are kernels, and nothing is read back -> the filled GreedyBuffers (read_back()
    is the call's one synchronisation).  cons: a parsed _Constraints or None, applied to the log-probs."""
    st = N.stream_ptr()
    logits = torch.empty(B, V1, device=dev)
    bufs = GreedyBuffers(B, S, V1, dev, bos=True)      # `it` = the BOS token fed at t = 0
    logp_all, seq, seq_lp, unf, it = bufs.logp_all, bufs.seq, bufs.seq_lp, bufs.unf, bufs.it
    if cons is not None:
        cons.bind(B, dev)
    for t in range(S + 1):
        if t >= 1:
            prev = logp_all[:, t - 1]
            if cons is not None:
                cons.blocklist(seq, seq.stride(0), 1, t)
                cons.mask(prev)
            N.check(N.lib.rfn_greedy_pick(prev.data_ptr(), prev.stride(0), B, V1, t, it.data_ptr(),
                                          seq[:, t - 1].data_ptr(), seq.stride(0), seq_lp[:, t - 1].data_ptr(),
                                          seq_lp.stride(0), unf[t - 1].data_ptr() if t > 1 else None,
                                          unf[t].data_ptr(), st), 'rfn_greedy_pick')
        step(it, logits)
        out = logp_all[:, t]
        N.check(N.lib.rfn_log_softmax_fwd(logits.data_ptr(), V1, B, V1, B, out.stride(0), 0, out.data_ptr(), st))
    return bufs


def host_beam_loop(step, reorder, B, W, S, V1, dev, cons=None, div=None):
    """The beam search stepped from the host on B * W rows (row k * W + q = image k): step(ids, out) as in host_greedy_loop on
    out (B * W, V1); reorder(order) re-gathers the rows' decoder state after a fork.  The candidate / stable-sort / fork /
    done-beam rules run on the device (rfn_beam_step_topk / _div) on the W best entries of each row's log-softmax
    (rfn_log_softmax_topk, masked under constraints) -> the filled BeamBuffers for _sorted_done_beams."""
    st = N.stream_ptr()
    b = BeamBuffers(B, W, S, dev, div.groups if div is not None else 1)
    rows = b.rows
    topv, topi = b.top_lists()
    logits = torch.empty(rows, V1, device=dev)
    if cons is not None:
        cons.bind(rows, dev)
    for t in range(S + 1):
        if t >= 1:
            b.step(topv, topi, V1, t, div)
            if t == S:
                break                      # the reference runs one more decoder step whose output is never used
            reorder(b.order)
        step(b.ids, logits)
        if cons is not None:     # the lists of step t + 1 from the beam arrays rfn_beam_step_topk has just forked
            cons.blocklist(b.bs, 1, rows, t + 1)
            cons.topk(logits, W, topv, topi)
        else:
            N.check(N.lib.rfn_log_softmax_topk(logits.data_ptr(), V1, rows, V1, W, topv.data_ptr(), topi.data_ptr(), st),
                    'rfn_log_softmax_topk')
    return b


def run_greedy_loop(stepper, bufs, mode, inv_temp, u, cons, samp=None):
    """The whole free-running loop (pick, embed, cell, logit, log-softmax) in one call.  mode 0: greedy; 1: draw with the
    uniforms u (S, B) at inverse temperature inv_temp.  cons: a parsed _Constraints or None; samp: a parsed _Sampling or None
    (with samp.n > 1 the stepper's B rows are n per thought vector, image-major)."""
    b, B = bufs, stepper.B
    _refuse_mos_device_loop(stepper, 'rfn_decoder_loop')
    N.check(N.lib.rfn_decoder_loop_ex2(C.byref(stepper.d), B, b.S + 1, stepper.table, stepper.comb.data_ptr(),
                                       stepper.cproj.data_ptr(), stepper.h.data_ptr(), stepper.c.data_ptr(), mode, inv_temp,
                                       N.ptr(u), b.logp_all.data_ptr(), b.logp_all.stride(0), b.logp_all.stride(1),
                                       b.seq.data_ptr(), b.seq.stride(0), b.seq_lp.data_ptr(), b.seq_lp.stride(0), b.unf.data_ptr(),
                                       b.it.data_ptr(), stepper.ws.data_ptr(), stepper.ws_bytes, stepper.seed,
                                       C.byref(cons.bind(B, stepper.h.device).struct) if cons is not None else None,
                                       C.byref(samp.struct()) if samp is not None else None,
                                       N.stream_ptr()), 'rfn_decoder_loop_ex2')


class _BeamArrays:
    """The arrays every beam search over B images x W rows x S steps keeps: the rows' tokens and log-probs so far (`bs`, `bl`), the
    fork order and the tokens fed next.  The rows' top-W lists are uninitialised storage, one float buffer (`top_flat`,
    rfn_beam_loop).  What a search does not keep reads as None (the stochastic search has no sums and no done beams)."""

    bsum = done_seq = done_lp = done_p = done_n = active = None

    def __init__(self, B, W, S, dev):
        self.B, self.W, self.S, self.dev = B, W, S, dev
        self.rows, self.max_done = B * W, W * S
        self.bs = torch.zeros(S, B, W, dtype=torch.long, device=dev)
        self.bl = torch.zeros(S, B, W, device=dev)
        self.order = torch.zeros(self.rows, dtype=torch.int32, device=dev)
        self.ids = torch.zeros(self.rows, dtype=torch.long, device=dev)

    def top_flat(self):
        return torch.empty(2 * self.rows * self.W, device=self.dev)


class BeamBuffers(_BeamArrays):
    """The state of a beam search with done beams.  A host-stepped search takes the rows' top-W lists as values and indices
    (`top_lists`) and advances with `step`.  `done_group` (the group of every done beam) exists only for a diverse search
    (groups > 1), `state_n` / `done_state` (the occupied rows of every state, the state of every done beam) only for a lexically
    constrained one (states = 2^C > 1; W then counts all rows)."""

    def __init__(self, B, W, S, dev, groups=1, states=1):
        super().__init__(B, W, S, dev)
        max_done = self.max_done
        self.bsum = torch.zeros(B, W, device=dev)
        self.done_seq = torch.zeros(B, max_done, S, dtype=torch.long, device=dev)
        self.done_lp = torch.zeros(B, max_done, S, device=dev)
        self.done_p = torch.zeros(B, max_done, device=dev)
        self.done_n = torch.zeros(B, dtype=torch.int32, device=dev)
        self.active = torch.ones(B, dtype=torch.int32, device=dev)
        self.done_group = torch.zeros(B, max_done, dtype=torch.int32, device=dev) if groups > 1 else None
        self.state_n = torch.zeros(B, states, dtype=torch.int32, device=dev) if states > 1 else None
        self.done_state = torch.zeros(B, max_done, dtype=torch.int32, device=dev) if states > 1 else None

    def top_lists(self):
        return torch.empty(self.rows, self.W, device=self.dev), torch.empty(self.rows, self.W, dtype=torch.int32, device=self.dev)

    def step(self, topv, topi, V1, t, div=None):
        """One step of a host-stepped search (the ensemble's) on the rows' top-W lists: rfn_beam_step_topk, or rfn_beam_step_div
        with a parsed _Diversity."""
        tail = (self.S, t, self.B, self.max_done, self.bs.data_ptr(), self.bl.data_ptr(), self.bsum.data_ptr(), self.order.data_ptr(),
                self.ids.data_ptr(), self.done_seq.data_ptr(), self.done_lp.data_ptr(), self.done_p.data_ptr(), self.done_n.data_ptr())
        if div is not None:
            N.check(N.lib.rfn_beam_step_div(topv.data_ptr(), topi.data_ptr(), V1, self.W, div.groups, div.lam, *tail,
                                            self.done_group.data_ptr(), self.active.data_ptr(), N.stream_ptr()), 'rfn_beam_step_div')
        else:
            N.check(N.lib.rfn_beam_step_topk(topv.data_ptr(), topi.data_ptr(), V1, self.W, *tail, self.active.data_ptr(),
                                             N.stream_ptr()), 'rfn_beam_step_topk')


def run_beam_loop(stepper, bufs, cons, div=None, lex=None, sbs_seed=None):
    """The whole search in one call (rfn_beam_loop_ex4): S x (bookkeeping, state re-gather, decoder step on the B * W rows).
    cons: a parsed _Constraints or None; div: a parsed _Diversity or None (bufs then holds done_group); lex: a parsed _Lexical or
    None (bufs then holds state_n / done_state); sbs_seed: the 64-bit key of the Gumbel noise of a stochastic search (bufs is then
    a StochasticBuffers; the stepper's own seed keys the dropout masks, as everywhere)."""
    b, logp = bufs, bufs.top_flat()
    _refuse_mos_device_loop(stepper, 'rfn_beam_loop')
    h_alt, c_alt = torch.empty_like(stepper.h), torch.empty_like(stepper.c)
    N.check(N.lib.rfn_beam_loop_ex4(C.byref(stepper.d), b.B, b.W, b.S, stepper.table, stepper.comb.data_ptr(),
                                    stepper.cproj.data_ptr(), stepper.h.data_ptr(), stepper.c.data_ptr(), h_alt.data_ptr(),
                                    c_alt.data_ptr(), logp.data_ptr(), b.bs.data_ptr(), b.bl.data_ptr(), N.ptr(b.bsum),
                                    b.order.data_ptr(), b.ids.data_ptr(), N.ptr(b.done_seq), N.ptr(b.done_lp),
                                    N.ptr(b.done_p), N.ptr(b.done_n), N.ptr(b.active), b.max_done,
                                    stepper.ws.data_ptr(), stepper.ws_bytes, stepper.seed,
                                    C.byref(cons.bind(b.rows, b.dev).struct) if cons is not None else None,
                                    C.byref(div.struct(b)) if div is not None else None,
                                    C.byref(lex.struct(b)) if lex is not None else None,
                                    C.byref(b.struct(sbs_seed)) if sbs_seed is not None else None, N.stream_ptr()),
            'rfn_beam_loop_ex4')


class _Stochastic:
    """Stochastic beam search of one call (rfn.h "stochastic beam search"; RecurrentFusionModel.sample_distinct): opt['seed'] (a
    64-bit integer, None = a fresh one from torch's generator) keys the Gumbel noise; the decoding constraints' keys are parsed by
    _Constraints.  Every other key is refused by name: the search samples the model's own distribution, so nothing that reshapes it
    (temperature, top_k, top_p), ranks its rows otherwise (length_penalty, consensus, group_size, require) or replays tokens
    (force_ids) applies."""

    KEYS = ('seed', 'block_ngram', 'banned_ids', 'bad_endings')
    MAX_N = MAX_BEAM

    @classmethod
    def parse(cls, opt, n, S):
        temp = opt.get('temperature', None)                  # the neutral value is not an error
        bad = sorted(k for k in opt if k not in cls.KEYS and not (k == 'temperature' and (temp is None or float(temp) == 1.0)))
        if bad:
            raise ValueError('sample_distinct takes %s, not %s' % (', '.join(cls.KEYS), ', '.join(map(repr, bad))))
        if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= cls.MAX_N:
            raise ValueError('sample_distinct draws 1 <= n <= %d captions per image, got %r' % (cls.MAX_N, n))
        if S > MAX_STEPS:
            raise N.RfnError('stochastic beam search supports seq_length <= 64')
        seed = opt.get('seed', None)
        if seed is not None and (isinstance(seed, bool) or int(seed) != seed):
            raise ValueError('seed must be an integer, got %r' % (seed,))
        s = cls()
        s.n, s.seed = int(n), (None if seed is None else int(seed) & (2 ** 64 - 1))
        return s


class StochasticBuffers(_BeamArrays):
    """The state of a stochastic beam search over B images x W rows x S steps: the beam arrays (it has no done beams: finished rows
    stay in the beam), and phi / gumbel / live, weight / n_live and the rows' keys."""

    def __init__(self, B, W, S, dev):
        super().__init__(B, W, S, dev)
        self.phi = torch.zeros(B, W, dtype=torch.float64, device=dev)
        self.gumbel = torch.zeros(B, W, dtype=torch.float64, device=dev)
        self.live = torch.zeros(B, W, dtype=torch.int32, device=dev)       # the loop sets the three (rfn_beam_sbs_begin)
        self.weight = torch.zeros(B, W, dtype=torch.float64, device=dev)
        self.n_live = torch.zeros(B, dtype=torch.int32, device=dev)
        self.topk64 = torch.empty(self.rows, W, dtype=torch.float64, device=dev)

    def struct(self, seed, offset0=0):
        self._struct = N.BeamStochastic(seed, offset0, self.phi.data_ptr(), self.gumbel.data_ptr(), self.live.data_ptr(),
                                        self.weight.data_ptr(), self.n_live.data_ptr(), self.topk64.data_ptr())
        return self._struct


class _Constraints:
    """The decoding constraints of one call (rfn.h "decoding constraints"): opt['block_ngram'] (0 = off, 2 .. 4),
    opt['banned_ids'] and opt['bad_endings'] (at most 64 ids each, token 0 never banned).  `parse` returns None when all of
    them are off, so an unconstrained call issues exactly the launches it always did.  `bind` uploads the id lists (once per
    call) and allocates the per-row block lists; `blocklist` / `mask` / `topk` are the three kernels for a host-side step
    loop (the ensemble's), `struct` is what the device loops take."""

    KEYS = ('block_ngram', 'banned_ids', 'bad_endings')

    @staticmethod
    def _ids(opt, key, V1):
        v = opt.get(key, None)
        if v is None:
            return []
        ids = sorted(set(int(x) for x in (v.tolist() if torch.is_tensor(v) else v)))
        if len(ids) > N.DECODE_MAX_IDS:
            raise ValueError('%s holds %d ids, at most %d are supported' % (key, len(ids), N.DECODE_MAX_IDS))
        if ids and (ids[0] < 0 or ids[-1] >= V1):
            raise ValueError('%s must hold token ids in [0, %d)' % (key, V1))
        return ids

    @classmethod
    def parse(cls, opt, V1, S):
        n = int(opt.get('block_ngram', 0) or 0)
        if n != 0 and not 2 <= n <= 4:
            raise ValueError('block_ngram must be 0 (off) or 2 .. 4, got %d' % n)
        banned, bad = cls._ids(opt, 'banned_ids', V1), cls._ids(opt, 'bad_endings', V1)
        if 0 in banned:
            raise ValueError('token 0 (END) cannot be banned')
        if not (n or banned or bad):
            return None
        if S > MAX_STEPS:
            raise N.RfnError('decoding constraints support seq_length <= 64')
        c = cls()
        c.n, c.banned, c.bad, c.V1, c.S = n, banned, bad, V1, S
        return c

    def bind(self, rows, dev):
        self.rows = rows
        self.banned_d = torch.tensor(self.banned or [0], dtype=torch.int32, device=dev)
        self.bad_d = torch.tensor(self.bad or [0], dtype=torch.int32, device=dev)
        self.blk = torch.empty(rows, N.DECODE_MAX_IDS + self.S, dtype=torch.int32, device=dev)
        self.blk_n = torch.empty(rows, dtype=torch.int32, device=dev)
        self.struct = N.DecodeConstraints(self.n, len(self.banned), len(self.bad), 0, self.banned_d.data_ptr(),
                                          self.bad_d.data_ptr(), self.blk.data_ptr(), self.blk_n.data_ptr())
        return self

    def blocklist(self, hist, s_row, s_tok, t):
        """The rows' blocked ids at step t (which picks the t-th token) from their histories (rfn_decode_blocklist)."""
        N.check(N.lib.rfn_decode_blocklist(hist.data_ptr(), s_row, s_tok, None, self.rows, self.S, t, self.n,
                                           self.banned_d.data_ptr(), len(self.banned), self.bad_d.data_ptr(), len(self.bad),
                                           self.V1, self.blk.data_ptr(), self.blk_n.data_ptr(), N.stream_ptr()),
                'rfn_decode_blocklist')

    def mask(self, logp):
        N.check(N.lib.rfn_logp_mask_rows(logp.data_ptr(), logp.stride(0), self.rows, self.V1, self.blk.data_ptr(),
                                         self.blk.stride(0), self.blk_n.data_ptr(), N.stream_ptr()), 'rfn_logp_mask_rows')

    def topk(self, logits, W, topv, topi):
        N.check(N.lib.rfn_log_softmax_topk_masked(logits.data_ptr(), logits.stride(0), self.rows, self.V1, W, self.blk.data_ptr(),
                                                  self.blk.stride(0), self.blk_n.data_ptr(), topv.data_ptr(), topi.data_ptr(),
                                                  N.stream_ptr()), 'rfn_log_softmax_topk_masked')


class _Sampling:
    """Truncated sampling of one call (rfn.h "truncated sampling"): opt['top_k'] (int, 0 = off), opt['top_p'] (float in (0, 1],
    1.0 = off) and opt['sample_n'] (int >= 1 draws per image).  `parse` returns None when all three are off, so such a call
    issues exactly the launches it always did."""

    KEYS = ('top_k', 'top_p', 'sample_n')

    @classmethod
    def parse(cls, opt):
        k, p, n = opt.get('top_k', 0), opt.get('top_p', 1.0), opt.get('sample_n', 1)
        k, p, n = int(0 if k is None else k), float(1.0 if p is None else p), int(1 if n is None else n)
        if k < 0:
            raise ValueError('top_k must be >= 0 (0 = off), got %d' % k)
        if not 0.0 < p <= 1.0:
            raise ValueError('top_p must be in (0, 1] (1 = off), got %r' % p)
        if n < 1:
            raise ValueError('sample_n must be >= 1, got %d' % n)
        if k == 0 and p == 1.0 and n == 1:
            return None
        s = cls()
        s.k, s.p, s.n = k, p, n
        return s

    def struct(self):
        self._struct = N.DecodeSampling(self.k, self.p, self.n, 0)
        return self._struct


class _Diversity:
    """Diverse beam search of one call (rfn.h "diverse beam search"): opt['group_size'] = G (default 1) groups of beam_size / G
    beams each, opt['diversity_lambda'] (default 0.5) the Hamming penalty per earlier group that chose the token at this step.
    `parse` returns None for G == 1, whatever lambda is, so such a call issues exactly the launches it always did."""

    @classmethod
    def parse(cls, opt, W):
        g, lam = opt.get('group_size', 1), opt.get('diversity_lambda', 0.5)
        g, lam = int(1 if g is None else g), float(0.5 if lam is None else lam)
        if g < 1:
            raise ValueError('group_size must be >= 1, got %d' % g)
        if W % g:
            raise ValueError('beam_size %d is not a multiple of group_size %d' % (W, g))
        if not lam >= 0.0:
            raise ValueError('diversity_lambda must be >= 0, got %r' % lam)
        if g == 1:
            return None
        d = cls()
        d.groups, d.lam = g, lam
        return d

    def struct(self, bufs):
        self._struct = N.BeamDiversity(self.groups, self.lam, bufs.done_group.data_ptr())
        return self._struct


class _Lexical:
    """Lexically constrained beam search of one call (rfn.h "lexically constrained beam search"): opt['require'] names, per image,
    up to 3 sets of token ids, and the returned caption should hold one id of every set -- a (B, C, K) integer tensor padded with
    -1, or B lists of lists of ids.  opt['beam_size'] = Wb is then the beam of every one of the 2^C states, and the search runs
    W = Wb * 2^C <= 32 rows per image.  `parse` returns None when no image has a non-empty set, so such a call issues exactly the
    launches it always did.  Per image the unique ids (at most 16, and at most W - Wb: the bound under which the rows' W-wide top
    lists suffice) become `want` with a set mask each in `want_bits`; `init_state` holds the bits of the image's empty sets."""

    @staticmethod
    def _sets(req, B):
        if torch.is_tensor(req):
            if req.dim() != 3 or req.is_floating_point():
                raise ValueError('require must be a (B, C, K) integer tensor, got %s %s' % (tuple(req.shape), req.dtype))
            req = [[[v for v in ids if v != -1] for ids in img] for img in req.tolist()]
        else:
            req = [[[int(v) for v in (ids.tolist() if torch.is_tensor(ids) else ids)] for ids in img] for img in req]
        if len(req) != B:
            raise ValueError('require names the sets of %d images, the batch holds %d' % (len(req), B))
        return req

    @classmethod
    def parse(cls, opt, B, V1, Wb):
        req = opt.get('require', None)
        if req is None:
            return None
        req = cls._sets(req, B)
        if not any(len(ids) for img in req for ids in img):
            return None
        nsets = max(len(img) for img in req)
        if nsets > N.LEX_MAX_SETS:
            raise ValueError('require holds %d sets for an image, at most %d are supported' % (nsets, N.LEX_MAX_SETS))
        W = Wb << nsets
        if W > MAX_BEAM:
            raise ValueError('beam_size %d with %d required sets needs %d rows per image, at most 32 are supported' % (Wb, nsets, W))
        want, bits, init = [], [], []
        for img in req:
            w, m, i0 = [], [], 0
            for i in range(nsets):
                ids = img[i] if i < len(img) else []
                if not ids:
                    i0 |= 1 << i
                for v in ids:
                    if not 1 <= v < V1:
                        raise ValueError('require must hold token ids in [1, %d), got %d' % (V1, v))
                    if v not in w:
                        w.append(v)
                        m.append(0)
                    m[w.index(v)] |= 1 << i
            want.append(w)
            bits.append(m)
            init.append(i0)
        nw = max(len(w) for w in want)
        if nw > N.LEX_MAX_IDS:
            raise ValueError('require holds %d ids for an image, at most %d are supported' % (nw, N.LEX_MAX_IDS))
        if nw > W - Wb:
            raise ValueError('require holds %d ids for an image: with beam_size %d and %d sets at most %d are supported'
                             % (nw, Wb, nsets, W - Wb))
        lx = cls()
        lx.C, lx.G, lx.Wb, lx.W, lx.NW = nsets, 1 << nsets, Wb, W, nw
        lx.want = [w + [-1] * (nw - len(w)) for w in want]
        lx.want_bits = [m + [0] * (nw - len(m)) for m in bits]
        lx.init_state = init
        return lx

    def bind(self, dev):
        up = lambda x: torch.tensor(x, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)  # noqa: E731
        self.want_d, self.bits_d, self.init_d = up(self.want), up(self.want_bits), up(self.init_state)
        return self

    def struct(self, bufs):
        self.wantv = torch.empty(bufs.rows, self.NW, device=bufs.dev)
        self._struct = N.BeamLexical(self.C, self.NW, self.want_d.data_ptr(), self.bits_d.data_ptr(), self.init_d.data_ptr(),
                                     self.wantv.data_ptr(), bufs.state_n.data_ptr(), bufs.done_state.data_ptr())
        return self._struct

    def met(self, state):
        """state (B,) int32, the state of every image's returned caption -> how many of the image's non-empty sets it satisfies."""
        table = torch.tensor([bin(x).count('1') for x in range(self.G)], dtype=torch.int32, device=state.device)
        return table[(state & ~self.init_d).long()]


class _Consensus:
    """Consensus reranking of one call (rfn.h "consensus reranking"): opt['consensus'] = a rewards.CiderD scorer keeps, of an
    image's candidates, the one that agrees most with the others under CIDEr-D.  sample: the candidates are the sample_n draws,
    uniformly weighted.  sample_beam: opt['consensus_n'] = m (default beam_size, at most 32) ranked done beams -- or, with
    group_size = G > 1, the G group bests -- weighted by opt['consensus_weights'] = 'uniform' (default) or 'prob' (w_j =
    exp(p_j - max_j p_j)).  `parse` returns None without the key, so such a call issues exactly the launches it always did."""

    KEYS = ('consensus', 'consensus_n', 'consensus_weights')
    MAX_N = 32

    @classmethod
    def parse(cls, opt, V1, S, default_n):
        scorer = opt.get('consensus', None)
        if scorer is None:
            stray = [k for k in cls.KEYS[1:] if opt.get(k, None) is not None]
            if stray:
                raise ValueError('%s without a \'consensus\' scorer' % ' / '.join(stray))
            return None
        from . import rewards as RW
        if not isinstance(scorer, RW.CiderD):
            raise NotImplementedError('consensus reranking is implemented for the CiderD scorer only, got %s'
                                      % type(scorer).__name__)
        if V1 > RW.MAX_ID + 1 or S > RW.MAX_T:
            raise N.RfnError('consensus reranking supports vocab_size + 1 <= %d and seq_length <= %d' % (RW.MAX_ID + 1, RW.MAX_T))
        m = opt.get('consensus_n', None)
        m = int(default_n if m is None else m)
        if not 1 <= m <= cls.MAX_N:
            raise ValueError('consensus_n must be in 1 .. %d, got %d' % (cls.MAX_N, m))
        how = opt.get('consensus_weights', None) or 'uniform'
        if how not in ('uniform', 'prob'):
            raise ValueError("consensus_weights is 'uniform' or 'prob', got %r" % (how,))
        c = cls()
        c.scorer, c.n, c.how, c.result = scorer, m, how, None
        return c

    @classmethod
    def parse_sample(cls, opt, V1, S, samp, sample_max):
        """sample's form of the keys: the candidates are the call's sample_n > 1 multinomial draws."""
        if opt.get('consensus', None) is None:
            return cls.parse(opt, V1, S, 1)
        if sample_max:
            raise ValueError('consensus reranks multinomial draws: it needs sample_max=0 (beam search takes it with beam_size > 1)')
        if samp is None or samp.n < 2:
            raise ValueError('consensus needs sample_n > 1 draws per image to choose from')
        if opt.get('consensus_n', None) is not None or opt.get('consensus_weights', None) not in (None, 'uniform'):
            raise ValueError('sample reranks all sample_n draws with uniform weights: consensus_n / consensus_weights are '
                             'sample_beam keys')
        return cls.parse(opt, V1, S, samp.n)

    def pick(self, cands, n_cand=None, p=None):
        """cands (B, n, S) int64 -> best (B,); sets self.result = {'index', 'scores'} (device tensors, nothing read back).
        p (B, n) float32 log-probs: the weights under 'prob'."""
        from . import rewards as RW
        weights = None
        if self.how == 'prob':
            pd = p.double()
            if n_cand is not None:
                valid = torch.arange(cands.size(1), device=cands.device)[None, :] < n_cand[:, None]
                pd = torch.where(valid, pd, torch.full_like(pd, float('-inf')))
            weights = (pd - pd.max(1, keepdim=True).values).exp()
        best, scores, _ = RW.consensus(self.scorer, cands, n_cand, weights)
        self.result = {'index': best, 'scores': scores}
        return best


class _Scoring:
    """Caption scoring of one call (rfn.h "caption scoring"; RecurrentFusionModel.score / EnsembleDecoder.score): opt['n'] (int >= 1
    captions per image when seq is (B * n, T); a (B, n, T) seq carries its own), opt['length_penalty'] = alpha >= 0 ('score' =
    logprob / length^alpha), opt['outputs'] (names among 'rank', 'entropy': the optional per-token outputs), opt['include_end']
    (bool, default True: the caption's END is scored with its words) and opt['max_rows'] (int >= 1: caption rows per native call).
    Unknown keys and bad values raise ValueError; nothing here touches a device."""

    KEYS = ('n', 'length_penalty', 'outputs', 'include_end', 'max_rows')
    OUTPUTS = ('rank', 'entropy')
    SLAB_BYTES = 1 << 30           # default max_rows: the (steps * rows, V+1) logits of one native call stay under this

    @classmethod
    def parse(cls, opt):
        bad = sorted(k for k in opt if k not in cls.KEYS)
        if bad:
            raise ValueError('score takes %s, not %s' % (', '.join(cls.KEYS), ', '.join(map(repr, bad))))
        s = cls()
        s.n = cls._count(opt, 'n')
        s.alpha = _length_penalty(opt)
        outs = opt.get('outputs', None)
        outs = () if outs is None else ((outs,) if isinstance(outs, str) else tuple(outs))
        unknown = [o for o in outs if o not in cls.OUTPUTS]
        if unknown:
            raise ValueError("outputs names 'rank' and / or 'entropy', got %r" % (unknown,))
        s.rank, s.entropy = 'rank' in outs, 'entropy' in outs
        end = opt.get('include_end', True)
        if not isinstance(end, (bool, int)) or end not in (0, 1):
            raise ValueError('include_end is True or False, got %r' % (end,))
        s.include_end = bool(end)
        s.max_rows = cls._count(opt, 'max_rows')
        return s

    @staticmethod
    def _count(opt, key):
        v = opt.get(key, None)
        if v is None:
            return None
        try:
            ok = not isinstance(v, bool) and int(v) == v and int(v) >= 1
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError('%s must be an integer >= 1, got %r' % (key, v))
        return int(v)

    def layout(self, shape, B, seq_length):
        """seq of `shape` for B images -> (rows, n, T): (B, T), (B, n, T), or (B * n, T) with opt['n']."""
        shape = tuple(int(x) for x in shape)
        if len(shape) == 3:
            if shape[0] != B or shape[1] < 1 or (self.n is not None and self.n != shape[1]):
                raise ValueError('seq %s does not hold n%s captions for each of %d images'
                                 % (shape, '' if self.n is None else ' = %d' % self.n, B))
            n, T = shape[1], shape[2]
        elif len(shape) == 2:
            n, T = (1 if self.n is None else self.n), shape[1]
            if shape[0] != B * n:
                raise ValueError('seq %s does not hold %d x %d caption rows' % (shape, B, n))
        else:
            raise ValueError('seq must be (B, T), (B, n, T) or (B * n, T), got %s' % (shape,))
        if not 1 <= T <= seq_length + 1:
            raise ValueError('seq holds %d columns, 1 .. seq_length + 1 = %d are scored' % (T, seq_length + 1))
        return B * n, n, T

    def rows_per_call(self, n, steps, V1):
        """max_rows rounded down to a multiple of n, at least n."""
        mr = self.max_rows if self.max_rows is not None else self.SLAB_BYTES // (4 * steps * V1)
        return max(n, mr // n * n)


class ScoreBuffers:
    """What a scoring pass over `rows` captions reads and writes: `feed` (rows, steps + 1) int64 with column 0 = BOS, the words
    behind it and zeros to the end -- column s feeds step s, column s + 1 is scored there -- and the outputs."""

    def __init__(self, so, seq, rows, T, seq_length, dev):
        L = min(T, seq_length)
        self.so, self.rows, self.steps = so, rows, L + 1
        self.feed = torch.zeros(rows, L + 2, dtype=torch.long, device=dev)
        self.feed[:, 1:L + 1] = seq.reshape(rows, T)[:, :L].to(dev)
        self.target = self.feed[:, 1:]
        self.tok_lp = torch.empty(rows, L + 1, device=dev)
        self.rank = torch.empty(rows, L + 1, dtype=torch.int32, device=dev) if so.rank else None
        self.ent = torch.empty(rows, L + 1, device=dev) if so.entropy else None
        self.cap_lp = torch.empty(rows, dtype=torch.float64, device=dev)
        self.cap_len = torch.empty(rows, dtype=torch.int32, device=dev)

    def result(self):
        """The dict score() returns.  'score' = logprob / length^alpha, one IEEE division in fp64 by the host table
        _sorted_done_beams ranks with (length 0 divides by 1)."""
        if self.so.alpha == 0.0:
            score = self.cap_lp.clone()                     # every divisor is 1.0
        else:
            # pinned and non-blocking: a pageable upload would make the host wait here for everything queued so far
            table = torch.tensor([1.0] + [float(k) ** self.so.alpha for k in range(1, self.steps + 1)], dtype=torch.float64)
            score = self.cap_lp / table.pin_memory().to(self.cap_lp.device, non_blocking=True)[self.cap_len.long()]
        out = {'token_logprobs': self.tok_lp, 'logprob': self.cap_lp, 'length': self.cap_len, 'score': score}
        if self.rank is not None:
            out['rank'] = self.rank
        if self.ent is not None:
            out['entropy'] = self.ent
        return out


def rescore(scorer, fc_feats, att_feats, cands, n_cand=None, opt={}, att_lens=None):
    """n-best rescoring: score an image's m candidates with `scorer` (anything with .score: a RecurrentFusionModel, an
    EnsembleDecoder) -> (best (B,) int64, scores (B, m) f64).  cands (B, m, T) int64 as `model.candidates['seq']` after
    keep_candidates, or a sample_n call's rows viewed per image; n_cand (B,) counts the valid ones (None: all m).  scores[k, j] is
    the scorer's 'score' (opt['length_penalty'] applies), -inf for j >= n_cand[k]; best[k] is the first maximum, -1 where
    n_cand[k] == 0 (rewards.consensus_gather writes zeros for it).  Nothing is read back.  att_lens: the scorer's keyword (ragged
    attention maps), passed on when given."""
    if cands.dim() != 3:
        raise ValueError('cands must be (B, m, T), got %s' % (tuple(cands.shape),))
    B, m = cands.size(0), cands.size(1)
    kw = {} if att_lens is None else {'att_lens': att_lens}
    scores = scorer.score(fc_feats, att_feats, cands, opt, **kw)['score'].view(B, m)
    if n_cand is not None:
        valid = torch.arange(m, device=scores.device)[None, :] < n_cand.to(scores.device)[:, None]
        scores = torch.where(valid, scores, torch.full_like(scores, float('-inf')))
    top = scores.max(1, keepdim=True).values
    best = (scores == top).to(torch.int8).argmax(1)                               # first maximum
    if n_cand is not None:
        best = torch.where(n_cand.to(best.device) > 0, best, torch.full_like(best, -1))
    return best, scores


def _beam_candidates(m, s_all, l_all, p_all, done_n, g_all, groups):
    """The candidate set of one sample_beam call, from _sorted_done_beams' gathers -> (cands (B, n, S), lps, p (B, n), n_cand or None
    (all valid), n).  groups == 1: the first min(done_n, m) ranked beams.  groups > 1: the G group bests -- the first ranked beam of
    every group, found here on the device (every group has a done beam: its beams are all done after the last step)."""
    S = s_all.size(2)
    if groups > 1:
        valid = torch.arange(s_all.size(1), device=s_all.device)[None, :] < done_n[:, None]
        of_group = (g_all[:, None, :] == torch.arange(groups, device=s_all.device, dtype=g_all.dtype)[None, :, None]) & valid[:, None, :]
        first = of_group.to(torch.int8).argmax(2)                                   # first maximum = first beam of the group
        pick = first[:, :, None].expand(-1, -1, S)
        return s_all.gather(1, pick), l_all.gather(1, pick), p_all.gather(1, first), None, groups
    m = min(m, s_all.size(1))
    return s_all[:, :m].contiguous(), l_all[:, :m].contiguous(), p_all[:, :m].contiguous(), done_n.clamp(max=m), m


def _consensus_beams(cs, cands, lps, p, n_cand, m):
    """sample_beam's pick among its candidates (_beam_candidates) -> (seq, seq_lp) of the chosen candidate per image; the index is
    the rank (groups == 1) or the group."""
    from . import rewards as RW
    best = cs.pick(cands, n_cand, p)
    seq, seq_lp, _ = RW.consensus_gather(best, m, cands, lps)
    return seq, seq_lp


def labels_from_seq(seq, seq_length=None):
    """Decoded ids -> the (labels, masks) a loader hands forward_loss, for sequence-level distillation: decode with the teacher
    (sample_beam, EnsembleDecoder.sample_beam, the rows of sample_distinct's candidates), turn the ids into labels here, train
    the student on them with the usual forward_loss.  seq (B, S') integer ids, 0 = END / padding; S = seq_length (default S',
    not below it).
      labels (B, S + 2) int64: column 0 is 0 (BOS), then the caption with everything from its first 0 onward zeroed;
      masks  (B, S + 2) float32: ones over the first n + 2 columns, n = the tokens before the first 0 (BOS, the n words, END)
    -- what the reference's loader writes for a ground-truth caption (dataloader.py:285, :312-315).  Tensor ops on seq's device
    only: no host synchronisation."""
    if not torch.is_tensor(seq) or seq.dim() != 2 or seq.is_floating_point() or seq.is_complex() or seq.dtype == torch.bool:
        raise ValueError('seq must be a (B, S) tensor of integer token ids')
    B, Sp = seq.shape
    S = Sp if seq_length is None else int(seq_length)
    if S < Sp:
        raise ValueError('seq_length = %d is below the %d columns of seq' % (S, Sp))
    s = seq.long()
    alive = (s != 0).long().cumprod(1)                       # 1 up to the first 0, 0 from there on
    labels = s.new_zeros(B, S + 2)
    labels[:, 1:Sp + 1] = s * alive
    n = alive.sum(1, keepdim=True)
    masks = (torch.arange(S + 2, device=seq.device).unsqueeze(0) < n + 2).float()
    return labels, masks


def keep_candidates_n(opt, beam_size):
    """opt['keep_candidates']: None without the key, else how many ranked done beams a plain search keeps (consensus_n or
    beam_size; a diverse search keeps its G group bests)."""
    if not opt.get('keep_candidates', None):
        return None
    m = opt.get('consensus_n', None)
    return int(beam_size if m is None else m)


def _diverse_beams(done_beams, groups):
    """Per image the G group bests: entry g is the first of the image's ranked done beams (length penalty included) that group
    g produced.  Lazy, as done_beams is."""
    return _LazyList(len(done_beams), lambda: [[next((d for d in img if d['group'] == g), None) for g in range(groups)]
                                               for img in done_beams])


def _length_penalty(opt):
    alpha = float(opt.get('length_penalty', 0.0) or 0.0)
    if alpha < 0.0 or alpha != alpha:
        raise ValueError('length_penalty must be >= 0, got %r' % alpha)
    return alpha


def _sorted_done_beams(bufs, length_penalty=0.0, consensus=None, groups=1, keep=None, lex=None):
    """The done beams of a finished search (bufs: its BeamBuffers) sorted by -p, stably, as the reference's
    sorted(..., key=-p) (:529) -- on the device, for all images at once: the caller returns with everything queued and nothing read back, so the host's next batch (and its stage-I/II
    GEMMs) starts while this one is still decoding.  -> (seq (B, S) best done beam per image, its log-probs, and the
    per-image Python structures top_seq / top_prob / done_beams: thousands of small objects that need the done counts on
    the host, so they are lists that fill themselves on first access -- a loop that only consumes the returned captions
    never waits for them).

    length_penalty = alpha > 0 ranks by p / len^alpha instead (len: the tokens up to and including the first 0, S without one);
    ties keep construction order, and `p` / top_prob stay the raw sums.  len^alpha comes from a host table of S + 1 doubles
    and the quotient is one IEEE division in fp64, so a host re-sort of the same (p, len) reproduces the order exactly.

    bufs.done_group (a diverse search): every done beam's group goes through the same gather, and every done_beams dict gets
    it as 'group'.

    consensus (a parsed _Consensus): the returned seq and its log-probs are the consensus pick among the ranked beams
    (_consensus_beams) instead of the first of them; the lists keep their meaning and order, and nothing more is read back.

    keep (a dict, with keep['n'] = keep_candidates_n): it receives 'seq' (B, m, S) int64 and 'n_cand' (B,) int32, the candidate
    set the consensus pick chooses from (_beam_candidates), on the device; with or without `consensus`.

    bufs.done_state (a lexically constrained search): the done beams are ordered by the number of satisfied sets descending
    first, then as above; every done_beams dict gets its 'state', and lex (a dict) receives 'state' (B,) int32, the returned caption's."""
    done_seq, done_lp, done_p, done_n, done_group, done_state = (bufs.done_seq, bufs.done_lp, bufs.done_p, bufs.done_n,
                                                                 bufs.done_group, bufs.done_state)
    dev, B, S, max_done = bufs.dev, bufs.B, bufs.S, bufs.max_done
    score = done_p
    if length_penalty:
        ended = done_seq == 0
        first0 = ended.to(torch.int8).argmax(2) + 1                                  # first maximum = first 0
        length = torch.where(ended.any(2), first0, torch.full_like(first0, S))
        table = torch.tensor([1.0] + [float(n) ** float(length_penalty) for n in range(1, S + 1)], dtype=torch.float64)
        score = done_p.double() / table.to(dev)[length]
    key = torch.where(torch.arange(max_done, device=dev)[None, :] < done_n[:, None], -score,
                      torch.full_like(score, float('inf')))
    rank = torch.sort(key, dim=1, stable=True).indices
    if done_state is not None:      # a second stable sort: satisfied sets descending, the order above within equal counts
        valid = torch.arange(max_done, device=dev)[None, :] < done_n[:, None]
        nsat = torch.tensor([bin(x).count('1') for x in range(8)], device=dev)[done_state.long().clamp(0, 7)]
        unmet = torch.where(valid, -nsat, torch.ones_like(nsat)).gather(1, rank)
        rank = rank.gather(1, torch.sort(unmet, dim=1, stable=True).indices)
    pick = rank[:, :, None].expand(-1, -1, S)
    s_all, l_all, p_all = done_seq.gather(1, pick), done_lp.gather(1, pick), done_p.gather(1, rank)
    g_all = done_group.gather(1, rank) if done_group is not None else None
    st_all = done_state.gather(1, rank) if done_state is not None else None
    if lex is not None:
        lex['state'] = st_all[:, 0].contiguous()
    src = _BeamResults(s_all, l_all, p_all, done_n, g_all, st_all)
    if consensus is not None or keep is not None:
        cands, lps, p, n_cand, m = _beam_candidates(consensus.n if consensus is not None else keep['n'], s_all, l_all, p_all, done_n,
                                                    g_all, groups)
        if keep is not None:
            keep['seq'] = cands
            keep['n_cand'] = (torch.full((B,), m, dtype=torch.int32, device=dev) if n_cand is None else n_cand.to(torch.int32))
    if consensus is not None:
        seq, seq_lp = _consensus_beams(consensus, cands, lps, p, n_cand, m)
    else:
        seq, seq_lp = s_all[:, 0].contiguous(), l_all[:, 0].contiguous()
    return (seq, seq_lp, _LazyList(B, lambda: src.top_seq()),
            _LazyList(B, lambda: src.top_prob()), _LazyList(B, lambda: src.done_beams()))


class _BeamResults:
    """Host copies of the sorted done beams, fetched once, on demand."""

    def __init__(self, s_all, l_all, p_all, done_n, g_all=None, st_all=None):
        self._dev = (s_all, l_all, p_all, done_n)
        self._g_dev, self._st_dev = g_all, st_all
        self._host = None

    def host(self):
        if self._host is None:
            s_all, l_all, p_all, done_n = self._dev
            self._host = (s_all.cpu(), l_all.cpu(), p_all.cpu().tolist(), done_n.cpu().tolist())
            self._g_host = self._g_dev.cpu().tolist() if self._g_dev is not None else None
            self._st_host = self._st_dev.cpu().tolist() if self._st_dev is not None else None
        return self._host

    def top_seq(self):
        s_all, _, _, counts = self.host()
        return [s_all[k, :n] for k, n in enumerate(counts)]

    def top_prob(self):
        _, _, probs, counts = self.host()
        return [probs[k][:n] for k, n in enumerate(counts)]

    def done_beams(self):
        """misc/RecurrentFusionModel.py:529-531: per image the list of {'seq', 'logps', 'p'} dicts, best first."""
        s_all, l_all, probs, counts = self.host()
        beams = [[{'seq': a, 'logps': b_, 'p': c_} for a, b_, c_ in zip(s_all[k, :n].unbind(0), l_all[k, :n].unbind(0), probs[k][:n])]
                 for k, n in enumerate(counts)]
        if self._g_host is not None:                 # a diverse search: the group that produced each beam
            for k, img in enumerate(beams):
                for d, g in zip(img, self._g_host[k]):
                    d['group'] = g
        if self._st_host is not None:                # a lexically constrained search: the sets each beam satisfies
            for k, img in enumerate(beams):
                for d, st in zip(img, self._st_host[k]):
                    d['state'] = st
        return beams


class _LazyList(collections.abc.MutableSequence):
    """A sequence of known length whose entries are produced (all at once) by `fill()` the first time anything but its
    length is asked for.  Deliberately NOT a subclass of `list`: C fast paths that take a list subclass (`PySequence_Fast`,
    `PyList_GET_ITEM`: json's C encoder, `str.join`, some torch / numpy converters) read the list's item array directly and
    would see unfilled placeholders without any Python-level hook running.  As a plain `MutableSequence` every consumer goes
    through `__getitem__` / `__iter__` / `__len__` (which fill first), and a consumer that insists on a real list fails
    loudly (`json.dumps(x)` raises TypeError; `json.dumps(list(x))` / `x.materialize()` is the spelling).  Indexing,
    slicing, iteration, comparison with lists, `+`, `in`, `reversed`, `sorted`, printing, copying, pickling (as a plain
    list) and in-place edits behave like the list the reference returns (misc/RecurrentFusionModel.py:529-543)."""

    __slots__ = ('_n', '_fill', '_items')
    __hash__ = None

    def __init__(self, n, fill):
        self._n, self._fill, self._items = int(n), fill, None

    def materialize(self):
        """The plain `list` behind this object (filled now if it was not)."""
        if self._items is None:
            fill, self._fill = self._fill, None
            items = list(fill())
            if len(items) != self._n:
                raise N.RfnError('lazy list promised %d entries, its producer made %d' % (self._n, len(items)))
            self._items = items
        return self._items

    def __len__(self):
        return self._n if self._items is None else len(self._items)

    def __getitem__(self, i):
        return self.materialize()[i]

    def __setitem__(self, i, v):
        self.materialize()[i] = v

    def __delitem__(self, i):
        del self.materialize()[i]

    def insert(self, i, v):
        self.materialize().insert(i, v)

    def __iter__(self):
        return iter(self.materialize())

    def __repr__(self):
        return repr(self.materialize())

    def _other(self, other):
        return other.materialize() if isinstance(other, _LazyList) else other

    def __eq__(self, other):
        return self.materialize() == self._other(other)

    def __ne__(self, other):
        return self.materialize() != self._other(other)

    def __lt__(self, other):
        return self.materialize() < self._other(other)

    def __le__(self, other):
        return self.materialize() <= self._other(other)

    def __gt__(self, other):
        return self.materialize() > self._other(other)

    def __ge__(self, other):
        return self.materialize() >= self._other(other)

    def __add__(self, other):
        return self.materialize() + list(self._other(other))

    def __radd__(self, other):
        return list(other) + self.materialize()

    def __mul__(self, k):
        return self.materialize() * k

    __rmul__ = __mul__

    def copy(self):
        return list(self.materialize())

    def sort(self, **kw):
        self.materialize().sort(**kw)

    def __reduce_ex__(self, protocol):
        return (list, (list(self.materialize()),))
