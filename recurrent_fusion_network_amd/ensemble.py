"""Ensemble decoding over the path's inference hooks.

Reference: eval_utils.model_ensemble_feat_array_one_step(_multi_gpu) (eval_utils.py:268-317) averages the members'
pre-softmax logits of one decoder step (sum, then / n), applies log_softmax, and every member continues with the
token chosen from the averaged distribution; the reference code around it is stale (it calls one_time_step /
get_thought_vectors with arities the model does not have) and moves logits between GPUs with
`.cuda()` copies.  Here the members' steps run through rfn_decoder_step, the logit sum / division / log-softmax /
greedy pick are HIP kernels, members living on other ranks contribute through ONE sum all-reduce of the (B, V+1)
logits per step, and nothing is read back until the loop ends.

`sample_beam` is the same averaging under the fusion model's beam search (eval_utils.eval_ensemble, eval_utils.py:387-720,
whose bookkeeping is misc/RecurrentFusionModel.py:451-531): all images' beams share one decoder batch of B * beam rows per
member, the candidate / stable-sort / fork / done-beam rules run on the device (rfn_beam_step_topk) on the W best entries of
the averaged log-softmax (rfn_log_softmax_topk), every member's state follows the same fork order.
"""
import torch
import torch.distributed as dist

from . import _native as N
from .decode import (MAX_BEAM, MAX_STEPS, _Consensus, _Constraints, _diverse_beams, _Diversity, _length_penalty, _Scoring,
                     _sorted_done_beams, _Stepper, ScoreBuffers, host_beam_loop, host_greedy_loop, keep_candidates_n)


# Every entry point takes `att_lens` as RecurrentFusionModel's do (INTEGRATION.md "Ragged attention maps"): the per-image row counts
# of the stage-I attention maps, handed to every member's stage I.
class EnsembleDecoder:
    def __init__(self, models, process_group=None, total_members=None):
        """models: the members held by THIS process (same device, same vocabulary / seq_length).
        process_group: if given, members of all ranks of the group are averaged (total_members = sum over ranks,
        default len(models) * world_size)."""
        if not models:
            raise ValueError('need at least one model')
        self.models = list(models)
        self.consensus = None           # sample_beam with opt['consensus']: {'index', 'scores'} of the pick (device tensors)
        self.candidates = None          # sample_beam with opt['keep_candidates']: {'seq' (B, m, S), 'n_cand' (B,)} (device tensors)
        self.group = process_group
        world = dist.get_world_size(process_group) if process_group is not None else 1
        self.n_total = total_members if total_members is not None else len(self.models) * world
        m0 = self.models[0]
        for m in self.models:
            if m.vocab_size != m0.vocab_size or m.seq_length != m0.seq_length:
                raise N.RfnError('ensemble members disagree on vocab_size / seq_length')

    def _steppers(self, fc_feats, att_feats, att_lens, rows_per_image=1):
        """One _Stepper per member, on the member's own thought vectors and initial state.  rows_per_image = n > 1: n rows per image,
        image-major (row k * n + j = image k), the thought vectors repeated physically -- a host-stepped stepper's rows do not
        share them."""
        n, steppers = rows_per_image, []
        for m in self.models:
            comb, h, c, _ = m._prefix(fc_feats, att_feats, False, 0, att_lens)
            if n > 1:
                comb, h, c = comb.repeat_interleave(n, dim=1), h.repeat_interleave(n, dim=0), c.repeat_interleave(n, dim=0)
            else:
                h, c = h.clone(), c.clone()
            steppers.append(_Stepper(m, comb, h, c))
        return steppers

    def _averaged_step(self, steppers, ids, logit_sum, logit_m):
        """One decoder step of every member on the SAME tokens (each embeds them with its own table): logit_sum becomes the
        members' mean pre-softmax logits, over all ranks of the group."""
        rows, V1 = logit_sum.shape
        st = N.stream_ptr()
        for j, sp in enumerate(steppers):
            sp.step(ids, out=logit_sum if j == 0 else logit_m, want='logits')
            if j:
                N.check(N.lib.rfn_axpby_2d(1.0, logit_m.data_ptr(), V1, 1.0, logit_sum.data_ptr(), V1, rows, V1, st))
        if self.group is not None:
            dist.all_reduce(logit_sum, op=dist.ReduceOp.SUM, group=self.group)
        N.check(N.lib.rfn_div_2d(logit_sum.data_ptr(), V1, rows, V1, float(self.n_total), st))

    @torch.no_grad()
    def sample(self, fc_feats, att_feats, opt={}, att_lens=None):
        """Greedy ensemble decode -> (seq (B,<=S), seqLogprobs, logprobs_all (B,<=S+1,V+1)) with the reference's
        sample() conventions (finished rows masked to 0, early exit when every row has finished).  opt: the decoding
        constraints of RecurrentFusionModel.sample ('block_ngram', 'banned_ids', 'bad_endings'), applied to the averaged
        log-probs."""
        m0 = self.models[0]
        B, S, V1 = fc_feats[0].size(0), m0.seq_length, m0.vocab_size + 1
        cons = _Constraints.parse(opt, V1, S)
        steppers = self._steppers(fc_feats, att_feats, att_lens)
        dev = steppers[0].h.device
        logit_m = torch.empty(B, V1, device=dev)
        bufs = host_greedy_loop(lambda ids, out: self._averaged_step(steppers, ids, out, logit_m), B, S, V1, dev, cons)
        return bufs.read_back()        # nothing is read back before this: the call synchronises here, once

    @torch.no_grad()
    def score(self, fc_feats, att_feats, seq, opt={}, att_lens=None):
        """RecurrentFusionModel.score under the members' averaged distribution: the same arguments, the same dict.  The members
        step teacher-forced on the given tokens, each step's mean logits go through rfn_score_logits (T = 1, t0 = t) and the
        captions are summed at the end; only one step's (rows, V+1) logits exist at a time, so opt['max_rows'] has nothing to
        bound here.  With n > 1 captions per image every member's thought vectors are repeated physically (a stepper's rows do
        not share them).  A one-member ensemble IS that model's score, bit for bit."""
        m0 = self.models[0]
        so = _Scoring.parse(opt)
        B = m0._check_inputs(fc_feats, att_feats)
        rows, n, T = so.layout(seq.shape, B, m0.seq_length)
        V1 = m0.vocab_size + 1
        steppers = self._steppers(fc_feats, att_feats, att_lens, n)
        dev = steppers[0].h.device
        st = N.stream_ptr()
        bufs = ScoreBuffers(so, seq, rows, T, m0.seq_length, dev)
        logit_sum = torch.empty(rows, V1, device=dev)
        logit_m = torch.empty(rows, V1, device=dev)
        feed = bufs.feed.t().contiguous()                  # row t = the tokens fed at step t
        for t in range(bufs.steps):
            self._averaged_step(steppers, feed[t], logit_sum, logit_m)
            N.check(N.lib.rfn_score_logits(logit_sum.data_ptr(), V1, rows, 1, t, V1, bufs.target.data_ptr(), bufs.target.stride(0),
                                           int(so.include_end), bufs.tok_lp.data_ptr(), N.ptr(bufs.rank), N.ptr(bufs.ent),
                                           bufs.tok_lp.stride(0), st), 'rfn_score_logits')
        N.check(N.lib.rfn_score_captions(bufs.tok_lp.data_ptr(), bufs.tok_lp.stride(0), bufs.target.data_ptr(), bufs.target.stride(0),
                                         rows, bufs.steps, V1, int(so.include_end), bufs.cap_lp.data_ptr(), bufs.cap_len.data_ptr(),
                                         st), 'rfn_score_captions')
        return bufs.result()

    @torch.no_grad()
    def teacher_logits(self, fc_feats, att_feats, seq, att_lens=None):
        """The members' mean pre-softmax logits on the ground-truth prefix, as the `teacher` of
        RecurrentFusionModel.forward_loss: -> (B, S, V+1), S as the model's forward finds it (the first all-zero label column).
        The members step teacher-forced on seq[:, :S]; step t's mean goes straight into row block t of ONE (S, B, V+1) buffer,
        whose transposed view is returned (the distillation kernels take the teacher through its two strides, so nothing is
        copied).  Members on other ranks of the process group contribute as in `score`.  The mean of logits, not of
        probabilities: the distribution the ensemble decodes with."""
        m0 = self.models[0]
        B = m0._check_inputs(fc_feats, att_feats)
        if seq.dim() != 2 or seq.size(0) != B:
            raise N.RfnError('seq has shape %s, the features hold %d rows' % (tuple(seq.shape), B))
        S = m0._decoder_steps(seq)
        V1 = m0.vocab_size + 1
        steppers = self._steppers(fc_feats, att_feats, att_lens)
        dev = steppers[0].h.device
        feed = seq[:, :S].to(dev).long().t().contiguous()      # row t = the tokens fed at step t
        out = torch.empty(S, B, V1, device=dev)
        logit_m = torch.empty(B, V1, device=dev) if len(steppers) > 1 else None
        for t in range(S):
            self._averaged_step(steppers, feed[t], out[t], logit_m)
        return out.transpose(0, 1)

    @torch.no_grad()
    def teacher_topk(self, fc_feats, att_feats, seq, k, att_lens=None):
        """`teacher_logits` as a compact teacher: -> distill.TopKTeacher (B, S, k), the k <= min(32, V+1) best entries of every
        row of the members' mean logits, as log-probs in rfn_log_softmax_topk's order.  Each step's mean goes through that
        kernel into slice t of one (S, B, k) pair of buffers, so only ONE (B, V+1) block of logits ever exists -- never
        (S, B, V+1) -- and what is returned can be kept for the whole training set.  Bit for bit
        TopKTeacher.from_dense(self.teacher_logits(...), k)."""
        from .distill import MAX_K, TopKTeacher
        m0 = self.models[0]
        B = m0._check_inputs(fc_feats, att_feats)
        if seq.dim() != 2 or seq.size(0) != B:
            raise N.RfnError('seq has shape %s, the features hold %d rows' % (tuple(seq.shape), B))
        V1 = m0.vocab_size + 1
        k = int(k)
        if not 1 <= k <= min(MAX_K, V1):
            raise ValueError('k = %d: 1 <= k <= min(%d, V+1 = %d)' % (k, MAX_K, V1))
        S = m0._decoder_steps(seq)
        steppers = self._steppers(fc_feats, att_feats, att_lens)
        dev = steppers[0].h.device
        st = N.stream_ptr()
        feed = seq[:, :S].to(dev).long().t().contiguous()      # row t = the tokens fed at step t
        ids = torch.empty(S, B, k, dtype=torch.int32, device=dev)
        logp = torch.empty(S, B, k, device=dev)
        logit_sum = torch.empty(B, V1, device=dev)
        logit_m = torch.empty(B, V1, device=dev) if len(steppers) > 1 else None
        for t in range(S):
            self._averaged_step(steppers, feed[t], logit_sum, logit_m)
            N.check(N.lib.rfn_log_softmax_topk(logit_sum.data_ptr(), V1, B, V1, k, logp[t].data_ptr(), ids[t].data_ptr(), st),
                    'rfn_log_softmax_topk')
        return TopKTeacher(ids.transpose(0, 1), logp.transpose(0, 1))

    @torch.no_grad()
    def sample_beam(self, fc_feats, att_feats, opt={}, att_lens=None):
        """Beam search on the members' averaged distribution -> (seq (B, S), seqLogprobs (B, S), top_seq, top_prob) with
        the conventions of RecurrentFusionModel.sample_beam (best done beam per image; per-image lists of all done beams,
        best first); `self.done_beams` as there, and with opt['group_size'] > 1 (diverse beam search) `self.diverse_beams` and the
        'group' key as there; opt['consensus'] (with 'consensus_n', 'consensus_weights') returns the consensus pick and fills
        `self.consensus` as there; opt['keep_candidates'] fills `self.candidates` as there.  A one-member ensemble IS that model's
        sample_beam, bit for bit."""
        W = opt.get('beam_size', 10)
        m0 = self.models[0]
        B, S, V1 = fc_feats[0].size(0), m0.seq_length, m0.vocab_size + 1
        if W > MAX_BEAM or S > MAX_STEPS or W > V1:
            raise N.RfnError('beam search supports beam_size <= 32 (and <= V+1) and seq_length <= 64')
        if opt.get('require', None) is not None:
            raise ValueError('require (lexically constrained beam search) is RecurrentFusionModel.sample_beam\'s: the ensemble\'s '
                             'host-stepped search does not implement it')
        cons, alpha, div = _Constraints.parse(opt, V1, S), _length_penalty(opt), _Diversity.parse(opt, W)
        cs = _Consensus.parse(opt, V1, S, W)
        keep_n = keep_candidates_n(opt, W)
        keep = None if keep_n is None else {'n': keep_n}
        steppers = self._steppers(fc_feats, att_feats, att_lens, W)       # row k * W + q = image k
        dev = steppers[0].h.device
        logit_m = torch.empty(B * W, V1, device=dev)

        def reorder(order):
            for sp in steppers:
                sp.reorder(order)
        b = host_beam_loop(lambda ids, out: self._averaged_step(steppers, ids, out, logit_m), reorder, B, W, S, V1, dev, cons, div)
        seq, seq_lp, top_seq, top_prob, self.done_beams = _sorted_done_beams(b, alpha, cs, div.groups if div is not None else 1, keep)
        self.consensus = cs.result if cs is not None else None
        self.candidates = None if keep is None else {'seq': keep['seq'], 'n_cand': keep['n_cand']}
        self.diverse_beams = _diverse_beams(self.done_beams, div.groups) if div is not None else None
        return seq, seq_lp, top_seq, top_prob

