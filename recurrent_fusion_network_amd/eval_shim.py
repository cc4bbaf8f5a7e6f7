"""The per-batch body of the reference's evaluation loop, for callers that port `eval_utils.eval_split`.

eval_utils.py:149-151 computes the XE loss on the caption batch (every image's features `seq_per_img` times in a
row, dataloader.py:251-252); :159-195 then keeps ONE row per image (`arange(batch) * seq_per_img`) and calls
`model.sample(..., {'beam_size', 'sample_max'})`; :206-208 scores each generated sentence as
`sum(seqLogprobs * (seq > 0))`.  Everything around it (vocabulary decoding, COCO json, Java metrics) is host-side
bookkeeping outside the accelerated path.

`eval_split` is that loop around `eval_step`, with the part of `language_eval` that is plain arithmetic (Bleu, ROUGE_L, CIDEr)
scored on the device by evalcap.LanguageEval.

Plumbing only: the arithmetic is `model.forward` / `model.sample` / the criterion / the scorers (HIP kernels).
"""
import torch


def unique_image_rows(n_rows, seq_per_img, device=None):
    """Row indices `np.arange(loader.batch_size) * loader.seq_per_img` (eval_utils.py:172-173)."""
    if n_rows % seq_per_img:
        raise ValueError('batch of %d rows is not a multiple of seq_per_img = %d' % (n_rows, seq_per_img))
    return torch.arange(n_rows // seq_per_img, device=device) * seq_per_img


def eval_step(model, crit, fc_feats, att_feats, labels, masks, top_words, seq_per_img, reason_weight=1.0,
              beam_size=1, sample_max=1, decode_opt=None):
    """-> dict(loss, seq, seqLogprobs, log_probs_sentence, sample): one iteration of eval_split's loop.

    fc_feats / att_feats: lists of caption-row tensors (each image repeated seq_per_img times), labels (rows, S+2),
    masks, top_words as the loader builds them.  `sample` is the full tuple model.sample returned (4 entries for
    beam_size 1, 5 with beam search: eval_utils.py:198-200).  decode_opt: further keys for model.sample's opt -- the decoding
    constraints 'block_ngram', 'banned_ids', 'bad_endings', 'length_penalty' (INTEGRATION.md)."""
    with torch.no_grad():
        log_prob, top_pred = model(fc_feats, att_feats, labels)
        loss = crit(log_prob, labels[:, 1:], masks[:, 1:], top_pred, top_words, reason_weight)
        rows = unique_image_rows(fc_feats[0].size(0), seq_per_img, fc_feats[0].device)
        fc_u = [f.index_select(0, rows) for f in fc_feats]
        att_u = [a.index_select(0, rows) for a in att_feats]
        out = model.sample(fc_u, att_u, dict(decode_opt or {}, beam_size=beam_size, sample_max=sample_max))
        seq, seq_lp = out[0], out[1]
        sentence = torch.sum(seq_lp * (seq > 0).to(seq_lp.dtype), 1)
    return dict(loss=loss, seq=seq, seqLogprobs=seq_lp, log_probs_sentence=sentence, sample=out)


def eval_split(model, crit, batches, seq_per_img, vocab, beam_size=1, sample_max=1, reason_weight=1.0, metrics=None,
               language_eval=None, decode_opt=None, diversity=None):
    """eval_utils.eval_split's loop with language_eval's Bleu / ROUGE_L / CIDEr computed on the device.

    batches: an iterable of dicts with the loader's 'fc_feats', 'att_feats' (lists of caption-row tensors), 'labels', 'masks',
    'top_words' on the model's device and 'gts' (per image, an (n_refs_i, T) id array; or a padded array with 'n_refs').  The
    module is put in eval mode for the loop and left in the mode it was found in.  -> (mean loss over the batches, metrics dict
    of evalcap.LanguageEval.compute()).  The losses stay on the device until the loop has ended; language_eval: a LanguageEval to
    feed instead of a new one (its per_image() and skipped are then the caller's to read).  decode_opt: as eval_step.

    diversity: an evalcap.DiversityEval to feed with every image's candidate set; the caller reads its compute().  The decoding
    must then yield several candidates per image: decode_opt['sample_n'] > 1 with sample_max = 0 (the B * n draws; the LanguageEval
    receives draw 0 of every image), or beam search (beam_size > 1; 'keep_candidates' is set for the call and the candidates are
    model.candidates: the ranked done beams, or the group bests of a diverse search)."""
    from .evalcap import METRICS, LanguageEval
    lang = language_eval if language_eval is not None else LanguageEval(vocab, METRICS if metrics is None else metrics)
    n_draws = int((decode_opt or {}).get('sample_n', None) or 1)
    if diversity is not None:
        if beam_size > 1:
            decode_opt = dict(decode_opt or {}, keep_candidates=True)
        elif n_draws < 2 or sample_max:
            raise ValueError('diversity needs several candidates per image: sample_n > 1 with sample_max = 0, or beam_size > 1')
        elif (decode_opt or {}).get('consensus', None) is not None:
            raise ValueError('sample with \'consensus\' returns one draw per image: the candidates are gone')
    was_training = model.training
    model.eval()
    losses = []
    try:
        for data in batches:
            out = eval_step(model, crit, data['fc_feats'], data['att_feats'], data['labels'], data['masks'], data['top_words'],
                            seq_per_img, reason_weight, beam_size, sample_max, decode_opt)
            losses.append(out['loss'].detach().reshape(1).to(torch.float64))
            seq = out['seq']
            if beam_size == 1 and n_draws > 1 and seq.size(0) == n_draws * len(data['gts']):
                if diversity is not None:
                    diversity.add(seq, data['gts'], data.get('n_refs'), n=n_draws)
                seq = seq.view(-1, n_draws, seq.size(1))[:, 0]        # draw 0: the call's one caption per image
            elif diversity is not None:
                diversity.add(model.candidates['seq'], data['gts'], data.get('n_refs'), n_cand=model.candidates['n_cand'])
            lang.add(seq, data['gts'], data.get('n_refs'))
    finally:
        model.train(was_training)
    if not losses:
        raise ValueError('eval_split needs at least one batch')
    scores = lang.compute()
    return float(torch.cat(losses).mean()), scores
