"""Validation metrics on the GPU: what eval_utils.language_eval gets from coco-caption's Bleu(4), Rouge() and Cider(), for a whole
split of token-id captions, without the JSON file, the Java tokenizer or a host round trip per batch.

LanguageEval collects the `seq` tensors model.sample / sample_beam return (one hypothesis row per image) and the loader's
reference ids, batch by batch, on the device; compute() scores the split once (rewards.BleuD / RougeL / CiderD with
end_token=False: a caption is the ids strictly before its first 0, as eval_utils.decode_sequence writes it) and reads the six
numbers back in one copy.  CIDEr is pycocoevalcap's Cider(): document frequencies over the split's images, ref_len = log(number
of images), the clipped and length-penalised similarity this checkout's cider_scorer has.

The metrics are computed in id space: language_eval first runs the PTB tokenizer (Java) over the decoded words, which can split
or drop some of them, so a number from here equals the reference's only where that tokenizer leaves the captions as they are.
METEOR and SPICE are Java programs and are not offered.
"""
from __future__ import annotations

import torch

from . import rewards as RW

METRICS = ('Bleu', 'ROUGE_L', 'CIDEr')


def _pad_to(t, shape):
    """t zero-padded at the end of every dimension up to `shape` (on its device)."""
    if tuple(t.shape) == tuple(shape):
        return t
    out = torch.zeros(shape, dtype=t.dtype, device=t.device)
    out[tuple(slice(0, n) for n in t.shape)] = t
    return out


class LanguageEval:
    """vocab: the largest word id (ids outside [0, vocab] make an image score NaN; the corpus numbers skip it and `skipped`
    counts it).  metrics: any of 'Bleu', 'ROUGE_L', 'CIDEr'."""

    def __init__(self, vocab, metrics=METRICS):
        for m in metrics:
            if m in ('METEOR', 'SPICE'):
                raise NotImplementedError('%s is a Java program and is not offered; use %s' % (m, ', '.join(METRICS)))
            if m not in METRICS:
                raise ValueError('unknown metric %r: choose from %s' % (m, ', '.join(METRICS)))
        if not 0 <= int(vocab) <= RW.MAX_ID:
            raise ValueError('vocab must lie in [0, %d]' % RW.MAX_ID)
        self.vocab, self.metrics = int(vocab), tuple(metrics)
        self._scorers = {'Bleu': RW.BleuD(), 'ROUGE_L': RW.RougeL(), 'CIDEr': RW.CiderD()}
        self.reset()

    def reset(self):
        self._seq, self._gts, self._n_refs = [], [], []
        self._per_image = self._result = None
        self.skipped = None

    def __len__(self):
        return sum(s.shape[0] for s in self._seq)

    def add(self, seq, gts, n_refs=None):
        """One batch: seq (B, <= S) ids on the GPU, one row per image; gts the loader's list of B per-image (n_refs_i, T) id
        arrays, or a padded (B, R, T) array / tensor with n_refs (B,).  seq is copied, so the caller may overwrite it (a
        sampler with a static output buffer); everything is kept on seq's device and nothing is scored.  With device tensors
        for gts and n_refs the call only enqueues copies and does not wait for the stream; host references (the loader's
        list, numpy arrays) are padded on the host and uploaded here, an ordinary blocking host-to-device copy."""
        if seq.device.type != 'cuda':
            raise RW.N.RfnError('seq must live on the GPU: the metrics have no CPU fallback')
        if seq.dim() != 2:
            raise ValueError('seq is (images, words)')
        if n_refs is None:
            gts, n_refs = RW.pad_gts(gts, seq.device)
        else:
            gts = torch.as_tensor(gts).to(seq.device, torch.int64, copy=True)
            n_refs = torch.as_tensor(n_refs).to(seq.device, torch.int32, copy=True)
        if gts.dim() != 3 or gts.shape[0] != seq.shape[0] or n_refs.numel() != seq.shape[0]:
            raise ValueError('gts needs one entry per row of seq (got %d for %d)' % (gts.shape[0], seq.shape[0]))
        if seq.shape[1] > RW.MAX_T or gts.shape[2] > RW.MAX_T or gts.shape[1] > RW.MAX_REFS:
            raise ValueError('limits: captions of at most %d ids, at most %d references per image' % (RW.MAX_T, RW.MAX_REFS))
        self._seq.append(seq.to(torch.int64, copy=True))
        self._gts.append(gts)
        self._n_refs.append(n_refs.reshape(-1))
        self._per_image = self._result = None

    def _score(self):
        if not self._seq:
            raise ValueError('no captions were added')
        dev = self._seq[0].device
        n = len(self)
        S = max(s.shape[1] for s in self._seq)
        R = max(g.shape[1] for g in self._gts)
        Tg = max(g.shape[2] for g in self._gts)
        seq = torch.cat([_pad_to(s, (s.shape[0], S)) for s in self._seq])
        gts = torch.cat([_pad_to(g, (g.shape[0], R, Tg)) for g in self._gts])
        n_refs = torch.cat(self._n_refs)
        row_img = torch.arange(n, dtype=torch.int32, device=dev)
        per, parts, names = {}, [], []
        kw = dict(vocab=self.vocab, end_token=False)
        if 'Bleu' in self.metrics:
            corpus = torch.empty(4, dtype=torch.float64, device=dev)
            per['Bleu'] = self._scorers['Bleu'].score_ids(seq, row_img, gts, n_refs, corpus=corpus, **kw)
            parts += [corpus, RW.mean_score(per['Bleu'])[1].to(torch.float64)]
            names += ['Bleu_1', 'Bleu_2', 'Bleu_3', 'Bleu_4', 'skipped:Bleu']
        for m in ('ROUGE_L', 'CIDEr'):
            if m in self.metrics:
                per[m] = self._scorers[m].score_ids(seq, row_img, gts, n_refs, **kw)
                mean, skipped = RW.mean_score(per[m])
                parts += [mean, skipped.to(torch.float64)]
                names += [m, 'skipped:' + m]
        host = torch.cat(parts).cpu().tolist()          # the one host read
        self._per_image = per
        self._result = {k: v for k, v in zip(names, host) if not k.startswith('skipped:')}
        self.skipped = {k[8:]: int(v) for k, v in zip(names, host) if k.startswith('skipped:')}

    def compute(self):
        """-> {'Bleu_1' .. 'Bleu_4', 'ROUGE_L', 'CIDEr'} (those asked for) as Python floats: corpus BLEU, and the means of
        ROUGE-L and CIDEr over the images.  `skipped` then holds, per metric, how many images scored NaN and were left out."""
        if self._result is None:
            self._score()
        return dict(self._result)

    def per_image(self):
        """-> {'Bleu': (n, 4), 'ROUGE_L': (n,), 'CIDEr': (n,)} float64 device tensors, in the order the images were added."""
        if self._per_image is None:
            self._score()
        return dict(self._per_image)
