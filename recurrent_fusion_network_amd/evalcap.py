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


DIVERSITY_METRICS = ('Div', 'mBleu', 'Self_CIDEr', 'CIDEr', 'Bleu_4', 'ROUGE_L')
_REFERENCE_METRICS = ('CIDEr', 'Bleu_4', 'ROUGE_L')


class DiversityEval:
    """The numbers the captioning literature reports for SETS of captions (n per image: sample_n draws, done beams, diverse group
    bests), for a whole split, on the device (rfn.h "caption-set diversity"; INTEGRATION.md "Diversity metrics"):

      'Div'        Div_1 .. Div_4: distinct m-grams of an image's set over its word count, averaged over the images;
      'mBleu'      mBleu_1 .. mBleu_4: corpus BLEU of every candidate slot against the image's other candidates, averaged over slots;
      'Self_CIDEr' the spectrum of the set's symmetrised pairwise CIDEr-D matrix, averaged over the images;
      'CIDEr', 'Bleu_4', 'ROUGE_L'   against the references: Oracle_<m> (best of n) and Mean_<m> (mean of n).

    Oracle_CIDEr / Mean_CIDEr and Oracle_ROUGE_L / Mean_ROUGE_L are means over the images of the per-image best and mean.
    Oracle_Bleu_4 is the corpus BLEU-4 of every image's best candidate by sentence BLEU-4; Mean_Bleu_4 the mean over the candidate
    slots of the slot's corpus BLEU-4.  With n = 1 every pair equals LanguageEval's number on the same captions.  Each candidate is
    scored as LanguageEval would score it had it been the returned caption: under a corpus df (scorer=None, or a CiderD()) that is
    one scoring call per slot, so the document frequencies and log(images) are LanguageEval's.

    vocab as LanguageEval; scorer: the rewards.CiderD whose df Self-CIDEr and the oracle CIDEr use (None: a corpus-df CiderD())."""

    def __init__(self, vocab, scorer=None, metrics=DIVERSITY_METRICS):
        for m in metrics:
            if m in ('METEOR', 'SPICE', 'AllSPICE'):
                raise NotImplementedError('%s is a Java program and is not offered; use %s' % (m, ', '.join(DIVERSITY_METRICS)))
            if m not in DIVERSITY_METRICS:
                raise ValueError('unknown metric %r: choose from %s' % (m, ', '.join(DIVERSITY_METRICS)))
        if not 0 <= int(vocab) <= RW.MAX_ID:
            raise ValueError('vocab must lie in [0, %d]' % RW.MAX_ID)
        if scorer is not None and not isinstance(scorer, RW.CiderD):
            raise NotImplementedError('the diversity metrics are implemented for the CiderD scorer only, got %s' % type(scorer).__name__)
        self.vocab, self.metrics = int(vocab), tuple(metrics)
        self._cider = scorer if scorer is not None else RW.CiderD()
        self._bleu, self._rouge = RW.BleuD(), RW.RougeL()
        self.reset()

    def reset(self):
        self._cands, self._n_cand, self._gts, self._n_refs = [], [], [], []
        self._per_image = self._result = None
        self.skipped = None

    def __len__(self):
        return sum(c.shape[0] for c in self._cands)

    def add(self, cands, gts=None, n_refs=None, n_cand=None, n=None):
        """One batch: cands (B, n, <= S) ids on the GPU, or (B * n, <= S) image-major with n=; n_cand (B,) valid candidates per
        image (None: all n); gts / n_refs as LanguageEval.add (gts may be None when no metric against the references was asked
        for).  Everything is copied and kept on the device; nothing is scored."""
        if cands.device.type != 'cuda':
            raise RW.N.RfnError('cands must live on the GPU: the metrics have no CPU fallback')
        if cands.dim() == 2:
            if n is None or int(n) < 1 or cands.shape[0] % int(n):
                raise ValueError('(rows, words) candidates need n=, the candidates per image, dividing the rows')
            cands = cands.reshape(cands.shape[0] // int(n), int(n), cands.shape[1])
        if cands.dim() != 3:
            raise ValueError('cands is (images, candidates, words)')
        B, nn, S = cands.shape
        if self._cands and self._cands[0].shape[1] != nn:
            raise ValueError('every batch needs the same number of candidates per image (%d, got %d)' % (self._cands[0].shape[1], nn))
        if S > RW.MAX_T or nn > RW.MAX_REFS:
            raise ValueError('limits: captions of at most %d ids, at most %d candidates per image' % (RW.MAX_T, RW.MAX_REFS))
        dev = cands.device
        if n_cand is None:
            n_cand = torch.full((B,), nn, dtype=torch.int32, device=dev)
        else:
            n_cand = torch.as_tensor(n_cand).to(dev, torch.int32, copy=True).reshape(-1)
            if n_cand.numel() != B:
                raise ValueError('n_cand needs one entry per image')
        if any(m in self.metrics for m in _REFERENCE_METRICS):
            if gts is None:
                raise ValueError('%s score against the references: pass gts' % ' / '.join(_REFERENCE_METRICS))
            if n_refs is None:
                gts, n_refs = RW.pad_gts(gts, dev)
            else:
                gts = torch.as_tensor(gts).to(dev, torch.int64, copy=True)
                n_refs = torch.as_tensor(n_refs).to(dev, torch.int32, copy=True)
            if gts.dim() != 3 or gts.shape[0] != B or n_refs.numel() != B:
                raise ValueError('gts needs one entry per image (got %d for %d)' % (gts.shape[0], B))
            if gts.shape[2] > RW.MAX_T or gts.shape[1] > RW.MAX_REFS:
                raise ValueError('limits: references of at most %d ids, at most %d per image' % (RW.MAX_T, RW.MAX_REFS))
            self._gts.append(gts)
            self._n_refs.append(n_refs.reshape(-1))
        self._cands.append(cands.to(torch.int64, copy=True))
        self._n_cand.append(n_cand)
        self._per_image = self._result = None

    def _score(self):
        if not self._cands:
            raise ValueError('no captions were added')
        dev = self._cands[0].device
        B, n = len(self), self._cands[0].shape[1]
        S = max(c.shape[2] for c in self._cands)
        cands = torch.cat([_pad_to(c, (c.shape[0], n, S)) for c in self._cands])
        n_cand = torch.cat(self._n_cand)
        per, parts, names = {}, [], []

        def mean_of(name, column):
            mean, skipped = RW.mean_score(column)
            parts.extend([mean, skipped.to(torch.float64)])
            names.extend([name, 'skipped:' + name])

        want = [w for m, ws in (('Div', ('distinct', 'words', 'div')), ('mBleu', ('mbleu', 'mbleu_comps', 'mbleu_corpus')),
                                ('Self_CIDEr', ('U', 'eig', 'self_cider'))) if m in self.metrics for w in ws]
        if want:
            d = self._cider.diversity(cands, n_cand, end_token=False, vocab=self.vocab, want=want)
            per.update(d)
            if 'Div' in self.metrics:
                for m, col in enumerate(d['div'].t().contiguous()):
                    mean_of('Div_%d' % (m + 1), col)
            if 'mBleu' in self.metrics:
                for m, col in enumerate(d['mbleu_corpus'].t().contiguous()):
                    mean_of('mBleu_%d' % (m + 1), col)
            if 'Self_CIDEr' in self.metrics:
                mean_of('Self_CIDEr', d['self_cider'])
        if self._gts:
            R = max(g.shape[1] for g in self._gts)
            Tg = max(g.shape[2] for g in self._gts)
            gts = torch.cat([_pad_to(g, (g.shape[0], R, Tg)) for g in self._gts])
            n_refs = torch.cat(self._n_refs)
            one_per_image = torch.arange(B, dtype=torch.int32, device=dev)
            image_major = torch.arange(B * n, dtype=torch.int32, device=dev) // n
            flat = cands.view(B * n, S)
            valid = torch.arange(n, device=dev)[None, :] < n_cand[:, None]                    # (B, n)
            kw = dict(vocab=self.vocab, end_token=False)
            if 'CIDEr' in self.metrics:
                if self._cider.df_mode == 'corpus':
                    # one call per slot, B rows: the df and log(B) LanguageEval would have; an invalid slot scores the image's
                    # candidate 0 so that every image keeps its one document, and the stats below ignore it
                    cols = [self._cider.score_ids(torch.where(valid[:, j, None], cands[:, j], cands[:, 0]), one_per_image, gts,
                                                  n_refs, **kw) for j in range(n)]
                    s = torch.stack(cols, 1).contiguous().view(B * n)
                else:
                    s = self._cider.score_ids(flat, image_major, gts, n_refs, **kw)
                best, _, mean = RW.group_stats(s, n, n_cand)
                per.update(CIDEr=s.view(B, n), Oracle_CIDEr=best, Mean_CIDEr=mean)
                mean_of('Oracle_CIDEr', best)
                mean_of('Mean_CIDEr', mean)
            if 'Bleu_4' in self.metrics:
                s = self._bleu.score_ids(flat, image_major, gts, n_refs, **kw)                # (B * n, 4), exact in one call
                best, arg, _ = RW.group_stats(s[:, 3].contiguous(), n, n_cand)
                chosen, _, _ = RW.consensus_gather(arg, n, cands)
                corpus = torch.empty(n + 1, 4, dtype=torch.float64, device=dev)
                self._bleu.score_ids(chosen, one_per_image, gts, n_refs, corpus=corpus[n], **kw)
                outside = torch.full_like(cands[:, 0], -1)                                    # an id no vocabulary holds: a NaN row
                for j in range(n):     # slot j's corpus BLEU over the images that have the slot
                    self._bleu.score_ids(torch.where(valid[:, j, None], cands[:, j], outside), one_per_image, gts, n_refs,
                                         corpus=corpus[j], **kw)
                per.update(Bleu=s.view(B, n, 4), Oracle_Bleu_4=best, Oracle_Bleu_4_index=arg, Bleu_corpus=corpus)
                parts.extend([corpus[n, 3:4], RW.mean_score(best)[1].to(torch.float64)])
                names.extend(['Oracle_Bleu_4', 'skipped:Oracle_Bleu_4'])
                mean_of('Mean_Bleu_4', corpus[:n, 3].contiguous())
            if 'ROUGE_L' in self.metrics:
                s = self._rouge.score_ids(flat, image_major, gts, n_refs, **kw)
                best, _, mean = RW.group_stats(s, n, n_cand)
                per.update(ROUGE_L=s.view(B, n), Oracle_ROUGE_L=best, Mean_ROUGE_L=mean)
                mean_of('Oracle_ROUGE_L', best)
                mean_of('Mean_ROUGE_L', mean)
        host = torch.cat([p.reshape(1) for p in parts]).cpu().tolist()          # the one host read
        self._per_image = per
        self._result = {k: v for k, v in zip(names, host) if not k.startswith('skipped:')}
        self.skipped = {k[8:]: int(v) for k, v in zip(names, host) if k.startswith('skipped:')}

    def compute(self):
        """-> {'Div_1' .. 'Div_4', 'mBleu_1' .. 'mBleu_4', 'Self_CIDEr', 'Oracle_CIDEr', 'Mean_CIDEr', 'Oracle_Bleu_4', 'Mean_Bleu_4',
        'Oracle_ROUGE_L', 'Mean_ROUGE_L'} (those asked for) as Python floats, after one host read.  `skipped` then holds, per
        number, how many images (for mBleu_m and Mean_Bleu_4: candidate slots) were NaN and left out of it."""
        if self._result is None:
            self._score()
        return dict(self._result)

    def per_image(self):
        """-> the device tensors behind the numbers, images in the order they were added: rewards.diversity's outputs ('div',
        'mbleu', 'self_cider', ...), the per-candidate scores 'CIDEr' (B, n), 'Bleu' (B, n, 4), 'ROUGE_L' (B, n), and
        'Oracle_<m>' / 'Mean_<m>' (B,)."""
        if self._per_image is None:
            self._score()
        return dict(self._per_image)
