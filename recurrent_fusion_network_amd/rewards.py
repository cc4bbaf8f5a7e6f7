"""Self-critical reward on the GPU: CIDEr-D and BLEU-D of token-id captions (csrc/rfn_reward.hip) and drop-ins for the
reference's get_rewards.py (get_self_critical_reward_feat_array / get_self_critical_reward).

CiderD reproduces cider/pyciderevalcap/ciderD's CiderD(n=4, sigma=6.0) as compute_reward calls it, on captions given as id
rows (the ids up to and including the first 0, as array_to_str keeps them).  Document frequencies come from the scored
rows themselves (df='corpus') or from a precomputed table (the reference's df='coco-train-idxs' pickle, or any dict of
id-string tuples).  Corpus df is per call: under data parallelism each rank scores its own shard, as per-rank runs of the
reference would.

BleuD reproduces cider/pyciderevalcap/bleuD's BleuD(4) (closest reference length) on the same id rows: four scores per row, the
row's integer components and the corpus-level four.  compute_reward's bleu4 * bleu4_weight + cider * cider_weight is mixed on
the device (scst_reward with bleu_scorer=).  SPICE-D (a Java server behind a socket) is not ported.

RougeL reproduces coco-caption/pycocoevalcap's Rouge() (ROUGE-L, beta = 1.2) on the same id rows.  Every score_ids takes
end_token=: True (the default) is the reward's caption, False the validation caption of eval_utils.decode_sequence, the ids
strictly before the first 0 (evalcap.LanguageEval scores a whole split that way).
"""
from __future__ import annotations

import ctypes as C
import os
import pickle

import numpy as np
import torch

from . import _native as N

MAX_T, MAX_REFS, MAX_ID = 64, 32, 32767
_DOC_COUNTS = (('coco-all', 123287), ('coco-train', 113287), ('coco-val', 5000))   # ciderD_scorer.compute_cider
# rfn_capset_diversity's outputs, in its argument order
DIVERSITY_OUTPUTS = ('distinct', 'words', 'div', 'mbleu', 'mbleu_comps', 'mbleu_corpus', 'U', 'eig', 'self_cider')


def _ref_docs_of(mode):
    for name, n in _DOC_COUNTS:
        if name in mode:
            return n
    raise ValueError('df mode %r names none of coco-all / coco-train / coco-val: its document count is unknown' % mode)


class _IdScorer:
    """What the scorers share: the head of score_ids and the workspace."""
    _NAME = None
    _ws = None

    def _inputs(self, res, row_img, gts, n_refs):
        """score_ids' arguments on res's device, in the types the C entry reads -> dev, res, row_img, gts, n_refs and the
        sizes (n_rows, T, n_img, R, Tg)."""
        dev = res.device
        if dev.type != 'cuda':
            raise N.RfnError('res must live on the GPU: the reward has no CPU fallback')
        res = res.to(torch.int64).contiguous()
        gts = gts.to(dev, torch.int64).contiguous()
        row_img = row_img.to(dev, torch.int32).contiguous()
        n_refs = n_refs.to(dev, torch.int32).contiguous()
        n_rows, T = res.shape
        n_img, R, Tg = gts.shape
        if row_img.numel() != n_rows or n_refs.numel() != n_img:
            raise ValueError('row_img needs one entry per row and n_refs one per image')
        return dev, res, row_img, gts, n_refs, (n_rows, T, n_img, R, Tg)

    def _workspace(self, dev, nbytes):
        """nbytes: the C entry's workspace query for the call's sizes (0 outside the limits)."""
        if nbytes == 0:
            raise ValueError('%s limits: 1 <= T <= %d, 1 <= refs per image <= %d' % (self._NAME, MAX_T, MAX_REFS))
        if self._ws is None or self._ws.device != dev or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return self._ws

    @staticmethod
    def _flags(end_token):
        return 0 if end_token else N.CAPTION_END_EXCLUDED


class CiderD(_IdScorer):
    """CIDEr-D scorer.  df: 'corpus', a dict {tuple of id strings: df}, a pickle path, or a reference mode name such as
    'coco-train-idxs' (read from data/<name>.p like the reference).  df_mode names the document count of a table
    (defaults to the name / file name of df)."""
    _NAME = 'CIDEr-D'

    def __init__(self, n=4, sigma=6.0, df='corpus', df_mode=None):
        if n != 4:
            raise NotImplementedError('only n = 4 (CiderD\'s default) is implemented')
        self._n, self._sigma = n, float(sigma)
        self._tables = {}
        self._table_src = None
        if isinstance(df, str) and df == 'corpus':
            self.df_mode, self.ref_docs = 'corpus', None
            return
        if isinstance(df, str):
            path = df if os.path.exists(df) else os.path.join('data', df + '.p')
            if df_mode is None:
                df_mode = os.path.splitext(os.path.basename(path))[0]
            with open(path, 'rb') as f:
                df = pickle.load(f)
        if not isinstance(df, dict):
            raise TypeError('df must be \'corpus\', a dict or a pickle path')
        if df_mode is None:
            raise ValueError('a df dict needs df_mode (e.g. \'coco-train\') for its document count')
        self.df_mode, self.ref_docs = df_mode, float(_ref_docs_of(df_mode))
        ids, counts = [], []
        for g, c in df.items():
            try:
                row = [_int_word(w) for w in g]
            except ValueError:
                continue          # not an id n-gram: can never match a caption of ids
            if not 1 <= len(row) <= 4 or min(row) < 0 or max(row) > MAX_ID:
                continue
            ids.append(row + [-1] * (4 - len(row)))
            counts.append(float(c))
        self._table_src = (np.array(ids, dtype=np.int32).reshape(-1, 4), np.array(counts, dtype=np.float64))
        self._slots = 1024
        while self._slots < 2 * max(1, len(counts)):
            self._slots *= 2

    # -- device state --------------------------------------------------------------------------------------------
    def _table(self, dev):
        """The device df table (built once per device, with every n-gram of ids <= MAX_ID)."""
        if self._table_src is None:
            return None
        key = str(dev)
        if key not in self._tables:
            ids, counts = self._table_src
            table = torch.empty(N.lib.rfn_ciderd_table_bytes(self._slots), dtype=torch.uint8, device=dev)
            ids_d = torch.from_numpy(ids).to(dev)
            counts_d = torch.from_numpy(counts).to(dev)
            N.check(N.lib.rfn_ciderd_table_build(N.ptr(ids_d) if len(counts) else None, N.ptr(counts_d) if len(counts) else None,
                                                 len(counts), MAX_ID, table.data_ptr(), self._slots, N.stream_ptr()),
                    'rfn_ciderd_table_build')
            torch.cuda.current_stream(dev).synchronize()   # the host arrays' device copies are freed below
            self._tables[key] = table
        return self._tables[key]

    # -- scoring ---------------------------------------------------------------------------------------------------
    def score_ids(self, res, row_img, gts, n_refs, vocab=MAX_ID, out=None, end_token=True):
        """res (N, T) int64 ids, row_img (N,) image of each row, gts (n_img, R, Tg) int64 references padded to R,
        n_refs (n_img,) references per image; all on one GPU.  -> (N,) float64 scores on the device (NaN for a row whose
        caption or references hold an id outside [0, vocab]).  end_token=False: a caption is the ids before its first 0, not up
        to and including it (then an image with an empty reference scores NaN too)."""
        dev, res, row_img, gts, n_refs, (n_rows, T, n_img, R, Tg) = self._inputs(res, row_img, gts, n_refs)
        table = self._table(dev)
        ws = self._workspace(dev, N.lib.rfn_ciderd_ws_bytes(n_rows, T, n_img, R, Tg, int(table is None)))
        if out is None:
            out = torch.empty(n_rows, dtype=torch.float64, device=dev)
        N.check(N.lib.rfn_ciderd_score_ex(res.data_ptr(), n_rows, T, row_img.data_ptr(), gts.data_ptr(), n_refs.data_ptr(),
                                          n_img, R, Tg, None if table is None else table.data_ptr(),
                                          0 if table is None else self._slots, C.c_double(self.ref_docs or 0.0), vocab,
                                          C.c_double(self._sigma), self._flags(end_token), out.data_ptr(), ws.data_ptr(),
                                          ws.numel(), N.stream_ptr()), 'rfn_ciderd_score_ex')
        return out

    def consensus(self, cands, n_cand=None, weights=None, end_token=True, want_pairs=False, vocab=MAX_ID):
        """Consensus (minimum-Bayes-risk) reranking under this scorer (rfn.h "consensus reranking"): cands (B, n, T) int64 ids,
        n_cand (B,) how many of an image's n candidates are valid (None: all), weights (B, n) float64 >= 0 (None: uniform).
        -> (best (B,) int64, scores (B, n) float64, U (B, n, n) float64 or None): scores[k, i] is the weighted mean CIDEr-D of
        candidate i against the image's other candidates, best[k] the lowest index of its maximum (-1, with NaN scores, for an
        image with a bad input), U[k, i, j] the pairwise utility (want_pairs=True).  Everything stays on the device; after the
        first call at a shape nothing is allocated but the results and nothing synchronises."""
        dev = cands.device
        if dev.type != 'cuda':
            raise N.RfnError('cands must live on the GPU: the reranking has no CPU fallback')
        if cands.dim() != 3:
            raise ValueError('cands must be (images, candidates, T), got %s' % (tuple(cands.shape),))
        cands = cands.to(torch.int64).contiguous()
        B, n, T = cands.shape
        if n_cand is not None:
            n_cand = n_cand.to(dev, torch.int32).contiguous()
            if n_cand.numel() != B:
                raise ValueError('n_cand needs one entry per image')
        if weights is not None:
            weights = weights.to(dev, torch.float64).contiguous()
            if tuple(weights.shape) != (B, n):
                raise ValueError('weights must be (%d, %d), got %s' % (B, n, tuple(weights.shape)))
        table = self._table(dev)
        ws = self._workspace(dev, N.lib.rfn_consensus_ws_bytes(B, n, T, int(table is None)))
        best = torch.empty(B, dtype=torch.int64, device=dev)
        scores = torch.empty(B, n, dtype=torch.float64, device=dev)
        U = torch.empty(B, n, n, dtype=torch.float64, device=dev) if want_pairs else None
        N.check(N.lib.rfn_consensus_ciderd(cands.data_ptr(), B, n, T, N.ptr(n_cand) or None, N.ptr(weights) or None,
                                           None if table is None else table.data_ptr(), 0 if table is None else self._slots,
                                           C.c_double(self.ref_docs or 0.0), vocab, C.c_double(self._sigma), self._flags(end_token),
                                           N.ptr(U) or None, scores.data_ptr(), best.data_ptr(), ws.data_ptr(), ws.numel(),
                                           N.stream_ptr()), 'rfn_consensus_ciderd')
        return best, scores, U

    def diversity(self, cands, n_cand=None, end_token=False, vocab=MAX_ID, want=DIVERSITY_OUTPUTS):
        """Caption-set diversity under this scorer's df (rfn.h "caption-set diversity"): cands (B, n, T) int64 ids, n_cand (B,)
        valid candidates per image (None: all).  end_token=False (the default): words only, as evalcap.LanguageEval reads
        captions.  -> dict of device tensors: 'distinct' (B, 4) int32, 'words' (B,) int32, 'div' (B, 4), 'mbleu' (B, n, 4),
        'mbleu_comps' (B, n, 10) int32, 'mbleu_corpus' (n, 4), 'U' (B, n, n), 'eig' (B, n), 'self_cider' (B,), float64 where no
        type is given; `want` names the ones to compute (the others' launches are skipped).  A bad image (n_cand outside [1, n],
        an id outside [0, vocab], an empty candidate under end_token=False) has NaN / 0 there.  Uses the scorer's workspace;
        nothing is read back and nothing synchronises."""
        dev = cands.device
        if dev.type != 'cuda':
            raise N.RfnError('cands must live on the GPU: the diversity metrics have no CPU fallback')
        if cands.dim() != 3:
            raise ValueError('cands must be (images, candidates, T), got %s' % (tuple(cands.shape),))
        unknown = [w for w in want if w not in DIVERSITY_OUTPUTS]
        if unknown:
            raise ValueError('unknown diversity outputs %s: choose from %s' % (unknown, ', '.join(DIVERSITY_OUTPUTS)))
        cands = cands.to(torch.int64).contiguous()
        B, n, T = cands.shape
        if n_cand is not None:
            n_cand = n_cand.to(dev, torch.int32).contiguous()
            if n_cand.numel() != B:
                raise ValueError('n_cand needs one entry per image')
        table = self._table(dev)
        ws = self._workspace(dev, N.lib.rfn_capset_ws_bytes(B, n, T, int(table is None)))
        shapes = {'distinct': ((B, 4), torch.int32), 'words': ((B,), torch.int32), 'div': ((B, 4), torch.float64),
                  'mbleu': ((B, n, 4), torch.float64), 'mbleu_comps': ((B, n, 10), torch.int32),
                  'mbleu_corpus': ((n, 4), torch.float64), 'U': ((B, n, n), torch.float64), 'eig': ((B, n), torch.float64),
                  'self_cider': ((B,), torch.float64)}
        out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in DIVERSITY_OUTPUTS if k in want}
        N.check(N.lib.rfn_capset_diversity(cands.data_ptr(), B, n, T, N.ptr(n_cand) or None,
                                           None if table is None else table.data_ptr(), 0 if table is None else self._slots,
                                           C.c_double(self.ref_docs or 0.0), vocab, C.c_double(self._sigma), self._flags(end_token),
                                           *[N.ptr(out.get(k)) or None for k in DIVERSITY_OUTPUTS], ws.data_ptr(), ws.numel(),
                                           N.stream_ptr()), 'rfn_capset_diversity')
        return out

    def compute_score(self, gts, res):
        """The reference's interface: gts {image_id: [caption, ...]}, res [{'image_id': id, 'caption': [caption]}], captions
        being space-separated id strings as array_to_str writes them.  -> (mean, np.ndarray of per-entry scores)."""
        res_a, row_img, gts_a, n_refs, vocab = _id_arrays(gts, res)
        dev = torch.device('cuda', torch.cuda.current_device())
        s = self.score_ids(torch.from_numpy(res_a).to(dev), row_img, torch.from_numpy(gts_a), n_refs, vocab=vocab).cpu().numpy()
        return np.mean(s), s

    def method(self):
        return 'CIDEr-D'


class BleuD(_IdScorer):
    """BLEU-D scorer: the reference's BleuD(4), whose rows take the closest reference length."""
    _NAME = 'BLEU-D'

    def __init__(self, n=4):
        if n != 4:
            raise NotImplementedError('only n = 4 (compute_reward\'s BleuD(4)) is implemented')
        self._n = n

    def score_ids(self, res, row_img, gts, n_refs, vocab=MAX_ID, out=None, comps=None, corpus=None, end_token=True):
        """Arguments as CiderD.score_ids.  -> (N, 4) float64 BLEU-1..4 per row on the device (NaN in all four for a row whose
        caption or references hold an id outside [0, vocab]).  comps: optional (N, 10) int32 device tensor that receives
        testlen, reflen, guess[4], correct[4] of every row; corpus: optional (4,) float64 device tensor that receives the
        corpus-level scores (one more small launch).  end_token: as CiderD.score_ids."""
        dev, res, row_img, gts, n_refs, (n_rows, T, n_img, R, Tg) = self._inputs(res, row_img, gts, n_refs)
        ws = self._workspace(dev, N.lib.rfn_bleud_ws_bytes(n_rows, T, n_img, R, Tg))
        if out is None:
            out = torch.empty(n_rows, 4, dtype=torch.float64, device=dev)
        for t, name, shape, dtype in ((out, 'out', (n_rows, 4), torch.float64), (comps, 'comps', (n_rows, 10), torch.int32),
                                      (corpus, 'corpus', (4,), torch.float64)):
            if t is not None and (t.device != dev or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()):
                raise ValueError('%s must be a contiguous %s %s tensor on %s' % (name, shape, dtype, dev))
        N.check(N.lib.rfn_bleud_score_ex(res.data_ptr(), n_rows, T, row_img.data_ptr(), gts.data_ptr(), n_refs.data_ptr(), n_img,
                                         R, Tg, vocab, self._flags(end_token), out.data_ptr(), N.ptr(comps), N.ptr(corpus),
                                         ws.data_ptr(), ws.numel(), N.stream_ptr()), 'rfn_bleud_score_ex')
        return out

    def compute_score(self, gts, res):
        """The reference's interface (see CiderD.compute_score) -> (the corpus-level [BLEU-1 .. BLEU-4], four lists of
        per-entry scores), as BleuD.compute_score returns them."""
        res_a, row_img, gts_a, n_refs, vocab = _id_arrays(gts, res)
        dev = torch.device('cuda', torch.cuda.current_device())
        corpus = torch.empty(4, dtype=torch.float64, device=dev)
        s = self.score_ids(torch.from_numpy(res_a).to(dev), row_img, torch.from_numpy(gts_a), n_refs, vocab=vocab, corpus=corpus)
        return corpus.cpu().tolist(), s.cpu().numpy().T.tolist()

    def method(self):
        return 'Bleu'


class RougeL(_IdScorer):
    """ROUGE-L scorer: pycocoevalcap's Rouge() (the F-measure of the longest common subsequence, beta = 1.2)."""
    _NAME = 'ROUGE-L'

    def __init__(self, beta=1.2):
        if not beta > 0:
            raise ValueError('beta must be positive')
        self.beta = float(beta)

    def score_ids(self, res, row_img, gts, n_refs, vocab=MAX_ID, out=None, lcs=None, end_token=True):
        """Arguments as CiderD.score_ids.  -> (N,) float64 ROUGE-L per row on the device (NaN for a row whose caption or
        references hold an id outside [0, vocab]; 0 for an empty caption).  lcs: optional (N, R) int32 device tensor that
        receives the LCS length of the row against every reference of its image (0 behind them)."""
        dev, res, row_img, gts, n_refs, (n_rows, T, n_img, R, Tg) = self._inputs(res, row_img, gts, n_refs)
        ws = self._workspace(dev, N.lib.rfn_rougel_ws_bytes(n_rows, T, n_img, R, Tg))
        if out is None:
            out = torch.empty(n_rows, dtype=torch.float64, device=dev)
        for t, name, shape, dtype in ((out, 'out', (n_rows,), torch.float64), (lcs, 'lcs', (n_rows, R), torch.int32)):
            if t is not None and (t.device != dev or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()):
                raise ValueError('%s must be a contiguous %s %s tensor on %s' % (name, shape, dtype, dev))
        N.check(N.lib.rfn_rougel_score(res.data_ptr(), n_rows, T, row_img.data_ptr(), gts.data_ptr(), n_refs.data_ptr(), n_img, R,
                                       Tg, vocab, self._flags(end_token), C.c_double(self.beta), out.data_ptr(), N.ptr(lcs),
                                       ws.data_ptr(), ws.numel(), N.stream_ptr()), 'rfn_rougel_score')
        return out

    def compute_score(self, gts, res, end_token=False):
        """The reference's interface: gts {image_id: [caption, ...]}, res {image_id: [caption]} (or CiderD.compute_score's list),
        captions being space-separated id strings.  end_token=False (the default): validation captions as
        eval_utils.decode_sequence writes them, without a 0 (a 0 token raises ValueError; an empty string is an empty caption);
        end_token=True: the reward's captions as array_to_str writes them.  -> (mean, np.ndarray of per-image scores, in res's
        order)."""
        if isinstance(res, dict):
            res = [{'image_id': k, 'caption': v} for k, v in res.items()]
        res_a, row_img, gts_a, n_refs, vocab = _id_arrays(gts, res, end_token=end_token)
        dev = torch.device('cuda', torch.cuda.current_device())
        s = self.score_ids(torch.from_numpy(res_a).to(dev), row_img, torch.from_numpy(gts_a), n_refs, vocab=vocab,
                           end_token=end_token)
        return mean_score(s)[0].item(), s.cpu().numpy()

    def method(self):
        return 'Rouge'


def mean_score(scores, out=None):
    """The mean of a (N,) or (N, k) float64 device tensor's first column over the rows that are not NaN, in a fixed order
    (bitwise repeatable) -> (mean, skipped): one-element float64 and int64 device tensors.  No synchronisation."""
    if scores.dtype != torch.float64 or scores.dim() not in (1, 2) or not scores.is_contiguous() or scores.device.type != 'cuda':
        raise ValueError('scores must be a contiguous float64 (N,) or (N, k) tensor on the GPU')
    mean = torch.empty(1, dtype=torch.float64, device=scores.device) if out is None else out
    skipped = torch.empty(1, dtype=torch.int64, device=scores.device)
    N.check(N.lib.rfn_score_mean(scores.data_ptr(), scores.shape[0], 1 if scores.dim() == 1 else scores.shape[1],
                                 mean.data_ptr(), skipped.data_ptr(), N.stream_ptr()), 'rfn_score_mean')
    return mean, skipped


def _int_word(w):
    x = int(w)
    if str(x) != str(w):
        raise ValueError('token %r is not an id in canonical form' % (w,))
    return x


def _words(s):
    try:
        return [_int_word(w) for w in s.split()]
    except ValueError as e:
        raise ValueError('CIDEr-D scores token-id captions: %s' % e) from None


def _row(words, T):
    """One id row whose array_to_str is `words`: a caption either ends at its only 0 or fills all T ids."""
    if words and words[-1] == 0 and 0 not in words[:-1]:
        return words + [0] * (T - len(words))
    if 0 not in words and len(words) == T:
        return words
    raise ValueError('caption %r is not an id row of width %d as array_to_str writes it (words up to and including the '
                     'first 0, or exactly T ids without one)' % (' '.join(map(str, words)), T))


def _plain_row(words, T):
    """One id row whose validation caption (the ids before the first 0) is `words`."""
    if 0 in words:
        raise ValueError('caption %r holds the end token 0: a validation caption stops before it (end_token=True scores the '
                         'reward\'s captions)' % ' '.join(map(str, words)))
    return words + [0] * (T - len(words))


def _id_arrays(gts, res, end_token=True):
    """compute_score's dicts (gts {image_id: [caption, ...]}, res [{'image_id': id, 'caption': [caption]}]) as id arrays:
    res (N, T) int64, row_img (N,) int32 tensor, gts (n_img, R, Tg) int64, n_refs (n_img,) int32 tensor, vocab.
    end_token=False: captions without a 0 (possibly empty), padded with 0."""
    row = _row if end_token else _plain_row
    images, img_of = [], {}
    rows = []
    for entry in res:
        hyp = entry['caption']
        if not isinstance(hyp, list) or len(hyp) != 1:
            raise ValueError('each res caption is a list of one string')
        iid = entry['image_id']
        if iid not in img_of:
            refs = gts[iid]
            if not isinstance(refs, list) or not refs:
                raise ValueError('gts[%r] must be a non-empty list of captions' % (iid,))
            img_of[iid] = len(images)
            images.append([_words(s) for s in refs])
        rows.append((_words(hyp[0]), img_of[iid]))
    T = max(1, max(len(w) for w, _ in rows))
    Tg = max(1, max(len(w) for refs in images for w in refs))
    res_a = np.array([row(w, T) for w, _ in rows], dtype=np.int64)
    R = max(len(refs) for refs in images)
    gts_a = np.zeros((len(images), R, Tg), dtype=np.int64)
    for i, refs in enumerate(images):
        for j, w in enumerate(refs):
            gts_a[i, j] = row(w, Tg)
    vocab = int(max(res_a.max(), gts_a.max(), 0))
    return (res_a, torch.tensor([i for _, i in rows], dtype=torch.int32), gts_a,
            torch.tensor([len(r) for r in images], dtype=torch.int32), min(vocab, MAX_ID))


_ROW_CACHE = {}


def _scst_row_img(B, seq_per_img, dev):
    key = (B, seq_per_img, str(dev))
    if key not in _ROW_CACHE:
        _ROW_CACHE[key] = torch.tensor([(r % B) // seq_per_img for r in range(2 * B)], dtype=torch.int32, device=dev)
    return _ROW_CACHE[key]


def pad_gts(gts_list, dev):
    """data['gts'] (a list of per-image (n_refs_i, T) id arrays) -> device (n_img, max_refs, T) int64, n_refs int32."""
    arrs = [np.asarray(g.cpu() if torch.is_tensor(g) else g) for g in gts_list]
    widths = {a.shape[1] for a in arrs}
    if len(widths) != 1:
        raise ValueError('every data[\'gts\'] array needs the same width (got %s)' % sorted(widths))
    n_refs = np.array([a.shape[0] for a in arrs], dtype=np.int32)
    out = np.zeros((len(arrs), int(n_refs.max()), widths.pop()), dtype=np.int64)
    for i, a in enumerate(arrs):
        out[i, :a.shape[0]] = a
    return torch.from_numpy(out).to(dev), torch.from_numpy(n_refs).to(dev)


def scst_reward(scorer, gen_result, greedy_res, gts, n_refs, seq_per_img, cider_weight=1.0, use_baseline=True, out64=None,
                bleu_scorer=None, bleu4_weight=0.0):
    """compute_reward on the device: scores the B sampled rows then the B greedy rows (row r points at image
    (r % B) // seq_per_img), -> (B, T) float32 reward = cider_weight * (s[b] - s[B + b]) (or cider_weight * s[b]).  gts:
    (n_img, R, Tg) padded references, n_refs (n_img,).  out64: optional (B, T) float64 tensor that receives the same reward
    before the cast.  bleu_scorer: a BleuD -> the reward is bleu4_weight * BLEU-4 + cider_weight * CIDEr-D, each as a
    difference to the greedy row under use_baseline (`scorer` may then be None: the CIDEr-D term is the reference's 0)."""
    B, T = gen_result.shape
    if greedy_res.shape != gen_result.shape:
        raise ValueError('gen_result and greedy_res must have the same shape')
    if scorer is None and bleu_scorer is None:
        raise ValueError('scst_reward needs a CIDEr-D scorer, a BLEU-D scorer or both')
    dev = gen_result.device
    res = torch.cat([gen_result.to(torch.int64), greedy_res.to(dev, torch.int64)], 0)
    row_img = _scst_row_img(B, seq_per_img, dev)
    scores = None if scorer is None else scorer.score_ids(res, row_img, gts, n_refs)
    bleu = None if bleu_scorer is None else bleu_scorer.score_ids(res, row_img, gts, n_refs)
    out = torch.empty(B, T, dtype=torch.float32, device=dev)
    N.check(N.lib.rfn_scst_reward_mix(N.ptr(scores), C.c_double(cider_weight), N.ptr(bleu),
                                      C.c_double(0.0 if bleu is None else bleu4_weight), B, T, int(bool(use_baseline)),
                                      out.data_ptr(), N.ptr(out64), N.stream_ptr()), 'rfn_scst_reward_mix')
    return out


_GROUP_CACHE = {}
_BASELINES = {'none': 0, 'loo': 1}


def _group_row_img(rows, n, dev):
    key = (rows, n, str(dev))
    if key not in _GROUP_CACHE:
        _GROUP_CACHE[key] = torch.tensor([r // n for r in range(rows)], dtype=torch.int32, device=dev)
    return _GROUP_CACHE[key]


def scst_group_reward(scorer, gen_result, gts, n_refs, n, cider_weight=1.0, baseline='loo', out64=None, bleu_scorer=None,
                      bleu4_weight=0.0):
    """The multi-sample self-critical reward on the device (rfn.h "multi-sample self-critical"): gen_result (B*n, T) holds n
    draws per image, image-major (row r is a draw of image r // n, as RecurrentFusionModel.sample_group returns them); gts
    (B, R, Tg) padded references, n_refs (B,).  The rows are scored once, then ONE launch forms the (B*n, T) float32 reward:
    baseline 'loo': a draw's score minus the mean score of the image's other n - 1 draws (n >= 2); 'none': the score itself.
    Weights, bleu_scorer and out64 as scst_reward.  After the first call at a shape nothing is allocated but the results and
    nothing synchronises."""
    if baseline not in _BASELINES:
        raise ValueError("baseline is 'loo' or 'none', got %r" % (baseline,))
    n = int(n)
    rows, T = gen_result.shape
    if n < 1 or rows % n:
        raise ValueError('%d rows are not n = %d draws per image' % (rows, n))
    if baseline == 'loo' and n < 2:
        raise ValueError("the leave-one-out baseline needs n >= 2 draws per image (baseline='none' takes n = 1)")
    if gts.shape[0] * n != rows:
        raise ValueError('%d rows of %d draws per image need %d images of references, got %d' % (rows, n, rows // n, gts.shape[0]))
    if scorer is None and bleu_scorer is None:
        raise ValueError('scst_group_reward needs a CIDEr-D scorer, a BLEU-D scorer or both')
    dev = gen_result.device
    res = gen_result.to(torch.int64)
    row_img = _group_row_img(rows, n, dev)
    scores = None if scorer is None else scorer.score_ids(res, row_img, gts, n_refs)
    bleu = None if bleu_scorer is None else bleu_scorer.score_ids(res, row_img, gts, n_refs)
    out = torch.empty(rows, T, dtype=torch.float32, device=dev)
    N.check(N.lib.rfn_scst_reward_group(N.ptr(scores), C.c_double(cider_weight), N.ptr(bleu),
                                        C.c_double(0.0 if bleu is None else bleu4_weight), rows, n, T, _BASELINES[baseline],
                                        out.data_ptr(), N.ptr(out64), N.stream_ptr()), 'rfn_scst_reward_group')
    return out


_DISTINCT_BASELINES = {'none': 0, 'weighted': 1}


def _distinct_weight(weight, rows, n, dev):
    """`weight` of a distinct-sample set -> a contiguous (rows,) float64 device tensor: RecurrentFusionModel.stochastic_beams
    ['weight'] (B, n), or the dict itself."""
    if isinstance(weight, dict):
        weight = weight['weight']
    if not torch.is_tensor(weight) or weight.numel() != rows:
        raise ValueError('weight needs one entry per row (%d = images * %d), got %s' % (rows, n, tuple(getattr(weight, 'shape', ()))))
    return weight.to(dev, torch.float64).contiguous().view(rows)


def scst_distinct_reward(scorer, cands_rows, weight, gts, n_refs, n, cider_weight=1.0, baseline='weighted', out64=None,
                         bleu_scorer=None, bleu4_weight=0.0):
    """The reward that makes a sample_distinct set trainable (rfn.h rfn_scst_reward_distinct; Kool, van Hoof and Welling 2019):
    cands_rows (B*n, T) are the n distinct captions per image, image-major, `weight` their importance weights
    (model.stochastic_beams['weight'], (B, n) float64, or that dict).  With q_j = w_j / sum_i w_i over the image's rows with
    w > 0 and s the mixed score: baseline 'weighted': reward = n * q_j * (s_j - sum_i q_i * s_i); 'none': n * q_j * s_j.  Dead
    rows and the threshold row (w = 0) get exactly 0.  Fed to rl_loss(..., n=n) this is the normalised importance-weighted
    policy gradient.  The weighted baseline needs n >= 3: with n = 2 the one weighted row's coefficient is identically zero.
    Weights, bleu_scorer and out64 as scst_group_reward; one launch behind the scoring, nothing synchronises."""
    if baseline not in _DISTINCT_BASELINES:
        raise ValueError("baseline is 'weighted' or 'none', got %r" % (baseline,))
    n = int(n)
    rows, T = cands_rows.shape
    if n < 1 or rows % n:
        raise ValueError('%d rows are not n = %d captions per image' % (rows, n))
    if baseline == 'weighted' and n < 3:
        raise ValueError("the weighted baseline needs n >= 3 captions per image: the last live row is the threshold and weighs 0, so "
                         "n = 2 leaves one weighted sample whose coefficient is identically zero (baseline='none' takes any n)")
    if gts.shape[0] * n != rows:
        raise ValueError('%d rows of %d captions per image need %d images of references, got %d' % (rows, n, rows // n, gts.shape[0]))
    if scorer is None and bleu_scorer is None:
        raise ValueError('scst_distinct_reward needs a CIDEr-D scorer, a BLEU-D scorer or both')
    dev = cands_rows.device
    w = _distinct_weight(weight, rows, n, dev)
    res = cands_rows.to(torch.int64)
    row_img = _group_row_img(rows, n, dev)
    scores = None if scorer is None else scorer.score_ids(res, row_img, gts, n_refs)
    bleu = None if bleu_scorer is None else bleu_scorer.score_ids(res, row_img, gts, n_refs)
    out = torch.empty(rows, T, dtype=torch.float32, device=dev)
    N.check(N.lib.rfn_scst_reward_distinct(N.ptr(scores), C.c_double(cider_weight), N.ptr(bleu),
                                           C.c_double(0.0 if bleu is None else bleu4_weight), w.data_ptr(), rows, n, T,
                                           _DISTINCT_BASELINES[baseline], out.data_ptr(), N.ptr(out64), N.stream_ptr()),
            'rfn_scst_reward_distinct')
    return out


def consensus(scorer, cands, n_cand=None, weights=None, end_token=True, want_pairs=False):
    """Consensus (minimum-Bayes-risk) reranking of decoded candidates: CiderD.consensus on `scorer` (table or corpus df).  Any
    other scorer raises NotImplementedError (only the CIDEr-D utility is on the device)."""
    if not isinstance(scorer, CiderD):
        raise NotImplementedError('consensus reranking is implemented for the CiderD scorer only, got %s' % type(scorer).__name__)
    return scorer.consensus(cands, n_cand, weights, end_token, want_pairs)


def consensus_gather(best, n, seq=None, seq_lp=None, p=None):
    """Row best[k] of image k's n rows, for each array given, in ONE launch (rfn_consensus_gather): seq (B*n, S) or (B, n, S)
    int64, seq_lp the same shape float32, p (B, n) float32 -> (seq (B, S), seq_lp (B, S), p (B,)), None where none was given.
    An image whose pick is -1 gets zeros."""
    B = best.numel()
    out, S = [], 1
    for t, dtype in ((seq, torch.int64), (seq_lp, torch.float32)):
        if t is not None:
            if t.dtype != dtype or not t.is_contiguous() or t.numel() % (B * n) or t.device != best.device:
                raise ValueError('consensus_gather takes contiguous (images * n, S) int64 / float32 tensors on the picks\' device')
            S = t.numel() // (B * n)
    if seq is not None and seq_lp is not None and seq.numel() != seq_lp.numel():
        raise ValueError('seq and seq_lp must have the same shape')
    if p is not None and (p.dtype != torch.float32 or not p.is_contiguous() or p.numel() != B * n or p.device != best.device):
        raise ValueError('p must be a contiguous (images, n) float32 tensor on the picks\' device')
    for t in (seq, seq_lp):
        out.append(None if t is None else torch.empty(B, S, dtype=t.dtype, device=t.device))
    out.append(None if p is None else torch.empty(B, dtype=torch.float32, device=p.device))
    N.check(N.lib.rfn_consensus_gather(best.data_ptr(), B, n, S, N.ptr(seq) or None, N.ptr(out[0]) or None, N.ptr(seq_lp) or None,
                                       N.ptr(out[1]) or None, N.ptr(p) or None, N.ptr(out[2]) or None, N.stream_ptr()),
            'rfn_consensus_gather')
    return tuple(out)


def diversity(scorer, cands, n_cand=None, end_token=False, want=DIVERSITY_OUTPUTS):
    """Div-m, mBLEU and Self-CIDEr of decoded caption sets: CiderD.diversity on `scorer` (table or corpus df).  Any other scorer
    raises NotImplementedError (Self-CIDEr is built on the CIDEr-D utility)."""
    if not isinstance(scorer, CiderD):
        raise NotImplementedError('the diversity metrics are implemented for the CiderD scorer only, got %s' % type(scorer).__name__)
    return scorer.diversity(cands, n_cand, end_token, want=want)


def group_stats(scores, n, n_cand=None):
    """Best-of-n, its lowest index and mean-of-n of a score column (rfn_score_group_stats): scores a contiguous float64 (B*n,) or
    (B*n, k) device tensor (the first column is read), rows image-major; n_cand (B,) valid candidates per image (None: all).
    -> (best (B,) float64, arg (B,) int64, mean (B,) float64); NaN, -1, NaN for an image one of whose valid scores is NaN.  One
    launch, no synchronisation."""
    if scores.dtype != torch.float64 or scores.dim() not in (1, 2) or not scores.is_contiguous() or scores.device.type != 'cuda':
        raise ValueError('scores must be a contiguous float64 (N,) or (N, k) tensor on the GPU')
    n = int(n)
    if n < 1 or scores.shape[0] % n or scores.shape[0] == 0:
        raise ValueError('%d rows are not n = %d scores per image' % (scores.shape[0], n))
    dev, B = scores.device, scores.shape[0] // n
    if n_cand is not None:
        n_cand = n_cand.to(dev, torch.int32).contiguous()
        if n_cand.numel() != B:
            raise ValueError('n_cand needs one entry per image')
    best = torch.empty(B, dtype=torch.float64, device=dev)
    arg = torch.empty(B, dtype=torch.int64, device=dev)
    mean = torch.empty(B, dtype=torch.float64, device=dev)
    N.check(N.lib.rfn_score_group_stats(scores.data_ptr(), 1 if scores.dim() == 1 else scores.shape[1], B, n, N.ptr(n_cand) or None,
                                        best.data_ptr(), arg.data_ptr(), mean.data_ptr(), N.stream_ptr()), 'rfn_score_group_stats')
    return best, arg, mean


_DEFAULT = {}


def default_scorer():
    """The reference's module-level scorer, CiderD(df='coco-train-idxs') (reads data/coco-train-idxs.p)."""
    if 'scorer' not in _DEFAULT:
        _DEFAULT['scorer'] = CiderD(df='coco-train-idxs')
    return _DEFAULT['scorer']


def _reward_terms(opt, scorer, bleu_scorer):
    """opt's reward weights as compute_reward reads them -> (scorer, bleu_scorer, cider_weight, bleu4_weight, use_baseline)."""
    if getattr(opt, 'spice_weight', 0) > 0:
        raise NotImplementedError('the SPICE-D reward is not ported (of BLEU-D and SPICE-D only BLEU-D is); set spice_weight = 0')
    w_b = getattr(opt, 'bleu4_weight', 0)
    if w_b > 0 and bleu_scorer is None:
        raise NotImplementedError('of BLEU-D and SPICE-D only BLEU-D is ported, and bleu4_weight > 0 needs its scorer: pass '
                                  'bleu_scorer=BleuD() (or set bleu4_weight = 0)')
    if not w_b > 0:
        bleu_scorer = None             # the reference does not run BleuD then
    w, base = getattr(opt, 'cider_weight', 1.0), getattr(opt, 'use_baseline', 1)
    if scorer is None and not (bleu_scorer is not None and w == 0):
        scorer = default_scorer()      # not with cider_weight == 0 beside BLEU-D: that mix needs no df pickle
    return scorer, bleu_scorer, w, w_b, base


def _reward(model_sample, data, gen_result, opt, device, scorer, bleu_scorer):
    scorer, bleu_scorer, w, w_b, base = _reward_terms(opt, scorer, bleu_scorer)
    with torch.no_grad():
        greedy_res = model_sample()[0]
    B, T = gen_result.shape
    gts, n_refs = pad_gts(data['gts'], gen_result.device)
    spi = B // len(data['gts'])
    if device:
        return scst_reward(scorer, gen_result, greedy_res, gts, n_refs, spi, w, base, bleu_scorer=bleu_scorer, bleu4_weight=w_b)
    out64 = torch.empty(B, T, dtype=torch.float64, device=gen_result.device)
    scst_reward(scorer, gen_result, greedy_res, gts, n_refs, spi, w, base, out64=out64, bleu_scorer=bleu_scorer, bleu4_weight=w_b)
    return out64.cpu().numpy()


def get_self_critical_reward_feat_array(idx_to_word, model, fc_feat_array, att_feat_array, data, gen_result, opt, device=False,
                                        scorer=None, bleu_scorer=None):
    """get_rewards.py:115-129: greedy baseline from model.sample (in the module's current mode, without gradients), then
    the reward.  -> numpy (B, T) float64 like the reference, or the device (B, T) float32 tensor with device=True.
    scorer: a CiderD (default: default_scorer(), the reference's df='coco-train-idxs'); bleu_scorer: a BleuD, needed when
    opt.bleu4_weight > 0 (NotImplementedError without it; opt.spice_weight > 0 always raises it)."""
    return _reward(lambda: model.sample(list(fc_feat_array), list(att_feat_array)), data, gen_result, opt, device, scorer,
                   bleu_scorer)


def get_self_critical_reward(idx_to_word, model, fc_feats, att_feats, data, gen_result, opt, device=False, scorer=None,
                             bleu_scorer=None):
    """get_rewards.py:132-140 (single-feature models): as get_self_critical_reward_feat_array."""
    return _reward(lambda: model.sample(fc_feats, att_feats), data, gen_result, opt, device, scorer, bleu_scorer)


def get_self_critical_reward_group(data, gen_result, n, opt, device=False, scorer=None, bleu_scorer=None):
    """The reward of a multi-sample self-critical step: gen_result (B*n, T) are RecurrentFusionModel.sample_group's n draws per
    image and data['gts'] holds the B images' references.  No greedy pass: with opt.use_baseline (the default) a draw's baseline
    is the mean score of the image's other draws, with opt.use_baseline = 0 there is none.  opt.cider_weight, opt.bleu4_weight
    and opt.spice_weight are honoured exactly as by get_self_critical_reward_feat_array.  -> numpy (B*n, T) float64, or the
    device (B*n, T) float32 tensor with device=True."""
    scorer, bleu_scorer, w, w_b, base = _reward_terms(opt, scorer, bleu_scorer)
    rows, T = gen_result.shape
    if len(data['gts']) * int(n) != rows:
        raise ValueError('%d rows of %d draws per image need %d images in data[\'gts\'], got %d'
                         % (rows, n, rows // max(1, int(n)), len(data['gts'])))
    gts, n_refs = pad_gts(data['gts'], gen_result.device)
    how = 'loo' if base else 'none'
    if device:
        return scst_group_reward(scorer, gen_result, gts, n_refs, n, w, how, bleu_scorer=bleu_scorer, bleu4_weight=w_b)
    out64 = torch.empty(rows, T, dtype=torch.float64, device=gen_result.device)
    scst_group_reward(scorer, gen_result, gts, n_refs, n, w, how, out64=out64, bleu_scorer=bleu_scorer, bleu4_weight=w_b)
    return out64.cpu().numpy()


def get_self_critical_reward_distinct(data, gen_result, stochastic_beams, opt, device=False, scorer=None, bleu_scorer=None):
    """The reward of a step trained on RecurrentFusionModel.sample_distinct's set: gen_result (B*n, T) are the n distinct captions
    per image, stochastic_beams the model's `stochastic_beams` (its 'weight' is (B, n)), data['gts'] the B images' references.
    With opt.use_baseline (the default) the estimator's built-in weighted baseline is used (n >= 3), with opt.use_baseline = 0
    none.  Weights of the scores as get_self_critical_reward_group.  -> numpy (B*n, T) float64, or the device (B*n, T) float32
    tensor with device=True."""
    scorer, bleu_scorer, w, w_b, base = _reward_terms(opt, scorer, bleu_scorer)
    rows, T = gen_result.shape
    weight = stochastic_beams['weight'] if isinstance(stochastic_beams, dict) else stochastic_beams
    if weight.dim() != 2 or weight.size(0) != len(data['gts']) or weight.numel() != rows:
        raise ValueError('%d rows need stochastic_beams[\'weight\'] of shape (%d images, n) with images * n = rows, got %s'
                         % (rows, len(data['gts']), tuple(weight.shape)))
    n = weight.size(1)
    gts, n_refs = pad_gts(data['gts'], gen_result.device)
    how = 'weighted' if base else 'none'
    if device:
        return scst_distinct_reward(scorer, gen_result, weight, gts, n_refs, n, w, how, bleu_scorer=bleu_scorer, bleu4_weight=w_b)
    out64 = torch.empty(rows, T, dtype=torch.float64, device=gen_result.device)
    scst_distinct_reward(scorer, gen_result, weight, gts, n_refs, n, w, how, out64=out64, bleu_scorer=bleu_scorer, bleu4_weight=w_b)
    return out64.cpu().numpy()
