"""Generate the caption-set diversity goldens (tests/golden/diversity_{table,edge}.npz).

Usage (where the reference checkout exists; RFN_REFERENCE names it, as for tools/make_ciderd_golden.py):
    python tools/make_diversity_golden.py            # (re)write the goldens
    python tools/make_diversity_golden.py --check    # regenerate in memory, compare with the committed files byte for byte

The candidates are those of the committed consensus goldens (tools/make_consensus_golden.py): `table` 16 images x n = 5 x T = 16,
`edge` 4 images x n = 7 x T = 8 with n_cand = 1, 2, 3, 7 (an END-only candidate, duplicates, repeated n-grams), each with its
table df.  Both caption conventions are stored: the keys without a suffix read a caption up to and including its first 0 (the
convention the consensus goldens' U was produced in), the keys ending in `_words` strictly before it (what evalcap scores).

What the reference pins here is mBLEU: its own coco-caption/pycocoevalcap/bleu Bleu(4).compute_score, called once per candidate
slot i with res = candidate i and gts = the image's other candidates, over the images that have the slot and at least one other
candidate.  That call returns the slot's corpus BLEU (mbleu_corpus[i]) and the per-image rows (mbleu[:, i]); the integer
components come from the BleuScorer it builds.  The reference has no Div-m and no Self-CIDEr: distinct, words, div, eig and
self_cider are the restatement's (tests/diversity_cpu.py), whose U is asserted against the consensus golden.  The restatement's
mBLEU is asserted here against every reference number.  Fixed zip timestamps: a rerun reproduces the files byte for byte.
"""
import argparse
import contextlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import ciderd_cpu as CPU  # noqa: E402
import diversity_cpu as DC  # noqa: E402
import make_ciderd_golden as MG  # noqa: E402


def reference_mbleu(cands, n_cand, end_token):
    """-> mbleu (B, n, 4), comps (B, n, 10) int32, corpus (n, 4), NaN / 0 where the reference was not asked."""
    sys.path.insert(0, os.path.join(MG.REF, 'coco-caption'))
    from pycocoevalcap.bleu.bleu import Bleu
    from pycocoevalcap.bleu.bleu_scorer import BleuScorer
    B, n, _ = cands.shape
    caps = DC.captions_of(cands, n_cand, end_token, 32767)
    text = lambda w: ' '.join(str(x) for x in w)   # noqa: E731
    mbleu, comps, corpus = np.full((B, n, 4), np.nan), np.zeros((B, n, 10), dtype=np.int32), np.full((n, 4), np.nan)
    for i in range(n):
        imgs = [k for k in range(B) if caps[k] is not None and len(caps[k]) > max(1, i)]
        if not imgs:
            continue
        res = {k: [text(caps[k][i])] for k in imgs}
        gts = {k: [text(w) for j, w in enumerate(caps[k]) if j != i] for k in imgs}
        with contextlib.redirect_stdout(io.StringIO()):
            score, rows = Bleu(4).compute_score(gts, res)
        sc = BleuScorer(n=4)
        for k in imgs:
            sc += (res[k][0], gts[k])
        score2, rows2 = sc.compute_score(option='closest', verbose=0)
        assert score2 == score and rows2 == rows
        corpus[i] = score
        for x, k in enumerate(imgs):
            mbleu[k, i] = [rows[m][x] for m in range(4)]
            c = sc.ctest[x]
            comps[k, i] = [c['testlen'], sc._single_reflen(c['reflen'], 'closest', c['testlen'])] + c['guess'] + c['correct']
    return mbleu, comps, corpus


def build_tiers():
    tiers = {}
    for name in ('table', 'edge'):
        g = dict(np.load(os.path.join(GOLDEN, 'consensus_%s.npz' % name)))
        df, docs = CPU.df_from_arrays(g['df_ids'], g['df_counts']), float(g['ref_docs'])
        t = {k: g[k] for k in ('cands', 'n_cand', 'df_ids', 'df_counts', 'ref_docs')}
        for end_token, sfx in ((True, ''), (False, '_words')):
            d = DC.diversity(g['cands'], g['n_cand'], df, docs, end_token=end_token)
            if end_token:
                assert np.allclose(d['U'], g['U'], rtol=1e-12, atol=1e-13, equal_nan=True), name
            mbleu, comps, corpus = reference_mbleu(g['cands'], g['n_cand'], end_token)
            assert np.allclose(d['mbleu'], mbleu, rtol=1e-12, atol=0, equal_nan=True), (name, sfx)
            assert np.allclose(d['mbleu_corpus'], corpus, rtol=1e-12, atol=0, equal_nan=True), (name, sfx)
            assert np.array_equal(d['mbleu_comps'], comps), (name, sfx)
            t.update({'mbleu' + sfx: mbleu, 'mbleu_comps' + sfx: comps, 'mbleu_corpus' + sfx: corpus})
            for k in ('distinct', 'words', 'div', 'eig', 'self_cider'):
                t[k + sfx] = d[k]
        tiers[name] = t
    return tiers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--check', action='store_true', help='compare with the committed goldens instead of writing them')
    args = ap.parse_args()
    if not os.path.isdir(MG.REF):
        sys.exit('the reference checkout (%s) does not exist: mBLEU is pinned by its own Bleu scorer' % MG.REF)
    bad = 0
    for name, t in build_tiers().items():
        path = os.path.join(GOLDEN, 'diversity_%s.npz' % name)
        data = MG.npz_bytes(t)
        assert len(data) < 1 << 20, (name, len(data))
        if args.check:
            same = os.path.exists(path) and open(path, 'rb').read() == data
            bad += not same
            print('%-32s %s' % (os.path.relpath(path, ROOT), 'identical' if same else 'DIFFERS'))
        else:
            with open(path, 'wb') as f:
                f.write(data)
            print('wrote %s (%d bytes, %d images x %d candidates)' % (os.path.relpath(path, ROOT), len(data), t['cands'].shape[0],
                                                                     t['cands'].shape[1]))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
