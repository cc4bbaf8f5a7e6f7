"""Generate the validation-metric golden tiers (tests/golden/evalcap_*.npz) by running the reference's own scorers.

Usage (where the reference checkout exists; RFN_REFERENCE, default /root/reference):
    python tools/make_evalcap_golden.py            # (re)write the goldens
    python tools/make_evalcap_golden.py --check    # regenerate in memory, compare with the committed files byte for byte
    python tools/make_evalcap_golden.py --time     # wall time of the reference's three scorers on the 5000 x 5 split that
                                                   # tools/bench_reward.py --eval times (prints one JSON line, writes nothing)

Imports coco-caption/pycocoevalcap's Bleu(4), Rouge() and Cider() and feeds them what eval_utils.language_eval would after
decode_sequence: per score row, the ids strictly BEFORE the first 0 joined by spaces.  There is NO PTB tokenizer step
(language_eval runs a Java tokenizer over words first; ids have nothing to tokenize), so these goldens pin the metrics' arithmetic
in id space, not a COCO leaderboard number.  Rouge() is also run on the reward's convention (ids up to and including the first 0).
Stored per tier: bleu (N x 4 per-sentence), comps (N x 10: testlen, reflen, guess[4], correct[4]), bleu_corpus (4), rouge (N),
lcs (N x R, 0 behind an image's references), rouge_end / lcs_end (the end-token convention), cider (N), and the corpus means
rouge_mean, rouge_end_mean, cider_mean.  Tiers:
  - edge (7 images: an empty hypothesis, a full-width caption without a 0, a hypothesis equal to a reference, one word repeated,
    a single-token caption, 1 to 7 references) and edge1 (n_img = 1); inputs stored;
  - near, near_spi: the inputs of the committed tests/golden/bleud_near.npz / bleud_near_spi5.npz (loaded, not stored again), all
    2B score rows with compute_reward's row -> image map, so n = 3 and 4 are reached;
  - val: 300 images, 3 to 7 references, T = 16, one hypothesis per image (tests/evalcap_cases.val_split); inputs stored.
Also asserts that tests/evalcap_cpu.py agrees with the reference on every tier.  Files are written with fixed zip timestamps, so a
rerun reproduces them byte for byte.
"""
import argparse
import contextlib
import io
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import ciderd_cpu as CPU  # noqa: E402
import evalcap_cases as CASES  # noqa: E402
import evalcap_cpu as ECPU  # noqa: E402
import make_ciderd_golden as CG  # noqa: E402


def string_dicts(res, row_img, gts, n_refs, end_token=False):
    def s(row):
        return ' '.join(str(x) for x in ECPU.caption(row, end_token))
    hyps = {r: [s(res[r])] for r in range(len(res))}
    refs = {r: [s(gts[int(row_img[r])][j]) for j in range(int(n_refs[int(row_img[r])]))] for r in range(len(res))}
    return refs, hyps


def scorers():
    sys.path.insert(0, os.path.join(CG.REF, 'coco-caption'))
    from pycocoevalcap.bleu.bleu import Bleu
    from pycocoevalcap.bleu.bleu_scorer import BleuScorer
    from pycocoevalcap.cider.cider import Cider
    from pycocoevalcap.rouge.rouge import Rouge, my_lcs
    return Bleu, BleuScorer, Cider, Rouge, my_lcs


def reference_metrics(res, row_img, gts, n_refs, timing=None):
    Bleu, BleuScorer, Cider, Rouge, my_lcs = scorers()
    refs, hyps = string_dicts(res, row_img, gts, n_refs)
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        corpus, rows = Bleu(4).compute_score(refs, hyps)
    t1 = time.perf_counter()
    rouge_mean, rouge = Rouge().compute_score(refs, hyps)
    t2 = time.perf_counter()
    cider_mean, cider = Cider().compute_score(refs, hyps)
    t3 = time.perf_counter()
    if timing is not None:
        timing.update(bleu_ms=(t1 - t0) * 1e3, rouge_ms=(t2 - t1) * 1e3, cider_ms=(t3 - t2) * 1e3, total_ms=(t3 - t0) * 1e3)
        return None
    sc = BleuScorer(n=4)
    for r in range(len(res)):
        sc += (hyps[r][0], refs[r])
    corpus2, rows2 = sc.compute_score(option='closest', verbose=0)
    assert corpus2 == corpus and rows2 == rows
    comps = np.array([[c['testlen'], sc._single_reflen(c['reflen'], 'closest', c['testlen'])] + c['guess'] + c['correct']
                      for c in sc.ctest], dtype=np.int32)
    o = dict(bleu=np.array(rows, dtype=np.float64).T.copy(), comps=comps, bleu_corpus=np.array(corpus, dtype=np.float64),
             rouge=np.asarray(rouge, dtype=np.float64), rouge_mean=np.float64(rouge_mean),
             cider=np.asarray(cider, dtype=np.float64), cider_mean=np.float64(cider_mean))
    refs_e, hyps_e = string_dicts(res, row_img, gts, n_refs, end_token=True)
    m, s = Rouge().compute_score(refs_e, hyps_e)
    o.update(rouge_end=np.asarray(s, dtype=np.float64), rouge_end_mean=np.float64(m))
    for key, (rf, hy) in (('lcs', (refs, hyps)), ('lcs_end', (refs_e, hyps_e))):
        t = np.zeros((len(res), gts.shape[1]), dtype=np.int32)
        for r in range(len(res)):
            for j, ref in enumerate(rf[r]):
                t[r, j] = my_lcs(ref.split(' '), hy[r][0].split(' '))
        o[key] = t
    return o


def inputs():
    tiers = {}
    for name, (res, gts, n_refs, vocab) in (('edge', CASES.edge_tier()), ('edge1', CASES.edge1_tier()),
                                            ('val', CASES.val_split(31, 300, 3, 7))):
        tiers[name] = dict(res=res, row_img=np.arange(len(res), dtype=np.int32), gts=gts, n_refs=n_refs, vocab=vocab, store=True)
    for name, src in (('near', 'near'), ('near_spi', 'near_spi5')):
        g = np.load(os.path.join(CG.GOLDEN, 'bleud_%s.npz' % src))
        tiers[name] = dict(res=g['res'], row_img=CPU.scst_rows(int(g['B']), int(g['seq_per_img'])), gts=g['gts'],
                           n_refs=g['n_refs'], vocab=int(g['vocab']), store=False)
    return tiers


def build_tiers():
    out = {}
    for name, t in inputs().items():
        res, row_img, gts, n_refs = t['res'], t['row_img'], t['gts'], t['n_refs']
        o = reference_metrics(res, row_img, gts, n_refs)
        # the restatement agrees with the reference
        bleu, comps, corpus = ECPU.bleu_rows(res, row_img, gts, n_refs)
        assert np.array_equal(comps, o['comps']), name
        assert np.allclose(bleu, o['bleu'], rtol=1e-12, atol=0) and np.allclose(corpus, o['bleu_corpus'], rtol=1e-12, atol=0), name
        for end, suffix in ((False, ''), (True, '_end')):
            rouge, lcs = ECPU.rouge_rows(res, row_img, gts, n_refs, end_token=end)
            assert np.array_equal(lcs, o['lcs' + suffix]), name
            assert np.allclose(rouge, o['rouge' + suffix], rtol=1e-14, atol=0), name
            assert np.isclose(np.mean(rouge), o['rouge%s_mean' % suffix], rtol=1e-13), name
        cider = ECPU.cider_rows(res, row_img, gts, n_refs)
        assert np.allclose(cider, o['cider'], rtol=1e-12, atol=1e-13), (name, np.abs(cider - o['cider']).max())
        assert np.isclose(np.mean(cider), o['cider_mean'], rtol=1e-12, atol=1e-13), name
        if t['store']:
            o.update(res=res, row_img=row_img, gts=gts, n_refs=n_refs, vocab=np.int64(t['vocab']))
        out[name] = o
    return out


def time_reference(n_img=5000, refs=5):
    seq, gts, n_refs, _ = CASES.val_split(77, n_img, refs, refs)
    timing = {}
    reference_metrics(seq, np.arange(n_img, dtype=np.int32), gts, n_refs, timing)
    print(json.dumps(dict(images=n_img, refs=refs, T=int(seq.shape[1]), host=platform.processor() or platform.machine(),
                          python=platform.python_version(), **{k: round(v, 1) for k, v in timing.items()})))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--check', action='store_true', help='compare with the committed goldens instead of writing them')
    ap.add_argument('--time', action='store_true', help='print the reference scorers\' wall time at 5000 x 5; writes nothing')
    args = ap.parse_args()
    if args.time:
        return time_reference()
    bad = 0
    for name, t in build_tiers().items():
        path = os.path.join(CG.GOLDEN, 'evalcap_%s.npz' % name)
        data = CG.npz_bytes(t)
        assert len(data) < 1 << 18, (name, len(data))
        if args.check:
            same = os.path.exists(path) and open(path, 'rb').read() == data
            bad += not same
            print('%-30s %s' % (os.path.relpath(path, ROOT), 'identical' if same else 'DIFFERS'))
        else:
            with open(path, 'wb') as f:
                f.write(data)
            print('wrote %s (%d bytes, %d rows; BLEU-4 %.4f, ROUGE-L %.4f, CIDEr %.4f; rows with a matching 4-gram %.2f)' % (
                os.path.relpath(path, ROOT), len(data), len(t['rouge']), float(t['bleu_corpus'][3]), float(t['rouge_mean']),
                float(t['cider_mean']), float((t['comps'][:, 9] > 0).mean())))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
