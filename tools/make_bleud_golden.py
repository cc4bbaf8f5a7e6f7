"""Generate the BLEU-D golden tiers (tests/golden/bleud_*.npz) by running the reference's own scorers.

Usage (where the reference checkout exists; RFN_REFERENCE, default /root/reference):
    python tools/make_bleud_golden.py            # (re)write the goldens
    python tools/make_bleud_golden.py --check    # regenerate in memory, compare with the committed files byte for byte
    python tools/make_bleud_golden.py --time     # wall time of the reference's BleuD(4).compute_score per tier (prints only)

`res` and `gts` are built as get_rewards.compute_reward builds them (tools/make_ciderd_golden.py) and scored by the reference's
BleuD(4).compute_score; the rows' integer components come from the same package's BleuScorer, whose scores are asserted equal.
Tiers:
  - edge, c5, spi5: the inputs of the committed tests/golden/ciderd_<name>.npz (loaded, not stored again).  Stored: bleu
    (2B x 4), comps (2B x 10: testlen, reflen, guess[4], correct[4]), corpus (4) and compute_reward's mixed reward
    bleu4 * w_b + cider * w_c + 0 for (w_b, w_c, use_baseline) = (1, 0, 1), (0.5, 1, 1), (0.3, 0.7, 0) in float64 and float32
    (mix_<k>_64 / mix_<k>_32, the weightings in mix_weights), CIDEr-D taken from the committed golden scores.
  - near, near_spi5: random captions barely reach n = 3, 4, so these build each hypothesis from a reference of its own image
    (words substituted with probability 0.12, then truncated, or one word repeated 2-4 times, or pool words appended; 15 % of
    the rows stay random) at 128 images x 1 and 64 images x 5 with 3-7 references, T = 16.  They also store their inputs and the
    reference's corpus-df CIDEr-D scores.
Also asserts that tests/bleud_cpu.py agrees with the reference on every tier.  Files are written with fixed zip timestamps, so a
rerun reproduces them byte for byte.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import bleud_cpu as BCPU  # noqa: E402
import ciderd_cpu as CPU  # noqa: E402
import make_ciderd_golden as CG  # noqa: E402

MIXES = ((1.0, 0.0, 1), (0.5, 1.0, 1), (0.3, 0.7, 0))


def string_dicts(res, gts, n_refs, B, spi):
    hyps = [{'image_id': r, 'caption': [CG.ids_to_str(res[r])]} for r in range(2 * B)]
    refs = {r: [CG.ids_to_str(gts[(r % B) // spi][j]) for j in range(int(n_refs[(r % B) // spi]))] for r in range(2 * B)}
    return refs, hyps


def reference_bleu(res, gts, n_refs, B, spi, timing=None):
    """-> bleu (2B, 4), comps (2B, 10) int32, corpus (4,) of the reference's BleuD(4) / BleuScorer."""
    sys.path.insert(0, os.path.join(CG.REF, 'cider'))
    from pyciderevalcap.bleuD.bleuD import BleuD
    from pyciderevalcap.bleuD.bleuD_scorer import BleuScorer
    refs, hyps = string_dicts(res, gts, n_refs, B, spi)
    t0 = time.perf_counter()
    corpus, rows = BleuD(4).compute_score(refs, hyps)
    if timing is not None:
        timing.append(time.perf_counter() - t0)
    sc = BleuScorer(n=4)
    for h in hyps:
        sc += (h['caption'][0], refs[h['image_id']])
    corpus2, rows2 = sc.compute_score(option='closest', verbose=0)
    assert corpus2 == corpus and rows2 == rows
    comps = np.array([[c['testlen'], sc._single_reflen(c['reflen'], 'closest', c['testlen'])] + c['guess'] + c['correct']
                      for c in sc.ctest], dtype=np.int32)
    return np.array(rows, dtype=np.float64).T.copy(), comps, np.array(corpus, dtype=np.float64)


def near_rows(rng, gts, n_refs, pools, B, spi, T):
    rows = np.zeros((2 * B, T), dtype=np.int64)
    vocab_hi = int(max(p.max() for p in pools))
    for r in range(2 * B):
        i = (r % B) // spi
        if rng.random() < 0.15:
            rows[r] = CG.captions(rng, 1, T, pools[i])[0]
            continue
        words = CPU.caption(gts[i, int(rng.integers(0, n_refs[i]))])
        ended = words[-1] == 0
        body = [int(rng.choice(pools[i])) if rng.random() < 0.12 else w for w in (words[:-1] if ended else words)]
        u = rng.random()
        if u < 0.25 and len(body) > 1:                       # truncate
            body = body[:int(rng.integers(1, len(body)))]
            ended = True
        elif u < 0.45 and body:                              # repeat one word 2-4 times
            p = int(rng.integers(0, len(body)))
            body = body[:p] + [body[p]] * int(rng.integers(2, 5)) + body[p:]
        elif u < 0.55:                                       # append pool words
            body = body + [int(x) for x in rng.choice(pools[i], int(rng.integers(1, 4)))]
        if len(body) >= T:
            rows[r] = body[:T]                               # fills the row: no end token
        else:
            rows[r, :len(body)] = body                       # a row shorter than T ends in 0 whether its source did or not
            rows[r, len(body) + 1:] = rng.integers(1, vocab_hi + 1, T - len(body) - 1)   # never read
    return rows


def tier_near(seed, n_img, spi, T=16, vocab=9487):
    rng = np.random.default_rng(seed)
    common = rng.integers(1, vocab + 1, 40)
    gts, n_refs, pools = CG.image_set(rng, n_img, 3, 7, T, vocab, common)
    B = n_img * spi
    return dict(res=near_rows(rng, gts, n_refs, pools, B, spi, T), gts=gts, n_refs=n_refs, B=B, seq_per_img=spi, vocab=vocab)


def coverage(t, bleu, comps):
    """Fractions of rows: a matching 4-gram, clipping active, brevity penalty, closest-length tie, no end token."""
    res, gts, n_refs, B, spi = t['res'], t['gts'], t['n_refs'], int(t['B']), int(t['seq_per_img'])
    clip = tie = 0
    for r in range(2 * B):
        i = (r % B) // spi
        refs = [CPU.caption(gts[i, j]) for j in range(int(n_refs[i]))]
        most = {}
        for ref in refs:
            for g, c in CPU.ngram_counts(ref).items():
                most[g] = max(most.get(g, 0), c)
        clip += any(0 < most.get(g, 0) < c for g, c in CPU.ngram_counts(CPU.caption(res[r])).items())
        d = sorted({(abs(len(ref) - int(comps[r, 0])), len(ref)) for ref in refs})
        tie += len(d) > 1 and d[0][0] == d[1][0]
    n = 2.0 * B
    return dict(match4=float((comps[:, 9] > 0).mean()), clip=clip / n, brevity=float((comps[:, 0] < comps[:, 1]).mean()),
                tie=tie / n, no_end=float((res != 0).all(axis=1).mean()))


def build_tiers(timing=None):
    tiers = {}
    for name in ('edge', 'c5', 'spi5'):
        g = np.load(os.path.join(CG.GOLDEN, 'ciderd_%s.npz' % name))
        tiers[name] = dict(_in=dict(res=g['res'], gts=g['gts'], n_refs=g['n_refs'], B=int(g['B']), seq_per_img=int(g['seq_per_img'])),
                           _cider=g['scores'])
    # seeds: of eight tried per shape (closest-length ties on 2.7-7.4 % of the rows, the other fractions alike), one whose
    # ties leave a margin to the 3 % that tests/test_bleud_cpu.py asks of these tiers
    tiers['near'] = dict(_in=tier_near(21, 128, 1), _store_inputs=True)
    tiers['near_spi5'] = dict(_in=tier_near(14, 64, 5), _store_inputs=True)
    out = {}
    for name, t in tiers.items():
        i = t['_in']
        res, gts, n_refs, B, spi = i['res'], i['gts'], i['n_refs'], int(i['B']), int(i['seq_per_img'])
        took = []
        bleu, comps, corpus = reference_bleu(res, gts, n_refs, B, spi, took)
        if timing is not None:
            timing[name] = (2 * B, took[0])
        c_bleu, c_comps, c_corpus = BCPU.score_rows(res, CPU.scst_rows(B, spi), gts, n_refs)
        assert np.array_equal(c_comps, comps), name
        assert np.allclose(c_bleu, bleu, rtol=1e-12, atol=0) and np.allclose(c_corpus, corpus, rtol=1e-12, atol=0), name
        assert (bleu > 0).all()
        o = dict(bleu=bleu, comps=comps, corpus=corpus, mix_weights=np.array(MIXES, dtype=np.float64))
        if t.get('_store_inputs'):
            cider = CG.reference_scores(res, gts, n_refs, B, spi)
            assert np.allclose(CPU.score_rows(res, CPU.scst_rows(B, spi), gts, n_refs), cider, rtol=1e-12, atol=1e-13), name
            o.update(res=res, gts=gts, n_refs=n_refs, B=np.int64(B), seq_per_img=np.int64(spi), vocab=np.int64(i['vocab']),
                     cider=cider)
        else:
            cider = t['_cider']
        for k, (w_b, w_c, base) in enumerate(MIXES):
            m = BCPU.mix(bleu, cider, B, res.shape[1], w_b, w_c, bool(base))
            o['mix_%d_64' % k], o['mix_%d_32' % k] = m, m.astype(np.float32)
        o['_coverage'] = coverage(dict(i), bleu, comps)
        out[name] = o
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--check', action='store_true', help='compare with the committed goldens instead of writing them')
    ap.add_argument('--time', action='store_true', help='print the reference scorer\'s wall time per tier; writes nothing')
    args = ap.parse_args()
    timing = {}
    tiers = build_tiers(timing)
    if args.time:
        for name, (rows, sec) in timing.items():
            print('%-10s %5d rows  reference BleuD(4).compute_score %.1f ms' % (name, rows, sec * 1e3))
        return
    bad = 0
    for name, t in tiers.items():
        cov = t.pop('_coverage')
        path = os.path.join(CG.GOLDEN, 'bleud_%s.npz' % name)
        data = CG.npz_bytes(t)
        assert len(data) < 1 << 20, (name, len(data))
        if args.check:
            same = os.path.exists(path) and open(path, 'rb').read() == data
            bad += not same
            print('%-28s %s' % (os.path.relpath(path, ROOT), 'identical' if same else 'DIFFERS'))
        else:
            with open(path, 'wb') as f:
                f.write(data)
            print('wrote %s (%d bytes, %d rows, corpus BLEU-4 %.4f; 4-gram match %.2f, clipping %.2f, brevity %.2f, ties %.2f, '
                  'no end token %.2f)' % (os.path.relpath(path, ROOT), len(data), len(t['bleu']), float(t['corpus'][3]),
                                          cov['match4'], cov['clip'], cov['brevity'], cov['tie'], cov['no_end']))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
