"""Generate the consensus-reranking golden tiers (tests/golden/consensus_*.npz) by running the reference's own CiderD.

Usage (where the reference checkout exists; RFN_REFERENCE, default /root/reference):
    python tools/make_consensus_golden.py            # (re)write the goldens
    python tools/make_consensus_golden.py --check    # regenerate in memory, compare with the committed files byte for byte

The reference has no consensus reranking; what it pins is the pairwise utility the reranking is built from (include/rfn.h,
"consensus reranking"):
  table   16 images x n = 5 candidates x T = 16 from make_ciderd_golden's caption generator, scored against the synthetic
          'coco-train-synth' df pickle.  ONE compute_score call whose 400 "images" are the (image, i, j) pairs, each with the
          single reference c_j: in table mode the pairs are independent, so the call returns U itself.
  edge    hand-made, T = 8, n_cand = 1, 2, 3 and 7 within n = 7 (an END-only candidate, a full-length one without a 0, two
          identical ones, repeated n-grams, a pair sharing only END, ids after the END that must not be read), against a small
          hand-made df in table mode, the same way.
  corpus  8 images x n = 3: CiderD(df='corpus') with refs[r] = all candidates of r's image.  That is the include-self mean of
          U's rows under the corpus df (a document is an image, weighted by its candidate count), so it pins that definition;
          the pairs of this tier are pinned by the restatement (tests/consensus_cpu.py), which is asserted here against every
          reference number, and the consensus scores and picks stored beside them are the restatement's.
Only the df entries the candidates can look up are stored (the others never matter).  Fixed zip timestamps: a rerun reproduces
the files byte for byte.
"""
import argparse
import os
import pickle
import sys
import tempfile
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import ciderd_cpu as CPU  # noqa: E402
import consensus_cpu as CC  # noqa: E402
import make_ciderd_golden as MG  # noqa: E402

RTOL, ATOL = 1e-12, 1e-13


def reference_compute(hyps, refs, df_mode, df=None):
    """One compute_score call of the reference's CiderD; df: a dict pickled to data/<df_mode>.p in a temporary directory."""
    sys.path.insert(0, os.path.join(MG.REF, 'cider'))
    from pyciderevalcap.ciderD.ciderD import CiderD
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as d:
        try:
            if df is not None:
                os.makedirs(os.path.join(d, 'data'))
                with open(os.path.join(d, 'data', df_mode + '.p'), 'wb') as f:
                    pickle.dump(df, f)
                os.chdir(d)
            _, scores = CiderD(df=df_mode).compute_score(refs, hyps)
        finally:
            os.chdir(cwd)
    return np.asarray(scores, dtype=np.float64)


def reference_pairs(cands, n_cand, df):
    """U from the reference: every (image, i, j) pair is one 'image' with the single reference c_j (table mode)."""
    B, n, _ = cands.shape
    pairs = [(k, i, j) for k in range(B) for i in range(int(n_cand[k])) for j in range(int(n_cand[k]))]
    hyps = [{'image_id': x, 'caption': [MG.ids_to_str(cands[k, i])]} for x, (k, i, _) in enumerate(pairs)]
    refs = {x: [MG.ids_to_str(cands[k, j])] for x, (k, _, j) in enumerate(pairs)}
    s = reference_compute(hyps, refs, 'coco-train-synth', df)
    U = np.full((B, n, n), np.nan)
    for x, (k, i, j) in enumerate(pairs):
        U[k, i, j] = s[x]
    return U


def df_arrays(df, cands, n_cand):
    """The df entries some valid candidate holds, as (ids (m, 4) int32 padded with -1, counts (m,))."""
    held = set()
    for k in range(cands.shape[0]):
        for j in range(int(n_cand[k])):
            held.update(CPU.ngram_counts(CPU.caption(cands[k, j])))
    keys = sorted(g for g in held if tuple(str(x) for x in g) in df)
    ids = np.full((len(keys), 4), -1, dtype=np.int32)
    for r, g in enumerate(keys):
        ids[r, :len(g)] = g
    return ids, np.array([df[tuple(str(x) for x in g)] for g in keys], dtype=np.float64)


def random_cands(seed, n_img, n, T, vocab, common):
    rng = np.random.default_rng(seed)
    pools = [np.concatenate([rng.choice(common, 12), rng.integers(1, vocab + 1, 6)]) for _ in range(n_img)]
    return np.stack([MG.captions(rng, n, T, pools[k]) for k in range(n_img)])


def edge_cands():
    T, z = 8, [0] * 8
    imgs = [
        [[4, 5, 6, 0] + z[:4]],                                                    # n_cand = 1: the empty sum
        [[3, 4, 5, 0, 9, 9, 9, 9], [3, 4, 5, 0, 1, 2, 3, 4]],                      # identical captions, ids after END differ
        [[0] + [5] * 7, [7, 8, 9, 10, 11, 12, 13, 14], [21, 22, 0] + z[:5]],       # END only; full length, no 0; shares only END
        [[2, 2, 2, 2, 2, 2, 0, 3], [2, 2, 0] + z[:5], [6, 2, 2, 0] + z[:4], [2, 2, 2, 2, 2, 2, 2, 2], [9, 8, 7, 9, 8, 7, 0, 1],
         [9, 8, 7, 0] + z[:4], [9, 8, 7, 9, 8, 7, 0, 0]],                           # repeated n-grams; two identical again
    ]
    n_cand = np.array([len(c) for c in imgs], dtype=np.int32)
    cands = np.zeros((len(imgs), 7, T), dtype=np.int64)
    cands[:, :, 1:] = 17                         # the candidates behind n_cand: never read
    cands[:, :, 0] = 16
    for k, c in enumerate(imgs):
        cands[k, :len(c)] = np.array(c)
    df = defaultdict(float)
    for g, v in {('0',): 400.0, ('2',): 50.0, ('9',): 3.0, ('8',): 3.0, ('2', '2'): 7.0, ('9', '8'): 2.0, ('2', '2', '2'): 5.0,
                 ('9', '8', '7'): 2.0, ('2', '2', '2', '2'): 4.0, ('5', '0'): 1.0, ('7', '0'): 9.0, ('3', '4'): 200000.0}.items():
        df[g] = v                                # ('3', '4') lies above the document count: a negative weight
    return cands, n_cand, df


def build_tiers():
    tiers = {}
    df, common, _ = MG.synth_table(7, 9487)
    cands = random_cands(13, 16, 5, 16, 9487, common)   # seed 13: every image's runner-up lies > 1e-3 (relative) below its best
    n_cand = np.full(16, 5, dtype=np.int32)
    tiers['table'] = dict(cands=cands, n_cand=n_cand, U=reference_pairs(cands, n_cand, df), _df=df)
    cands, n_cand, df = edge_cands()
    tiers['edge'] = dict(cands=cands, n_cand=n_cand, U=reference_pairs(cands, n_cand, df), _df=df)
    for name, t in tiers.items():
        t['df_ids'], t['df_counts'] = df_arrays(t.pop('_df'), t['cands'], t['n_cand'])
        t['ref_docs'] = np.float64(113287)
        best, c, U = CC.consensus(t['cands'], t['n_cand'], None, CPU.df_from_arrays(t['df_ids'], t['df_counts']), 113287)
        assert np.allclose(U, t['U'], rtol=RTOL, atol=ATOL, equal_nan=True), (name, np.nanmax(np.abs(U - t['U'])))
        t['c'], t['best'] = c, best
    # seed 13: no image whose best two candidates tie (with n = 3, an image one of whose candidates shares nothing with the other
    # two has c_1 = U[1][2] / 2 and c_2 = U[2][1] / 2, mathematically equal; tests/test_consensus_cpu.py asserts there is none)
    cands = random_cands(13, 8, 3, 16, 9487, np.random.default_rng(13).integers(1, 9488, 40))
    n_cand = np.full(8, 3, dtype=np.int32)
    res, row_img = CC.compact(cands, n_cand)
    hyps = [{'image_id': r, 'caption': [MG.ids_to_str(res[r])]} for r in range(len(res))]
    refs = {r: [MG.ids_to_str(cands[row_img[r], j]) for j in range(3)] for r in range(len(res))}
    means = reference_compute(hyps, refs, 'corpus').reshape(8, 3)
    best, c, U = CC.consensus(cands, n_cand)
    assert np.allclose(U.mean(2), means, rtol=RTOL, atol=ATOL), np.abs(U.mean(2) - means).max()
    tiers['corpus'] = dict(cands=cands, n_cand=n_cand, row_means=means, U=U, c=c, best=best)
    return tiers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--check', action='store_true', help='compare with the committed goldens instead of writing them')
    args = ap.parse_args()
    if not os.path.isdir(MG.REF):
        sys.exit('the reference checkout (%s) does not exist: the goldens are generated by its own CiderD' % MG.REF)
    bad = 0
    for name, t in build_tiers().items():
        path = os.path.join(GOLDEN, 'consensus_%s.npz' % name)
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
