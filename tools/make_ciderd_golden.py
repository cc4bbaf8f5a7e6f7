"""Generate the CIDEr-D golden tiers (tests/golden/ciderd_*.npz) by running the reference's own scorer.

Usage (where the reference checkout exists; RFN_REFERENCE, default /root/reference):
    python tools/make_ciderd_golden.py            # (re)write the goldens
    python tools/make_ciderd_golden.py --check    # regenerate in memory, compare with the committed files byte for byte

Builds `res` and `gts` exactly as get_rewards.compute_reward does (2B rows: the sampled rows then the greedy rows, each
pointing at image (r % B) // seq_per_img; ids up to and including the first 0 joined by spaces) and calls the reference's
CiderD(n=4, sigma=6.0).compute_score on them.  Stores inputs, n_refs, scores and the self-critical rewards (f64 and f32).
The `table` tier pickles a synthetic df (a defaultdict(float) of id-string tuples, as scripts/prepro_ngrams.py does) to a
temporary data/coco-train-synth.p, so that the reference's non-corpus branch loads it with ref_len = log(113287).
Also asserts that tests/ciderd_cpu.py agrees with the reference on every tier.  Files are written with fixed zip
timestamps, so a rerun reproduces them byte for byte.
"""
import argparse
import io
import os
import pickle
import sys
import tempfile
import zipfile
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('RFN_REFERENCE', '/root/reference')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import ciderd_cpu as CPU  # noqa: E402


def ids_to_str(row):
    words = []
    for x in row:
        words.append(str(int(x)))
        if int(x) == 0:
            break
    return ' '.join(words)


def reference_scores(res, gts, n_refs, B, spi, df_mode='corpus', workdir=None):
    sys.path.insert(0, os.path.join(REF, 'cider'))
    from pyciderevalcap.ciderD.ciderD import CiderD
    cwd = os.getcwd()
    try:
        if workdir:
            os.chdir(workdir)
        scorer = CiderD(df=df_mode)
        hyps = [{'image_id': r, 'caption': [ids_to_str(res[r])]} for r in range(2 * B)]
        refs = {r: [ids_to_str(gts[(r % B) // spi][j]) for j in range(int(n_refs[(r % B) // spi]))] for r in range(2 * B)}
        _, scores = scorer.compute_score(refs, hyps)
    finally:
        os.chdir(cwd)
    return np.asarray(scores, dtype=np.float64)


def captions(rng, n, T, pool, p_end=0.8):
    """n id rows of width T drawn from `pool`; most end in 0 after 1..T-1 words, the rest fill all T ids."""
    out = np.zeros((n, T), dtype=np.int64)
    for k in range(n):
        if rng.random() < p_end and T > 1:
            L = int(rng.integers(1, T))
            out[k, :L] = rng.choice(pool, L)
            out[k, L] = 0
            out[k, L + 1:] = rng.integers(1, pool.max() + 1, T - L - 1)   # ids after the end token are not read
        else:
            out[k] = rng.choice(pool, T)
    return out


def image_set(rng, n_img, refs_lo, refs_hi, T, vocab, common):
    pools = [np.concatenate([rng.choice(common, 12), rng.integers(1, vocab + 1, 6)]) for _ in range(n_img)]
    n_refs = rng.integers(refs_lo, refs_hi + 1, n_img).astype(np.int32)
    gts = np.zeros((n_img, int(n_refs.max()), T), dtype=np.int64)
    for i in range(n_img):
        gts[i, :n_refs[i]] = captions(rng, int(n_refs[i]), T, pools[i])
    return gts, n_refs, pools


def sampled_rows(rng, B, spi, T, pools):
    rows = np.zeros((2 * B, T), dtype=np.int64)
    for r in range(2 * B):
        rows[r] = captions(rng, 1, T, pools[(r % B) // spi])[0]
    return rows


def tier_random(seed, n_img, spi, refs_lo, refs_hi, T, vocab):
    rng = np.random.default_rng(seed)
    common = rng.integers(1, vocab + 1, 40)
    gts, n_refs, pools = image_set(rng, n_img, refs_lo, refs_hi, T, vocab, common)
    res = sampled_rows(rng, n_img * spi, spi, T, pools)
    return dict(res=res, gts=gts, n_refs=n_refs, B=n_img * spi, seq_per_img=spi, vocab=vocab)


def tier_edge():
    T = 8
    z = [0] * T
    gts = np.zeros((6, 7, T), dtype=np.int64)
    n_refs = np.array([1, 7, 3, 2, 5, 4], dtype=np.int32)
    refs = [
        [[4, 5, 6, 0] + z[:4]],
        [[4, 5, 6, 7, 8, 9, 10, 11], [4, 5, 0, 9, 9, 9, 9, 9], [3, 3, 3, 3, 0, 0, 0, 0], [0] * T, [7, 0, 7, 7, 7, 7, 7, 7],
         [1, 2, 3, 4, 5, 6, 7, 0], [5, 6, 7, 8, 9, 10, 11, 12]],
        [[2, 2, 2, 2, 2, 2, 2, 2], [2, 2, 0] + z[:5], [6, 2, 2, 0] + z[:4]],
        [[0] * T, [1, 0] + z[:6]],
        [[13, 14, 15, 16, 0] + z[:3], [13, 14, 15, 16, 17, 18, 19, 20], [14, 15, 0] + z[:5], [16, 13, 0] + z[:5],
         [20, 19, 18, 17, 16, 15, 14, 13]],
        [[9, 8, 7, 0] + z[:4], [9, 8, 7, 9, 8, 7, 0, 0], [9, 0] + z[:6], [8, 7, 9, 8, 7, 9, 8, 7]],
    ]
    for i, rs in enumerate(refs):
        gts[i, :len(rs)] = np.array(rs)
    sample = [[0] + [5] * (T - 1),               # only the end token (ids after it are ignored)
              [4, 5, 6, 7, 8, 9, 10, 11],         # full length, no 0, equal to a ref
              [2, 2, 2, 2, 2, 2, 0, 3],           # repeated n-grams
              [1, 0] + z[:6],                     # equal to a ref
              [13, 14, 15, 16, 17, 18, 19, 20],   # full length, equal to a ref
              [9, 8, 7, 9, 8, 7, 0, 1]]
    greedy = [[4, 5, 6, 0] + z[:4],               # equal to the only ref
              [3, 3, 3, 3, 3, 3, 3, 3],
              [2, 2, 0] + z[:5],
              [0] * T,
              [21, 22, 23, 0] + z[:4],            # no common n-gram but the end token
              [8, 7, 0] + z[:5]]
    res = np.array(sample + greedy, dtype=np.int64)
    return dict(res=res, gts=gts, n_refs=n_refs, B=6, seq_per_img=1, vocab=23)


def synth_table(seed, vocab, n_train=500):
    """df of a synthetic 500-image 'train' set: per image, the distinct n-grams of all of its references."""
    rng = np.random.default_rng(seed)
    common = rng.integers(1, vocab + 1, 40)
    gts, n_refs, _ = image_set(rng, n_train, 5, 5, 16, vocab, common)
    df = defaultdict(float)
    for i in range(n_train):
        seen = set()
        for j in range(int(n_refs[i])):
            seen.update(CPU.ngram_counts(CPU.caption(gts[i, j])))
        for g in seen:
            df[tuple(str(x) for x in g)] += 1.0
    # the scored images come from the same word distribution
    t = tier_random(seed + 1, 64, 1, 5, 5, 16, vocab)
    return df, common, t


def build_tiers():
    tiers = {}
    tiers['edge'] = tier_edge()
    tiers['c5'] = tier_random(5, 128, 1, 5, 5, 16, 9487)
    tiers['spi5'] = tier_random(6, 128, 5, 5, 7, 16, 9487)
    df, _, t = synth_table(7, 9487)
    keys = sorted(df)
    ids = np.full((len(keys), 4), -1, dtype=np.int32)
    for k, g in enumerate(keys):
        ids[k, :len(g)] = [int(x) for x in g]
    t['df_ids'], t['df_counts'], t['ref_docs'] = ids, np.array([df[g] for g in keys]), np.float64(113287)
    t['_df'] = df
    tiers['table'] = t
    for name, t in tiers.items():
        B, spi = t['B'], t['seq_per_img']
        if name == 'table':
            with tempfile.TemporaryDirectory() as d:
                os.makedirs(os.path.join(d, 'data'))
                with open(os.path.join(d, 'data', 'coco-train-synth.p'), 'wb') as f:
                    pickle.dump(t.pop('_df'), f)
                s = reference_scores(t['res'], t['gts'], t['n_refs'], B, spi, 'coco-train-synth', d)
            cpu = CPU.score_rows(t['res'], CPU.scst_rows(B, spi), t['gts'], t['n_refs'],
                                 CPU.df_from_arrays(t['df_ids'], t['df_counts']), 113287)
        else:
            s = reference_scores(t['res'], t['gts'], t['n_refs'], B, spi)
            cpu = CPU.score_rows(t['res'], CPU.scst_rows(B, spi), t['gts'], t['n_refs'])
        assert np.allclose(cpu, s, rtol=1e-12, atol=1e-13), (name, np.abs(cpu - s).max())
        T = t['res'].shape[1]
        t['scores'] = s
        t['reward64'] = CPU.reward(s, B, T, 1.0, True)
        t['reward32'] = t['reward64'].astype(np.float32)
        t['reward64_nobase'] = CPU.reward(s, B, T, 0.5, False)
        t['reward32_nobase'] = t['reward64_nobase'].astype(np.float32)
        t['B'], t['seq_per_img'], t['vocab'] = np.int64(B), np.int64(spi), np.int64(t['vocab'])
    return tiers


def npz_bytes(arrays):
    """An .npz with fixed member timestamps (np.savez stamps the current time)."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, 'w', zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            a = io.BytesIO()
            np.lib.format.write_array(a, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, a.getvalue())
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--check', action='store_true', help='compare with the committed goldens instead of writing them')
    args = ap.parse_args()
    bad = 0
    for name, t in build_tiers().items():
        path = os.path.join(GOLDEN, 'ciderd_%s.npz' % name)
        data = npz_bytes(t)
        assert len(data) < 1 << 20, (name, len(data))
        if args.check:
            same = os.path.exists(path) and open(path, 'rb').read() == data
            bad += not same
            print('%-28s %s' % (os.path.relpath(path, ROOT), 'identical' if same else 'DIFFERS'))
        else:
            with open(path, 'wb') as f:
                f.write(data)
            print('wrote %s (%d bytes, %d rows, mean score %.4f)' % (os.path.relpath(path, ROOT), len(data),
                                                                     len(t['scores']), float(np.mean(t['scores']))))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
