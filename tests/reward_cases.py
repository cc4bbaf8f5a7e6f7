"""Inputs that tests/test_ciderd_gpu.py and tests/test_bleud_gpu.py share: fuzzed scoring cases, a golden tier on the device,
compute_score's string dicts and the small model and data['gts'] of the get_rewards drop-in tests."""
import types

import numpy as np
import torch

import ciderd_cpu as CPU


def fuzz_case(seed_base, seed):
    """One random scoring case: sizes T, Tg, vocab, n_img, spi, max_refs, B; arrays n_refs (n_img,), gts (n_img, max_refs, Tg),
    res (2B, T), row_img (2B,).  Ids come from small per-image pools, so repeats and matches occur."""
    rng = np.random.default_rng(seed_base + seed)
    T, Tg = int(rng.integers(1, 65)), int(rng.integers(1, 65))
    vocab = int(rng.choice([5, 50, 9487, 32767]))
    n_img = int(rng.integers(1, 9))
    spi = int(rng.integers(1, 5))
    max_refs = int(rng.integers(1, 33))
    n_refs = rng.integers(1, max_refs + 1, n_img).astype(np.int32)
    n_refs[0] = max_refs
    pools = [rng.integers(0, vocab + 1, int(rng.integers(2, 12))) for _ in range(n_img)]

    def rows(n, width, pool):
        out = rng.choice(pool, (n, width)).astype(np.int64)
        cut = rng.random(n) < 0.6       # the others keep whatever ids the pool gives (with or without a 0)
        out[cut, rng.integers(0, width, int(cut.sum()))] = 0
        return out
    gts = np.zeros((n_img, max_refs, Tg), dtype=np.int64)
    for i in range(n_img):
        gts[i, :n_refs[i]] = rows(int(n_refs[i]), Tg, pools[i])
    B = n_img * spi
    res = np.concatenate([rows(1, T, pools[(r % B) // spi]) for r in range(2 * B)])
    return types.SimpleNamespace(T=T, Tg=Tg, vocab=vocab, n_img=n_img, spi=spi, max_refs=max_refs, B=B, n_refs=n_refs, gts=gts,
                                 res=res, row_img=CPU.scst_rows(B, spi))


def device_inputs(g, dev):
    """A golden tier -> B, seq_per_img and its res, row_img, gts, n_refs on the device."""
    B, spi = int(g['B']), int(g['seq_per_img'])
    return (B, spi, torch.from_numpy(g['res']).to(dev), torch.from_numpy(CPU.scst_rows(B, spi)).to(dev),
            torch.from_numpy(g['gts']).to(dev), torch.from_numpy(g['n_refs']).to(dev))


def string_dicts(g):
    """A golden tier as compute_reward hands it to compute_score (one image_id per score row) -> its gts dict, its res list."""
    B, spi = int(g['B']), int(g['seq_per_img'])

    def s(row):
        return ' '.join(str(int(x)) for x in CPU.caption(row))
    res = [{'image_id': r, 'caption': [s(g['res'][r])]} for r in range(2 * B)]
    gts = {r: [s(g['gts'][(r % B) // spi][j]) for j in range(int(g['n_refs'][(r % B) // spi]))] for r in range(2 * B)}
    return gts, res


def small_model(dev):
    import recurrent_fusion_network_amd as R
    from oracle import rfn_oracle as O
    info = [dict(att_num=49, att_feat_size=96, fc_feat_size=64), dict(att_num=20, att_feat_size=72, fc_feat_size=72)]
    cfg = O.make_cfg(info, vocab_size=200, rnn_size=64, input_encoding_size=64, att_hid_size=64, num_review_steps_0=4,
                     num_review_steps=4, top_words_count=40, seq_length=8)
    model = R.RecurrentFusionModel(cfg)
    model.load_state_dict(O.seeded_params(cfg, 123))
    fc, att, labels, masks, top = O.synthetic_batch(cfg, 8, seed=7)
    d = lambda ts: [t.to(dev) for t in ts]  # noqa: E731
    return R, cfg, model.to(dev), d(fc), d(att), top.to(dev)


def drop_in_data(cfg):
    """-> data (its 'gts': variable caption counts per image, as dataloader.py collects them), B, spi for small_model's batch."""
    rng = np.random.default_rng(3)
    data = {'gts': [rng.integers(1, 40, (int(k), cfg.seq_length + 2)) for k in (5, 3, 7, 1)]}
    for a in data['gts']:
        a[:, -2:] = 0
    return data, 8, 2
