"""Time the on-device CIDEr-D reward (recurrent_fusion_network_amd/rewards.py) and print one JSON line.

  - ms per scst_reward call (B sampled + B greedy rows, T = 16, 5 refs per image, random ids of the C5 vocabulary) at
    B = 128 (1 row per image), 640 and 1280 (5 rows per image), in corpus mode and in table mode (a synthetic df table);
  - the C5 self-critical step (bench.py's RL leg: multinomial sample, greedy baseline, reward criterion, backward, clamp +
    Adam at B = 128) with the real reward against the same step with a randn reward, and the difference.
  - --bleu: instead, the BLEU-D legs (profiles/bleud_reward.json): at the C5 shape (128 + 128 rows, 5 refs) and at the shape
    of the spi5 golden tier (640 + 640 rows, 128 images, 5-7 refs) the CIDEr-only call (corpus mode, the call timed above), the
    BLEU-only call and the mixed call, alternated in blocks of --block calls over --rounds rounds; min / median / max per leg.
  - --rouge: instead, the ROUGE-L call alone (rewards.RougeL.score_ids, validation captions) at the C5 shape, at the spi5 shape
    and at 5000 rows x 5 refs, in blocks as --bleu.
  - --eval: instead, one whole-split evalcap.LanguageEval.compute() (Bleu, ROUGE_L, CIDEr; 5000 images x 5 references, T = 16, the
    split tools/make_evalcap_golden.py --time scores with the reference's scorers) including its one host read, per call and per
    metric.
  - --diversity: instead, one full rewards.diversity call (Div-m, mBLEU, Self-CIDEr; every output) next to one
    rewards.consensus(want_pairs=True) call on the same candidates (B = 128 images x n = 5 x T = 16, corpus df), alternating call
    by call, each between two device events; the launches of either call as its entry point lists them (include/rfn.h); and the
    worst eigenvalue error of the call against numpy.linalg.eigvalsh in units of n * 2^-52 * ||K||_F
    (profiles/diversity_metrics.json; --json PATH also writes the line there).  Both calls are chains of small dependent
    launches: the figures are launch gaps, and nothing gates them.
Usage: python tools/bench_reward.py [--steps 50] [--warmup 5] | --bleu [--block 2000] [--rounds 7] | --rouge | --eval |
       --diversity [--json PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scoring_case(B, spi, dev, seed, T=16, refs=5, vocab=9487):
    rng = np.random.default_rng(seed)
    n_img = B // spi
    gts = torch.from_numpy(rng.integers(1, vocab + 1, (n_img, refs, T))).to(dev)
    gts[:, :, -1] = 0
    n_refs = torch.full((n_img,), refs, dtype=torch.int32, device=dev)
    gen = torch.from_numpy(rng.integers(1, vocab + 1, (B, T))).to(dev)
    greedy = torch.from_numpy(rng.integers(1, vocab + 1, (B, T))).to(dev)
    return gen, greedy, gts, n_refs


def synthetic_table(seed, vocab=9487, n=200000):
    rng = np.random.default_rng(seed)
    df = {}
    for k in range(n):
        L = 1 + k % 4
        df[tuple(str(x) for x in rng.integers(1, vocab + 1, L))] = float(rng.integers(1, 500))
    return df


def time_calls(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def bleu_legs(args):
    from recurrent_fusion_network_amd import rewards as RW
    dev = torch.device('cuda:0')
    out = {'metric': 'self-critical reward, ms per scst_reward call (sample + greedy rows, T = 16): CIDEr-D only (corpus df), '
                     'BLEU-D only, mixed', 'unit': 'ms', 'calls_per_block': args.block, 'rounds': args.rounds,
           'device': torch.cuda.get_device_name(0)}
    cider, bleu = RW.CiderD(), RW.BleuD()
    for tag, B, spi, refs in (('c5_128x2', 128, 1, 5), ('spi5_640x2', 640, 5, 7)):
        gen, greedy, gts, n_refs = scoring_case(B, spi, dev, B, refs=refs)
        if refs > 5:
            n_refs = torch.from_numpy(np.random.default_rng(B).integers(5, refs + 1, B // spi).astype(np.int32)).to(dev)
        legs = {'cider': lambda: RW.scst_reward(cider, gen, greedy, gts, n_refs, spi),
                'bleu': lambda: RW.scst_reward(None, gen, greedy, gts, n_refs, spi, 0.0, bleu_scorer=bleu, bleu4_weight=1.0),
                'mixed': lambda: RW.scst_reward(cider, gen, greedy, gts, n_refs, spi, 1.0, bleu_scorer=bleu, bleu4_weight=0.5)}
        times = {k: [] for k in legs}
        for k, fn in legs.items():
            time_calls(fn, args.block // 4, 20)           # warm every leg at this shape
        for _ in range(args.rounds):
            for k, fn in legs.items():
                times[k].append(time_calls(fn, args.block, 0))
        for k, v in times.items():
            v = sorted(v)
            out['%s_%s' % (tag, k)] = {'min': round(v[0], 4), 'median': round(v[len(v) // 2], 4), 'max': round(v[-1], 4)}
        out['%s_mixed_over_cider' % tag] = round(out[tag + '_mixed']['median'] / out[tag + '_cider']['median'], 3)
    print(json.dumps(out), flush=True)


def spread(v):
    v = sorted(v)
    return {'min': round(v[0], 4), 'median': round(v[len(v) // 2], 4), 'max': round(v[-1], 4)}


def rouge_legs(args):
    from recurrent_fusion_network_amd import rewards as RW
    dev = torch.device('cuda:0')
    out = {'metric': 'ROUGE-L, ms per RougeL.score_ids call (validation captions, T = 16)', 'unit': 'ms',
           'calls_per_block': args.block, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0)}
    sc = RW.RougeL()
    for tag, rows, spi, refs in (('c5_256', 256, 1, 5), ('spi5_1280', 1280, 5, 7), ('val_5000', 5000, 1, 5)):
        gen, _, gts, n_refs = scoring_case(rows, spi, dev, rows, refs=refs)
        row_img = torch.arange(rows, dtype=torch.int32, device=dev) // spi
        scores = torch.empty(rows, dtype=torch.float64, device=dev)

        def call():
            sc.score_ids(gen, row_img, gts, n_refs, out=scores, end_token=False)
        time_calls(call, args.block // 4, 20)
        out[tag] = spread([time_calls(call, args.block, 0) for _ in range(args.rounds)])
    print(json.dumps(out), flush=True)


def eval_legs(args):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import evalcap_cases as CASES
    from recurrent_fusion_network_amd.evalcap import LanguageEval
    dev = torch.device('cuda:0')
    seq, gts, n_refs, vocab = CASES.val_split(77, 5000, 5, 5)
    batches = [(torch.from_numpy(seq[lo:lo + 500]).to(dev), torch.from_numpy(gts[lo:lo + 500]).to(dev),
                torch.from_numpy(n_refs[lo:lo + 500]).to(dev)) for lo in range(0, 5000, 500)]
    out = {'metric': 'validation metrics, ms per whole-split LanguageEval.compute() (5000 images x 5 references, T = 16, fed as ten '
                     'device batches; concatenation, the scorers, the corpus reductions and the one host read)', 'unit': 'ms',
           'calls_per_block': args.steps, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0)}
    for tag, metrics in (('all', ('Bleu', 'ROUGE_L', 'CIDEr')), ('bleu', ('Bleu',)), ('rouge', ('ROUGE_L',)), ('cider', ('CIDEr',))):
        le = LanguageEval(vocab, metrics)
        for b in batches:
            le.add(*b)

        def call():
            le._result = None
            return le.compute()
        time_calls(call, args.warmup, 2)
        out[tag] = spread([time_calls(call, args.steps, 0) for _ in range(args.rounds)])
        if tag == 'all':
            out['scores'] = {k: round(v, 6) for k, v in call().items()}
    print(json.dumps(out), flush=True)


def diversity_legs(args):
    from recurrent_fusion_network_amd import rewards as RW
    dev = torch.device('cuda:0')
    B, n, T = 128, 5, 16
    rng = np.random.default_rng(5)
    pool = rng.integers(1, 9488, (B, 24))                      # an image's candidates draw from one small pool, so they overlap
    cands = np.take_along_axis(pool[:, None, :].repeat(n, 1), rng.integers(0, 24, (B, n, T)), 2)
    cands[:, :, -1] = 0
    for k, j in zip(*np.nonzero(rng.random((B, n)) < 0.7)):
        cands[k, j, rng.integers(5, T)] = 0
    cands_d = torch.from_numpy(cands).to(dev)
    sc = RW.CiderD()
    legs = {'diversity': lambda: RW.diversity(sc, cands_d), 'consensus_pairs': lambda: RW.consensus(sc, cands_d, want_pairs=True)}
    for fn in legs.values():
        for _ in range(args.warmup + 5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.steps):                                # alternating, call by call
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    d = {k: v.cpu().numpy() for k, v in legs['diversity']().items()}
    worst = 0.0
    for k in range(B):
        K = (d['U'][k] + d['U'][k].T) / 2 / 10
        unit = n * 2.0 ** -52 * np.linalg.norm(K)
        worst = max(worst, float(np.abs(d['eig'][k] - np.linalg.eigvalsh(K)).max() / unit))
    out = {'metric': 'caption-set diversity, ms per rewards.diversity call (every output) next to rewards.consensus(want_pairs=True) '
                     'on the same candidates: B = 128 images x n = 5 x T = 16, corpus df; device events around one call, '
                     'alternating', 'unit': 'ms', 'calls': args.steps, 'device': torch.cuda.get_device_name(0),
           'diversity': spread(times['diversity']), 'consensus_pairs': spread(times['consensus_pairs']),
           # include/rfn.h: counts, clear, cook, vectors, Div, mBLEU rows, mBLEU corpus, pairs, eigen / ..., pairs, pick
           'launches': {'diversity': 9, 'consensus_pairs': 6, 'how': 'the entry points\' launch lists (include/rfn.h), corpus df'},
           'eig_worst_over_n_eps_normK': round(worst, 3),
           'scores': {'Div_1': round(float(d['div'][:, 0].mean()), 6), 'mBleu_4': round(float(d['mbleu_corpus'][:, 3].mean()), 6),
                      'Self_CIDEr': round(float(d['self_cider'].mean()), 6)}}
    line = json.dumps(out)
    if args.json:
        with open(args.json, 'w') as f:
            f.write(line + '\n')
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--bleu', action='store_true', help='time the BLEU-D and mixed reward calls next to the CIDEr-D call')
    ap.add_argument('--block', type=int, default=2000)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--rouge', action='store_true', help='time the ROUGE-L call')
    ap.add_argument('--eval', action='store_true', help='time a whole-split LanguageEval.compute() at 5000 x 5')
    ap.add_argument('--diversity', action='store_true', help='time rewards.diversity next to rewards.consensus(want_pairs=True)')
    ap.add_argument('--json', default=None, help='--diversity: also write the result line to this file')
    args = ap.parse_args()
    if args.diversity:
        return diversity_legs(args)
    if args.bleu:
        return bleu_legs(args)
    if args.rouge:
        return rouge_legs(args)
    if args.eval:
        return eval_legs(args)
    import bench
    import recurrent_fusion_network_amd as R
    from recurrent_fusion_network_amd import rewards as RW
    dev = torch.device('cuda:0')
    out = {'metric': 'CIDEr-D self-critical reward, ms per call (sample + greedy rows, T = 16, 5 refs)', 'unit': 'ms',
           'steps': args.steps, 'warmup': args.warmup, 'device': torch.cuda.get_device_name(0)}
    corpus, table = RW.CiderD(), RW.CiderD(df=synthetic_table(1), df_mode='coco-train')
    for B, spi in ((128, 1), (640, 5), (1280, 5)):
        gen, greedy, gts, n_refs = scoring_case(B, spi, dev, B)
        for name, sc in (('corpus', corpus), ('table', table)):
            out['%s_%dx2' % (name, B)] = round(time_calls(lambda: RW.scst_reward(sc, gen, greedy, gts, n_refs, spi),
                                                          args.steps, args.warmup), 4)
    # the C5 self-critical step, bench.py's RL leg, with the real reward and with randn
    w = dict(bench.WORKLOADS['c5'])
    B = w['B']
    cfg = bench.make_cfg(w)
    model = R.RecurrentFusionModel(cfg).to(dev)
    bench.seeded_weights_(model, 100)
    fc, att, labels, masks, top = bench.synthetic_inputs(cfg, B, 100, dev)
    rl_crit = R.ReviewNetRewardCriterion(cfg)
    opt = R.FusedClampAdam(model, lr=5e-5, weight_decay=0.0, grad_clip=1.0)
    _, _, gts, n_refs = scoring_case(B, 1, dev, 7, T=cfg.seq_length)
    steps = max(5, args.steps // 5)

    def rl_step(real):
        model.train()
        opt.zero_grad()
        seq, lp, lp_all, reason = model.sample(fc, att, {'sample_max': 0})
        with torch.no_grad():
            model.eval()
            greedy = model.sample(fc, att, {'sample_max': 1})[0]
            model.train()
        if real:
            reward = RW.scst_reward(corpus, seq, greedy, gts, n_refs, 1)
        else:
            reward = torch.randn(B, 1, device=dev).expand(B, seq.size(1)).contiguous()
        rl_crit(lp, seq, reward, lp_all, 0.01, reason, top, 1.0, None, cfg).backward()
        opt.step()
    t_randn = time_calls(lambda: rl_step(False), steps, 2)
    t_real = time_calls(lambda: rl_step(True), steps, 2)
    t_randn2 = time_calls(lambda: rl_step(False), steps, 2)
    t_randn = min(t_randn, t_randn2)
    out.update({'c5_rl_step_randn_ms': round(t_randn, 3), 'c5_rl_step_ciderd_ms': round(t_real, 3),
                'c5_rl_step_added_ms': round(t_real - t_randn, 3), 'c5_rl_steps': steps})
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
