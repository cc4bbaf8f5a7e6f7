#!/usr/bin/env python3
"""Scoring given captions at config 5 (M=4, L=196, D=2048, 128 images, S=16, V=9487) on one MI355X -> profiles/caption_scoring.json.

For n in {1, 5, 20} captions per image, two versions that give the same per-token log-probs, in alternating windows of at least
one second that end in a device synchronise (every version warmed first):
  score   model.score(fc, att, ids, {'n': n})
  parent  what the tree offered before score(): n = 1: model(features, labels) + gather; n > 1: sample_group(..., {'force_ids': ids})
          + its seqLogprobs.  Both materialise the (rows, 17, 9488) log-probs.
Per version: the median ms per call over the windows, their spread, and torch.cuda.max_memory_allocated of one call.
And the two kernels on the same (17 * 128 * n, 9488) logits, timed with device events around back-to-back launches, alternating:
rfn_score_logits (all three outputs) and rfn_log_softmax_fwd.  The scorer's achieved bytes/s is live rows x V1 x 4 B over its time.
Two conditions, judged on the medians against the spread of the alternating windows (no thresholds):
  rfn_score_logits is not slower than rfn_log_softmax_fwd on the same rows;  model.score is not slower than the parent's route."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'profiles', 'caption_scoring.json')
IMAGES = 128


def summary(ms):
    return {'ms': round(statistics.median(ms), 4), 'min': round(min(ms), 4), 'max': round(max(ms), 4),
            'spread_ms': round(max(ms) - min(ms), 4), 'windows_ms': [round(x, 4) for x in ms]}


def alternate(fns, rounds, min_window_s, timer):
    """fns: {name: callable}.  Each is warmed and sized so that one window lasts min_window_s; then `rounds` alternating windows.
    timer(fn, calls) -> (seconds the window took, ms per call as the version is to be judged)."""
    calls = {}
    for k, fn in fns.items():
        fn()
        fn()
        calls[k], sec = 3, timer(fn, 3)[0]
        while sec < 1.05 * min_window_s:                        # untimed windows, grown until one lasts long enough
            calls[k] = int(math.ceil(calls[k] * 1.15 * min_window_s / sec))
            sec = timer(fn, calls[k])[0]
    ms, short = {k: [] for k in fns}, 0
    for _ in range(rounds):
        for k, fn in fns.items():
            sec, per = timer(fn, calls[k])
            short += sec < min_window_s
            ms[k].append(per)
    return ms, calls, short


def host_timer(fn, calls):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    return sec, sec / calls * 1e3


def event_timer(fn, calls):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, a.elapsed_time(b) / calls


def peak_of(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del out
    return {'max_memory_allocated': int(peak), 'allocated_before_the_call': int(base)}


def run(rounds, min_window_s, ns):
    import torch
    import bench as HB
    import recurrent_fusion_network_amd as R
    import recurrent_fusion_network_amd._native as N
    dev = torch.device('cuda:0')
    cfg = HB.make_cfg(dict(HB.WORKLOADS['c3']))
    model = R.RecurrentFusionModel(cfg).to(dev).eval()
    HB.seeded_weights_(model, 100)
    fc, att, _, _, _ = HB.synthetic_inputs(cfg, IMAGES, 100, dev)
    S, V1 = cfg.seq_length, cfg.vocab_size + 1
    res = {'config': 'M=4, L=196, D=2048, R=512, V+1=%d, seq=%d, %d images' % (V1, S, IMAGES), 'rounds': rounds,
           'min_window_s': min_window_s,
           'timing': 'model: wall clock between device synchronisations; kernels: device events around back-to-back launches; '
                     'versions alternate in one process, each warmed first', 'n': {}}
    for n in ns:
        rows = IMAGES * n
        gen = torch.Generator().manual_seed(1000 + n)
        ids = torch.randint(1, V1, (rows, S), generator=gen)
        for r in range(rows):                                   # ragged captions: 6 .. 16 words
            ids[r, 6 + (r * 7) % 11:] = 0
        ids = ids.to(dev)
        labels = torch.cat([ids.new_zeros(rows, 1), ids, ids.new_zeros(rows, 1)], 1).contiguous()

        def score():
            return model.score(fc, att, ids, {'n': n})['token_logprobs']

        def parent():
            with torch.no_grad():
                if n == 1:
                    lp = model(fc, att, labels)[0]
                    return lp.gather(2, labels[:, 1:1 + lp.size(1)].unsqueeze(2)).squeeze(2)
                return model.sample_group(fc, att, n, {'force_ids': ids})[1]

        entry = {'rows': rows, 'parent_route': 'model(features, labels) + gather' if n == 1 else "sample_group(.., {'force_ids': ids})"}
        got, want = score(), parent()
        w = min(got.size(1), want.size(1))
        live = torch.cat([ids.new_ones(rows, 1), ids], 1)[:, :w] > 0 if n == 1 else ids[:, :w] > 0
        entry['same_log_probs_bit_for_bit'] = bool(torch.equal(got[:, :w][live], want[:, :w][live]))
        del got, want
        ms, calls, short = alternate({'score': score, 'parent': parent}, rounds, min_window_s, host_timer)
        for k in ms:
            entry[k] = dict(summary(ms[k]), calls_per_window=calls[k], **peak_of(score if k == 'score' else parent))
        entry['windows_shorter_than_min'] = int(short)
        entry['score_minus_parent_ms'] = round(entry['score']['ms'] - entry['parent']['ms'], 4)
        entry['score_not_slower_than_parent'] = bool(entry['score']['ms'] <= entry['parent']['ms'] + entry['parent']['spread_ms'])
        torch.cuda.empty_cache()

        # the two kernels on the same logits
        T = S + 1
        logits = torch.randn(T * rows, V1, device=dev) * 3
        target = torch.cat([ids, ids.new_zeros(rows, 1)], 1).contiguous()
        tok, rank, ent = torch.empty(rows, T, device=dev), torch.empty(rows, T, dtype=torch.int32, device=dev), torch.empty(rows, T, device=dev)
        logp = torch.empty(rows, T, V1, device=dev)
        st = N.stream_ptr()

        def k_score():
            N.check(N.lib.rfn_score_logits(logits.data_ptr(), V1, rows, T, 0, V1, target.data_ptr(), target.stride(0), 1,
                                           tok.data_ptr(), rank.data_ptr(), ent.data_ptr(), T, st), 'rfn_score_logits')

        def k_lsm():
            N.check(N.lib.rfn_log_softmax_fwd(logits.data_ptr(), V1, T * rows, V1, rows, T * V1, V1, logp.data_ptr(), st),
                    'rfn_log_softmax_fwd')

        kms, kcalls, kshort = alternate({'rfn_score_logits': k_score, 'rfn_log_softmax_fwd': k_lsm}, rounds, min_window_s, event_timer)
        live_rows = int((target > 0).sum() + rows)              # the words and each caption's END
        kern = {k: dict(summary(kms[k]), calls_per_window=kcalls[k]) for k in kms}
        kern['logits'] = [T * rows, V1]
        kern['live_rows'] = live_rows
        kern['rfn_score_logits']['achieved_GB_per_s'] = round(live_rows * V1 * 4 / (kern['rfn_score_logits']['ms'] * 1e-3) / 1e9, 1)
        kern['rfn_log_softmax_fwd']['achieved_GB_per_s_read_plus_write'] = round(
            2 * T * rows * V1 * 4 / (kern['rfn_log_softmax_fwd']['ms'] * 1e-3) / 1e9, 1)
        kern['windows_shorter_than_min'] = int(kshort)
        kern['score_not_slower_than_log_softmax'] = bool(
            kern['rfn_score_logits']['ms'] <= kern['rfn_log_softmax_fwd']['ms'] + kern['rfn_log_softmax_fwd']['spread_ms'])
        entry['kernels'] = kern
        res['n'][str(n)] = entry
        print(json.dumps({str(n): entry}), flush=True)
        del logits, logp
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=OUT)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--min-window-s', type=float, default=1.0)
    ap.add_argument('--n', type=int, nargs='+', default=[1, 5, 20])
    args = ap.parse_args()
    res = run(args.rounds, args.min_window_s, args.n)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
