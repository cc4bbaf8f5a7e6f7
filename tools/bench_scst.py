#!/usr/bin/env python3
"""Multi-sample self-critical training at config 5 (M=4, L=196, D=2048, B = 128 images) on one MI355X -> profiles/scst_group.json.

Three legs, in alternating windows of `--calls` steps with device-synchronised timing (as tools/bench_decode.py --diverse):
  a  today's RL step (train_rl.py:160-203): sample() under grad on 128 rows, the greedy pass, the CIDEr-D reward with the
     greedy baseline, ReviewNetRewardCriterion, backward, clamp + Adam;
  b  the group step with n = 5: sample_group on 128 images = 640 rows, the leave-one-out reward (no greedy pass), the same
     criterion, backward, clamp + Adam;
  c  the same 640-row work built only from the calls that existed before sample_group: the features repeated 5 times through
     sample() under grad, the rows scored once and the leave-one-out reward formed in torch.
b does strictly less work than c (stages I / II on 128 rows, not 640; the decoder's thought-vector products and their
gradients on a fifth of the rows), so median(b) must not exceed median(c) by more than c's own spread over its windows.  a
against b is what a user pays: b differentiates five times the rows.

--bench-ab PARENT: additionally the default `bench.py --gpus 1` line of this checkout and of a built checkout of the parent
commit, fresh processes, alternating, recorded in the same file."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'profiles', 'scst_group.json')
N_DRAWS = 5


def bench_line(tree, steps, warmup):
    out = subprocess.run([sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup)],
                         check=True, capture_output=True, text=True, cwd=tree, timeout=900).stdout
    line = json.loads([l for l in out.splitlines() if l.startswith('{"metric"')][-1])
    return {'value': line['value'], 'ms_per_step': line.get('ms_per_step')}


def bench_ab(parent, rounds, steps, warmup):
    """The default bench.py line, this checkout and the parent's alternating, `rounds` runs each (fresh processes)."""
    runs = {'parent': [], 'this': []}
    for _ in range(rounds):
        runs['parent'].append(bench_line(parent, steps, warmup))
        runs['this'].append(bench_line(ROOT, steps, warmup))
    res = {'cmd': 'bench.py --gpus 1 --steps %d --warmup %d' % (steps, warmup), 'runs_each': rounds, 'order': 'parent, this, parent, this, ...'}
    for k, v in runs.items():
        vals = [r['value'] for r in v]
        res[k] = {'captions_per_s': vals, 'median': statistics.median(vals), 'spread': round(max(vals) - min(vals), 2),
                  'ms_per_step': [r['ms_per_step'] for r in v]}
    res['this_within_parent_spread'] = bool(res['this']['median'] >= res['parent']['median'] - res['parent']['spread'])
    return res


def legs():
    import torch
    import bench as HB
    import recurrent_fusion_network_amd as R
    from recurrent_fusion_network_amd import rewards as RW
    dev = torch.device('cuda:0')
    B, n = 128, N_DRAWS
    cfg = HB.make_cfg(dict(HB.WORKLOADS['c3']))
    model = R.RecurrentFusionModel(cfg).to(dev)
    HB.seeded_weights_(model, 100)
    fc, att, labels, masks, top = HB.synthetic_inputs(cfg, B, 100, dev)
    fc5, att5 = [f.repeat_interleave(n, 0) for f in fc], [a.repeat_interleave(n, 0) for a in att]
    top5 = top.repeat_interleave(n, 0)
    crit = R.ReviewNetRewardCriterion(cfg)
    opt = R.FusedClampAdam(model, lr=5e-5, weight_decay=0.0, grad_clip=1.0)
    scorer = RW.CiderD()
    g = torch.Generator().manual_seed(3)
    gts = torch.randint(1, cfg.vocab_size + 1, (B, 5, cfg.seq_length + 1), generator=g)
    gts[:, :, -1] = 0
    gts, n_refs = gts.to(dev), torch.full((B,), 5, dtype=torch.int32, device=dev)
    row_img5 = (torch.arange(B * n, dtype=torch.int32) // n).to(dev)

    def finish(lp, seq, reward, lp_all, reason, top_words):
        crit(lp, seq, reward, lp_all, 0.01, reason, top_words, 1.0, None, cfg).backward()
        opt.step()

    def leg_a():
        model.train()
        opt.zero_grad()
        seq, lp, lp_all, reason = model.sample(fc, att, {'sample_max': 0})
        with torch.no_grad():
            model.eval()
            greedy = model.sample(fc, att, {'sample_max': 1})[0]
            model.train()
        T = max(seq.size(1), greedy.size(1))
        pad = lambda t: torch.nn.functional.pad(t, (0, T - t.size(1)))  # noqa: E731
        reward = RW.scst_reward(scorer, pad(seq), pad(greedy), gts, n_refs, 1)[:, :seq.size(1)].contiguous()
        finish(lp, seq, reward, lp_all, reason, top)

    def leg_b():
        model.train()
        opt.zero_grad()
        seq, lp, lp_all, reason = model.sample_group(fc, att, n)
        reward = RW.scst_group_reward(scorer, seq, gts, n_refs, n)
        finish(lp, seq, reward, lp_all, reason, top)

    def leg_c():
        model.train()
        opt.zero_grad()
        seq, lp, lp_all, reason = model.sample(fc5, att5, {'sample_max': 0})
        s = scorer.score_ids(seq, row_img5, gts, n_refs).view(B, n)
        base = (s.sum(1, keepdim=True) - s) / (n - 1)
        reward = (s - base).float().view(B * n, 1).expand(B * n, seq.size(1)).contiguous()
        finish(lp, seq, reward, lp_all, reason, top5)

    def same_results():
        """Faster and different is not faster: at the timed size, in eval mode, on one set of given tokens (`force_ids`) and one
        fixed reward, so that no draw can amplify a last-bit difference.
        decoder_alone: the thought vectors of ONE run of stages I / II through the decoder with 5 rows per image against the same
          vectors repeated 5 times through the plain decoder -- log-probs bit for bit, every gradient of the whole model within
          the project's bar 1e-5 + 1e-3 * max|g| (the tail products sum over other row counts).
        whole_step: sample_group against sample() on features repeated 5 times (leg c's pass) -- stages I / II run on 128 against
          640 rows, whose GEMMs split K differently, so the log-probs agree to rounding only."""
        S, rows = cfg.seq_length, B * n
        gen = torch.Generator().manual_seed(11)
        ids = torch.randint(1, cfg.vocab_size + 1, (rows, S), generator=gen).to(dev)
        fed = torch.cat([ids.new_zeros(rows, 1), ids], 1).contiguous()
        reward = torch.randn(rows, 1, generator=gen).to(dev).expand(rows, S).contiguous()
        model.eval()

        def grads_of(lp_all, reason, top_words):
            lp = lp_all[:, :S].gather(2, ids.unsqueeze(2)).squeeze(2)
            model.zero_grad(set_to_none=True)
            crit(lp, ids, reward, lp_all, 0.01, reason, top_words, 1.0, None, cfg).backward()
            return lp_all.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}

        def decoder(repeat):
            comb, h, c, reason = model._prefix(fc, att, False, 0)
            h, c = h.repeat_interleave(n, 0), c.repeat_interleave(n, 0)
            if repeat:
                return grads_of(model._decode_teacher_forced(fed, comb.repeat_interleave(n, 1), h, c, False, 0), list(reason.unbind(0)), top)
            return grads_of(model._decode_teacher_forced(fed, comb, h, c, False, 0, n=n), list(reason.unbind(0)), top)

        def report(got, want):
            worst = max(((float((got[1][k] - want[1][k]).abs().max()) / (1e-5 + 1e-3 * float(want[1][k].abs().max())), k) for k in want[1]))
            return {'log_probs_bit_equal': bool(torch.equal(got[0], want[0])),
                    'log_prob_max_abs_diff': float((got[0] - want[0]).abs().max()),
                    'worst_gradient_err_over_bar': round(worst[0], 5), 'worst_gradient': worst[1], 'gradients_compared': len(want[1])}

        out = {'rows': rows, 'steps': S + 1, 'decoder_alone': report(decoder(False), decoder(True))}
        _, _, all_b, reason_b = model.sample_group(fc, att, n, {'force_ids': ids})
        got = grads_of(all_b, reason_b, top)
        _, _, all_c, reason_c = model.sample(fc5, att5, {'sample_max': 0, 'force_ids': ids})
        out['whole_step'] = report(got, grads_of(all_c, reason_c, top5))
        model.zero_grad(set_to_none=True)
        return out

    return cfg, {'a': leg_a, 'b': leg_b, 'c': leg_c}, same_results


def time_legs(rounds, calls):
    import torch
    cfg, fns, same_results = legs()

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    same = same_results()                 # before any optimiser step: both passes see the seeded weights
    for fn in fns.values():              # every shape warmed before the first window
        fn()
        fn()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(window(fn))
    what = {'a': "today's RL step: sample() under grad on 128 rows + greedy pass + CIDEr-D reward + criterion + backward + clamp/Adam",
            'b': 'group step, n = 5: sample_group on 128 images (640 rows) + leave-one-out reward + criterion + backward + clamp/Adam',
            'c': 'the 640-row work from the older calls: features repeated 5x through sample() under grad, reward formed in torch'}
    res = {'config': 'M=4, L=196, D=2048, R=512, V+1=%d, seq=%d, B=128 images, n=%d' % (cfg.vocab_size + 1, cfg.seq_length, N_DRAWS),
           'rounds': rounds, 'calls_per_window': calls, 'timing': 'wall clock between device synchronisations, legs alternating'}
    for k in fns:
        res['leg_' + k] = {'what': what[k], 'ms': round(statistics.median(ms[k]), 3), 'min': round(min(ms[k]), 3),
                           'max': round(max(ms[k]), 3), 'spread_ms': round(max(ms[k]) - min(ms[k]), 3),
                           'windows_ms': [round(x, 3) for x in ms[k]]}
    res['b_against_c_same_results'] = same
    b, c = res['leg_b'], res['leg_c']
    res['b_minus_c_ms'] = round(b['ms'] - c['ms'], 3)
    res['b_within_c_plus_its_spread'] = bool(b['ms'] <= c['ms'] + c['spread_ms'])
    res['a_to_b'] = {'ms_per_step': [res['leg_a']['ms'], b['ms']], 'rows_differentiated': [128, 128 * N_DRAWS],
                     'note': 'what a user pays, not a comparison of equal work: b differentiates five times the rows'}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=OUT)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--bench-ab', metavar='PARENT', default=None, help='a built checkout of the parent commit')
    ap.add_argument('--bench-rounds', type=int, default=3)
    ap.add_argument('--bench-steps', type=int, default=10)
    ap.add_argument('--bench-warmup', type=int, default=3)
    ap.add_argument('--only-bench-ab', action='store_true', help='keep the legs of an existing --out file, redo the bench.py A/B')
    ap.add_argument('--only-check', action='store_true', help='keep an existing --out file, redo b_against_c_same_results')
    args = ap.parse_args()
    if args.only_bench_ab or args.only_check:
        with open(args.out) as f:
            res = json.load(f)
        if args.only_check:
            res['b_against_c_same_results'] = legs()[2]()
            print(json.dumps(res['b_against_c_same_results']), flush=True)
    else:
        res = time_legs(args.rounds, args.calls)
        print(json.dumps({k: v for k, v in res.items() if k.startswith(('leg_', 'b_'))}), flush=True)
    if args.bench_ab:
        # fresh processes, after this one has released the device's memory
        import torch
        torch.cuda.empty_cache()
        res['bench_py_default_line'] = bench_ab(os.path.abspath(args.bench_ab), args.bench_rounds, args.bench_steps, args.bench_warmup)
        print(json.dumps(res['bench_py_default_line']), flush=True)
    elif 'bench_py_default_line' not in res:
        res['bench_py_default_line'] = 'not measured (no --bench-ab checkout given)'
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
