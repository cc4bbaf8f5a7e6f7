#!/usr/bin/env python3
"""The policy-gradient loss from the logits at profiles/scst_group.json's configuration (config 5: M=4, L=196, D=2048, B = 128
images, n = 5 rows per image, 640 rows) on one MI355X -> profiles/rl_loss.json.

Three legs, in alternating windows of `--calls` steps in one process, wall clock between device synchronisations, with
torch.cuda.max_memory_allocated per leg:
  a  today's group step: sample_group under grad, the leave-one-out reward, ReviewNetRewardCriterion, backward, clamp + Adam --
     the pass that is sampled is the pass that is differentiated, through logprobs_all (640, 17, 9488) and its gradient;
  b  sample(..., {'sample_max': 0, 'sample_n': 5}) under no_grad (the device loop), the same reward, rl_loss (one more decoder
     forward, no dense tensors), backward, clamp + Adam;
  c  sample_distinct(n = 5) under no_grad, the distinct-sample reward, rl_loss, backward, clamp + Adam.
Nobody promised an ordering: the numbers are reported as they come.

--cases FILE: the per-case error / bound figures tests/test_rl_logits_gpu.py appends with RFN_RL_LOSS_JSON set; their worst ratios
are recorded under 'kernel_error_over_bar'.
--bench-ab PARENT: additionally the default `bench.py --gpus 1` line of this checkout and of a built checkout of the parent
commit, fresh processes, alternating, recorded in the same file."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
OUT = os.path.join(ROOT, 'profiles', 'rl_loss.json')
N_DRAWS = 5
ENTROPY_REG = 0.01


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
    crit = R.ReviewNetRewardCriterion(cfg)
    opt = R.FusedClampAdam(model, lr=5e-5, weight_decay=0.0, grad_clip=1.0)
    scorer = RW.CiderD()
    g = torch.Generator().manual_seed(3)
    gts = torch.randint(1, cfg.vocab_size + 1, (B, 5, cfg.seq_length + 1), generator=g)
    gts[:, :, -1] = 0
    gts, n_refs = gts.to(dev), torch.full((B,), 5, dtype=torch.int32, device=dev)

    def leg_a():
        model.train()
        opt.zero_grad()
        seq, lp, lp_all, reason = model.sample_group(fc, att, n)
        reward = RW.scst_group_reward(scorer, seq, gts, n_refs, n)
        crit(lp, seq, reward, lp_all, ENTROPY_REG, reason, top, 1.0, None, cfg).backward()
        opt.step()

    def leg_b():
        model.train()
        opt.zero_grad()
        with torch.no_grad():
            seq = model.sample(fc, att, {'sample_max': 0, 'sample_n': n})[0].contiguous()
        reward = RW.scst_group_reward(scorer, seq, gts, n_refs, n)
        model.rl_loss(fc, att, seq, reward, top, entropy_reg=ENTROPY_REG, n=n)[0].backward()
        opt.step()

    def leg_c():
        model.train()
        opt.zero_grad()
        with torch.no_grad():
            seq = model.sample_distinct(fc, att, n)[0]
        reward = RW.scst_distinct_reward(scorer, seq, model.stochastic_beams['weight'], gts, n_refs, n)
        model.rl_loss(fc, att, seq, reward, top, entropy_reg=ENTROPY_REG, n=n)[0].backward()
        opt.step()

    def same_results():
        """At the timed size, in eval mode, on one set of given tokens and one fixed reward: rl_loss against sample_group(force_ids) +
        the criterion -- loss, token log-probs, and every gradient against the project's bar 1e-5 + 1e-3 * max|g|."""
        S, rows = cfg.seq_length, B * n
        gen = torch.Generator().manual_seed(11)
        ids = torch.randint(1, cfg.vocab_size + 1, (rows, S), generator=gen)
        ids[::3, S // 2:] = 0
        ids = ids.to(dev)
        reward = torch.randn(rows, 1, generator=gen).to(dev).expand(rows, S).contiguous()
        model.eval()
        seq, lp, lp_all, reason = model.sample_group(fc, att, n, {'force_ids': ids})
        model.zero_grad(set_to_none=True)
        want_loss = crit(lp, seq, reward, lp_all, ENTROPY_REG, reason, top, 1.0, None, cfg)
        want_loss.backward()
        want = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
        del lp_all
        model.zero_grad(set_to_none=True)
        loss, _ = model.rl_loss(fc, att, ids, reward, top, entropy_reg=ENTROPY_REG, n=n)
        loss.backward()
        got = {k: p.grad.detach() for k, p in model.named_parameters()}
        worst = max(((float((got[k] - want[k]).abs().max()) / (1e-5 + 1e-3 * float(want[k].abs().max())), k) for k in want))
        out = {'rows': rows, 'steps': S, 'loss': [float(loss.detach()), float(want_loss.detach())],
               'token_logprob_max_abs_diff': float((model.last_rl['logprobs'] - lp.detach()).abs().max()),
               'worst_gradient_err_over_bar': round(worst[0], 5), 'worst_gradient': worst[1], 'gradients_compared': len(want)}
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

    same = same_results()                 # before any optimiser step: both forms see the seeded weights
    peak = {}
    for k, fn in fns.items():            # every shape warmed before the first window; the peak of a leg on its own
        fn()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(window(fn))
    what = {'a': "today's group step, n = 5: sample_group under grad on 128 images (640 rows) + leave-one-out reward + criterion + "
                 'backward + clamp/Adam',
            'b': "sample(sample_max=0, sample_n=5) under no_grad (device loop) + the same reward + rl_loss + backward + clamp/Adam",
            'c': 'sample_distinct(n=5) under no_grad + the distinct-sample reward + rl_loss + backward + clamp/Adam'}
    res = {'config': 'M=4, L=196, D=2048, R=512, V+1=%d, seq=%d, B=128 images, n=%d, entropy_reg=%g, training mode'
                     % (cfg.vocab_size + 1, cfg.seq_length, N_DRAWS, ENTROPY_REG),
           'rounds': rounds, 'calls_per_window': calls, 'timing': 'wall clock between device synchronisations, legs alternating in one process'}
    for k in fns:
        res['leg_' + k] = {'what': what[k], 'ms': round(statistics.median(ms[k]), 3), 'min': round(min(ms[k]), 3),
                           'max': round(max(ms[k]), 3), 'spread_ms': round(max(ms[k]) - min(ms[k]), 3),
                           'windows_ms': [round(x, 3) for x in ms[k]], 'max_memory_allocated_bytes': int(peak[k])}
    res['rl_loss_against_two_call_form'] = same
    res['note'] = ('b pays one more decoder forward than a and saves logprobs_all, its gradient and four passes over them; c decodes by '
                   'stochastic beam search instead of sampling.  Nothing becomes a default on these numbers.')
    return res


def kernel_cases(path):
    rows = [json.loads(l) for l in open(path) if l.strip()]
    worst = lambda key: max(rows, key=lambda r: r[key])  # noqa: E731
    return {'source': 'tests/test_rl_logits_gpu.py with RFN_RL_LOSS_JSON set', 'cases': len(rows),
            'worst_grad_err_over_bar': {'value': round(worst('grad_err_over_bar')['grad_err_over_bar'], 5), 'case': worst('grad_err_over_bar')['case']},
            'worst_loss_err_over_bar': {'value': round(worst('loss_err_over_bar')['loss_err_over_bar'], 5), 'case': worst('loss_err_over_bar')['case']},
            'worst_stats_err_over_bar': {'value': round(worst('stats_err_over_bar')['stats_err_over_bar'], 5), 'case': worst('stats_err_over_bar')['case']}}


def main():
    from bench_scst import bench_ab
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=OUT)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--cases', metavar='FILE', default=None, help='the figures of tests/test_rl_logits_gpu.py (RFN_RL_LOSS_JSON)')
    ap.add_argument('--bench-ab', metavar='PARENT', default=None, help='a built checkout of the parent commit')
    ap.add_argument('--bench-rounds', type=int, default=3)
    ap.add_argument('--bench-steps', type=int, default=10)
    ap.add_argument('--bench-warmup', type=int, default=3)
    ap.add_argument('--only-bench-ab', action='store_true', help='keep the legs of an existing --out file, redo the bench.py A/B')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():      # a measurement path that finds no GPU does not fall back: the file says so
        with open(args.out, 'w') as f:
            json.dump({'legs': 'not measured (no GPU in this run)', 'bench_py_default_line': 'not measured (no GPU in this run)'}, f, indent=1)
            f.write('\n')
        print('no GPU: wrote "not measured" to %s' % args.out)
        return 1
    if args.only_bench_ab:
        with open(args.out) as f:
            res = json.load(f)
    else:
        res = time_legs(args.rounds, args.calls)
        print(json.dumps({k: v for k, v in res.items() if k.startswith(('leg_', 'rl_loss_'))}), flush=True)
    if args.cases:
        res['kernel_error_over_bar'] = kernel_cases(args.cases)
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
    sys.exit(main())
