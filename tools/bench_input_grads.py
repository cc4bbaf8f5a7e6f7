#!/usr/bin/env python3
"""Gradients of fc_feats / att_feats (INTEGRATION.md "Input gradients"): what they cost (profiles/input_gradients.json).

  (i)  the XE train step's forward + backward (model.forward_loss + loss.backward(), no optimizer) at the bench.py shape (c3)
       and at BASELINE config 2 (c2), two arms alternating in one process:
           params     the features do not require grad -- the step bench.py times, launch for launch
           features   every fc_feats / att_feats tensor requires grad (RFN_PATH_OPT_INPUT_GRADS + rfn_prefix_bwd_inputs)
  (ii) the new kernel alone on the benchmark map (B x L x D of the c3 encoder, T = T1 steps), arms alternating in the same run:
           steps        rfn_attn_context_bwd_dseq_steps, accumulate = 0   (what rfn_prefix_bwd_inputs launches)
           steps_acc    the same, accumulate = 1
           per_step     T successive rfn_attn_context_bwd_dseq calls on the same buffers
           copy         a device-to-device copy that moves the bytes `steps` moves (a copy of n bytes moves 2 n)

    python tools/bench_input_grads.py --out profiles/input_gradients.json          (needs the GPU)

Times are device events around `--steps` passes (i) or `--reps` calls (ii) after warm-up; every arm reports the median, the
minimum and the spread over `--rounds` rounds.  Byte figures are computed from the shapes.  Nothing here is a threshold except
that `steps` must beat `per_step` (the script exits non-zero otherwise)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def summary(ms):
    med = statistics.median(ms)
    return dict(median_ms=med, min_ms=min(ms), max_ms=max(ms), spread_pct=100.0 * (max(ms) - min(ms)) / med, rounds=len(ms))


def alternate(torch, arms, rounds, n, warmup):
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(rounds):          # the arms alternate: a drifting clock or a busy host hits all of them
        for k, fn in arms.items():
            ms[k].append(timed(torch, fn, n))
    return {k: summary(v) for k, v in ms.items()}


def train_step(args, workload):
    import torch
    import bench
    import recurrent_fusion_network_amd as R
    w = bench.WORKLOADS[workload]
    B = w['B']
    cfg = bench.make_cfg(w)
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = R.RecurrentFusionModel(cfg).to(dev).train()
    bench.seeded_weights_(model, 3)
    crit = R.ReviewNetEnsembleCriterion(cfg)
    fc, att, labels, masks, top = bench.synthetic_inputs(cfg, B, 1, dev)

    def step(need):
        def run():
            model.zero_grad(set_to_none=True)
            f = [t.detach().requires_grad_(need) for t in fc]
            a = [t.detach().requires_grad_(need) for t in att]
            loss, _ = model.forward_loss(f, a, labels, masks, top, crit, 1.0)
            loss.backward()
            if need:
                assert all(t.grad is not None for t in f + a)
        return run

    arms = alternate(torch, {'params': step(False), 'features': step(True)}, args.rounds, args.steps, args.warmup)
    A, T1 = cfg.att_hid_size, cfg.num_review_steps_0
    extra_flop = sum(2.0 * B * L * D * A * T1 + 2.0 * B * L * D * T1 + 2.0 * B * F * cfg.rnn_size for (L, D, F) in w['enc'])
    proj_flop = sum(2.0 * B * L * D * A * T1 for (L, D, F) in w['enc'])
    delta = arms['features']['median_ms'] - arms['params']['median_ms']
    return dict(workload=workload, B=B, encoders=w['enc'], steps_per_round=args.steps, arms=arms,
                features_minus_params_ms=delta, features_over_params=arms['features']['median_ms'] / arms['params']['median_ms'],
                extra_gflop_per_step=extra_flop / 1e9, forward_projection_gflop_per_step=proj_flop / 1e9,
                extra_tflops_over_delta=extra_flop / 1e9 / delta if delta > 0 else None)


def kernel(args):
    import torch
    import bench
    import recurrent_fusion_network_amd._native as N
    w = bench.WORKLOADS['c3']
    B, (L, D, _) = w['B'], w['enc'][0]
    T = bench.make_cfg(w).num_review_steps_0
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(2)
    alpha = torch.softmax(torch.randn(T, B, L, generator=g, device=dev), 2)
    dz = torch.randn(T, B, D, generator=g, device=dev) * 1e-3
    out = torch.zeros(B, L, D, device=dev)
    st = N.stream_ptr()
    map_bytes = 4 * B * L * D
    moved = map_bytes + 4 * T * B * (D + L)               # `steps`: the map written once, dz and alpha read once
    src = torch.randn(moved // 8, generator=g, device=dev)     # a copy of n bytes moves 2 n
    dst = torch.empty_like(src)

    def steps(acc):
        def run():
            N.check(N.lib.rfn_attn_context_bwd_dseq_steps(T, alpha.data_ptr(), B * L, dz.data_ptr(), B * D, D, B, L, D, out.data_ptr(),
                                                          L * D, D, acc, None, st), 'rfn_attn_context_bwd_dseq_steps')
        return run

    def per_step():
        for t in range(T):
            N.check(N.lib.rfn_attn_context_bwd_dseq(alpha[t].data_ptr(), dz[t].data_ptr(), D, B, L, D, out.data_ptr(), L * D, D, st),
                    'rfn_attn_context_bwd_dseq')

    # same values first: T per-step calls on a zeroed map against one overwriting call (another summation form: to rounding)
    out.zero_()
    per_step()
    ref = out.clone()
    steps(0)()
    torch.cuda.synchronize()
    err = float((out - ref).abs().max())
    assert err <= 1e-5 * float(ref.abs().max()), err
    arms = alternate(torch, {'steps': steps(0), 'steps_acc': steps(1), 'per_step': per_step, 'copy': lambda: dst.copy_(src)},
                     args.rounds, args.reps, args.warmup)
    ms = {k: v['median_ms'] for k, v in arms.items()}
    rate = lambda nbytes, t: nbytes / (t * 1e-3) / 1e12        # noqa: E731  TB/s
    res = dict(B=B, L=L, D=D, T=T, reps_per_round=args.reps, arms=arms, map_bytes=map_bytes,
               bytes_moved=dict(steps=moved, steps_acc=moved + map_bytes, per_step=T * (2 * map_bytes + 4 * B * (D + L)), copy=2 * src.numel() * 4),
               max_abs_diff_steps_vs_per_step=err)
    res['tb_per_s'] = {k: rate(res['bytes_moved'][k], ms[k]) for k in ms}
    res['per_step_over_steps'] = ms['per_step'] / ms['steps']
    res['steps_fraction_of_copy_rate'] = res['tb_per_s']['steps'] / res['tb_per_s']['copy']
    res['steps_acc_fraction_of_copy_rate'] = res['tb_per_s']['steps_acc'] / res['tb_per_s']['copy']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=3, help='train steps per timed round (i)')
    ap.add_argument('--reps', type=int, default=20, help='kernel calls per timed round (ii)')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--workloads', nargs='+', default=['c3', 'c2'])
    ap.add_argument('--out')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_input_grads.py measures on the GPU: no device found')
    out = dict(what='feature gradients: train step forward + backward with / without them, and the kernel of term (B) alone; '
                    'ms from device events; tools/bench_input_grads.py',
               device=torch.cuda.get_device_name(0), kernel=kernel(args), train_step=[])
    for wl in args.workloads:
        out['train_step'].append(train_step(args, wl))
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    print(text)
    if out['kernel']['per_step_over_steps'] <= 1.0:
        sys.exit('rfn_attn_context_bwd_dseq_steps is not faster than the per-step sequence')


if __name__ == '__main__':
    main()
