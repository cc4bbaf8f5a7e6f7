#!/usr/bin/env python3
"""The published XE recipe (train_recurrent_fusion_model.sh:15-29) in the launch-paced regime: the five shipped encoders
(bench.py's `c3het` workload), B = 10 images x 5 captions = 50, drop_prob_lm 0.3 (the other dropout probabilities at
opts.py's defaults, 0), label smoothing, ss_prob 0.25 -- one eager XE train step against the same step replayed from a HIP
graph (graphed.GraphedTrainStep(device_rng=True)), in one process, the legs alternating block by block.

    python tools/bench_recipe.py                       # eager and replayed, this checkout
    python tools/bench_recipe.py --eager-only --package-root <checkout of the parent commit>     # the baseline leg
    python tools/bench_recipe.py --baseline <file of --eager-only lines> --out profiles/recipe_graph.json

A block is `--steps` steps (>= 20) between two device synchronisations; every leg runs `--rounds` blocks after `--settle`
seconds of untimed steps and `--warmup` steps, and reports min / median / max of its blocks' ms per step.  The eager-only
form touches nothing newer than the parent commit (package, bench.py helpers), so it can time the parent's package on the same
box; run it three times to learn the run-to-run spread the comparison has to clear.  Prints one JSON line."""
import argparse
import json
import os
import socket
import statistics
import sys
import time


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=50)
    ap.add_argument('--steps', type=int, default=20, help='timed steps per block')
    ap.add_argument('--rounds', type=int, default=5, help='timed blocks per leg')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--settle', type=float, default=2.0, help='seconds of untimed steps first')
    ap.add_argument('--eager-only', action='store_true', help='the eager leg alone (what the parent commit can run)')
    ap.add_argument('--package-root', default=None, help='checkout whose package and bench.py are timed (default: this one)')
    ap.add_argument('--baseline', default=None, help='file of --eager-only result lines of the parent commit, same box')
    ap.add_argument('--out', default=None, help='also write the result (pretty-printed) here')
    return ap.parse_args()


def summary(ms):
    return {'min': round(min(ms), 3), 'median': round(statistics.median(ms), 3), 'max': round(max(ms), 3), 'blocks': [round(x, 3) for x in ms]}


def main():
    args = parse_args()
    if args.steps < 20:
        raise SystemExit('--steps: at least 20 timed steps per block')
    root = os.path.abspath(args.package_root or os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
    sys.path.insert(0, root)
    import torch
    import bench
    import recurrent_fusion_network_amd as R
    if os.path.dirname(os.path.dirname(os.path.abspath(R.__file__))) != root:
        raise SystemExit('imported %s, not the package under %s' % (R.__file__, root))
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: this tool measures, it has no fallback')
    dev = torch.device('cuda:0')
    w = bench.WORKLOADS['c3het']
    cfg = bench.make_cfg(w)
    cfg.drop_prob_lm, cfg.use_label_smoothing = 0.3, 1
    B = args.batch
    model = R.RecurrentFusionModel(cfg).to(dev)
    bench.seeded_weights_(model, 100)
    model.train()
    model.ss_prob = 0.25
    crit = R.ReviewNetEnsembleCriterion(cfg)
    opt = R.FusedClampAdam(model, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5, grad_clip=1.0)
    fc, att, labels, masks, top = bench.synthetic_inputs(cfg, B, 100, dev)
    torch.manual_seed(100)

    def eager():
        opt.zero_grad()
        log_prob, top_pred = model(fc, att, labels)
        loss = crit(log_prob, labels[:, 1:], masks[:, 1:], top_pred, top, 1.0)
        loss.backward()
        opt.step()
        return loss

    legs = {'eager': eager}
    ts = time.perf_counter()
    while time.perf_counter() - ts < args.settle:
        eager()
        torch.cuda.synchronize()
    launches = bench.count_launches(eager)
    if not args.eager_only:
        from recurrent_fusion_network_amd.graphed import GraphedTrainStep
        legs['replay'] = GraphedTrainStep(model, crit, opt, fc, att, labels, masks, top, device_rng=True)
    for fn in legs.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    loss = None
    for _ in range(args.rounds):
        for name, fn in legs.items():          # alternating: both legs see the same stretch of the box's time
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss = fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
    loss = float(loss.detach())
    if loss != loss:
        raise SystemExit('the loss is NaN')
    prop = torch.cuda.get_device_properties(dev)
    res = {
        'workload': 'XE train step under the published recipe: 5 shipped encoders (bench.py c3het), B = %d, drop_prob_lm 0.3, '
                    'label smoothing 0.1, ss_prob 0.25, seq 16 (17 decoder steps)' % B,
        'package_root': 'this checkout' if args.package_root is None else 'other checkout (--package-root)',
        'abi': int(R._native.ABI_VERSION), 'steps_per_block': args.steps, 'rounds': args.rounds, 'settle_s': args.settle,
        'eager_ms': summary(ms['eager']),
        'replay_ms': summary(ms['replay']) if 'replay' in ms else None,
        'launches_per_step': launches, 'last_loss': round(loss, 4),
        'box': {'host': socket.gethostname(), 'gpu': prop.name, 'arch': getattr(prop, 'gcnArchName', None),
                'cus': prop.multi_processor_count, 'torch': torch.__version__, 'hip': torch.version.hip},
    }
    if args.baseline:
        with open(args.baseline) as f:
            base = [json.loads(line) for line in f if line.strip().startswith('{')]
        res['parent_eager_ms'] = [b['eager_ms'] for b in base]
        res['parent_box'] = [b['box']['host'] for b in base]
        med = [b['eager_ms']['median'] for b in base]
        res['parent_eager_median_spread'] = {'min': min(med), 'max': max(med)} if med else None
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
