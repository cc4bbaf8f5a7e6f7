#!/usr/bin/env python3
"""Ragged attention maps (`att_lens`): what the train step's prefix (stages I and II, forward + backward) costs at the bench.py
shape, three ways, alternating in one process (profiles/ragged_attention.json):

    none      att_lens=None                          -- must be the time it always was
    full      every length = L                       -- the same launches with a row count that changes nothing
    ragged    lengths uniform in [L / 4, L]          -- shorter trip counts in the stage-I attention passes

    python tools/bench_ragged.py --label this --rounds 5 --steps 4 > this.jsonl        (needs the GPU; one JSON line)
    python tools/bench_ragged.py --label this_alone --arms none >> this.jsonl          (only that arm, as a parent process runs)
    python tools/bench_ragged.py --merge parent.jsonl this.jsonl --out profiles/ragged_attention.json

The same file runs in a checkout of the parent commit (it then has only the `none` arm): processes of the two trees are
alternated by the caller, and --merge states the run-to-run spread of identical arms next to every difference.  Times are
device events around whole forward + backward passes; the byte figure is computed from the shapes."""
import argparse
import inspect
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def unread_bytes(lens, L, A, D, T1):
    """Bytes of proj and att_seq rows the stage-I attention passes skip, per train step: per step t and image, the score kernel
    reads a proj row (A floats) and the context kernel an att_seq row (D floats) per valid row; the backward reads both again
    (d alpha: att_seq; softmax / tanh backward: proj).  The dproj rows are still written (as zeros)."""
    skipped = sum(L - n for n in lens)
    return 4 * skipped * T1 * 2 * (A + D)


def run(args):
    import torch
    import bench
    import recurrent_fusion_network_amd as R
    w = bench.WORKLOADS[args.workload]
    B = args.batch or w['B']
    cfg = bench.make_cfg(w)
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = R.RecurrentFusionModel(cfg).to(dev).train()
    g = torch.Generator(device='cpu').manual_seed(1)
    fc = [torch.randn(B, F, generator=g).to(dev) for (_, _, F) in w['enc']]
    att = [torch.randn(B, L, D, generator=g).to(dev) for (L, D, _) in w['enc']]
    taught = 'att_lens' in inspect.signature(model._prefix).parameters
    arms = {'none': None}
    lens_host = None
    if taught:
        arms['full'] = [torch.full((B,), L, dtype=torch.int32, device=dev) for (L, _, _) in w['enc']]
        lens_host = [torch.randint(L // 4, L + 1, (B,), generator=g) for (L, _, _) in w['enc']]
        arms['ragged'] = [v.to(dev, torch.int32) for v in lens_host]
    if args.arms:      # e.g. --arms none: the process then does exactly what a process of the parent tree does
        arms = {k: v for k, v in arms.items() if k in args.arms}
    grads = None

    def step(lens):
        nonlocal grads
        model.zero_grad(set_to_none=True)
        out = model._prefix(fc, att, False, 0, lens) if taught else model._prefix(fc, att, False, 0)
        if grads is None:
            grads = [torch.randn_like(o) * 1e-3 for o in out]
        torch.autograd.backward(list(out), grads)

    for lens in arms.values():
        for _ in range(args.warmup):
            step(lens)
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(args.rounds):                   # the arms alternate: a drifting clock or a busy host hits all of them
        for name, lens in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                step(lens)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.steps)
    line = dict(label=args.label, workload=args.workload, B=B, steps=args.steps, rounds=args.rounds, ms=times)
    if lens_host is not None:
        line['ragged_mean_fraction'] = [float(v.float().mean()) / L for v, (L, _, _) in zip(lens_host, w['enc'])]
        line['ragged_unread_bytes_per_step'] = sum(unread_bytes(v.tolist(), L, cfg.att_hid_size, D, cfg.num_review_steps_0)
                                                   for v, (L, D, _) in zip(lens_host, w['enc']))
        line['attention_bytes_per_step_full'] = sum(unread_bytes([0] * B, L, cfg.att_hid_size, D, cfg.num_review_steps_0)
                                                    for (L, D, _) in w['enc'])
    print(json.dumps(line), flush=True)


def merge(args):
    lines = [json.loads(s) for f in args.merge for s in open(f) if s.strip().startswith('{')]
    by = {}
    for ln in lines:
        for arm, ms in ln['ms'].items():
            by.setdefault('%s/%s' % (ln['label'], arm), []).append(ms)
    out = dict(what='prefix (stages I and II) forward + backward, ms per pass, device events; tools/bench_ragged.py',
               workload=lines[0]['workload'], B=lines[0]['B'], steps_per_round=lines[0]['steps'], arms={})
    for k, runs in sorted(by.items()):
        flat = [x for r in runs for x in r]
        meds = [statistics.median(r) for r in runs]
        out['arms'][k] = dict(median_ms=statistics.median(flat), min_ms=min(flat), max_ms=max(flat), process_medians_ms=meds,
                              rounds=len(flat))
    # run-to-run spread: identical code, identical arm, another process / another round
    out['spread'] = {k: dict(across_processes_pct=100.0 * (max(v['process_medians_ms']) - min(v['process_medians_ms'])) / v['median_ms'],
                             across_rounds_pct=100.0 * (v['max_ms'] - v['min_ms']) / v['median_ms'])
                     for k, v in out['arms'].items()}
    for ln in lines:
        for k in ('ragged_mean_fraction', 'ragged_unread_bytes_per_step', 'attention_bytes_per_step_full'):
            if k in ln:
                out[k] = ln[k]
    med = lambda k: out['arms'][k]['median_ms'] if k in out['arms'] else None  # noqa: E731
    cmp_ = {}
    for a, b in (('this_alone/none', 'parent_alone/none'), ('this/none', 'parent/none'), ('this/full', 'this/none'),
                 ('this/ragged', 'this/none')):
        if med(a) is not None and med(b) is not None:
            cmp_['%s vs %s' % (a, b)] = dict(delta_pct=100.0 * (med(a) - med(b)) / med(b))
    out['compare'] = cmp_
    text = json.dumps(out, indent=1)
    if args.out:
        open(args.out, 'w').write(text + '\n')
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--label', default='this')
    ap.add_argument('--workload', default='c3')
    ap.add_argument('--batch', type=int, default=0)
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--arms', nargs='+', help='time only these arms (default: all the tree knows)')
    ap.add_argument('--merge', nargs='+')
    ap.add_argument('--out')
    args = ap.parse_args()
    merge(args) if args.merge else run(args)


if __name__ == '__main__':
    main()
