#!/usr/bin/env python3
"""Attention maps at config 5 (M=4, L=196, D=2048, 128 images, S=16, V=9487) on one MI355X -> profiles/attention_maps.json.

For n in {1, 5} captions per image, in alternating windows of at least one second that end in a device synchronise (every version
warmed first; the window and timer helpers are tools/bench_score.py's):
  attention   model.attention(fc, att, ids, {'n': n})          score   model.score(fc, att, ids, {'n': n}) on the same captions
And the composition alone on the same device tensors, device events around back-to-back calls, alternating:
  rollout     the M rfn_attn_rollout launches of one call
  einsum      per encoder torch.einsum('kti,kil->ktl') then einsum('rst,rtl->rsl') with the image's rows repeated, then the host-side
              masking of dead steps -- it materialises the (B, T2, L) intermediate
Per version the median ms per call, the spread, and the bytes each must move (computed from the shapes): the rollout reads the three
weight families and writes the maps once; the einsum chain also writes and re-reads its intermediate, the n-fold repeat of it and
the masked copy.  Achieved bytes/s is those bytes over the median time; the operands are replayed back to back and stay warm in the
last-level cache, so these are not HBM rates.  Nothing is gated on these numbers."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
OUT = os.path.join(ROOT, 'profiles', 'attention_maps.json')
IMAGES = 128


def commit_of(given):
    if given:
        return given
    try:
        return subprocess.check_output(['git', '-C', ROOT, 'rev-parse', 'HEAD'], stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return 'unknown (not a git checkout)'


def run(rounds, min_window_s, ns, commit):
    import torch
    import bench as HB
    import recurrent_fusion_network_amd as R
    import recurrent_fusion_network_amd._native as N
    from bench_score import alternate, event_timer, host_timer, summary
    dev = torch.device('cuda:0')
    cfg = HB.make_cfg(dict(HB.WORKLOADS['c3']))
    model = R.RecurrentFusionModel(cfg).to(dev).eval()
    HB.seeded_weights_(model, 100)
    fc, att, _, _, _ = HB.synthetic_inputs(cfg, IMAGES, 100, dev)
    S, V1 = cfg.seq_length, cfg.vocab_size + 1
    M, T1, T2, L = len(att), cfg.num_review_steps_0, cfg.num_review_steps, att[0].size(1)
    res = {'commit': commit, 'config': 'M=%d, L=%d, D=2048, R=512, V+1=%d, seq=%d, %d images' % (M, L, V1, S, IMAGES),
           'rounds': rounds, 'min_window_s': min_window_s,
           'timing': 'model calls: wall clock between device synchronisations; the composition: device events around back-to-back '
                     'calls; versions alternate in one process, each warmed first.  The composition replays the same 10 - 39 MB of '
                     'operands back to back, so they are warm in the last-level cache: its bytes/s are not HBM rates', 'n': {}}
    for n in ns:
        rows = IMAGES * n
        gen = torch.Generator().manual_seed(1000 + n)
        ids = torch.randint(1, V1, (rows, S), generator=gen)
        for r in range(rows):                                   # ragged captions: 6 .. 16 words
            ids[r, 6 + (r * 7) % 11:] = 0
        ids = ids.to(dev)
        entry = {'rows': rows}
        ms, calls, short = alternate({'attention': lambda: model.attention(fc, att, ids, {'n': n}),
                                      'score': lambda: model.score(fc, att, ids, {'n': n})}, rounds, min_window_s, host_timer)
        for k in ms:
            entry[k] = dict(summary(ms[k]), calls_per_window=calls[k])
        entry['windows_shorter_than_min'] = int(short)
        entry['attention_minus_score_ms'] = round(entry['attention']['ms'] - entry['score']['ms'], 4)

        # the composition alone, on the tensors one call returned
        got = model.attention(fc, att, ids, {'n': n})
        steps = got['decoder'].size(1)
        dec, fus, enc, length = got['decoder'], got['fusion'], got['encoder'], got['length']
        outs = [torch.empty(rows, steps, L, device=dev) for _ in range(M)]
        st = N.stream_ptr()

        def k_rollout():
            for i in range(M):
                N.check(N.lib.rfn_attn_rollout(dec.data_ptr(), T2, steps * T2, fus[:, :, i].data_ptr(), M * T1, T2 * M * T1,
                                               enc[i].data_ptr(), L, T1 * L, length.data_ptr(), None, rows, n, steps, T1, T2, L,
                                               outs[i].data_ptr(), steps * L, L, st), 'rfn_attn_rollout')

        dead = torch.arange(steps, device=dev)[None, :] >= length[:, None]

        def k_einsum():
            res_ = []
            for i in range(M):
                C = torch.einsum('kti,kil->ktl', fus[:, :, i], enc[i])
                G = torch.einsum('rst,rtl->rsl', dec, C.repeat_interleave(n, 0) if n > 1 else C)
                res_.append(G.masked_fill(dead[:, :, None], 0.0))
            return res_

        k_rollout()
        ref = k_einsum()
        entry['rollout_minus_einsum_max_abs'] = max(float((a - b).abs().max()) for a, b in zip(outs, ref))
        del ref
        kms, kcalls, kshort = alternate({'rollout': k_rollout, 'einsum': k_einsum}, rounds, min_window_s, event_timer)
        kern = {k: dict(summary(kms[k]), calls_per_window=kcalls[k]) for k in kms}
        f = 4
        inputs = rows * steps * T2 * f * M + IMAGES * T2 * M * T1 * f + M * T1 * IMAGES * L * f     # aD is read once per encoder
        maps = M * rows * steps * L * f
        inter = M * IMAGES * T2 * L * f
        kern['rollout']['bytes'] = inputs + maps
        # einsum chain: + the intermediate written and read, its n-fold repeat written and read (n > 1), the unmasked maps
        # written, read and written again by masked_fill
        kern['einsum']['bytes'] = inputs + 2 * inter + (2 * n * inter if n > 1 else 0) + 3 * maps
        for k in ('rollout', 'einsum'):
            kern[k]['achieved_GB_per_s'] = round(kern[k]['bytes'] / (kern[k]['ms'] * 1e-3) / 1e9, 1)
        kern['windows_shorter_than_min'] = int(kshort)
        entry['composition'] = kern
        res['n'][str(n)] = entry
        print(json.dumps({str(n): entry}), flush=True)
        del got, outs
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=OUT)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--min-window-s', type=float, default=1.0)
    ap.add_argument('--n', type=int, nargs='+', default=[1, 5])
    ap.add_argument('--commit', default=None, help='the commit the numbers are taken on (default: git rev-parse HEAD)')
    args = ap.parse_args()
    res = run(args.rounds, args.min_window_s, args.n, commit_of(args.commit))
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
