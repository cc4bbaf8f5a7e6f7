#!/usr/bin/env python3
"""BASELINE.json configs[4]: beam-search eval (beam=5) + self-critical RL sample path, M=4, L=196, D=2048, B=128 on one
MI355X.  Prints one JSON line per mode (images/s, inputs resident in HBM).  Not the headline metric: see bench.py."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench as HB
import recurrent_fusion_network_amd as R

dev = torch.device('cuda:0')
w = dict(HB.WORKLOADS['c3']); B = 128
cfg = HB.make_cfg(w)
model = R.RecurrentFusionModel(cfg).to(dev)
HB.seeded_weights_(model, 100)
fc, att, labels, masks, top = HB.synthetic_inputs(cfg, B, 100, dev)
rl_crit = R.ReviewNetRewardCriterion(cfg)
opt = R.FusedClampAdam(model, lr=5e-5, weight_decay=0.0, grad_clip=1.0)

def timed(fn, reps):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out

def greedy():
    model.eval()
    with torch.no_grad():
        return model.sample(fc, att, {'sample_max': 1})
def beam():
    model.eval()
    with torch.no_grad():
        return model.sample(fc, att, {'beam_size': 5})
def rl_step():
    # train_rl.py:160-203: multinomial sample with grad, greedy baseline sample, reward criterion, backward, step
    model.train(); opt.zero_grad()
    seq, lp, lp_all, reason = model.sample(fc, att, {'sample_max': 0})
    with torch.no_grad():
        model.eval(); base = model.sample(fc, att, {'sample_max': 1})[0]; model.train()
    reward = torch.randn(B, 1, device=dev).expand(B, seq.size(1)).contiguous()   # CIDEr-D scoring is out of scope
    loss = rl_crit(lp, seq, reward, lp_all, 0.01, reason, top, 1.0, None, cfg)
    loss.backward(); opt.step()
    return loss

def rl_step_reuse():
    model.reuse_prefix = True
    try:
        return rl_step()
    finally:
        model.reuse_prefix = False

def constraints_ab(out_path, rounds=5):
    """--constraints: config 5 greedy and beam 5 with block_ngram = 3, one banned id and five bad endings against the
    unconstrained calls (which issue the launches they always did), alternating between the two; medians of `rounds`."""
    S = cfg.seq_length
    cons = {'block_ngram': 3, 'banned_ids': [cfg.vocab_size], 'bad_endings': [1, 2, 3, 4, 5]}
    model.eval()
    res = {'config': 'M=4, L=196, D=2048, R=512, V+1=9488, seq=%d, B=%d' % (S, B), 'constraints': cons, 'rounds': rounds}
    for mode, base, extra in (('greedy', {'sample_max': 1}, 2 * S), ('beam5', {'beam_size': 5}, S)):
        run = lambda o: timed(lambda: model.sample(fc, att, o), 3)[0] * 1e3  # noqa: E731
        with torch.no_grad():
            plain, masked = [], []
            for _ in range(rounds):
                plain.append(run(dict(base)))
                masked.append(run(dict(base, **cons)))
        res[mode] = {'ms_unconstrained': round(sorted(plain)[rounds // 2], 3), 'ms_constrained': round(sorted(masked)[rounds // 2], 3),
                     'added_launches_per_call': extra}
        print(json.dumps({mode: res[mode]}), flush=True)
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')

if '--constraints' in sys.argv:
    constraints_ab(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'decode_constraints.json'))
    sys.exit(0)

for name, fn, reps in (('greedy sample', greedy, 5), ('beam=5 sample_beam', beam, 3), ('RL step (sample+baseline+loss+bwd+Adam)', rl_step, 3),
                       ('RL step, model.reuse_prefix (baseline sample reuses stages I/II)', rl_step_reuse, 3)):
    dt, out = timed(fn, reps)
    print(json.dumps({'mode': name, 'images_per_s': round(B / dt, 1), 'ms': round(dt * 1e3, 2), 'B': B,
                      'config': 'M=4, L=196, D=2048, R=512, V+1=9488, seq=16'}), flush=True)
