#!/usr/bin/env python3
"""BASELINE.json configs[4]: beam-search eval (beam=5) + self-critical RL sample path, M=4, L=196, D=2048, B=128 on one
MI355X.  Prints one JSON line per mode (images/s, inputs resident in HBM).  Not the headline metric: see bench.py."""
import json, os, sys, time
# --tree DIR: import the package (and bench.py) from another checkout of this repository -- the --diverse comparison's parent
TREE = sys.argv[sys.argv.index('--tree') + 1] if '--tree' in sys.argv else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(TREE))
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

def truncation_ab(out_path, rounds=7):
    """--truncate: config 5, the mode-1 (multinomial) device loop untruncated, with top_k = 50, top_p = 0.9, both, and with
    sample_n = 5 against the same call on features repeated five times; calls alternate, medians of `rounds`, kernel launches
    per call by the profiler.  Every setting runs stages I / II and then the device loop (untruncated plain multinomial is
    served by the replayed pass in sample(), so the loop is called directly here).  Plus one rfn_logp_truncate_rows launch at
    (128, 9488) next to one rfn_multinomial_pick launch, by device events around the single launch."""
    import ctypes as C
    from recurrent_fusion_network_amd import _native as N
    from recurrent_fusion_network_amd.decode import _Sampling
    S, V1 = cfg.seq_length, cfg.vocab_size + 1
    model.eval()
    fc5, att5 = [f.repeat_interleave(5, dim=0) for f in fc], [a.repeat_interleave(5, dim=0) for a in att]

    def loop(o, f=fc, a=att):
        with torch.no_grad():
            comb, h, c, _ = model._prefix(f, a, False, 0)
            return model._sample_device_loop(comb, h, c, False, 0, 0, 1.0, None, _Sampling.parse(o))

    settings = [('untruncated', lambda: loop({})), ('top_k_50', lambda: loop({'top_k': 50})), ('top_p_0.9', lambda: loop({'top_p': 0.9})),
                ('top_k_50_top_p_0.9', lambda: loop({'top_k': 50, 'top_p': 0.9})),
                ('sample_n_5_on_128_images', lambda: loop({'sample_n': 5})), ('features_repeated_5x_640_rows', lambda: loop({}, fc5, att5))]
    res = {'config': 'M=4, L=196, D=2048, R=512, V+1=%d, seq=%d, B=%d' % (V1, S, B), 'rounds': rounds,
           'what': 'ms per call of stages I / II + the mode-1 device loop (rfn_decoder_loop_ex2), calls alternating'}
    ms = {k: [] for k, _ in settings}
    for _ in range(rounds):
        for k, fn in settings:
            ms[k].append(timed(fn, 3)[0] * 1e3)
    with torch.no_grad():
        greedy_n = HB.count_launches(lambda: model.sample(fc, att, {'sample_max': 1}))
        never = {'sample_max': 0, 'banned_ids': [cfg.vocab_size]}
        cons_n = HB.count_launches(lambda: model.sample(fc, att, never))
    for k, fn in settings:
        res[k] = {'ms': round(sorted(ms[k])[rounds // 2], 3), 'launches_per_call': HB.count_launches(fn)}
        print(json.dumps({k: res[k]}), flush=True)
    res['launch_check'] = {'greedy_sample (the parent\'s path)': greedy_n, 'constrained multinomial sample (the parent\'s mode-1 loop)': cons_n,
                           'steps': S,
                           'note': 'the untruncated mode-1 loop must issue the greedy call\'s launches + one multinomial pick per step, '
                                   'and the parent\'s constrained mode-1 loop\'s minus blocklist and mask per step; a truncated loop one more per step',
                           'untruncated_is_greedy_plus_S': (res['untruncated']['launches_per_call'] == greedy_n + S) if greedy_n else None,
                           'untruncated_is_constrained_minus_2S': (res['untruncated']['launches_per_call'] == cons_n - 2 * S) if cons_n else None}
    # one launch of each kernel on log-probs of randn * 3 logits
    g = torch.Generator().manual_seed(1)
    src = torch.log_softmax(torch.randn(B, V1, generator=g) * 3.0, 1).to(dev)
    u, ids, work = torch.rand(B, generator=g).to(dev), torch.zeros(B, dtype=torch.long, device=dev), src.clone()

    def one(call, reps=50):
        t = []
        for _ in range(reps + 5):
            work.copy_(src)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            N.check(call())
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3)
        return round(sorted(t[5:])[reps // 2], 2)

    tr = lambda k, p: one(lambda: N.lib.rfn_logp_truncate_rows(work.data_ptr(), V1, B, V1, k, p, 1.0, None, N.stream_ptr()))  # noqa: E731
    res['single_launch_us'] = {
        'shape': [B, V1], 'note': 'median of 50, device events around one launch (they include the launch gap)',
        'rfn_multinomial_pick': one(lambda: N.lib.rfn_multinomial_pick(work.data_ptr(), V1, B, V1, 1.0, u.data_ptr(), None, 1.0,
                                                                       ids.data_ptr(), 1, N.stream_ptr())),
        'rfn_logp_truncate_rows top_k=50': tr(50, 1.0), 'rfn_logp_truncate_rows top_p=0.9': tr(0, 0.9),
        'rfn_logp_truncate_rows top_k=50 top_p=0.9': tr(50, 0.9)}
    print(json.dumps(res['single_launch_us']), flush=True)
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')

def _beam6_ms(extra, reps=10):
    with torch.no_grad():
        return timed(lambda: model.sample_beam(fc, att, dict(extra, beam_size=6)), reps)[0] * 1e3

def diverse_child(rounds):
    """--diverse-child: the plain beam_size = 6 call of whatever checkout --tree names, `rounds` windows -> one JSON line."""
    model.eval()
    _beam6_ms({})
    print(json.dumps({'beam6_ms': [round(_beam6_ms({}), 3) for _ in range(rounds)]}), flush=True)

def diverse_ab(out_path, parent_tree, rounds=7):
    """--diverse [--parent DIR]: config 5, one sample_beam call at beam_size = 6 with group_size in {1, 2, 3, 6} (diversity_lambda
    0.5), windows of 10 calls after a warm-up call, the four settings alternating, medians of `rounds`.  The parent commit's
    plain call is timed by this same script in a fresh child process on a built checkout of it (--parent), once before and
    once after, so its numbers come from the same box in the same session; its spread is the range of all its windows."""
    import statistics, subprocess
    S = cfg.seq_length
    model.eval()
    res = {'config': 'M=4, L=196, D=2048, R=512, V+1=9488, seq=%d, B=%d, beam_size=6' % (S, B), 'rounds': rounds, 'calls_per_window': 10,
           'diversity_lambda': 0.5}

    def parent_run():
        if not parent_tree:
            return None
        out = subprocess.run([sys.executable, os.path.abspath(__file__), '--tree', parent_tree, '--diverse-child', str(rounds)],
                             check=True, capture_output=True, text=True, timeout=600).stdout
        return json.loads([l for l in out.splitlines() if l.startswith('{')][-1])['beam6_ms']

    before = parent_run()
    groups = (1, 2, 3, 6)
    ms = {g: [] for g in groups}
    for g in groups:
        _beam6_ms({'group_size': g})                     # every shape warmed before the first window
    for _ in range(rounds):
        for g in groups:
            ms[g].append(_beam6_ms({'group_size': g}))
    after = parent_run()
    for g in groups:
        res['group_size_%d' % g] = {'ms': round(statistics.median(ms[g]), 3), 'min': round(min(ms[g]), 3), 'max': round(max(ms[g]), 3)}
    with torch.no_grad():
        res['launches_per_call'] = {('group_size_%d' % g): HB.count_launches(lambda: model.sample_beam(fc, att, {'beam_size': 6, 'group_size': g}))
                                    for g in groups}
    if before is None:
        res['parent'] = 'not measured (no --parent checkout given)'
    else:
        both = before + after
        spread = max(both) - min(both)
        pm = statistics.median(both)
        res['parent'] = {'ms': round(pm, 3), 'ms_before': round(statistics.median(before), 3), 'ms_after': round(statistics.median(after), 3),
                         'min': round(min(both), 3), 'max': round(max(both), 3), 'spread_ms': round(spread, 3)}
        res['minus_parent_ms'] = {('group_size_%d' % g): round(statistics.median(ms[g]) - pm, 3) for g in groups}
        res['group_size_1_within_parent_spread'] = bool(abs(statistics.median(ms[1]) - pm) <= spread)
    print(json.dumps(res), flush=True)
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')

def consensus_ab(out_path, rounds=7):
    """--consensus [--out FILE]: config 5, sample(sample_n = 5) and sample_beam(beam_size = 5), each without and with
    'consensus' (a corpus-df CiderD), windows of 3 calls after a warm-up call, the settings alternating, medians of `rounds`;
    kernel launches per call by the profiler; and the pick's own launches (rewards.consensus on the 128 x 5 candidates) next to
    one CiderD.score_ids call on the same 640 rows, by device events around each."""
    import statistics
    from recurrent_fusion_network_amd import rewards as RW
    S, V1 = cfg.seq_length, cfg.vocab_size + 1
    model.eval()
    sc = RW.CiderD()
    settings = [('sample_n_5', {'sample_max': 0, 'sample_n': 5}), ('sample_n_5_consensus', {'sample_max': 0, 'sample_n': 5, 'consensus': sc}),
                ('beam_5', {'beam_size': 5}), ('beam_5_consensus', {'beam_size': 5, 'consensus': sc})]
    res = {'config': 'M=4, L=196, D=2048, R=512, V+1=%d, seq=%d, B=%d' % (V1, S, B), 'rounds': rounds, 'calls_per_window': 3,
           'what': 'ms per sample() call (one read-back each), calls alternating; consensus scorer: CiderD(df=\'corpus\')'}

    def call(o):
        with torch.no_grad():
            return model.sample(fc, att, o)

    ms = {k: [] for k, _ in settings}
    for k, o in settings:
        call(o)
    for _ in range(rounds):
        for k, o in settings:
            ms[k].append(timed(lambda: call(o), 3)[0] * 1e3)
    for k, o in settings:
        res[k] = {'ms': round(statistics.median(ms[k]), 3), 'min': round(min(ms[k]), 3), 'max': round(max(ms[k]), 3),
                  'launches_per_call': HB.count_launches(lambda: call(o))}
        print(json.dumps({k: res[k]}), flush=True)
    res['added_ms'] = {'sample_n_5': round(res['sample_n_5_consensus']['ms'] - res['sample_n_5']['ms'], 3),
                       'beam_5': round(res['beam_5_consensus']['ms'] - res['beam_5']['ms'], 3)}
    # the pick alone, on the draws of one call
    with torch.no_grad():
        seq = call({'sample_max': 0, 'sample_n': 5})[0]
    cands = torch.zeros(B, 5, S, dtype=torch.long, device=dev)
    cands[:, :, :seq.size(1)] = seq.view(B, 5, -1)
    rows, row_img, n_refs = cands.view(B * 5, S), torch.arange(B * 5, device=dev, dtype=torch.int32) // 5, torch.full((B,), 5, dtype=torch.int32, device=dev)

    def one(fn, reps=50):
        t = []
        for _ in range(reps + 5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3)
        return round(sorted(t[5:])[reps // 2], 2)

    pick, score = (lambda: RW.consensus(sc, cands)), (lambda: sc.score_ids(rows, row_img, cands, n_refs))
    res['pick_alone_us'] = {'shape': [B, 5, S], 'note': 'median of 50, device events around the call\'s launches (launch gaps included)',
                            'rewards.consensus (6 launches, corpus df)': one(pick), 'launches': HB.count_launches(pick),
                            'CiderD.score_ids on the same 640 rows against the 5 candidates': one(score),
                            'score_ids_launches': HB.count_launches(score)}
    print(json.dumps(res['pick_alone_us']), flush=True)
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')

def _kernel_us(fn):
    """Device time of one call of `fn` per kernel name (us, summed over its launches; the profiler's device-activity records)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.events():
        if getattr(ev, 'device_type', None) is not None and 'cuda' in str(ev.device_type).lower():
            name = ev.name.split('(')[0].split('<')[0]
            if 'memcpy' in name.lower() or 'memset' in name.lower():
                continue
            t = out.setdefault(name, [0, 0.0])
            t[0] += 1
            t[1] += float(getattr(ev, 'device_time', 0.0) or getattr(ev, 'cuda_time', 0.0) or 0.0)
    return out

def lexical_ab(out_path, rounds=7):
    """--lexical [--out FILE]: config 5, one sample_beam call with beam_size = 3 and two single-id required sets per image (four
    states of three beams: 12 rows per image) against the plain beam_size = 12 call of this same tree, which issues the parent's
    launches by construction and so stands in for the parent.  Windows of 5 calls after a warm-up call, the two settings
    alternating, medians of `rounds`; kernel launches per call and the device time per kernel name by the profiler, each in a
    call of its own."""
    import statistics
    S, V1 = cfg.seq_length, cfg.vocab_size + 1
    model.eval()
    g = torch.Generator().manual_seed(5)
    req = torch.randint(1, V1, (B, 2, 1), generator=g)
    req[:, 1, 0] = torch.where(req[:, 1, 0] == req[:, 0, 0], req[:, 1, 0] % (V1 - 1) + 1, req[:, 1, 0])   # two distinct ids per image
    settings = [('plain_beam_12', {'beam_size': 12}), ('lexical_beam_3_two_sets', {'beam_size': 3, 'require': req})]
    res = {'config': 'M=4, L=196, D=2048, R=512, V+1=%d, seq=%d, B=%d, 12 rows per image' % (V1, S, B), 'rounds': rounds,
           'calls_per_window': 5, 'what': 'ms per sample_beam call, the two settings alternating'}

    def call(o):
        with torch.no_grad():
            return model.sample_beam(fc, att, o)

    ms = {k: [] for k, _ in settings}
    for k, o in settings:
        call(o)
    for _ in range(rounds):
        for k, o in settings:
            ms[k].append(timed(lambda: call(o), 5)[0] * 1e3)
    kernels = {}
    for k, o in settings:
        res[k] = {'ms': round(statistics.median(ms[k]), 3), 'min': round(min(ms[k]), 3), 'max': round(max(ms[k]), 3),
                  'launches_per_call': HB.count_launches(lambda: call(o))}
        kernels[k] = _kernel_us(lambda: call(o))
        print(json.dumps({k: res[k]}), flush=True)
    a, b = kernels['plain_beam_12'], kernels['lexical_beam_3_two_sets']
    diff = sorted(((b.get(n, [0, 0.0])[1] - a.get(n, [0, 0.0])[1], n) for n in set(a) | set(b)), key=lambda x: -abs(x[0]))
    res['kernel_us_lexical_minus_plain'] = [{'kernel': n, 'us': round(d, 1), 'plain': [a.get(n, [0, 0.0])[0], round(a.get(n, [0, 0.0])[1], 1)],
                                             'lexical': [b.get(n, [0, 0.0])[0], round(b.get(n, [0, 0.0])[1], 1)]} for d, n in diff[:8]]
    res['lexical_minus_plain_ms'] = round(res['lexical_beam_3_two_sets']['ms'] - res['plain_beam_12']['ms'], 3)
    call(settings[1][1])
    res['mean_sets_met_of_2'] = round(float(model.lexical_met.float().mean()), 3)
    print(json.dumps(res), flush=True)
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')

def stochastic_ab(out_path, rounds=7):
    """--stochastic [--out FILE]: config 5, sample_distinct with n = 5 alternating with the plain sample_beam(beam_size = 5) call of this
    same tree -- which issues the parent's launches by construction and so stands in for the parent -- and with sample(sample_n = 5).
    Windows of 5 calls after a warm-up call, medians of `rounds`; kernel launches per call by the profiler; and one
    rfn_log_softmax_topk_gumbel launch next to one rfn_log_softmax_topk launch at 640 x 9488, W = 5, by device events around the
    single launch."""
    import statistics
    from recurrent_fusion_network_amd import _native as N
    S, V1, W = cfg.seq_length, cfg.vocab_size + 1, 5
    model.eval()

    def call(kind):
        with torch.no_grad():
            if kind == 'sample_distinct_5':
                return model.sample_distinct(fc, att, W, {'seed': 7})
            if kind == 'plain_beam_5':
                return model.sample_beam(fc, att, {'beam_size': W})
            return model.sample(fc, att, {'sample_max': 0, 'sample_n': W})

    kinds = ('plain_beam_5', 'sample_distinct_5', 'sample_n_5')
    res = {'config': 'M=4, L=196, D=2048, R=512, V+1=%d, seq=%d, B=%d, 5 rows per image' % (V1, S, B), 'rounds': rounds,
           'calls_per_window': 5, 'what': 'ms per call, the three settings alternating; sample_n_5 includes its one read-back'}
    ms = {k: [] for k in kinds}
    for k in kinds:
        call(k)
    for _ in range(rounds):
        for k in kinds:
            ms[k].append(timed(lambda: call(k), 5)[0] * 1e3)
    for k in kinds:
        res[k] = {'ms': round(statistics.median(ms[k]), 3), 'min': round(min(ms[k]), 3), 'max': round(max(ms[k]), 3),
                  'launches_per_call': HB.count_launches(lambda: call(k))}
        print(json.dumps({k: res[k]}), flush=True)
    res['sample_distinct_over_plain_beam'] = round(res['sample_distinct_5']['ms'] / res['plain_beam_5']['ms'], 4)
    res['sample_distinct_minus_plain_beam_ms'] = round(res['sample_distinct_5']['ms'] - res['plain_beam_5']['ms'], 3)
    call('sample_distinct_5')
    res['distinct_captions_of_5'] = {'sample_distinct_5': round(float(model.stochastic_beams['n_live'].float().mean()), 3)}
    rows = call('sample_n_5')[0].view(B, W, -1).cpu()
    res['distinct_captions_of_5']['sample_n_5'] = round(sum(len({tuple(r) for r in img.tolist()}) for img in rows) / B, 3)
    # one launch of each top-W kernel on randn * 3 logits
    g = torch.Generator().manual_seed(1)
    R_ = B * W
    x = (torch.randn(R_, V1, generator=g) * 3.0).to(dev)
    tv, ti = torch.empty(R_, W, device=dev), torch.empty(R_, W, dtype=torch.int32, device=dev)
    tk, live = torch.empty(R_, W, dtype=torch.float64, device=dev), torch.ones(R_, dtype=torch.int32, device=dev)

    def one(fn, reps=50):
        t = []
        for _ in range(reps + 5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            N.check(fn())
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3)
        return round(sorted(t[5:])[reps // 2], 2)

    res['single_launch_us'] = {
        'shape': [R_, V1], 'W': W, 'note': 'median of 50, device events around one launch (they include the launch gap)',
        'rfn_log_softmax_topk': one(lambda: N.lib.rfn_log_softmax_topk(x.data_ptr(), V1, R_, V1, W, tv.data_ptr(), ti.data_ptr(), N.stream_ptr())),
        'rfn_log_softmax_topk_gumbel': one(lambda: N.lib.rfn_log_softmax_topk_gumbel(x.data_ptr(), V1, R_, V1, W, None, 0, None, live.data_ptr(),
                                                                                     7, 1, tk.data_ptr(), tv.data_ptr(), ti.data_ptr(),
                                                                                     N.stream_ptr()))}
    print(json.dumps(res), flush=True)
    with open(out_path, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')

PROFILES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles')
if '--stochastic' in sys.argv:
    stochastic_ab(sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(PROFILES, 'decode_stochastic.json'))
    sys.exit(0)
if '--lexical' in sys.argv:
    lexical_ab(sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(PROFILES, 'decode_lexical.json'))
    sys.exit(0)
if '--consensus' in sys.argv:
    consensus_ab(sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(PROFILES, 'decode_consensus.json'))
    sys.exit(0)
if '--diverse-child' in sys.argv:
    diverse_child(int(sys.argv[sys.argv.index('--diverse-child') + 1]))
    sys.exit(0)
if '--diverse' in sys.argv:
    diverse_ab(sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(PROFILES, 'diverse_beam.json'),
               sys.argv[sys.argv.index('--parent') + 1] if '--parent' in sys.argv else None)
    sys.exit(0)
if '--truncate' in sys.argv:
    truncation_ab(os.path.join(PROFILES, 'decode_truncation.json'))
    sys.exit(0)
if '--constraints' in sys.argv:
    constraints_ab(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'decode_constraints.json'))
    sys.exit(0)

for name, fn, reps in (('greedy sample', greedy, 5), ('beam=5 sample_beam', beam, 3), ('RL step (sample+baseline+loss+bwd+Adam)', rl_step, 3),
                       ('RL step, model.reuse_prefix (baseline sample reuses stages I/II)', rl_step_reuse, 3)):
    dt, out = timed(fn, reps)
    print(json.dumps({'mode': name, 'images_per_s': round(B / dt, 1), 'ms': round(dt * 1e3, 2), 'B': B,
                      'config': 'M=4, L=196, D=2048, R=512, V+1=9488, seq=16'}), flush=True)
