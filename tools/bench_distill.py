#!/usr/bin/env python3
"""Distillation at the bench shape (C3: M=4, L=196, D=2048, R=512, V=9487, B=256, seq 16) on one MI355X -> profiles/distillation.json.

Three forms of one train step's forward + backward (no optimizer), eval-mode weights, the same inputs, in alternating windows of
at least one second that end in a device synchronise (every form warmed first); the median ms per step of each:
  plain     model.forward_loss(...) + backward, no teacher -- the launches of the commit before distillation existed
  fused     model.forward_loss(..., teacher=t, kd_alpha=0.5, kd_temperature=2.0) + backward (rfn_kd_logits_fwd / _bwd)
  composed  the same loss written in torch ops on model(...)'s log_prob (B, S, V+1), + backward
The teacher is the no-grad log-probs of a second model with other weights, computed once outside the windows.
And the two criterion kernel pairs alone on the same (S * B, V+1) logits rows, timed with device events around back-to-back
launches, alternating: rfn_xe_logits_fwd + _bwd against rfn_kd_logits_fwd + _bwd, with the bytes each pair has to move.
No threshold is set: the numbers are the record.

--topk K (-> profiles/distillation_topk.json): the compact teacher.  The step forms are then plain, fused (the dense teacher) and
  topk      model.forward_loss(..., teacher=TopKTeacher.from_dense(t, K), ...) + backward (rfn_kd_topk_fwd / _bwd)
(composed is left out), a third kernel pair kd_topk_pair joins xe_pair and kd_pair in the same alternation, and
EnsembleDecoder.teacher_logits is timed against teacher_topk (one member: the teacher model), with the peak memory of each."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'profiles', 'distillation.json')
OUT_TOPK = os.path.join(ROOT, 'profiles', 'distillation_topk.json')
ALPHA, TEMPERATURE = 0.5, 2.0


def run(rounds, min_window_s, batch, topk=0):
    import torch
    import bench as HB
    import bench_score as BS
    import recurrent_fusion_network_amd as R
    import recurrent_fusion_network_amd._native as N
    from recurrent_fusion_network_amd.criteria import _MLMFn
    from recurrent_fusion_network_amd.ensemble import EnsembleDecoder
    dev = torch.device('cuda:0')
    w = dict(HB.WORKLOADS['c3'])
    cfg = HB.make_cfg(w)
    B = batch or w['B']
    model = R.RecurrentFusionModel(cfg).to(dev).eval()
    HB.seeded_weights_(model, 100)
    teacher_model = R.RecurrentFusionModel(cfg).to(dev).eval()
    HB.seeded_weights_(teacher_model, 101)
    crit = R.ReviewNetEnsembleCriterion(cfg)
    fc, att, labels, masks, top = HB.synthetic_inputs(cfg, B, 100, dev)
    with torch.no_grad():
        t = teacher_model(fc, att, labels)[0]
    tk = R.TopKTeacher.from_dense(t, topk) if topk else None
    ens = EnsembleDecoder([teacher_model]) if topk else None
    del teacher_model
    torch.cuda.empty_cache()
    S, V1 = t.size(1), cfg.vocab_size + 1
    it = float(torch.tensor(1.0 / TEMPERATURE, dtype=torch.float32))

    def plain():
        model.zero_grad(set_to_none=True)
        loss, _ = model.forward_loss(fc, att, labels, masks, top, crit, 1.0)
        loss.backward()
        return loss.detach()

    def fused():
        model.zero_grad(set_to_none=True)
        loss, _ = model.forward_loss(fc, att, labels, masks, top, crit, 1.0, teacher=t, kd_alpha=ALPHA, kd_temperature=TEMPERATURE)
        loss.backward()
        return loss.detach()

    def sparse():
        model.zero_grad(set_to_none=True)
        loss, _ = model.forward_loss(fc, att, labels, masks, top, crit, 1.0, teacher=tk, kd_alpha=ALPHA, kd_temperature=TEMPERATURE)
        loss.backward()
        return loss.detach()

    def composed():
        model.zero_grad(set_to_none=True)
        lp, reason = model(fc, att, labels)
        m = masks[:, 1:S + 1]
        xe = -(m * lp.gather(2, labels[:, 1:S + 1].unsqueeze(2)).squeeze(2)).sum() / B
        log_pt, log_ps = torch.log_softmax(t * it, 2), torch.log_softmax(lp * it, 2)
        kd = (m * (log_pt.exp() * (log_pt - log_ps)).sum(2)).sum() / (it * it) / B
        loss = (1 - ALPHA) * xe + ALPHA * kd + _MLMFn.apply(1.0 / len(reason), top, *reason)
        loss.backward()
        return loss.detach()

    res = {'config': 'M=4, L=196, D=2048, R=512, V+1=%d, seq=%d (S=%d steps), B=%d' % (V1, cfg.seq_length, S, B),
           'kd_alpha': ALPHA, 'kd_temperature': TEMPERATURE, 'rounds': rounds, 'min_window_s': min_window_s,
           'what': 'ms per forward + backward of one train step (no optimizer), the three forms alternating in one process',
           'timing': 'steps: wall clock between device synchronisations; kernels: device events around back-to-back launches'}
    forms = {'plain': plain, 'fused': fused, 'topk': sparse} if topk else {'plain': plain, 'fused': fused, 'composed': composed}
    res['loss'] = {k: float(fn()) for k, fn in forms.items()}
    if topk:
        res['topk'], res['last_distill_topk'] = topk, {k: float(v) for k, v in model.last_distill.items()}
        fused()
    else:
        res['loss']['fused_minus_composed'] = res['loss']['fused'] - res['loss']['composed']
    res['last_distill'] = {k: float(v) for k, v in model.last_distill.items()}
    ms, calls, short = BS.alternate(forms, rounds, min_window_s, BS.host_timer)
    for k in ms:
        res[k if k != 'topk' else 'topk_step'] = dict(BS.summary(ms[k]), calls_per_window=calls[k], **BS.peak_of(forms[k]))
    res['windows_shorter_than_min'] = int(short)
    res['fused_minus_plain_ms'] = round(res['fused']['ms'] - res['plain']['ms'], 4)
    if topk:
        res['topk_minus_plain_ms'] = round(res['topk_step']['ms'] - res['plain']['ms'], 4)
        # the teacher itself: the dense (B, S, V+1) tensor against the (B, S, K) pair, one member
        tfns = {'teacher_logits': lambda: ens.teacher_logits(fc, att, labels), 'teacher_topk': lambda: ens.teacher_topk(fc, att, labels, topk)}
        tms, tcalls, tshort = BS.alternate(tfns, rounds, min_window_s, BS.host_timer)
        res['teacher'] = {k: dict(BS.summary(tms[k]), calls_per_window=tcalls[k], **BS.peak_of(tfns[k])) for k in tms}
        res['teacher']['windows_shorter_than_min'] = int(tshort)
        res['teacher']['bytes_per_batch'] = {'teacher_logits': S * B * V1 * 4, 'teacher_topk': S * B * topk * 8}
        del ens
    else:
        res['composed_minus_fused_ms'] = round(res['composed']['ms'] - res['fused']['ms'], 4)
    model.zero_grad(set_to_none=True)
    torch.cuda.empty_cache()

    # the two criterion kernel pairs on the same rows (the backward overwrites the logits: the next forward reads gradients,
    # which are as good a set of floats to time on)
    logits = torch.randn(S * B, V1, device=dev) * 3
    tgt, msk = labels[:, 1:S + 1].contiguous(), masks[:, 1:S + 1].contiguous()
    stats, scratch, loss = torch.empty(3 * S * B, device=dev), torch.empty(2 * B * S, device=dev), torch.zeros(1, device=dev)
    terms, one = torch.empty(2, device=dev), torch.ones(1, device=dev)
    st = N.stream_ptr()

    def xe_pair():
        N.check(N.lib.rfn_xe_logits_fwd(logits.data_ptr(), V1, B, S, V1, tgt.data_ptr(), tgt.stride(0), msk.data_ptr(), msk.stride(0),
                                        0.0, stats.data_ptr(), scratch.data_ptr(), loss.data_ptr(), 0, st), 'rfn_xe_logits_fwd')
        N.check(N.lib.rfn_xe_logits_bwd(logits.data_ptr(), V1, B, S, V1, tgt.data_ptr(), tgt.stride(0), msk.data_ptr(), msk.stride(0),
                                        0.0, stats.data_ptr(), 1.0, one.data_ptr(), st), 'rfn_xe_logits_bwd')

    def kd_pair():
        N.check(N.lib.rfn_kd_logits_fwd(logits.data_ptr(), V1, B, S, V1, tgt.data_ptr(), tgt.stride(0), msk.data_ptr(), msk.stride(0),
                                        0.0, t.data_ptr(), t.stride(0), t.stride(1), ALPHA, it, stats.data_ptr(), scratch.data_ptr(),
                                        loss.data_ptr(), 0, terms.data_ptr(), st), 'rfn_kd_logits_fwd')
        N.check(N.lib.rfn_kd_logits_bwd(logits.data_ptr(), V1, B, S, V1, tgt.data_ptr(), tgt.stride(0), msk.data_ptr(), msk.stride(0),
                                        0.0, t.data_ptr(), t.stride(0), t.stride(1), ALPHA, it, stats.data_ptr(), 1.0, one.data_ptr(),
                                        st), 'rfn_kd_logits_bwd')

    def kd_topk_pair():
        N.check(N.lib.rfn_kd_topk_fwd(logits.data_ptr(), V1, B, S, V1, tgt.data_ptr(), tgt.stride(0), msk.data_ptr(), msk.stride(0),
                                      0.0, *tk._abi(), ALPHA, it, stats.data_ptr(), scratch.data_ptr(), loss.data_ptr(), 0,
                                      terms.data_ptr(), st), 'rfn_kd_topk_fwd')
        N.check(N.lib.rfn_kd_topk_bwd(logits.data_ptr(), V1, B, S, V1, tgt.data_ptr(), tgt.stride(0), msk.data_ptr(), msk.stride(0),
                                      0.0, *tk._abi(), ALPHA, it, stats.data_ptr(), 1.0, one.data_ptr(), st), 'rfn_kd_topk_bwd')

    pairs = {'xe_pair': xe_pair, 'kd_pair': kd_pair}
    if topk:
        pairs['kd_topk_pair'] = kd_topk_pair
    kms, kcalls, kshort = BS.alternate(pairs, rounds, min_window_s, BS.event_timer)
    rows_bytes = S * B * V1 * 4
    kern = {k: dict(BS.summary(kms[k]), calls_per_window=kcalls[k]) for k in kms}
    kern['rows_bytes'] = rows_bytes
    kern['xe_pair']['bytes'] = 3 * rows_bytes                # fwd reads x; bwd reads x, writes d x
    kern['kd_pair']['bytes'] = 5 * rows_bytes                # ... and each direction reads the teacher row once
    if topk:
        kern['kd_topk_pair']['bytes'] = 3 * rows_bytes + 2 * S * B * topk * 8     # the XE pair's, plus the K entries each way
        kern['kd_topk_minus_xe_ms'] = round(kern['kd_topk_pair']['ms'] - kern['xe_pair']['ms'], 4)
        kern['kd_topk_minus_kd_ms'] = round(kern['kd_topk_pair']['ms'] - kern['kd_pair']['ms'], 4)
    for k in pairs:
        kern[k]['achieved_GB_per_s'] = round(kern[k]['bytes'] / (kern[k]['ms'] * 1e-3) / 1e9, 1)
    kern['kd_minus_xe_ms'] = round(kern['kd_pair']['ms'] - kern['xe_pair']['ms'], 4)
    kern['windows_shorter_than_min'] = int(kshort)
    res['kernels'] = kern
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='default: profiles/distillation.json, with --topk profiles/distillation_topk.json')
    ap.add_argument('--topk', type=int, default=0, help='K <= 32: measure the compact teacher next to the dense one')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--min-window-s', type=float, default=1.0)
    ap.add_argument('--batch', type=int, default=0, help='captions (default: the workload value, 256)')
    args = ap.parse_args()
    res = run(args.rounds, args.min_window_s, args.batch, args.topk)
    print(json.dumps(res), flush=True)
    with open(args.out or (OUT_TOPK if args.topk else OUT), 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
