"""Time the mixture-of-softmaxes head (include/rfn.h, "mixture of softmaxes") at the headline shape and write
profiles/mos_head.json:

    python tools/bench_mos.py [--rows 4352 --experts 10 --vocab 9488 --rnn 512] [--iters 10] [--out profiles/mos_head.json]

What is timed (HIP events around each call, median of --iters after 3 warm-up calls, one stream):
  head forward   rfn_mos_fwd                  } each as a whole, and its PRODUCTS alone: the same GEMM calls issued through
  loss form      rfn_mos_loss_fwd (eps 0, .1) } rfn_gemm_f32 on the same operands (c, the K latent maps in groups of at most 8,
  backward       rfn_mos_loss_bwd (eps 0, .1) } the vocabulary product; backward: its five products).  mix = whole - products
                                                (it includes the small tanh pass).
  plain pair     the `logit` product of the same rows, rfn_xe_logits_fwd and rfn_xe_logits_bwd.
The mix kernels' achieved bytes/s count the bytes they must move -- every read of the K * rows * V1 expert logits, the write of
d x or of the log-probs -- against the 6.29 TB/s copy rate of the MI355X microarchitecture guide.
Without a GPU the file says "not measured".
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_RATE = 6.29e12
NOTES = ('mix = whole call - products replayed through rfn_gemm_f32 on the same operands: it carries the tanh pass and, backward, '
         'the tanh backward and the separate column-sum pass over d x that the library takes for decoder.bias at this size '
         '(the replay rides it on the GEMM), so the backward figures are upper bounds; a rate above the copy rate means part of '
         'the second read of x was served from cache')


def timed(fn, iters, prepare=None):
    ts = []
    for i in range(iters + 3):
        if prepare is not None:
            prepare()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= 3:
            ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=4352)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--experts', type=int, default=10)
    ap.add_argument('--vocab', type=int, default=9488)
    ap.add_argument('--rnn', type=int, default=512)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mos_head.json'))
    a = ap.parse_args()
    rows, B, K, V1, R = a.rows, a.batch, a.experts, a.vocab, a.rnn
    shape = dict(rows=rows, K=K, V1=V1, R=R, E=R)
    if not torch.cuda.is_available():
        with open(a.out, 'w') as f:
            json.dump({'status': 'not measured', 'shape': shape, 'note': 'tools/bench_mos.py has not run on an MI355X'}, f, indent=1)
            f.write('\n')
        print('no GPU: wrote "not measured" to', a.out)
        return
    import recurrent_fusion_network_amd._native as N
    assert rows % B == 0
    T = rows // B
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(1)
    md = N.mos_dims(R, R, K, V1)
    names = N.mos_param_names(md)
    prm = []
    for i, n in enumerate(names):
        r, c = N.mos_param_shape(md, i)
        scale = 3.0 if n == 'decoder.bias' else (1.5 if n == 'decoder.weight' else 1.0) / max(c, 1) ** 0.5
        prm.append((torch.randn(r, c, generator=g) * scale).reshape((r,) if c == 1 else (r, c)).to(dev))
    grd = [torch.empty_like(p) for p in prm]
    h = torch.randn(rows, R, generator=g).to(dev)
    target = torch.randint(0, V1, (B, T), generator=g).to(dev)
    mask = (torch.rand(B, T, generator=g) > 0.2).float().to(dev)
    ws = N.mos_workspace(md, rows, True, dev)
    logp = torch.empty(rows, V1, device=dev)
    scratch, loss, d_h = torch.empty(rows, device=dev), torch.zeros(1, device=dev), torch.empty(rows, R, device=dev)
    gws = torch.empty(64 << 20, dtype=torch.uint8, device=dev)
    x = N.mos_ws_x(md, rows, ws)
    z = torch.empty(K, rows, R, device=dev)
    cbuf, dc, dz = torch.empty(rows, K, device=dev), torch.randn(rows, K, device=dev), torch.randn(K, rows, R, device=dev)
    Wp, Wd, bd = prm[0], prm[-2], prm[-1]
    lat = [(prm[1 + 2 * k], prm[2 + 2 * k]) for k in range(K)]

    def fwd_products():
        N.gemm(rows, K, [(cbuf, K, [(h, R, 1, Wp, R, 1, R, None)])])
        for k0 in range(0, K, 8):
            N.gemm(rows, R, [(z[k], R, [(h, R, 1, lat[k][0], R, 1, R, lat[k][1])]) for k in range(k0, min(K, k0 + 8))])
        N.gemm(K * rows, V1, [(x.view(K * rows, V1), V1, [(z.view(K * rows, R), R, 1, Wd, R, 1, R, bd)])])

    def bwd_products():
        xs, zs = x.view(K * rows, V1), z.view(K * rows, R)
        N.gemm(V1, R, [(grd[-2], R, [(xs, V1, 0, zs, R, 0, K * rows, None)], grd[-1])], ws=gws)
        N.gemm(K * rows, R, [(dz.view(K * rows, R), R, [(xs, V1, 1, Wd, R, 0, V1, None)])], ws=gws)
        for k0 in range(0, K, 8):
            N.gemm(R, R, [(grd[1 + 2 * k], R, [(dz[k], R, 0, h, R, 0, rows, None)], grd[2 + 2 * k])
                          for k in range(k0, min(K, k0 + 8))], ws=gws)
        N.gemm(K, R, [(grd[0], R, [(dc, K, 0, h, R, 0, rows, None)])], ws=gws)
        segs = [(dc, K, 1, Wp, R, 0, K, None)] + [(dz[k], R, 1, lat[k][0], R, 0, R, None) for k in range(K)]
        for s0 in range(0, len(segs), 8):
            N.gemm(rows, R, [(d_h, R, segs[s0:s0 + 8])], accumulate=s0 > 0, ws=gws)

    n_x = K * rows * V1 * 4.0
    res = {'status': 'measured', 'device': torch.cuda.get_device_name(0), 'shape': shape, 'iters': a.iters, 'copy_rate_bytes_per_s': COPY_RATE,
           'ms': {}, 'mix': {}}
    ms = res['ms']
    ms['fwd_products'] = timed(fwd_products, a.iters)
    ms['bwd_products'] = timed(bwd_products, a.iters)
    ms['head_fwd'] = timed(lambda: N.mos_fwd(md, h, prm, logp, ws, train=True), a.iters)
    for eps in (0.0, 0.1):
        tag = 'eps%g' % eps
        fwd = lambda: N.mos_loss_fwd(md, B, T, h, prm, target, mask, eps, scratch, loss, ws)          # noqa: E731
        ms['loss_fwd_' + tag] = timed(fwd, a.iters)
        ms['loss_bwd_' + tag] = timed(lambda: N.mos_loss_bwd(md, B, T, h, prm, target, mask, eps, 1.0, None, d_h, grd, ws),
                                      a.iters, prepare=fwd)
    # bytes the mix kernels must move: reads of x (the K log-sum-exps, then one more pass where one is needed), writes
    moved = {'head_fwd': 2 * n_x + rows * V1 * 4.0, 'loss_fwd_eps0': n_x, 'loss_fwd_eps0.1': 2 * n_x,
             'loss_bwd_eps0': 2 * n_x, 'loss_bwd_eps0.1': 3 * n_x}
    for k, nbytes in moved.items():
        prod = ms['bwd_products'] if 'bwd' in k else ms['fwd_products']
        mix_ms = ms[k] - prod
        res['mix'][k] = {'ms': mix_ms, 'bytes': nbytes, 'bytes_per_s': nbytes / (mix_ms * 1e-3) if mix_ms > 0 else None,
                         'of_copy_rate': nbytes / (mix_ms * 1e-3) / COPY_RATE if mix_ms > 0 else None}
    # the plain output layer on the same rows
    Wl, bl = torch.randn(V1, R, generator=g).mul(0.05).to(dev), torch.zeros(V1, device=dev)
    lg, lse = torch.empty(rows, V1, device=dev), torch.empty(rows, device=dev)
    st = N.stream_ptr()
    logit = lambda: N.gemm(rows, V1, [(lg, V1, [(h, R, 1, Wl, R, 1, R, bl)])])          # noqa: E731
    ms['plain_logit_product'] = timed(logit, a.iters)
    xe_f = lambda: N.check(N.lib.rfn_xe_logits_fwd(lg.data_ptr(), V1, B, T, V1, target.data_ptr(), target.stride(0), mask.data_ptr(),   # noqa: E731
                                                   mask.stride(0), 0.1, lse.data_ptr(), scratch.data_ptr(), loss.data_ptr(), 0, st))
    ms['plain_xe_logits_fwd_eps0.1'] = timed(xe_f, a.iters, prepare=logit)
    xe_b = lambda: N.check(N.lib.rfn_xe_logits_bwd(lg.data_ptr(), V1, B, T, V1, target.data_ptr(), target.stride(0), mask.data_ptr(),   # noqa: E731
                                                   mask.stride(0), 0.1, lse.data_ptr(), 1.0, None, st))
    ms['plain_xe_logits_bwd_eps0.1'] = timed(xe_b, a.iters, prepare=lambda: (logit(), xe_f()))
    for k in list(ms):
        ms[k] = round(ms[k], 4)
    res['notes'] = NOTES
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
