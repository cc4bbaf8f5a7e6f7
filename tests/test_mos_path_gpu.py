"""GPU: the decoder pass without its output layer (rfn_decoder_fwd_hidden / rfn_decoder_hidden / rfn_decoder_bwd_hidden, rfn.h
"mixture of softmaxes") against the plain pass on the golden configurations: the hidden rows are the plain pass's bits, and
the sweep started from d logits . logit.weight reproduces the plain pass's gradients (the project's gradient rule:
1e-7 + 2e-5 * max|reference|) with the logit.* slots zero-filled."""
import ctypes as C

import pytest
import torch

from conftest import load_case

pytestmark = pytest.mark.gpu


def _view(ws, ptr, n):
    off = ptr - ws.data_ptr()
    assert 0 <= off and off + 4 * n <= ws.numel()
    return ws[off:off + 4 * n].view(torch.float32)


@pytest.mark.parametrize('name', ['tiny0', 'odd', 'tinymax'])
def test_hidden_pass_matches_the_plain_pass(dev, name):
    import recurrent_fusion_network_amd as R
    import recurrent_fusion_network_amd._native as N
    cfg, spec, P, (fc, att, labels, masks, top), gold = load_case(name)
    model = R.RecurrentFusionModel(cfg)
    model.load_state_dict(P)
    model = model.to(dev).eval()
    fc, att, labels = [t.to(dev) for t in fc], [t.to(dev) for t in att], labels.to(dev)
    S = model._decoder_steps(labels)
    ids = labels[:, :S].contiguous()
    B = ids.size(0)
    with torch.no_grad():
        comb, h0, c0, _ = model._prefix(fc, att, False, 0)
    comb, h0, c0 = comb.contiguous(), h0.contiguous(), c0.contiguous()
    d = model._dims_for(False)
    Rn, V1 = d.R, d.V1
    params = model._params_lookup(model._decoder_slots)
    table = model._param_table(params, model._decoder_slots)
    st = N.stream_ptr()
    ws_bytes = N.lib.rfn_decoder_ws_bytes(C.byref(d), B, S, 1)
    ws1 = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    ws2 = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    log_prob = torch.empty(B, S, V1, device=dev)
    N.check(N.lib.rfn_decoder_fwd_ex(C.byref(d), B, S, table, comb.data_ptr(), h0.data_ptr(), c0.data_ptr(), ids.data_ptr(),
                                     ids.stride(0), log_prob.data_ptr(), ws1.data_ptr(), ws_bytes, 1, 0, 1, st), 'rfn_decoder_fwd_ex')
    N.check(N.lib.rfn_decoder_fwd_hidden(C.byref(d), B, S, table, comb.data_ptr(), h0.data_ptr(), c0.data_ptr(), ids.data_ptr(),
                                         ids.stride(0), ws2.data_ptr(), ws_bytes, 1, 0, st), 'rfn_decoder_fwd_hidden')
    hid1 = _view(ws1, N.lib.rfn_decoder_hidden(C.byref(d), B, S, 1, ws1.data_ptr()), S * B * Rn)
    hid2 = _view(ws2, N.lib.rfn_decoder_hidden(C.byref(d), B, S, 1, ws2.data_ptr()), S * B * Rn)
    assert float(hid1.abs().max()) > 0 and torch.equal(hid1, hid2)
    # the logit layer reads exactly these rows: log_softmax(hid . W^T + b) is the plain pass's log_prob
    W, b = model.logit.weight.detach().double(), model.logit.bias.detach().double()
    lp = torch.log_softmax(hid2.view(S, B, Rn).double() @ W.t() + b, 2).transpose(0, 1)
    assert float((lp - log_prob.double()).abs().max()) <= 1e-5

    # backward: the plain pass from a d log_prob, then the hidden sweep from that pass's d logits . logit.weight
    g = torch.Generator().manual_seed(17)
    d_lp = (torch.randn(B, S, V1, generator=g) * 0.05).to(dev)
    outs = []
    for plain in (True, False):
        flats, by_slot, gtable = model._grad_buffers(['decoder'], dev)
        flats['decoder'].fill_(float('nan'))          # every slot must be overwritten
        d_comb, d_h0, d_c0 = torch.empty_like(comb), torch.empty_like(h0), torch.empty_like(c0)
        if plain:
            N.check(N.lib.rfn_decoder_bwd_ex(C.byref(d), B, S, table, comb.data_ptr(), h0.data_ptr(), c0.data_ptr(), ids.data_ptr(),
                                             ids.stride(0), log_prob.data_ptr(), d_lp.data_ptr(), d_comb.data_ptr(), d_h0.data_ptr(),
                                             d_c0.data_ptr(), gtable, ws1.data_ptr(), ws_bytes, 0, 1, st), 'rfn_decoder_bwd_ex')
            dlg = _view(ws1, N.lib.rfn_decoder_logits(C.byref(d), B, S, 1, ws1.data_ptr()), S * B * V1).view(S * B, V1)
            d_hidden = (dlg.double() @ W).float().contiguous()
        else:
            N.check(N.lib.rfn_decoder_bwd_hidden(C.byref(d), B, S, table, comb.data_ptr(), h0.data_ptr(), c0.data_ptr(),
                                                 ids.data_ptr(), ids.stride(0), d_hidden.data_ptr(), d_comb.data_ptr(),
                                                 d_h0.data_ptr(), d_c0.data_ptr(), gtable, ws2.data_ptr(), ws_bytes, 0, st),
                    'rfn_decoder_bwd_hidden')
        outs.append((d_comb, d_h0, d_c0, {model._slot_names[s]: v.clone() for s, v in by_slot.items()}))
    (dc1, dh1, dcc1, g1), (dc2, dh2, dcc2, g2) = outs

    def close(a, ref, what):
        tol = 1e-7 + 2e-5 * float(ref.abs().max())
        err = float((a - ref).abs().max())
        assert err <= tol, '%s: %.3e > %.3e' % (what, err, tol)
    close(dc2, dc1, 'd_comb')
    close(dh2, dh1, 'd_h0')
    close(dcc2, dcc1, 'd_c0')
    seen = 0
    for k in g1:
        if k.startswith('logit.'):
            assert float(g1[k].abs().max()) > 0 and float(g2[k].abs().max()) == 0.0, k
        else:
            close(g2[k], g1[k], k)
            seen += 1
    assert seen == len(g1) - 2 and seen >= 13          # embed + the 12 decoder.* slots


def test_hidden_pass_refuses_the_unhoisted_forms(dev):
    import recurrent_fusion_network_amd as R
    import recurrent_fusion_network_amd._native as N
    cfg, spec, P, (fc, att, labels, masks, top), gold = load_case('tiny0')
    model = R.RecurrentFusionModel(cfg).to(dev).eval()
    model.path_flags = N.PATH_OPT_DEC_UNHOISTED
    d = model._dims_for(False)
    B, S = 2, 3
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    table = model._param_table(model._params_lookup(model._decoder_slots), model._decoder_slots)
    ids = torch.zeros(B, S, dtype=torch.long, device=dev)
    rc = N.lib.rfn_decoder_fwd_hidden(C.byref(d), B, S, table, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), ids.data_ptr(), S,
                                      buf.data_ptr(), buf.numel(), 0, 0, N.stream_ptr())
    assert rc == -2          # RFN_ERR_UNSUPPORTED, before anything is launched
