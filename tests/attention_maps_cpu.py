"""fp64 restatement of RecurrentFusionModel.attention from the oracle's own cells (not a test module; test_attention_maps_cpu.py
pins it, the GPU tests compare against it).

The loops are those of oracle.rfn_oracle.thought_vectors / forward with the cells' `alpha` kept: stage I a1_i (B, T1, L_i), stage II
a2 (B, T2, M, T1), decoder aD (rows, steps, T2).  The rollout is the plain nested sum
    G_i[r, s, l] = sum_t2 aD[r, s, t2] * (sum_t1 a2[k, t2, i, t1] * a1_i[k, t1, l]),   k = r // n,
with zeros at dead steps (s >= length[r]) and, under ragged maps, past an image's length."""
import numpy as np
import torch

from oracle import rfn_oracle as O


def feed_of(seq, seq_length):
    """seq (rows, T) words as sample() returns them -> (feed (rows, steps + 1) with column 0 = BOS, steps, length (rows,)):
    column s feeds step s; a caption's words and its END are live."""
    seq = torch.as_tensor(seq).long()
    rows, T = seq.shape
    L = min(T, seq_length)
    feed = torch.zeros(rows, L + 2, dtype=torch.long)
    feed[:, 1:L + 1] = seq[:, :L]
    words = (feed[:, 1:L + 2] != 0).long().cumprod(1).sum(1)
    return feed, L + 1, torch.clamp(words + 1, max=L + 1).to(torch.int32).numpy()


def run_cells(cfg, P, fc, att, feed, steps, n=1):
    """The oracle's loops on one batch in the dtype of P -> (a1 list of (B, T1, L_i), a2 (B, T2, M, T1), aD (rows, steps, T2),
    comb (B, T2, R), log_prob (rows, steps, V + 1))."""
    M, R = len(cfg.feat_array_info), cfg.rnn_size
    T1, T2 = cfg.num_review_steps_0, cfg.num_review_steps
    hs, cs = O.init_state(cfg, P, fc)
    a1, outs = [[] for _ in range(M)], [[] for _ in range(M)]
    for t in range(T1):
        H = torch.cat(hs, 1)
        nh, nc = [], []
        for i in range(M):
            h_, c_, aux = O.fusion_cell(H, att[i], hs[i], cs[i], P, 'review_steps_individual.%d.lstm.%d.' % (t, i), R)
            nh.append(h_)
            nc.append(c_)
            a1[i].append(aux['alpha'])
        hs, cs = nh, nc
        for j in range(M):
            outs[j].append(hs[j])
    thoughts = [torch.stack(outs[i]).transpose(0, 1).contiguous() for i in range(M)]
    h = sum(hs) / M
    c = sum(cs) / M
    comb, a2 = [], []
    for t in range(T2):
        h, c, aux = O.review_cell(thoughts, h, c, P, t, R, cfg.review_maxout)
        comb.append(h)
        a2.append(torch.stack([x['alpha'] for x in aux['att']], 1))          # (B, M, T1)
    comb = torch.stack(comb).transpose(0, 1).contiguous()
    comb_r, h, c = comb, h, c
    if n > 1:
        comb_r, h, c = comb.repeat_interleave(n, 0), h.repeat_interleave(n, 0), c.repeat_interleave(n, 0)
    aD, lps = [], []
    for s in range(steps):
        xt = P['embed.weight'][feed[:, s]]
        h, c, aux = O.decoder_cell(xt, comb_r, h, c, P, R, cfg.maxout)
        logits = h @ P['logit.weight'].t() + P['logit.bias']
        lps.append(torch.log_softmax(logits, dim=1))
        aD.append(aux['alpha'])
    return ([torch.stack(a, 1) for a in a1], torch.stack(a2, 1), torch.stack(aD, 1), comb, torch.stack(lps, 1))


def rollout_np(aD, a2, a1, n=1, length=None, att_len=None):
    """Plain nested sums in fp64, both ascending: aD (rows, S, T2), a2 (B, T2, T1), a1 (B, T1, L) -> G (rows, S, L)."""
    aD, a2, a1 = (np.asarray(x, dtype=np.float64) for x in (aD, a2, a1))
    rows, S, T2 = aD.shape
    B, T1, L = a1.shape
    C = np.zeros((B, T2, L))
    for t1 in range(T1):
        C = C + a2[:, :, t1, None] * a1[:, None, t1, :]
    Cr = np.repeat(C, n, axis=0)
    G = np.zeros((rows, S, L))
    for t2 in range(T2):
        G = G + aD[:, :, t2, None] * Cr[:, None, t2, :]
    if length is not None:
        G[np.arange(S)[None, :] >= np.asarray(length)[:, None]] = 0.0
    if att_len is not None:
        dead = np.arange(L)[None, :] >= np.repeat(np.asarray(att_len), n)[:, None]
        G[np.broadcast_to(dead[:, None, :], G.shape)] = 0.0
    return G


def stats_np(G, length=None, mask=None):
    """-> (peak (rows, S) first argmax, top-two gap (rows, S), entropy in nats, mass or None); dead steps: -1, inf, 0, 0."""
    G = np.asarray(G, dtype=np.float64)
    rows, S, L = G.shape
    peak = G.argmax(2).astype(np.int32)
    srt = np.sort(G, axis=2)
    gap = srt[:, :, -1] - srt[:, :, -2] if L > 1 else np.full((rows, S), np.inf)
    with np.errstate(divide='ignore', invalid='ignore'):
        ent = -np.where(G > 0, G * np.log(np.where(G > 0, G, 1.0)), 0.0).sum(2)
    mass = None if mask is None else (G * (np.asarray(mask) != 0)).sum(2)
    if length is not None:
        dead = np.arange(S)[None, :] >= np.asarray(length)[:, None]
        peak[dead], gap[dead], ent[dead] = -1, np.inf, 0.0
        if mass is not None:
            mass[dead] = 0.0
    return peak, gap, ent, mass


def attention_maps(cfg, P, fc, att, seq, n=1, att_lens=None, dtype=torch.float64):
    """The restated model.attention(fc, att, seq) -> a dict of numpy arrays under the keys of the returned dict, plus 'comb' and
    'log_prob' (the thought vectors and log-probs of the same pass).  seq (B * n, T) words.  att_lens: None, or a list of M
    entries (None or B ints): each image then runs ALONE on its truncated maps and its weights are padded with zeros."""
    Pd = {k: v.to(dtype) for k, v in P.items()}
    fc = [t.to(dtype) for t in fc]
    att = [t.to(dtype) for t in att]
    M = len(att)
    B = fc[0].size(0)
    feed, steps, length = feed_of(seq, cfg.seq_length)
    if att_lens is None:
        a1, a2, aD, comb, lp = run_cells(cfg, Pd, fc, att, feed, steps, n)
        lens = [None] * M
    else:
        lens = [None if v is None else [int(x) for x in v] for v in att_lens]
        parts = []
        for b in range(B):
            att_b = [att[i][b:b + 1, :(att[i].size(1) if lens[i] is None else lens[i][b])] for i in range(M)]
            p = run_cells(cfg, Pd, [f[b:b + 1] for f in fc], att_b, feed[b * n:(b + 1) * n], steps, n)
            pad = [torch.nn.functional.pad(p[0][i], (0, att[i].size(1) - p[0][i].size(2))) for i in range(M)]
            parts.append((pad,) + p[1:])
        a1 = [torch.cat([p[0][i] for p in parts], 0) for i in range(M)]
        a2, aD, comb, lp = (torch.cat([p[j] for p in parts], 0) for j in (1, 2, 3, 4))
    a1 = [a.numpy() for a in a1]
    a2, aD = a2.numpy(), aD.numpy().copy()
    dead = np.arange(steps)[None, :] >= length[:, None]
    aD[dead] = 0.0
    out = {'encoder': a1, 'fusion': a2, 'decoder': aD, 'length': length, 'comb': comb.numpy(), 'log_prob': lp.numpy(),
           'rollout': [rollout_np(aD, a2[:, :, i], a1[i], n, length, lens[i]) for i in range(M)]}
    return out
