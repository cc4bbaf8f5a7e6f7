"""NumPy fp64 restatements of the policy-gradient loss from the logits (include/rfn.h rfn_rl_logits_fwd / _bwd) and of the reward of
a distinct-sample set (rfn_scst_reward_distinct); not a test module.

rl_logits(x (B, T, V1), seq (B, T), reward (B, T), ...): per row, with lp_v = x_v - lse, p_v = exp(lp_v), tok = seq[b, t] (an id
outside [0, V1) reads as 0), m0 = seq[b, t] > 0, mk = 1 at t == 0 and seq[b, t - 1] > 0 after it:
    Hm   = sum_v lp_v * p_v            (0 where entropy_reg * m0 == 0: the sum is skipped)
    pol  = lp_tok * rw, or min(s1, clamp(s1, 1 - c, 1 + c) * rw) with s1 = exp(lp_tok) / (1e-5 + exp(old)) * rw  (misc/utils.py:
           64-66: the reference clamps surr1, not the ratio)
    loss = sum (-pol * mk + entropy_reg * m0 * Hm) / B
    d x_v = a * ([v == tok] - p_v) + e * p_v * (lp_v - Hm),  a = -(g / B) * mk * d pol / d lp_tok,  e = (g / B) * entropy_reg * m0
A row with a == 0 and e == 0 is exactly zero.

distinct_reward: every sum, product and quotient is one fp64 operation in the header's order, written as Python loops."""
import numpy as np


def rl_logits(x, seq, reward, entropy_reg=0.0, old=None, ppo_clip=0.2, g=1.0):
    """-> dict(loss, rows (B, T), policy, entropy, lse (B, T), Hm (B, T), tok_lp (B, T), grad (B, T, V1)), all float64."""
    x = np.asarray(x, dtype=np.float64)
    seq = np.asarray(seq, dtype=np.int64)
    reward = np.asarray(reward, dtype=np.float64)
    B, T, V1 = x.shape
    assert seq.shape == (B, T) and reward.shape == (B, T) and (old is None or np.shape(old) == (B, T))
    ent, clip = np.float64(np.float32(entropy_reg)), np.float64(np.float32(ppo_clip))
    mx = x.max(axis=2, keepdims=True)
    lse = (mx + np.log(np.exp(x - mx).sum(axis=2, keepdims=True)))[:, :, 0]
    lp = x - lse[:, :, None]
    p = np.exp(lp)
    rows, Hm, tok_lp, grad = np.zeros((B, T)), np.zeros((B, T)), np.zeros((B, T)), np.zeros((B, T, V1))
    pol_rows, ent_rows = np.zeros((B, T)), np.zeros((B, T))
    for b in range(B):
        for t in range(T):
            s = int(seq[b, t])
            tok = s if 0 <= s < V1 else 0
            m0 = 1.0 if s > 0 else 0.0
            mk = 1.0 if t == 0 or seq[b, t - 1] > 0 else 0.0
            rw = reward[b, t]
            lpt = lp[b, t, tok]
            tok_lp[b, t] = lpt
            if ent != 0.0 and m0 != 0.0:
                Hm[b, t] = float((lp[b, t] * p[b, t]).sum())
            if old is None:
                pol, dpol = lpt * rw, rw
            else:
                ratio = np.exp(lpt) / (1e-5 + np.exp(np.float64(old[b][t])))
                s1 = ratio * rw
                s2 = min(max(s1, 1.0 - clip), 1.0 + clip) * rw
                pol = min(s1, s2)
                ds1 = ratio * rw
                ds2 = ds1 * rw if 1.0 - clip < s1 < 1.0 + clip else 0.0
                dpol = ds1 if s1 <= s2 else ds2
            pol_rows[b, t] = -pol * mk
            ent_rows[b, t] = ent * m0 * Hm[b, t]
            rows[b, t] = pol_rows[b, t] + ent_rows[b, t]
            a = -(g / B) * mk * dpol if mk != 0.0 else 0.0
            e = (g / B) * ent * m0
            if a == 0.0 and e == 0.0:
                continue
            hot = np.zeros(V1)
            hot[tok] = 1.0
            grad[b, t] = a * (hot - p[b, t])
            if e != 0.0:
                grad[b, t] += e * p[b, t] * (lp[b, t] - Hm[b, t])
    return dict(loss=float(rows.sum() / B), rows=rows, policy=float(pol_rows.sum() / B), entropy=float(ent_rows.sum() / B), lse=lse,
                Hm=Hm, tok_lp=tok_lp, grad=grad)


def make_case(B, T, V1, seed, scale=3.0):
    """Inputs that reach every branch -> dict(x (B, T, V1) f32, seq (B, T) i64, reward (B, T) f32, old (B, T) f32): rewards of
    both signs and an exact zero, a finished row (zeros from its END on), a row that draws 0 first when B > 1, an id outside
    [0, V1) on a scored position, and `old` chosen so that surr1 of the positive-reward positions cycles through 0.5 (below the
    clamp at ppo_clip 0.2), 1.0 (inside) and 1.5 (above); negative rewards sit below it."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, T, V1)) * scale).astype(np.float32)
    seq = rng.integers(1, V1, (B, T)).astype(np.int64)
    if T > 1:
        seq[0, T // 2:] = 0                                   # END at T // 2, zeros after it
    if B > 1:
        seq[1, :] = 0                                         # draws 0 first: only step 0 is scored
    if B > 2 and T > 1:
        seq[2, 1] = V1 + 5                                    # clamped to class 0, still m0 = 1
    reward = (rng.standard_normal((B, T)) * 1.5).astype(np.float32)
    reward[:, 0] = np.abs(reward[:, 0]) + 0.25                # every row has a positive reward somewhere
    reward[B - 1, T - 1] = 0.0
    base = rl_logits(x, seq, reward)
    target = np.array([0.5, 1.0, 1.5])[(np.arange(B * T).reshape(B, T)) % 3]
    with np.errstate(invalid='ignore', divide='ignore'):
        old = np.where(reward > 0, base['tok_lp'] - np.log(target / reward.astype(np.float64)), base['tok_lp'] + 0.1)
    return dict(x=x, seq=seq, reward=reward, old=old.astype(np.float32))


def mixed_score(cider, bleu, B, cider_weight=1.0, bleu4_weight=0.0):
    """s[r] = ((bleu4 * bleu4_weight) + (cider * cider_weight)) + 0.0; a missing scorer is the reference's 0 * weight."""
    out = np.empty(B, dtype=np.float64)
    for r in range(B):
        sb = np.float64(bleu[r][3]) if bleu is not None else np.float64(0.0)
        sc = np.float64(cider[r]) if cider is not None else np.float64(0.0)
        out[r] = (sb * np.float64(bleu4_weight) + sc * np.float64(cider_weight)) + 0.0
    return out


def distinct_reward(cider, bleu, weight, n, T, cider_weight=1.0, bleu4_weight=0.0, baseline='weighted'):
    """weight (B,) or (B / n, n) float64 importance weights, rows image-major -> (B, T) float64 (q_j * (s_j - base)) * n over the
    rows with w > 0 (j ascending); rows with w <= 0 or NaN, images without a weighted row or with a non-finite weight sum: 0.0."""
    assert (cider is not None or bleu is not None) and baseline in ('weighted', 'none')
    w = np.asarray(weight, dtype=np.float64).reshape(-1)
    B = w.shape[0]
    assert n >= 1 and B % n == 0
    if baseline == 'weighted' and n < 3:
        raise ValueError('the weighted baseline needs n >= 3')
    with np.errstate(invalid='ignore', over='ignore'):
        s = mixed_score(cider, bleu, B, cider_weight, bleu4_weight)
        out = np.zeros((B, T), dtype=np.float64)
        for k0 in range(0, B, n):
            live = [k0 + i for i in range(n) if w[k0 + i] > 0.0]
            wsum = np.float64(0.0)
            for r in live:
                wsum = wsum + w[r]
            if not live or not np.isfinite(wsum):
                continue
            base = np.float64(0.0)
            if baseline == 'weighted':
                for r in live:
                    base = base + (w[r] / wsum) * s[r]
            for r in live:
                out[r, :] = ((w[r] / wsum) * (s[r] - base)) * np.float64(n)
    return out
