"""The mixture-of-softmaxes head (include/rfn.h, "mixture of softmaxes") restated in torch fp64 on the CPU: forward in the
log-sum-exp form, the hand-written backward of the header, and the loss form.  The GPU tests compare the kernels against this;
tests/test_mos_cpu.py compares this against the reference module's recorded output and against autograd.

Parameters travel as a dict under the reference's state_dict names (misc/MixtureOfSoftmax.py): prior.weight (K, R),
latent.k.0.weight (E, R), latent.k.0.bias (E), decoder.weight (V1, E), decoder.bias (V1)."""
import numpy as np
import torch


def param_names(K):
    out = ['prior.weight']
    for k in range(K):
        out += ['latent.%d.0.weight' % k, 'latent.%d.0.bias' % k]
    return out + ['decoder.weight', 'decoder.bias']


def n_experts(P):
    return P['prior.weight'].shape[0]


def as64(P):
    return {k: torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).double() for k, v in P.items()}


def random_params(R, E, K, V1, seed, logit_std=3.0):
    """Weights that give expert logits of standard deviation ~ logit_std (mostly through the decoder bias, so that the
    scale does not depend on E) and prior logits of order one."""
    g = torch.Generator().manual_seed(seed)
    P = {'prior.weight': torch.randn(K, R, generator=g) / R ** 0.5}
    for k in range(K):
        P['latent.%d.0.weight' % k] = torch.randn(E, R, generator=g) / R ** 0.5
        P['latent.%d.0.bias' % k] = torch.randn(E, generator=g) * 0.1
    P['decoder.weight'] = torch.randn(V1, E, generator=g) * (0.5 * logit_std / E ** 0.5)
    P['decoder.bias'] = torch.randn(V1, generator=g) * logit_std
    return P


def forward_parts(P, h):
    """c (rows, K), log pi (rows, K), z (K, rows, E), x (K, rows, V1), lse (K, rows), logp (rows, V1), all fp64."""
    P, h = as64(P), h.double()
    K = n_experts(P)
    c = h @ P['prior.weight'].t()
    logpi = c - torch.logsumexp(c, 1, keepdim=True)
    z = torch.stack([torch.tanh(h @ P['latent.%d.0.weight' % k].t() + P['latent.%d.0.bias' % k]) for k in range(K)])
    x = z @ P['decoder.weight'].t() + P['decoder.bias']
    lse = torch.logsumexp(x, 2)
    a = logpi.t().unsqueeze(2) + x - lse.unsqueeze(2)
    return dict(c=c, logpi=logpi, z=z, x=x, lse=lse, a=a, logp=torch.logsumexp(a, 0))


def log_prob(P, h):
    return forward_parts(P, h)['logp']


def backward(P, h, G):
    """The header's backward from G = dL / dlogp (rows, V1): dx (K, rows, V1), dc (rows, K), d_h (rows, R) and the parameter
    gradients under their names."""
    P64, h = as64(P), h.double()
    G = G.double()
    f = forward_parts(P, h)
    K = n_experts(P)
    r = torch.exp(f['a'] - f['logp'].unsqueeze(0))
    p = torch.exp(f['x'] - f['lse'].unsqueeze(2))
    s = (G.unsqueeze(0) * r).sum(2)                        # (K, rows)
    dx = G.unsqueeze(0) * r - p * s.unsqueeze(2)
    pi = torch.exp(f['logpi'])
    dc = s.t() - pi * s.sum(0).unsqueeze(1)
    dz = dx @ P64['decoder.weight']
    du = dz * (1.0 - f['z'] ** 2)
    grads = {'prior.weight': dc.t() @ h,
             'decoder.weight': torch.einsum('krv,kre->ve', dx, f['z']),
             'decoder.bias': dx.sum((0, 1))}
    d_h = dc @ P64['prior.weight']
    for k in range(K):
        grads['latent.%d.0.weight' % k] = du[k].t() @ h
        grads['latent.%d.0.bias' % k] = du[k].sum(0)
        d_h = d_h + du[k] @ P64['latent.%d.0.weight' % k]
    return dict(dx=dx, dc=dc, d_h=d_h, grads=grads)


def smoothed_targets(target, V1, eps):
    """q (rows..., V1): eps / V1 everywhere plus (1 - eps) at the target; ids outside [0, V1) read as 0 (rfn_xe_logits_*)."""
    tg = target.clone()
    tg[(tg < 0) | (tg >= V1)] = 0
    q = torch.full(tuple(tg.shape) + (V1,), eps / V1, dtype=torch.float64)
    q.scatter_add_(-1, tg.unsqueeze(-1), torch.full(tuple(tg.shape) + (1,), 1.0 - eps, dtype=torch.float64))
    return q


def loss(P, h_tm, B, T, target, mask, eps):
    """The masked, label-smoothed NLL of time-major rows h_tm (T * B, R): -sum mask * q . logp / B (misc/utils.py:163-184)."""
    logp = log_prob(P, h_tm).view(T, B, -1).transpose(0, 1)                     # (B, T, V1)
    q = smoothed_targets(target[:, :T], logp.shape[2], eps)
    return -(mask[:, :T].double().unsqueeze(2) * q * logp).sum() / B


def loss_G(B, T, V1, target, mask, eps, g=1.0):
    """dL / dlogp of the loss form for time-major rows: (T * B, V1)."""
    q = smoothed_targets(target[:, :T], V1, eps)
    G = -(g / B) * mask[:, :T].double().unsqueeze(2) * q                         # (B, T, V1)
    return G.transpose(0, 1).reshape(T * B, V1)
