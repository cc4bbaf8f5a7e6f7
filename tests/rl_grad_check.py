"""Helpers of the self-critical RL gradient checks (not a test module; exercised on the CPU by tests/test_rl_oracle_cpu.py and
used on the GPU by tests/test_rl_grads_gpu.py): the element-wise comparison of two gradient dicts, and the RL inputs of a
golden tier.

`compare_grads(got, want, bar)` compares EVERY element of EVERY tensor: the key sets must be equal, shapes must match,
nothing may be non-finite, and per tensor max|got - want| <= bar(want tensor).  It returns a report (the worst err / bar
ratio with the tensor name, the flat index and the value pair of that element) and, with `check=True`, raises an
AssertionError that names them.  Everything is compared in fp64 on the CPU."""
import numpy as np
import torch


def grad_bar(g):
    """The project's gradient bar (tests/test_model_gpu.py): 1e-5 + 1e-3 * max|g_oracle| per tensor."""
    return 1e-5 + 1e-3 * float(g.detach().abs().max())


def _cpu64(t):
    return torch.as_tensor(t).detach().double().cpu()


def compare_grads(got, want, bar=grad_bar, check=True):
    """-> dict(ratio, name, index, got, want, err, bar, failures): `failures` lists every finding as text."""
    failures = []
    only_got, only_want = sorted(set(got) - set(want)), sorted(set(want) - set(got))
    if only_got:
        failures.append('tensors without a reference: %s' % only_got)
    if only_want:
        failures.append('tensors missing from the result: %s' % only_want)
    worst = dict(ratio=-1.0, name=None, index=None, got=None, want=None, err=None, bar=None)
    for k in sorted(set(got) & set(want)):
        if got[k] is None or want[k] is None:
            failures.append('%s: no gradient on %s' % (k, 'the result' if got[k] is None else 'the reference'))
            continue
        a, b = _cpu64(got[k]), _cpu64(want[k])
        if tuple(a.shape) != tuple(b.shape):
            failures.append('%s: shape %s, reference %s' % (k, tuple(a.shape), tuple(b.shape)))
            continue
        if not bool(torch.isfinite(a).all()) or not bool(torch.isfinite(b).all()):
            failures.append('%s: non-finite values' % k)
            continue
        if a.numel() == 0:
            continue
        tol = float(bar(b))
        diff = (a - b).abs().reshape(-1)
        i = int(diff.argmax())
        err = float(diff[i])
        ratio = err / tol
        if ratio > worst['ratio']:
            idx = tuple(int(x) for x in np.unravel_index(i, tuple(b.shape)))
            worst = dict(ratio=ratio, name=k, index=idx, got=float(a.reshape(-1)[i]), want=float(b.reshape(-1)[i]), err=err,
                         bar=tol)
        if err > tol:
            idx = tuple(int(x) for x in np.unravel_index(i, tuple(b.shape)))
            failures.append('%s%s: got %.9g, want %.9g, |diff| %.3g > bar %.3g' % (
                k, list(idx), float(a.reshape(-1)[i]), float(b.reshape(-1)[i]), err, tol))
    worst['failures'] = failures
    if check and failures:
        raise AssertionError('%d finding(s); worst element %s%s got %r want %r (err / bar = %.3g)\n  ' % (
            len(failures), worst['name'], list(worst['index'] or ()), worst['got'], worst['want'], worst['ratio'])
            + '\n  '.join(failures[:20]))
    return worst


RL_TIERS = ('tiny0', 'tiny1', 'tinymax', 'odd', 'mid', 'c2', 'evalmid')


def fed_from_raw(raw):
    """The golden `rl_raw_ids` (B, seq_length) are the unmasked draws; the token matrix the pass fed has BOS in front."""
    raw = torch.as_tensor(raw).long()
    return torch.cat([torch.zeros(raw.size(0), 1, dtype=torch.long), raw], 1)


def load_rl_case(name):
    """(cfg, P, fc, att, top, gold) of a tier's self-critical section (oracle/make_golden.py rl_section): the tier's own rows,
    or -- decode tiers -- one row per image of the seq_per_img-replicated caption batch (train_rl.py samples per image)."""
    from conftest import load_case
    cfg, spec, P, batch, gold = load_case(name)
    fc, att, labels, masks, top = batch
    if 'decode' in spec:
        spi = spec['decode']['spi']
        rows = torch.arange(len(fc[0]) // spi) * spi
        fc, att, top = [f[rows].contiguous() for f in fc], [a[rows].contiguous() for a in att], top[rows]
    return cfg, P, fc, att, top, gold
