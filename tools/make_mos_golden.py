"""Generate the mixture-of-softmaxes golden (tests/golden/mos_ref.npz) by running the reference's own MixtureOfSoftmax module.

Usage (where the reference checkout exists; RFN_REFERENCE, default /root/reference):
    python tools/make_mos_golden.py            # (re)write the golden
    python tools/make_mos_golden.py --check    # regenerate in memory, compare with the committed file byte for byte

Two tiers, stored under the prefixes t0. and t1.:
  t0   rows 5, R = E = 24, K = 3,  V1 = 37
  t1   rows 4, R = E = 32, K = 10, V1 = 301   (the reference's default expert count)
Per tier: the module's state_dict (its own keys: prior.weight, latent.k.0.weight / .bias, decoder.weight / .bias), the hidden
rows `h`, and `prob`, the module's float32 output (probabilities, misc/MixtureOfSoftmax.py:23-34).  The weights come from
tests/mos_cpu.random_params and are loaded into the module with load_state_dict, so the file also pins the key names and shapes.
Data only; a few tens of KB.  Fixed zip timestamps: a rerun reproduces the file byte for byte.
"""
import argparse
import io
import os
import sys
import warnings
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('RFN_REFERENCE', '/root/reference')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'mos_ref.npz')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import mos_cpu as MC  # noqa: E402

TIERS = [dict(rows=5, R=24, K=3, V1=37, seed=101), dict(rows=4, R=32, K=10, V1=301, seed=202)]


def build():
    sys.path.insert(0, REF)
    from misc.MixtureOfSoftmax import MixtureOfSoftmax
    out = {}
    for i, t in enumerate(TIERS):
        R = E = t['R']
        P = MC.random_params(R, E, t['K'], t['V1'], t['seed'])
        h = torch.randn(t['rows'], R, generator=torch.Generator().manual_seed(t['seed'] + 1))
        mod = MixtureOfSoftmax(R, E, t['K'], t['V1'])
        assert list(mod.state_dict().keys()) == MC.param_names(t['K'])
        mod.load_state_dict(P)
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter('ignore')          # F.softmax without dim: dim 1 of a 2-D input
            prob = mod(h)
        assert prob.dtype == torch.float32 and prob.shape == (t['rows'], t['V1'])
        for k, v in mod.state_dict().items():
            out['t%d.%s' % (i, k)] = v.numpy()
        out['t%d.h' % i] = h.numpy()
        out['t%d.prob' % i] = prob.numpy()
    return out


def npz_bytes(arrays):
    """An .npz with fixed member timestamps (np.savez stamps the current time)."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, 'w', zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            a = io.BytesIO()
            np.lib.format.write_array(a, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, a.getvalue())
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--check', action='store_true', help='compare with the committed golden instead of writing it')
    args = ap.parse_args()
    data = npz_bytes(build())
    assert len(data) < 1 << 20, len(data)
    if args.check:
        same = os.path.exists(GOLDEN) and open(GOLDEN, 'rb').read() == data
        print('%s %s' % (os.path.relpath(GOLDEN, ROOT), 'identical' if same else 'DIFFERS'))
        sys.exit(0 if same else 1)
    with open(GOLDEN, 'wb') as f:
        f.write(data)
    print('wrote %s (%d bytes)' % (os.path.relpath(GOLDEN, ROOT), len(data)))


if __name__ == '__main__':
    main()
