"""GPU: diverse beam search (include/rfn.h "diverse beam search"): rfn_beam_step_div against the NumPy restatement
(tests/diverse_beam_cpu.py) over whole synthetic searches, lambda = 0 against the plain step kernel, and the device loop of
the model and the ensembles against a search stepped from the host whose bookkeeping is the full-row restatement.

Everything is exact: ids equal, log-probs bit-equal.  The step selects and copies, and its only arithmetic (p, and the
penalised key) is stated operation by operation in fp32, so there is no tolerance to derive."""
import numpy as np
import pytest
import torch

import decode_constraints_cpu as D
import diverse_beam_cpu as Dv
import test_decode_constraints_gpu as T

pytestmark = pytest.mark.gpu
bits, same, beams_of = T.bits, T.same, T.beams_of


def nat():
    import recurrent_fusion_network_amd._native as N
    return N


# =================================================================================================================
# the step kernel
# =================================================================================================================
class DevBeams:
    """The arrays rfn_beam_step_div / rfn_beam_step_topk update, for NB images of W beams."""

    def __init__(self, NB, W, S, dev):
        self.NB, self.W, self.S, self.max_done = NB, W, S, W * S
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731
        self.bs, self.bl, self.bsum = z(S, NB, W, dt=torch.long), z(S, NB, W), z(NB, W)
        self.order, self.ids = z(NB * W, dt=torch.int32), z(NB * W, dt=torch.long)
        self.done_seq, self.done_lp = z(NB, self.max_done, S, dt=torch.long), z(NB, self.max_done, S)
        self.done_p, self.done_n = z(NB, self.max_done), z(NB, dt=torch.int32)
        self.done_group = torch.full((NB, self.max_done), -1, dtype=torch.int32, device=dev)
        self.active = torch.ones(NB, dtype=torch.int32, device=dev)

    def step_div(self, N, topv, topi, V1, G, lam, t):
        N.check(N.lib.rfn_beam_step_div(topv.data_ptr(), topi.data_ptr(), V1, self.W, G, lam, self.S, t, self.NB, self.max_done,
                                        self.bs.data_ptr(), self.bl.data_ptr(), self.bsum.data_ptr(), self.order.data_ptr(),
                                        self.ids.data_ptr(), self.done_seq.data_ptr(), self.done_lp.data_ptr(), self.done_p.data_ptr(),
                                        self.done_n.data_ptr(), self.done_group.data_ptr(), self.active.data_ptr(), N.stream_ptr()),
                'rfn_beam_step_div')

    def step_topk(self, N, topv, topi, V1, t):
        N.check(N.lib.rfn_beam_step_topk(topv.data_ptr(), topi.data_ptr(), V1, self.W, self.S, t, self.NB, self.max_done,
                                         self.bs.data_ptr(), self.bl.data_ptr(), self.bsum.data_ptr(), self.order.data_ptr(),
                                         self.ids.data_ptr(), self.done_seq.data_ptr(), self.done_lp.data_ptr(), self.done_p.data_ptr(),
                                         self.done_n.data_ptr(), self.active.data_ptr(), N.stream_ptr()), 'rfn_beam_step_topk')

    def state(self):
        return [bits(x) if x.is_floating_point() else x.cpu() for x in (self.bs, self.bl, self.bsum, self.order, self.ids, self.active)]

    def done(self, k):
        """Image k's done beams in construction order: (ids, log-prob bits, p bits, group)."""
        n = int(self.done_n[k])
        seq, lp, p, g = self.done_seq[k, :n].cpu(), bits(self.done_lp[k, :n]), bits(self.done_p[k, :n]), self.done_group[k, :n].cpu()
        return [(seq[i].tolist(), lp[i].tolist(), int(p[i]), int(g[i])) for i in range(n)]


def top_lists(rows, W, dev):
    """(NB, W, V1) log-prob rows -> the (NB * W, W) top lists rfn_log_softmax_topk would hand the step (value descending, token
    ascending); with V1 < W the columns past V1 hold a poison the step must not read."""
    NB, _, V1 = rows.shape
    ys, ix = Dv.sorted_rows(rows.reshape(NB * W, V1), min(W, V1))
    tv, ti = np.full((NB * W, W), np.nan, dtype=np.float32), np.full((NB * W, W), -7, dtype=np.int32)
    tv[:, :ys.shape[1]], ti[:, :ix.shape[1]] = ys, ix
    return torch.from_numpy(tv).to(dev), torch.from_numpy(ti).to(dev)


def i32(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


def want_done(b):
    return [([int(x) for x in d['seq']], i32(d['logps']).tolist(), int(i32([d['p']])[0]), d['group']) for d in b.done]


SHAPES = [(2, 2), (4, 2), (6, 3), (6, 6), (12, 4), (32, 2), (32, 8), (32, 32)]


@pytest.mark.parametrize('W,G', SHAPES)
def test_step_kernel_matches_the_restatement(dev, W, G):
    """Whole synthetic searches, the state carried from step to step on the device and in the restatement (which reads FULL
    rows): after every step order, next_ids, active and the beam arrays, at the end the done beams with their groups."""
    N = nat()
    for NB in (1, 3):
        for S in (1, 4, 17):
            for V1 in (W, 37):
                rows = Dv.synthetic_rows(10000 * W + 100 * G + 10 * NB + S + V1, NB, W, S, V1)
                lists = [top_lists(r, W, dev) for r in rows]
                final = {}
                for lam in (0.0, 0.5, 1e30):
                    d = DevBeams(NB, W, S, dev)
                    ref = [Dv.Beams(W, S) for _ in range(NB)]
                    for t in range(1, S + 1):
                        d.step_div(N, lists[t - 1][0], lists[t - 1][1], V1, G, lam, t)
                        for k in range(NB):
                            Dv.step(ref[k], rows[t - 1][k], t, G, lam)
                        got = d.state()
                        where = (NB, S, V1, lam, t)
                        assert got[0].permute(1, 0, 2).tolist() == [b.seq.tolist() for b in ref], where
                        assert got[1].permute(1, 0, 2).tolist() == [i32(b.lp).tolist() for b in ref], where
                        assert got[2].tolist() == [i32(b.sum).tolist() for b in ref], where
                        assert got[3].view(NB, W).tolist() == [(k * W + b.order).tolist() for k, b in enumerate(ref)], where
                        assert got[4].view(NB, W).tolist() == [b.next_ids.tolist() for b in ref], where
                        assert got[5].tolist() == [int(b.active) for b in ref], where
                    for k in range(NB):
                        assert d.done(k) == want_done(ref[k]), (NB, S, V1, lam, k)
                    assert (d.done_group.cpu()[torch.arange(d.max_done)[None, :] >= d.done_n.cpu()[:, None]] == -1).all()
                    final[lam] = [(b.seq.tolist(), want_done(b)) for b in ref]
                assert final[0.5] != final[0.0] and final[1e30] != final[0.0], (NB, S, V1)   # the penalty changed the search


def test_some_case_has_an_inert_group_beside_a_live_one():
    """Non-vacuity of the stopping rule, asserted on the restatement alone: on rows of the kernel test above some image has a
    group without candidates while another group of it goes on."""
    inert = 0
    for W, G in SHAPES[:5]:
        NB, S, V1 = 3, 17, 37
        rows = Dv.synthetic_rows(10000 * W + 100 * G + 10 * NB + S + V1, NB, W, S, V1)
        ref = [Dv.Beams(W, S) for _ in range(NB)]
        for t in range(1, S + 1):
            for k in range(NB):
                Dv.step(ref[k], rows[t - 1][k], t, G, 0.5)
        inert += sum(len(b.inert_groups) > 0 for b in ref)
    assert inert > 0


@pytest.mark.parametrize('W,G', SHAPES)
def test_lambda_zero_is_the_plain_kernel_per_group(dev, W, G):
    """The G > 1 kernel at lambda = 0 against rfn_beam_step_topk run at width Wg with every group as an image of its own: the
    rows k * W + g * Wg + j of the one are the rows (k * G + g) * Wg + j of the other, so the beam arrays, order and next_ids
    compare bit for bit as they lie in memory; the done beams compare group by group."""
    N = nat()
    Wg = W // G
    for NB, S, V1 in ((1, 1, W), (3, 4, 37), (3, 17, W), (1, 17, 37)):
        rows = Dv.synthetic_rows(500 * W + G + S + V1, NB, W, S, V1)
        a, b = DevBeams(NB, W, S, dev), DevBeams(NB * G, Wg, S, dev)
        for t in range(1, S + 1):
            tv, ti = top_lists(rows[t - 1], W, dev)
            a.step_div(N, tv, ti, V1, G, 0.0, t)
            b.step_topk(N, tv[:, :Wg].contiguous(), ti[:, :Wg].contiguous(), V1, t)
            for x, y in zip(a.state()[:5], b.state()[:5]):
                assert torch.equal(x.reshape(-1), y.reshape(-1)), (NB, S, V1, t)
            assert a.active.tolist() == b.active.view(NB, G).max(1).values.tolist()
        for k in range(NB):
            mine = a.done(k)
            for g in range(G):
                assert [m[:3] for m in mine if m[3] == g] == [m[:3] for m in b.done(k * G + g)], (NB, S, V1, k, g)


@pytest.mark.parametrize('W', [1, 5, 32])
def test_one_group_forwards_to_the_plain_kernel(dev, W):
    """G == 1 through rfn_beam_step_div, whatever lambda: rfn_beam_step_topk bit for bit, done_group NULL."""
    N = nat()
    NB, S, V1 = 3, 6, 37
    rows = Dv.synthetic_rows(77 + W, NB, W, S, V1)
    a, b = DevBeams(NB, W, S, dev), DevBeams(NB, W, S, dev)
    for t in range(1, S + 1):
        tv, ti = top_lists(rows[t - 1], W, dev)
        N.check(N.lib.rfn_beam_step_div(tv.data_ptr(), ti.data_ptr(), V1, W, 1, 3.0, S, t, NB, a.max_done, a.bs.data_ptr(),
                                        a.bl.data_ptr(), a.bsum.data_ptr(), a.order.data_ptr(), a.ids.data_ptr(),
                                        a.done_seq.data_ptr(), a.done_lp.data_ptr(), a.done_p.data_ptr(), a.done_n.data_ptr(), None,
                                        a.active.data_ptr(), N.stream_ptr()))
        b.step_topk(N, tv, ti, V1, t)
        for x, y in zip(a.state(), b.state()):
            assert torch.equal(x, y), (W, t)
    for k in range(NB):
        assert [m[:3] for m in a.done(k)] == [m[:3] for m in b.done(k)]


# =================================================================================================================
# whole path
# =================================================================================================================
@torch.no_grad()
def host_diverse_beam(models, fc, att, W, G, lam, cons, alpha=0.0):
    """sample_beam stepped from the host: every step's full log-prob rows come back, get the constraints' mask, and the
    full-row restatement does the bookkeeping.  -> (seq (B, S), seq_lp (B, S), done_beams, diverse_beams), the done beams
    as (ids, log-prob bits, p bytes, group) ranked by p / len^alpha, stably."""
    N = nat()
    m0 = models[0]
    B, S, V1 = fc[0].size(0), m0.seq_length, m0.vocab_size + 1
    dev = fc[0].device
    steppers = T._members(models, fc, att, repeat=W)
    rows = B * W
    ref = [Dv.Beams(W, S) for _ in range(B)]
    ids = torch.zeros(rows, dtype=torch.long, device=dev)
    logit_sum, logit_m, logp = (torch.empty(rows, V1, device=dev) for _ in range(3))
    for t in range(S + 1):
        if t >= 1:
            for k in range(B):
                Dv.step(ref[k], masked[k * W:(k + 1) * W], t, G, lam)
            if t == S:
                break
            order = torch.from_numpy(np.concatenate([k * W + b.order for k, b in enumerate(ref)])).to(torch.int32).to(dev)
            ids = torch.from_numpy(np.concatenate([b.next_ids for b in ref])).to(dev)
            for sp in steppers:
                sp.reorder(order)
        T._averaged_logp(N, steppers, ids, logit_sum, logit_m, logp)
        hist = np.concatenate([b.seq[:t].T for b in ref])                       # row k * W + w continues beam (k, w)
        masked = D.mask_rows(logp.cpu().numpy(), hist, t + 1, **cons)
    seq, seq_lp = torch.zeros(B, S, dtype=torch.long), torch.zeros(B, S)
    done_beams, diverse = [], []
    for k, b in enumerate(ref):
        rank = D.rank_done([d['p'] for d in b.done], [D.caption_len(d['seq'], S) for d in b.done], alpha)
        ranked = [b.done[i] for i in rank]
        seq[k], seq_lp[k] = torch.from_numpy(ranked[0]['seq']), torch.from_numpy(ranked[0]['logps'])
        as_tuple = lambda d: (d['seq'].tolist(), i32(d['logps']).tolist(), np.float32(d['p']).tobytes(), d['group'])  # noqa: E731
        done_beams.append([as_tuple(d) for d in ranked])
        diverse.append([next(as_tuple(d) for d in ranked if d['group'] == g) for g in range(G)])
    return seq, seq_lp, done_beams, diverse


def with_groups(done_beams):
    return [[t + (d['group'],) for t, d in zip(img_t, img)] for img_t, img in zip(beams_of(done_beams), done_beams)]


def check_owner(out, owner, want, G, tag):
    assert same(out[0], want[0]) and same(out[1], want[1]), tag
    assert with_groups(owner.done_beams) == want[2], tag
    assert len(owner.diverse_beams) == len(want[3]) and all(len(img) == G for img in owner.diverse_beams), tag
    assert with_groups(owner.diverse_beams) == want[3], tag


CASES = [(4, 2), (6, 3), (5, 5)]


@pytest.mark.parametrize('members', [1, 2])
@pytest.mark.parametrize('name', ['tiny0', 'mid'])
def test_device_loop_equals_the_host_stepped_search(dev, name, members):
    """members = 1: RecurrentFusionModel.sample_beam AND the one-member EnsembleDecoder against the host-stepped search;
    members = 2: the two-member ensemble against it.  lambda = 0.5; once more under block_ngram = 2 and a length penalty."""
    from recurrent_fusion_network_amd.ensemble import EnsembleDecoder
    model, fc, att = T.setup(name, dev)
    models = [model] + [T.setup(name, dev, seed_shift=1)[0]] * (members - 1)
    ens = EnsembleDecoder(models)
    runs = [(W, G, {}) for W, G in CASES] + [(6, 3, {'block_ngram': 2, 'length_penalty': 0.7})]
    for W, G, extra in runs:
        opt = dict(extra, beam_size=W, group_size=G, diversity_lambda=0.5)
        want = host_diverse_beam(models, fc, att, W, G, 0.5, T.cons_of(extra), extra.get('length_penalty', 0.0))
        with torch.no_grad():
            check_owner(ens.sample_beam(fc, att, opt), ens, want, G, (name, members, W, G, 'ensemble'))
            if members == 1:
                check_owner(model.sample_beam(fc, att, opt), model, want, G, (name, W, G, 'model'))
                check_owner(model.sample(fc, att, opt), model, want, G, (name, W, G, 'sample'))


def distinct_group_bests(diverse):
    return sum(len({tuple(d[0]) for d in img}) for img in diverse)


BITE_LAMBDA = 0.5


def test_diversity_bites(dev):
    """Premise: at lambda = 0 the G group bests of an image are as many distinct captions as a plain search of width Wg finds
    best captions -- one; the count over the batch equals the host-stepped G == 1 search's, on the same rows.  Bite: at
    BITE_LAMBDA the count is strictly larger."""
    model, fc, att = T.setup('mid', dev)
    W, G = 6, 3
    plain = host_diverse_beam([model], fc, att, W // G, 1, 0.0, T.cons_of({}))
    base = distinct_group_bests(plain[3])
    assert base == fc[0].size(0)
    with torch.no_grad():
        model.sample_beam(fc, att, {'beam_size': W, 'group_size': G, 'diversity_lambda': 0.0})
        off = sum(len({tuple(d['seq'].tolist()) for d in img}) for img in model.diverse_beams)
        out = model.sample_beam(fc, att, {'beam_size': W, 'group_size': G, 'diversity_lambda': BITE_LAMBDA})
        on = sum(len({tuple(d['seq'].tolist()) for d in img}) for img in model.diverse_beams)
        # every group best is one of the image's done beams, and the returned caption is the best of the group bests
        for k, img in enumerate(model.diverse_beams):
            assert [d['group'] for d in img] == list(range(G))
            assert any(d is model.done_beams[k][0] for d in img) and out[0][k].tolist() == model.done_beams[k][0]['seq'].tolist()
    want = distinct_group_bests(host_diverse_beam([model], fc, att, W, G, BITE_LAMBDA, T.cons_of({}))[3])
    print('distinct group bests over the batch: G == 1 at width Wg %d, lambda 0 %d, lambda %g %d (host-stepped %d)'
          % (base, off, BITE_LAMBDA, on, want))
    assert off == base
    assert on == want and on > base


@pytest.mark.parametrize('name', ['tiny0', 'mid'])
def test_off_equals_today(dev, name):
    """group_size = 1 with any diversity_lambda: sample_beam's tensors and done_beams bit for bit, no 'group' key, no
    diverse_beams -- for the model and for the ensemble."""
    from recurrent_fusion_network_amd.ensemble import EnsembleDecoder
    model, fc, att = T.setup(name, dev)
    for owner in (model, EnsembleDecoder([model])):
        for W in (1, 3, 6):
            with torch.no_grad():
                a = owner.sample_beam(fc, att, {'beam_size': W})
                want = beams_of(owner.done_beams)
                for off in ({'group_size': 1}, {'group_size': 1, 'diversity_lambda': 8.0}, {'group_size': None, 'diversity_lambda': 0.0}):
                    b = owner.sample_beam(fc, att, dict(off, beam_size=W))
                    assert same(a[0], b[0]) and same(a[1], b[1]) and beams_of(owner.done_beams) == want
                    assert list(a[3]) == list(b[3]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
                    assert all('group' not in d for img in owner.done_beams for d in img) and owner.diverse_beams is None


def test_refusals(dev):
    from recurrent_fusion_network_amd.ensemble import EnsembleDecoder
    model, fc, att = T.setup('mid', dev)
    N = nat()
    for owner in (model, EnsembleDecoder([model])):
        for bad in ({'group_size': 0}, {'group_size': -1}, {'group_size': 4}, {'group_size': 2, 'diversity_lambda': -0.1},
                    {'group_size': 2, 'diversity_lambda': float('nan')}):
            with pytest.raises(ValueError), torch.no_grad():
                owner.sample_beam(fc, att, dict(bad, beam_size=6))
    d = DevBeams(1, 6, 4, dev)
    tv, ti = top_lists(Dv.synthetic_rows(1, 1, 6, 1, 37)[0], 6, dev)
    call = lambda G, lam: N.lib.rfn_beam_step_div(tv.data_ptr(), ti.data_ptr(), 37, 6, G, lam, 4, 1, 1, d.max_done, d.bs.data_ptr(),  # noqa: E731
                                                  d.bl.data_ptr(), d.bsum.data_ptr(), d.order.data_ptr(), d.ids.data_ptr(),
                                                  d.done_seq.data_ptr(), d.done_lp.data_ptr(), d.done_p.data_ptr(), d.done_n.data_ptr(),
                                                  d.done_group.data_ptr(), d.active.data_ptr(), N.stream_ptr())
    assert call(4, 0.5) == -1 and call(0, 0.5) == -1 and call(-3, 0.5) == -1 and call(3, -0.5) == -1 and call(3, float('nan')) == -1
    assert int(d.done_n[0]) == 0 and int(d.bs.abs().sum()) == 0                      # nothing ran
