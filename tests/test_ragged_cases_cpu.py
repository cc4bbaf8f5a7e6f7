"""Ragged attention maps, the parts that need no GPU: the fp64 restatement of masked attention (tests/ragged_cases.py) equals
plain attention on truncated inputs; the case table of the kernel sweep reaches what it is meant to reach; the new entries are
declared in rfn.h, exported and bound, and the ABI version did not move; host-side validation of `att_lens`."""
import inspect
import os
import re

import pytest
import torch

import ragged_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def native():
    import recurrent_fusion_network_amd._native as N
    return N


def tiny_model():
    import recurrent_fusion_network_amd as R
    from oracle import rfn_oracle as O
    info = [dict(att_num=7, att_feat_size=8, fc_feat_size=8), dict(att_num=12, att_feat_size=12, fc_feat_size=12)]
    cfg = O.make_cfg(info, vocab_size=50, rnn_size=16, input_encoding_size=16, att_hid_size=16, num_review_steps_0=3,
                     num_review_steps=3, top_words_count=20, seq_length=5)
    return cfg, R.RecurrentFusionModel(cfg)


# ---- the fp64 restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c['name'] for c in RC.CASES])
def test_masked_attention_is_plain_attention_on_the_truncated_rows(name):
    c = RC.CASE_BY_NAME[name]
    for gi, o in enumerate(RC.fill_padding(c, RC.operands(c), 1e4)):
        lens = [RC.n_of(c, gi, b) for b in range(c['B'])]
        alpha, z, dproj, dhp, dw = RC.masked_attention(o['proj'], o['hproj'], o['w'], o['bo'], o['x'], o['dz'], lens)
        for b, n in enumerate(lens):
            ra, rz, rdp, rdh, rdw = RC.plain_attention(o['proj'][b, :n], o['hproj'][b], o['w'], o['bo'], o['x'][b, :n], o['dz'][b])
            assert float((alpha[b, :n] - ra).abs().max()) < 1e-14
            assert float((z[b] - rz).abs().max()) < 1e-12
            assert float((dproj[b, :n] - rdp).abs().max()) < 1e-12
            assert float((dhp[b] - rdh).abs().max()) < 1e-12 and float((dw[b] - rdw).abs().max()) < 1e-12
            assert float(alpha[b, n:].abs().sum()) == 0.0 and float(dproj[b, n:].abs().sum()) == 0.0
            assert abs(float(alpha[b].sum()) - 1.0) < 1e-14


def test_masked_attention_ignores_the_padding():
    c = RC.CASE_BY_NAME['het']
    a = RC.fill_padding(c, RC.operands(c), 0.0)
    b = RC.fill_padding(c, RC.operands(c), 1e4)
    for gi in range(len(a)):
        lens = [RC.n_of(c, gi, i) for i in range(c['B'])]
        ra = RC.masked_attention(*[a[gi][k] for k in ('proj', 'hproj', 'w', 'bo', 'x', 'dz')], lens)
        rb = RC.masked_attention(*[b[gi][k] for k in ('proj', 'hproj', 'w', 'bo', 'x', 'dz')], lens)
        for x, y in zip(ra, rb):
            assert torch.equal(x, y)


# ---- the case table -----------------------------------------------------------------------------------------------
def test_case_table_reaches_every_path():
    by = RC.CASE_BY_NAME
    assert len(by) == len(RC.CASES)
    # the two instantiations at the issue's shapes and lengths
    assert (by['vec']['B'], by['vec']['maps'], by['vec']['A'], by['vec']['lens']) == (3, [(9, 8)], 8, [[9, 1, 5]])
    assert (by['scalar']['B'], by['scalar']['maps'], by['scalar']['A'], by['scalar']['lens']) == (3, [(9, 6)], 6, [[9, 1, 5]])
    for c in RC.CASES:
        vec = c['A'] % 4 == 0 and all(D % 4 == 0 for _, D in c['maps'])
        scalar = c['A'] % 4 != 0 and all(D % 4 != 0 for _, D in c['maps'])
        assert vec != scalar, c['name']            # never half and half: the all-or-nothing rule would hide one of them
        for gi, v in enumerate(c['lens']):
            assert v is None or all(1 <= n <= c['maps'][gi][0] for n in v)
    # score blocks wholly past a length: L = 2 * SC_ROWS + 1 has three blocks; the lengths leave 2, 2, 1 and 0 of them idle
    for name in ('score_blocks_vec', 'score_blocks_scalar'):
        c = by[name]
        L = c['maps'][0][0]
        assert L == 2 * RC.SC_ROWS + 1 and c['lens'][0] == [RC.SC_ROWS - 1, RC.SC_ROWS, RC.SC_ROWS + 1, L]
        idle = [sum(1 for blk in range(-(-L // RC.SC_ROWS)) if blk * RC.SC_ROWS >= n) for n in c['lens'][0]]
        assert idle == [2, 2, 1, 0]
    # the unroll and the row-group tails, in the first sweep and in the second
    for name in ('mod4_vec', 'mod4_scalar'):
        assert sorted(n % RC.CTX_UNROLL for n in by[name]['lens'][0]) == [0, 1, 2, 3]
        assert sorted(n % RC.DAL_GROUP for n in by[name]['lens'][0]) == [0, 1, 2, 3]
    sw = by['second_sweep']['lens'][0]
    assert all(n >= RC.SWEEP for n in sw) and {n % RC.DAL_GROUP for n in sw} == {0, 1, 2, 3}
    # two context blocks: 1024 columns per block with 16-byte loads, 256 scalar
    assert by['two_ctx_blocks_vec']['maps'][0][1] > 1024 and by['two_ctx_blocks_scalar']['maps'][0][1] > 256
    # heterogeneous maps (7, 8) and (12, 12), lengths on the first, a NULL entry on the second
    assert by['het']['maps'] == [(7, 8), (12, 12)] and by['het']['lens'][0] is not None and by['het']['lens'][1] is None
    # every case has a full row and a short one somewhere; len = 1 is covered
    assert any(1 in v for c in RC.CASES for v in c['lens'] if v is not None)
    # small enough to run in well under a second each
    assert all(c['B'] * L * max(c['A'], D) <= 1 << 16 for c in RC.CASES for L, D in c['maps'])


# ---- the ABI ------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_exported_and_bound():
    N = native()
    src = open(os.path.join(ROOT, 'include', 'rfn.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(rfn_[a-z0-9_]+)\s*\(', src))
    for s in RC.NEW_SYMBOLS:
        assert s in declared, '%s is not declared in rfn.h' % s
        assert hasattr(N.lib, s), 'librfn_hip.so does not export %s' % s
        assert s in N.EXPORTS, '_native.py does not bind %s' % s
        assert getattr(N.lib, s).argtypes is not None
    # the _het signatures plus one pointer; the prefix entries plus one pointer
    for new, old in (('rfn_attn_fwd_ragged', 'rfn_attn_fwd_het'), ('rfn_attn_bwd_ragged', 'rfn_attn_bwd_het'),
                     ('rfn_prefix_fwd_ex', 'rfn_prefix_fwd'), ('rfn_prefix_fwd_from_state_ex', 'rfn_prefix_fwd_from_state'),
                     ('rfn_prefix_bwd_ex', 'rfn_prefix_bwd')):
        a, b = getattr(N.lib, new).argtypes, getattr(N.lib, old).argtypes
        assert len(a) == len(b) + 1 and list(a[:len(b) - 1]) == list(b[:-1])


def test_abi_version_did_not_move():
    N = native()
    assert N.lib.rfn_abi_version() == 9 and N.ABI_VERSION == 9
    assert re.search(r'#define\s+RFN_ABI_VERSION\s+9\b', open(os.path.join(ROOT, 'include', 'rfn.h')).read())


def test_entry_points_take_the_keyword():
    import recurrent_fusion_network_amd as R
    from recurrent_fusion_network_amd.ensemble import EnsembleDecoder
    from recurrent_fusion_network_amd.graphed import GraphedTrainStep
    for cls, names in ((R.RecurrentFusionModel, RC.ATT_LENS_METHODS), (EnsembleDecoder, RC.ENSEMBLE_METHODS)):
        for name in names:
            p = inspect.signature(getattr(cls, name)).parameters
            assert 'att_lens' in p and p['att_lens'].default is None, '%s.%s' % (cls.__name__, name)
    # positional use is unchanged: the keyword comes last
    for name in RC.ATT_LENS_METHODS:
        assert list(inspect.signature(getattr(R.RecurrentFusionModel, name)).parameters)[-1] == 'att_lens'
    assert 'att_lens' in inspect.signature(GraphedTrainStep.__init__).parameters


# ---- host-side validation --------------------------------------------------------------------------------------------
def test_att_lens_forms():
    N = native()
    L = [7, 12]
    assert N.att_lens_arg(None, L, 3, 'cpu') is None
    assert N.att_lens_arg([None, None], L, 3, 'cpu') is None
    one = N.att_lens_arg([7, 1, 4], L, 3, 'cpu')                    # one vector for every encoder
    assert len(one) == 2 and all(v.dtype == torch.int32 and v.tolist() == [7, 1, 4] for v in one)
    one = N.att_lens_arg(torch.tensor([7, 1, 4]), L, 3, 'cpu')
    assert [v.tolist() for v in one] == [[7, 1, 4], [7, 1, 4]]
    per = N.att_lens_arg([[7, 1, 4], None], L, 3, 'cpu')            # per encoder, None = a full map
    assert per[0].tolist() == [7, 1, 4] and per[1] is None
    per = N.att_lens_arg([torch.tensor([7, 1, 4], dtype=torch.int16), (12, 5, 9)], L, 3, 'cpu')
    assert per[0].dtype == torch.int32 and per[1].tolist() == [12, 5, 9]


@pytest.mark.parametrize('bad, words', [
    ([[7, 0, 4], None], ['att_lens[0][1]', '= 0', 'encoder 0', 'image 1']),                  # a length of 0
    ([None, [12, 5, 13]], ['att_lens[1][2]', '= 13', '<= 12', 'encoder 1', 'image 2']),      # a length of L + 1
    ([8, 1, 4], ['att_lens[0][0]', '= 8', '<= 7']),                                          # one vector: checked per encoder
    ([[7, 1], None], ['att_lens[0]', '2 entries', '3 images']),                              # a wrong batch size
    ([[7, 1, 4], None, None], ['3 entries', '2 encoders']),                                  # a list of the wrong length
    ([[7.0, 1.0, 4.0], None], ['integer']),
])
def test_host_validation_errors(bad, words):
    N = native()
    with pytest.raises(ValueError) as e:
        N.att_lens_arg(bad, [7, 12], 3, 'cpu')
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_model_validates_before_any_native_call():
    """The model's entry points reach the same check first: CPU tensors never get as far as the library."""
    cfg, model = tiny_model()
    from oracle import rfn_oracle as O
    fc, att, labels, masks, top = O.synthetic_batch(cfg, 3, seed=1)
    with pytest.raises(ValueError, match=r'encoder 0, image 1'):
        model(fc, att, labels, att_lens=[[7, 0, 4], None])
    with pytest.raises(ValueError, match=r'encoder 1, image 0'):
        model.sample(fc, att, {'sample_max': 1}, att_lens=[None, [13, 5, 9]])
    with pytest.raises(ValueError, match=r'3 images'):
        model.score(fc, att, labels[:, 1:], att_lens=[7, 1])
    with pytest.raises(ValueError, match=r'2 encoders'):
        model.get_thought_vectors(fc, att, att_lens=[[7, 1, 4]] * 3)
    N = native()
    model.path_flags = N.PATH_OPT_PERSIST_S2_FWD
    with pytest.raises(N.RfnError, match='RFN_PATH_OPT_PERSIST_S2_FWD'):
        model(fc, att, labels, att_lens=[7, 1, 4])


def test_graphed_step_refuses_att_lens():
    N = native()
    from recurrent_fusion_network_amd.graphed import GraphedTrainStep
    with pytest.raises(N.RfnError, match='att_lens'):
        GraphedTrainStep(None, None, None, None, None, None, None, None, att_lens=[7, 1, 4])
    step = GraphedTrainStep.__new__(GraphedTrainStep)      # an unbuilt step: the refusal comes before anything else
    with pytest.raises(N.RfnError, match='att_lens'):
        step(att_lens=[7, 1, 4])
