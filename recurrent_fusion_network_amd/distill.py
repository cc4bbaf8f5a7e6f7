"""A compact distillation teacher: the K <= 32 best entries of every teacher row instead of the dense (B, S, V+1) tensor.

`forward_loss(..., teacher=)` takes a dense teacher of 4 * (V+1) bytes per row, too much to keep for a training set; only the
head of a teacher's distribution carries information.  A TopKTeacher holds K (id, log-prob) pairs per row -- 8 * K bytes -- which
can be computed once (TopKTeacher.from_dense, EnsembleDecoder.teacher_topk), stored (state_dict / from_state_dict with torch.save)
and streamed with the features.  forward_loss dispatches on the type to rfn_kd_topk_fwd / _bwd (include/rfn.h): the meaning is
exactly the dense teacher's with -inf off the K ids, i.e. the K entries are renormalised and the tail mass is dropped."""
from __future__ import annotations

import torch

from . import _native as N

MAX_K = 32


class TopKTeacher:
    """ids (B, T, K) int32, logp (B, T, K) float32 on one device, unit stride in the last dimension, any strides in the first
    two (batch-major, or the transposed view of a time-major buffer), 1 <= K <= 32.  Row (b, t) is the K pairs
    (ids[b, t, k], logp[b, t, k]); logp may be logits or log-probs (every loss term is invariant to a per-row shift).  An entry
    whose id is outside [0, V+1) or whose logp is -inf is padding.  The live ids of a row must be distinct and every row that
    the mask keeps needs a live entry: `check(V1)` verifies both (one host synchronisation)."""

    def __init__(self, ids, logp):
        if not torch.is_tensor(ids) or not torch.is_tensor(logp):
            raise ValueError('ids and logp must be tensors, got %s and %s' % (type(ids).__name__, type(logp).__name__))
        if ids.dim() != 3 or logp.dim() != 3 or ids.shape != logp.shape:
            raise ValueError('ids and logp must share one shape (B, T, K), got %s and %s' % (tuple(ids.shape), tuple(logp.shape)))
        if ids.dtype != torch.int32 or logp.dtype != torch.float32:
            raise ValueError('ids must be int32 and logp float32, got dtype %s and %s' % (ids.dtype, logp.dtype))
        if ids.device != logp.device:
            raise ValueError('ids live on device %s, logp on %s' % (ids.device, logp.device))
        K = ids.size(2)
        if not 1 <= K <= MAX_K:
            raise ValueError('K = %d entries per row: 1 <= K <= %d' % (K, MAX_K))
        for name, a in (('ids', ids), ('logp', logp)):
            if K > 1 and a.stride(2) != 1:
                raise ValueError('%s needs unit stride in its last dimension: strides %s' % (name, tuple(a.stride())))
            if any(a.size(d) > 1 and abs(a.stride(d)) < K for d in (0, 1)):
                raise ValueError('%s rows must not overlap: strides %s' % (name, tuple(a.stride())))
        self.ids, self.logp = ids.detach(), logp.detach()

    # ---- shape ---------------------------------------------------------------------------------------------------------
    @property
    def shape(self):
        return self.ids.shape

    @property
    def device(self):
        return self.ids.device

    @property
    def k(self):
        return self.ids.size(2)

    def size(self, d):
        return self.ids.size(d)

    def __len__(self):
        return self.ids.size(0)

    def __repr__(self):
        return 'TopKTeacher(B=%d, T=%d, K=%d, device=%s)' % (tuple(self.ids.shape) + (self.ids.device,))

    # ---- construction --------------------------------------------------------------------------------------------------
    @classmethod
    def from_dense(cls, t, k):
        """The k best entries of every row of a dense teacher `t` -- anything forward_loss accepts as one: (B, T, V+1) f32 logits
        or log-probs on the device, unit stride in the last dimension -- as rfn_log_softmax_topk lists them: the row's
        log-softmax values, ordered (value descending, token ascending).  k <= min(32, V+1).  Rows that do not lie at one
        stride (neither batch-major nor time-major) are made contiguous first."""
        if not torch.is_tensor(t) or t.dim() != 3:
            raise ValueError('a dense teacher is a tensor (B, T, V+1)')
        if t.dtype != torch.float32:
            raise ValueError('the teacher must be float32, got %s' % t.dtype)
        B, T, V1 = t.shape
        k = int(k)
        if not 1 <= k <= min(MAX_K, V1):
            raise ValueError('k = %d: 1 <= k <= min(%d, V+1 = %d)' % (k, MAX_K, V1))
        if not t.is_cuda:
            raise N.RfnError('the teacher must live on the GPU: the HIP path has no CPU fallback')
        t = t.detach()
        sb, st = t.stride(0), t.stride(1)
        if t.stride(2) == 1 and st >= V1 and (sb == T * st or B == 1):
            time_major, ldl = False, st
        elif t.stride(2) == 1 and sb >= V1 and (st == B * sb or T == 1):
            time_major, ldl = True, sb
        else:
            t, time_major, ldl = t.contiguous(), False, V1
        with torch.cuda.device(t.device):
            ids = torch.empty(B * T, k, dtype=torch.int32, device=t.device)
            logp = torch.empty(B * T, k, device=t.device)
            N.check(N.lib.rfn_log_softmax_topk(t.data_ptr(), ldl, B * T, V1, k, logp.data_ptr(), ids.data_ptr(), N.stream_ptr()),
                    'rfn_log_softmax_topk')
        if time_major:
            return cls(ids.view(T, B, k).transpose(0, 1), logp.view(T, B, k).transpose(0, 1))
        return cls(ids.view(B, T, k), logp.view(B, T, k))

    def state_dict(self):
        """Plain contiguous tensors, for torch.save."""
        return {'ids': self.ids.contiguous(), 'logp': self.logp.contiguous()}

    @classmethod
    def from_state_dict(cls, d):
        return cls(d['ids'], d['logp'])

    # ---- moving and slicing --------------------------------------------------------------------------------------------
    def __getitem__(self, rows):
        """The teacher of a subset of the batch rows (a slice, a list or an index tensor)."""
        if isinstance(rows, tuple):
            raise IndexError('a TopKTeacher is indexed by batch rows only')
        if isinstance(rows, int):
            rows = slice(rows, rows + 1 if rows != -1 else None)
        return TopKTeacher(self.ids[rows], self.logp[rows])

    def to(self, device, non_blocking=False):
        return TopKTeacher(self.ids.to(device, non_blocking=non_blocking), self.logp.to(device, non_blocking=non_blocking))

    def cpu(self):
        return TopKTeacher(self.ids.cpu(), self.logp.cpu())

    def pin_memory(self):
        return TopKTeacher(self.ids.contiguous().pin_memory(), self.logp.contiguous().pin_memory())

    # ---- tests and debugging -------------------------------------------------------------------------------------------
    def _live(self, V1):
        return (self.ids >= 0) & (self.ids < V1) & (self.logp != float('-inf'))

    def dense(self, V1):
        """(B, T, V1) float32, contiguous: logp at the live ids, -inf elsewhere -- the dense teacher this one stands for.  For
        tests and debugging; it is the tensor a TopKTeacher exists to avoid."""
        B, T, _ = self.ids.shape
        out = torch.full((B, T, V1 + 1), float('-inf'), device=self.ids.device)
        idx = torch.where(self._live(V1), self.ids, torch.full_like(self.ids, V1)).long()     # padding lands in a spare column
        out.scatter_(2, idx, self.logp)
        return out[:, :, :V1].contiguous()

    def check(self, V1):
        """Raise ValueError if a row has two live entries with one id, or no live entry at all.  One host synchronisation:
        meant for a cache loaded from disk, not for every step."""
        live = self._live(V1)
        K = self.ids.size(2)
        pad = V1 + torch.arange(K, device=self.ids.device)                                    # distinct keys for padding entries
        key = torch.where(live, self.ids.long(), pad.expand_as(self.ids)).sort(2).values
        dup = (key[:, :, 1:] == key[:, :, :-1]).any() if K > 1 else torch.zeros((), dtype=torch.bool, device=self.ids.device)
        empty = (~live.any(2)).any()
        dup, empty = torch.stack([dup, empty]).tolist()
        if dup:
            raise ValueError('a teacher row holds the same live id twice')
        if empty:
            raise ValueError('a teacher row has no live entry (every id outside [0, %d) or every value -inf)' % V1)
        return self

    # ---- the native calls ----------------------------------------------------------------------------------------------
    def _abi(self):
        """(t_ids, i_sb, i_st, t_val, v_sb, v_st, K) as rfn_kd_topk_* take them; a dimension of size 1 is never stepped along,
        so its stride is handed over as K."""
        K = self.ids.size(2)

        def strides(a):
            return tuple(a.stride(d) if a.size(d) > 1 else K for d in (0, 1))
        return (self.ids.data_ptr(),) + strides(self.ids) + (self.logp.data_ptr(),) + strides(self.logp) + (K,)
