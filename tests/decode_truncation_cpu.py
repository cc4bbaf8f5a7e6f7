"""NumPy fp64 restatement of truncated sampling (include/rfn.h "truncated sampling"), shared by the CPU and the
GPU tests, and the generator of the rows both use.

Definition.  x[0 .. V1) log-probs, possibly with -inf entries; w_v = exp(x_v * inv_temp); the order is x descending, then token
id ascending.  top_k = k in (0, V1): the first min(k, number of finite entries) survive.  top_p = p in (0, 1), over the
survivors: with c_j the sum of the first j weights and c_n the sum of all, the first J = min{ j : c_j >= p * c_n } are kept.
A row without finite entry, or with a NaN, is untouched.  Here the order is a stable argsort of -x (ties keep ascending ids),
the weights exp((x - max) * inv_temp) (the common factor cancels) and c = np.cumsum, all in fp64; top_p and inv_temp are rounded
to fp32 first, because that is what the C ABI receives.

The near margin, derived, not measured.  A row is `near` when |c_{J-1} - p c_n| (for J >= 2: no kept set has 0 entries, so c_0 is
no boundary a kernel could stop at) or |c_J - p c_n| is at most NEAR of c_n; on such a row a correct kernel may stop one entry
earlier or later.  For a kernel that sums fp32 __expf weights in blocks of at most 128 per thread and a 256-way tree the margin
would be 1e-4 (sum (128 + 8) * 2^-24 = 8e-6, weight |x| * 2^-24 + 2 ulp, times ten).  But 1e-4 of the total is about the mass of
ONE entry at a top_p = 0.9 cut of a 9488-word row of randn * 3 logits (the entry at the cut weighs 2e-4 of the total), so under
that margin nearly every such row is near and the cap below cannot hold for any kernel.  The kernel (csrc/rfn_pick.hip)
therefore accumulates differently, and the margin is re-derived for it: each weight is exp((x - max) * inv_temp) in fp64,
rounded DOWN to a multiple of 2^-47 of the largest weight, and all sums are exact 64-bit integer sums.  Against exact arithmetic:
  - the rounding down: less than 2^-47 of the largest weight per entry, so V1 * 2^-47 <= 2.4e-10 of c_n for V1 <= 32768 (a
    weight below 2^-47 of the largest counts as 0: the same bound);
  - the weight: x - max is exact in fp64, the product with inv_temp rounds the argument a by |a| * 2^-53 with |a| <= 32.6 for
    every weight that counts, exp adds 1 ulp: 4e-15;
  - the target ceil(p * total) in fp64: 2^-53, plus one unit of 2^-47;
  - this restatement's own np.cumsum of V1 fp64 terms: V1 * 2^-53 <= 4e-12.
Together below 3e-10 of c_n.  NEAR = 1e-8 leaves a factor of thirty and is ten thousand times tighter than 1e-4: every row that
is near here is near under the wider margin too, so the comparison only got stricter.

The cap: at most 1 row in 100 of any generated case may be near (NEAR_CAP) -- asserted on the restatement alone by the CPU test
for every case the GPU test uses, so the GPU test cannot pass by calling everything near."""
import numpy as np

NEAR = 1e-8
NEAR_CAP = 0.01

# every V1 of the GPU test: 1, odd sizes, around the 256 threads of a block, the flagship 9488, and both sides of the kernel's
# switch from keys staged in LDS to re-read rows (15360 / 15361), up to 32768
V1S = (1, 5, 64, 65, 255, 256, 257, 1000, 9488, 15360, 15361, 32768)
ROWS = (1, 3, 130)
INV_TEMPS = (1.0, 2.5, 0.4)


def params(V1):
    """(top_k, top_p, inv_temp) of the kernel test: each knob alone, both together, the temperatures in turn.  (No top_k = 2
    with top_p = 0.5: two tied leaders, which the rounded rows have often, put c_1 exactly on the target.)"""
    ks = (1, 2, V1 - 1, V1, 50)
    ps = (1e-6, 0.5, 0.9, 1.0)
    out = [(k, 1.0) for k in ks] + [(0, p) for p in ps] + [(50, 0.9), (2, 0.7), (V1 - 1, 0.5), (50, 1e-6), (1, 0.9)]
    return [(k, p, INV_TEMPS[i % 3]) for i, (k, p) in enumerate(out)]


def log_probs(logits):
    """fp64 log-softmax rounded to fp32: equal logits stay equal log-probs."""
    z = logits.astype(np.float64)
    m = z.max(1, keepdims=True)
    return (z - m - np.log(np.exp(z - m).sum(1, keepdims=True))).astype(np.float32)


def case(V1, rows):
    """The rows of one kernel case, seeded by its shape.  Row r: r % 3 picks the logits (randn * 3; the same rounded to multiples
    of 0.5, so that many tie; randn * 3 with one token 15 above), (r // 3) % 3 how many entries are -inf beforehand (none, one,
    about half).  With 130 rows, row 7 is all -inf and row 11 holds a NaN."""
    rng = np.random.default_rng(1000 * V1 + rows)
    z = rng.standard_normal((rows, V1)) * 3.0
    for r in range(rows):
        if r % 3 == 1:
            z[r] = np.round(z[r] * 2.0) / 2.0
        elif r % 3 == 2:
            z[r, int(rng.integers(0, V1))] += 15.0
    x = log_probs(z)
    for r in range(rows):
        kind = (r // 3) % 3 if rows > 3 else r % 3
        if kind == 1:
            x[r, int(rng.integers(0, V1))] = -np.inf
        elif kind == 2:
            x[r, rng.random(V1) < 0.5] = -np.inf
    if rows >= 130:
        x[7] = -np.inf
        x[11, int(rng.integers(0, V1))] = np.nan
    return x


def flat_case():
    """All entries equal: V1 = 1000 and p = 0.3333, away from the multiples of 1 / V1 (333.3 entries: J = 334, and the two
    cumulative sums around the target are 3e-4 and 7e-4 of the total away from it)."""
    return np.full((3, 1000), np.float32(-np.log(1000.0))), 0.3333


class Prepared:
    """The sorted view of a matrix of rows, computed once and reused for every (top_k, top_p, inv_temp)."""

    def __init__(self, X):
        X = np.atleast_2d(np.asarray(X, dtype=np.float32))
        self.X = X
        self.rows, self.V1 = X.shape
        self.touched = ~np.isnan(X).any(1) & (X > -np.inf).any(1)
        safe = np.where(self.touched[:, None], X, np.float32(0.0))
        self.order = np.argsort(-safe, axis=1, kind='stable')
        self.xs = np.take_along_axis(safe.astype(np.float64), self.order, 1)
        self.nfin = (self.xs > -np.inf).sum(1)

    def first(self, J):
        """The mask of the first J[r] entries of every row in the order; an untouched row is all True (it keeps every bit)."""
        sel = np.arange(self.V1)[None, :] < np.asarray(J)[:, None]
        mask = np.zeros((self.rows, self.V1), dtype=bool)
        np.put_along_axis(mask, self.order, sel, 1)
        mask[~self.touched] = True
        return mask

    def keep(self, top_k, top_p, inv_temp):
        """-> (mask, J, near, n): n = the survivors of top-k, J = the kept entries (0 on untouched rows)."""
        top_p, inv_temp = float(np.float32(top_p)), float(np.float32(inv_temp))
        n = self.nfin.copy()
        if 0 < top_k < self.V1:
            n = np.minimum(n, top_k)
        J, near = n.copy(), np.zeros(self.rows, dtype=bool)
        if top_p < 1.0:
            with np.errstate(invalid='ignore'):
                w = np.exp((self.xs - self.xs[:, :1]) * inv_temp)
            w[np.arange(self.V1)[None, :] >= n[:, None]] = 0.0
            c = np.cumsum(w, axis=1)
            cn = c[:, -1]
            target = top_p * cn
            J = np.minimum((c < target[:, None]).sum(1) + 1, n)
            rows = np.arange(self.rows)
            c_at = c[rows, np.maximum(J, 1) - 1]
            c_before = c[rows, np.maximum(J, 2) - 2]
            near = (np.abs(c_at - target) <= NEAR * cn) | ((J >= 2) & (np.abs(c_before - target) <= NEAR * cn))
        J = np.where(self.touched, J, 0)
        near &= self.touched
        return self.first(J), J, near, n


def keep_mask(x, top_k, top_p, inv_temp):
    """One row -> (mask, J, near); mask is None for a row that is left untouched."""
    P = Prepared(x)
    mask, J, near, _ = P.keep(top_k, top_p, inv_temp)
    if not P.touched[0]:
        return None, 0, False
    return mask[0], int(J[0]), bool(near[0])


def agrees(P, got_mask, top_k, top_p, inv_temp):
    """got_mask (rows, V1) bool against the restatement under the near rule -> (ok per row, near per row): exact on every row
    that is not near; on a near row the first J - 1, J or J + 1 entries (within 1 .. n)."""
    mask, J, near, n = P.keep(top_k, top_p, inv_temp)
    ok = (got_mask == mask).all(1)
    for dJ in (-1, 1) if near.any() else ():
        alt = np.clip(J + dJ, 1, np.maximum(n, 1))
        ok |= near & (got_mask == P.first(np.where(P.touched, alt, 0))).all(1)
    return ok, near
