"""Float64 checkers for the token selectors and the residual norms (tests/test_select_norm_gpu.py).

Host only (numpy): importable and testable without a device.

The sampler contract, for one row of fp32 logits x, a temperature T and a top_p, all in float64:
  p        = softmax(x / T)
  before_i = mass of the tokens with p > p_i strictly (every member of a tie group gets the same value)
  K        = {i : p_i > 0 and before_i <= top_p}                      the kept set
  F        = CDF of p over a kept set, renormalised to 1, in vocabulary order
and a draw `id` for a uniform u must have F(id - 1) - tol <= u <= F(id) + tol.
"""
import numpy as np

KEPT_SLACK = 1e-5   # a token whose `before` lies this close to top_p may fall on either side of the cut


def draw_tol(V: int) -> float:
    """(per + 11) * 2^-24 + 2^-19 with per = ceil(V / 1024): the fp32 summation of the kernel's CDF (per sequential
    adds in a thread's chunk, 10 scan levels, the u * kept product) plus exp computed as exp2(x * log2 e), whose
    argument (|x/T - max| <= 32, product below 64) rounds by at most 2^-19 absolute."""
    per = -(-V // 1024)
    return (per + 11) * 2.0 ** -24 + 2.0 ** -19


class TopPRow:
    def __init__(self, logits, temperature: float, top_p: float):
        x = np.asarray(logits)
        assert x.ndim == 1 and x.dtype == np.float32
        self.x = x
        self.V = x.shape[0]
        self.top_p = float(top_p)
        z = x.astype(np.float64) / float(temperature)
        e = np.exp(z - z.max())
        self.p = e / e.sum()
        # tie groups are groups of equal logits (equal p by construction); `before` is the mass strictly above
        vals, inv = np.unique(x, return_inverse=True)          # ascending
        mass = np.bincount(inv, weights=self.p, minlength=vals.shape[0])
        above = np.concatenate([np.cumsum(mass[::-1])[::-1][1:], [0.0]])
        self.group = inv
        self.before = above[inv]
        self.K = (self.p > 0) & (self.before <= self.top_p)
        self.tol = draw_tol(self.V)

    # ------------------------------------------------------------------ kept set
    def check_kept(self, kept):
        """kept: bool [V], the kernel's set (probs_out != 0).  Returns a list of complaints (empty = pass)."""
        kept = np.asarray(kept, dtype=bool)
        assert kept.shape == (self.V,)
        bad = []
        if not kept.any():
            bad.append("empty kept set")
        zero = kept & (self.p == 0)
        if zero.any():
            bad.append(f"zero-probability tokens kept: {np.nonzero(zero)[0][:8].tolist()}")
        diff = np.nonzero(kept != self.K)[0]
        far = diff[np.abs(self.before[diff] - self.top_p) > KEPT_SLACK]
        if far.size:
            bad.append(f"{far.size} tokens on the wrong side of the cut, e.g. {far[:8].tolist()} "
                       f"before={self.before[far[:8]].tolist()} top_p={self.top_p}")
        n_in = np.bincount(self.group, weights=kept.astype(np.float64))
        n_all = np.bincount(self.group)
        split = np.nonzero((n_in > 0) & (n_in < n_all))[0]
        if split.size:
            bad.append(f"{split.size} tie groups split by the cut")
        return bad

    # ------------------------------------------------------------------ draws
    def cdf(self, kept=None):
        """F as [V + 1] with F[0] = 0: F[i + 1] = renormalised mass of the kept tokens 0..i."""
        kept = self.K if kept is None else np.asarray(kept, dtype=bool)
        q = np.where(kept, self.p, 0.0)
        c = np.concatenate([[0.0], np.cumsum(q)])
        return c / c[-1]

    def check_draw(self, u, ids, kept=None):
        """u: uniforms (fp32 values), ids: the tokens drawn for them.  Returns a bool array, True where the draw
        violates the contract: a token outside the kept set, or u outside [F(id-1) - tol, F(id) + tol]."""
        kept = self.K if kept is None else np.asarray(kept, dtype=bool)
        u = np.atleast_1d(np.asarray(u)).astype(np.float64)
        ids = np.atleast_1d(np.asarray(ids)).astype(np.int64)
        assert u.shape == ids.shape
        F = self.cdf(kept)
        inside = (ids >= 0) & (ids < self.V)
        safe = np.where(inside, ids, 0)
        ok = inside & kept[safe] & (F[safe] - self.tol <= u) & (u <= F[safe + 1] + self.tol)
        return ~ok

    def chunk_starts(self, kept=None):
        """c_t for t = 1..1023 with a non-empty chunk: F at the start of thread t's chunk [t * per, ...)."""
        per = -(-self.V // 1024)
        F = self.cdf(kept)
        t = np.arange(1, 1024)
        t = t[t * per < self.V]
        return F[t * per]


def ulp_window(centres, radius: int):
    """Every fp32 value within +-radius ulp of each centre, kept inside [0, 1)."""
    c = np.asarray(centres, dtype=np.float32).view(np.int32).astype(np.int64)
    bits = (c[:, None] + np.arange(-radius, radius + 1, dtype=np.int64)[None, :]).ravel()
    one = int(np.float32(1.0).view(np.int32))
    bits = bits[(bits >= 0) & (bits < one)]
    return bits.astype(np.int32).view(np.float32)


# ---------------------------------------------------------------------- residual norms
def slab_sum_f32(resid, partials, nsplit: int):
    """x = resid + partials[0] + partials[1] + ... in fp32, one slab after the other as the kernel adds them
    (bit-comparable with the written-back residual)."""
    x = np.array(resid, dtype=np.float32, copy=True)
    for s in range(nsplit):
        x = (x + np.asarray(partials[s], dtype=np.float32)).astype(np.float32)
    return x


def norm_f64(x, w, b, mode: int, eps: float):
    """mode 0: LayerNorm (x - mean) / sqrt(var + eps) * w + b ; mode 1: Gemma RMSNorm x * rsqrt(mean x^2 + eps) * (1 + w)."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    if mode == 0:
        mean = x.mean(-1, keepdims=True)
        var = ((x - mean) ** 2).mean(-1, keepdims=True)
        return (x - mean) / np.sqrt(var + eps) * w + np.asarray(b, dtype=np.float64)
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * (1.0 + w)


def row_err(got, ref):
    """max |got - ref| per row over the row's max |ref|: [rows]."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return np.abs(got - ref).max(-1) / np.maximum(np.abs(ref).max(-1), 1e-30)
