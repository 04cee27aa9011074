"""Direct float64 references for the fused block sums, and the per-entry bound their results are held to.

The kernels form a squared distance by an expanded product (``x.y - |x|^2/2 - |y|^2/2`` on points packed around a centre), and so
does the CPU stand-in (``tests/cpu_stand_in.py``) -- a comparison between the two cannot see an error in that expansion.  These
references evaluate ``sum_k ((x_k - y_k) / l)^2`` on the raw points instead, in float64, with no expansion and no packing.

The bound is per entry and relative.  One kernel value is held to ``term_bound`` (the per-value form of
``test_blocksum_single_values_over_the_whole_exponent_range``: the table exponential, plus what the expanded product can lose at
the size of its terms, plus the argument's own rounding).  A set sum of terms with non-negative weights has a relative error of at
most the worst of its terms' bounds plus the summation's ``count * 2^-52``.  Unlike a bound normalised by the largest entry, this
one does not let a small entry be wrong in its leading digits.
"""
from __future__ import annotations

import math

import torch

U = 2.0 ** -52
FAMILY_ID = {"rbf": 0, "matern52": 1, "matern32": 2}


def kp(d: int) -> int:
    return 4 * ((d + 2 + 3) // 4)


def kernel_direct(family: str, x, y, ell: float):
    """-> ``(k, arg)`` [len(x), len(y)]: the unit-outputscale kernel from direct differences, and its exponent argument."""
    diff = (x[:, None, :] - y[None, :, :]) / ell
    r2 = (diff * diff).sum(-1)
    if family == "rbf":
        arg = -0.5 * r2
        return torch.exp(arg), arg
    r = r2.sqrt()
    c = math.sqrt(5.0) if family == "matern52" else math.sqrt(3.0)
    arg = -c * r
    poly = (1.0 + c * r + (5.0 / 3.0) * r2) if family == "matern52" else (1.0 + c * r)
    return poly * torch.exp(arg), arg


def term_bound(x, y, center, ell: float, arg, accurate: bool):
    """Relative bound of one kernel value computed by the block sums (see the module docstring)."""
    size = ((x - center) / ell).pow(2).sum(1)[:, None] + ((y - center) / ell).pow(2).sum(1)[None, :]
    return (2e-15 if accurate else 1e-13) + 4e-15 * size + 1e-15 * arg.abs()


def set_chunk_of(Rl, off, n_full, S, n_chunks, class_mod=0, class0=0):
    """-> ``(sets, chunk, sel)`` per local position, as the block sums assign them: positions below ``n_full`` belong to set
    ``pg % S``, the ragged tail to set S - 1; chunks are contiguous block ranges (the tail in the last one) or residue classes of
    the global block index (``sel``: the positions a class launch covers)."""
    pg = off + torch.arange(Rl)
    sets = torch.where(pg < n_full, pg % S, torch.full_like(pg, S - 1))
    lim = min(off + Rl, n_full)
    blk_lo, blk_hi = (off // S, (lim + S - 1) // S) if lim > off else (0, 0)
    per = max(1, -(-(blk_hi - blk_lo) // n_chunks))
    chunk = torch.where(pg < n_full, (pg // S - blk_lo) // per, torch.full_like(pg, n_chunks - 1))
    sel = torch.ones(Rl, dtype=torch.bool)
    if class_mod > 0:
        cls = (pg // S) % class_mod - class0
        sel = (cls >= 0) & (cls < n_chunks)
        chunk = cls.clamp(0, n_chunks - 1)
    return sets, chunk, sel


def blocksum_direct(family, ell, nys, cand, mu, wx, off, n_full, S, n_chunks, accurate, class_mod=0, class0=0, step=512):
    """-> ``(X [n_chunks, m, S], tot [n_chunks, S], rel_bound [n_chunks, m, S])`` on the raw points (``cand`` = the Rl local
    candidates).  ``rel_bound`` is the per-entry relative bound; entries with no weighted term must come out exactly 0."""
    m, Rl = nys.shape[0], cand.shape[0]
    center = nys.mean(0)
    sets, chunk, sel = set_chunk_of(Rl, off, n_full, S, n_chunks, class_mod, class0)
    w = mu * (wx if wx is not None else 1.0)
    w = torch.where(sel, w, torch.zeros_like(w))
    flat = chunk * S + sets
    X = torch.zeros(m, n_chunks * S, dtype=torch.float64)
    B = torch.zeros(m, n_chunks * S, dtype=torch.float64)
    cnt = torch.zeros(n_chunks * S, dtype=torch.float64)
    for lo in range(0, Rl, step):
        hi = min(Rl, lo + step)
        k, arg = kernel_direct(family, nys, cand[lo:hi], ell)
        X.index_add_(1, flat[lo:hi], k * w[lo:hi])
        tb = term_bound(nys, cand[lo:hi], center, ell, arg, accurate)
        tb = torch.where((w[lo:hi] != 0)[None, :], tb, torch.zeros_like(tb))
        B.scatter_reduce_(1, flat[lo:hi].expand(m, -1), tb, "amax")
        cnt.index_add_(0, flat[lo:hi], (w[lo:hi] != 0).double())
    tot = torch.zeros(n_chunks * S, dtype=torch.float64).index_add_(0, flat, torch.where(sel, mu, torch.zeros_like(mu)))
    bound = B + cnt[None, :] * U
    to3 = lambda t: t.reshape(m, n_chunks, S).permute(1, 0, 2).contiguous()   # noqa: E731
    return to3(X), tot.reshape(n_chunks, S), to3(bound)


def worst_ratio(got, want, rel_bound, floor=1e-280):
    """-> ``max |got - want| / (rel_bound |want|)`` over the entries above ``floor`` (0 if there are none).  Entries at or below
    it must be non-negative and no larger than ``10 * floor``, and entries whose reference is exactly 0 must be exactly 0."""
    got, want = got.reshape(-1), want.reshape(-1)
    rel_bound = rel_bound.reshape(-1)
    zero = want == 0
    assert (got[zero] == 0).all(), f"{int((got[zero] != 0).sum())} entries without a weighted term are not exactly 0"
    tiny = (want <= floor) & ~zero
    assert ((got[tiny] >= 0) & (got[tiny] <= 10 * floor)).all()
    big = want > floor
    if not big.any():
        return 0.0
    return ((got[big] - want[big]).abs() / (rel_bound[big] * want[big])).max().item()
