"""Every instantiation of the fused block sums against direct float64 references.

``blocksum_kernel<KK, FAM, JT, XS, NOWX>`` is compiled for KK = KP/4 = 1..10 (KP = 4 ceil((d + 2)/4)), three families, two
exponential schemes (XS 2: stationary kernels; XS 1, the accurate table: GP posteriors and WSABI), with and without per-candidate
kernel weights (the lean ``NOWX`` form where ``BASQ_BS_NOWX_FOR`` asks for it); the row tiles per wave (JT) and the prefetch depth
follow from KK.  ``SWEEP_D`` reaches every KK, padded and unpadded, and the product below reaches every instantiation the
dispatcher can launch -- ``tests/test_blocksum_coverage.py`` checks that against the build's own list of kernels.

The references are ``tests/blocksum_reference.py``: distances by direct differences on the raw points (no expansion), set sums in
float64, and a per-entry relative bound (no normalisation by the largest entry)."""
import dataclasses
import math

import pytest
import torch

from tests.blocksum_reference import blocksum_direct, kernel_direct, worst_ratio

pytestmark = pytest.mark.gpu

SWEEP_D = [2, 5, 10, 13, 16, 22, 24, 30, 31, 38]          # KK 1..10; KP = d + 2 exactly at d = 2, 10, 22, 30, 38
FAMILIES = ["rbf", "matern52", "matern32"]

# (m, S, off, n_full, Rl, n_chunks): every launch geometry runs at every KK
GEOMETRIES = [
    # m not a multiple of 32; S = 37; a ragged tail of 23; 13 blocks per chunk (fast ranges of >= 3 blocks)
    (97, 37, 0, 37 * 38, 37 * 38 + 23, 3),
    # a shard starting mid-block (off = 125 = 2.5 blocks); two blocks per chunk; the last chunk holds only the tail of 31
    (130, 50, 125, 2000, 2000 - 125 + 31, 20),
    # one block per chunk (fast ranges of one block); S = 200 (not a multiple of 16); the shard ends mid-block, no tail
    (65, 200, 0, 2400, 2300, 12),
]


def _spec(family, d, accurate):
    from basq_amd.kernels import StationaryKernel

    ell = 1.2 * math.sqrt(d)                                  # kernel values of order 0.01..1, not all underflow
    return dataclasses.replace(StationaryKernel(family, ell, 1.3).spec(d), accurate_exp=accurate)


def _points(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, d, generator=g, dtype=torch.float64) * 1.5


def _weights(Rl, off, S, seed, with_wx):
    """Positive mu with exact zeros: every 5th candidate and every candidate of set 3."""
    g = torch.Generator().manual_seed(seed)
    mu = torch.rand(Rl, generator=g, dtype=torch.float64) + 0.1
    pg = off + torch.arange(Rl)
    mu[(torch.arange(Rl) % 5) == 4] = 0.0
    mu[pg % S == 3] = 0.0
    wx = (torch.rand(Rl, generator=g, dtype=torch.float64) + 0.5) if with_wx else None
    return mu, wx


def _pack(ops, spec, nys, cand):
    center = ops.to_device(nys.mean(0))
    pa = ops.pack(spec, ops.to_device(nys), center, 0, pad_rows_to=64)
    pb = ops.pack(spec, ops.to_device(cand), center, 1)
    return pa, pb


def _geo_row(ops, R, S, reg_hi, off=0, Rl=None):
    """A round descriptor {R, n_full, reg_hi, violation, nb, n_tail, off, Rl} (see ``basq_blocksum_geo_f64``)."""
    nb = R // S
    row = torch.tensor([R, nb * S, reg_hi, 0, nb, R - nb * S, off, R if Rl is None else Rl], dtype=torch.int64)
    return ops.to_device(row)


SWEEP = [(d, fam, acc, wx) for d in SWEEP_D for fam in FAMILIES for acc in (False, True) for wx in (False, True)]


@pytest.mark.parametrize("d,family,accurate,with_wx", SWEEP,
                         ids=[f"d{d}-{f}-xs{1 if a else 2}-{'wx' if w else 'nowx'}" for d, f, a, w in SWEEP])
def test_blocksum_instantiation_vs_direct_reference(hip_ops, d, family, accurate, with_wx):
    """Every (chunk, row, set) entry of the block sums within the per-entry bound of the direct reference, the set weights to
    1e-13 relative, entries without a weighted candidate exactly 0, and candidates of zero weight contributing exactly
    nothing (moving them leaves the result bit for bit the same)."""
    spec = _spec(family, d, accurate)
    dev = hip_ops.to_device
    worst = 0.0
    for gi, (m, S, off, n_full, Rl, n_ch) in enumerate(GEOMETRIES):
        nys, cand = _points(m, d, 100 + gi), _points(Rl, d, 200 + gi)
        mu, wx = _weights(Rl, off, S, 300 + gi, with_wx)
        pa, pb = _pack(hip_ops, spec, nys, cand)
        X, t = hip_ops.blocksum(spec, pa, m, pb, dev(mu), None if wx is None else dev(wx), Rl, off, n_full, S, n_ch)
        X, t = X.cpu(), t.cpu()
        Xr, tr, bound = blocksum_direct(family, spec.lengthscale, nys, cand, mu, wx, off, n_full, S, n_ch, accurate)
        r = worst_ratio(X, Xr, bound)
        assert r <= 1.0, f"geometry {gi}: an entry is off by {r:.2f} x its bound"
        worst = max(worst, r)
        assert torch.equal(t == 0, tr == 0) and ((t - tr).abs() <= 1e-13 * tr).all(), f"geometry {gi}: set weights"
        assert not X[:, :, 3].any() and not t[:, 3].any()                   # set 3 carries no weight at all
        if gi == 0:
            moved = cand.clone()
            moved[mu == 0] = _points(int((mu == 0).sum()), d, 400)           # zero-weight candidates elsewhere
            _, pb2 = _pack(hip_ops, spec, nys, moved)
            X2, t2 = hip_ops.blocksum(spec, pa, m, pb2, dev(mu), None if wx is None else dev(wx), Rl, off, n_full, S, n_ch)
            assert torch.equal(X2.cpu(), X) and torch.equal(t2.cpu(), t)
    print(f"d={d} {family} XS {1 if accurate else 2} wx {with_wx}: worst entry at {worst:.3f} of its bound")


@pytest.mark.parametrize("d", SWEEP_D)
@pytest.mark.parametrize("family", FAMILIES)
def test_blocksum_residue_classes_every_kk(hip_ops, d, family):
    """Residue-class chunks (chunk c = the blocks b with b % C == class0 + c): each class against the direct reference with
    the per-entry bound, and all classes together equal to the contiguous launch over the same range to 1e-13 per entry."""
    spec = _spec(family, d, False)
    dev = hip_ops.to_device
    m, S, C = 97, 37, 4
    off, nb = 3 * S, 26                                         # a shard of 26 full blocks from block 3 (class 3 first)
    Rl, n_full = nb * S, off + nb * S
    nys, cand = _points(m, d, 11), _points(Rl, d, 12)
    for with_wx in (False, True):
        mu, wx = _weights(Rl, off, S, 13, with_wx)
        pa, pb = _pack(hip_ops, spec, nys, cand)
        wxd = None if wx is None else dev(wx)
        Xc, tc = hip_ops.blocksum(spec, pa, m, pb, dev(mu), wxd, Rl, off, n_full, S, C, class_mod=C, class0=0)
        X1, t1 = hip_ops.blocksum(spec, pa, m, pb, dev(mu), wxd, Rl, off, n_full, S, 1)
        Xl, _ = hip_ops.blocksum(spec, pa, m, pb, dev(mu), wxd, Rl, off, n_full, S, 2, class_mod=C, class0=2)
        Xc, tc, X1, t1, Xl = (v.cpu() for v in (Xc, tc, X1, t1, Xl))
        Xr, _, bound = blocksum_direct(family, spec.lengthscale, nys, cand, mu, wx, off, n_full, S, C, False, class_mod=C)
        assert worst_ratio(Xc, Xr, bound) <= 1.0
        assert torch.equal(Xl, Xc[2:4])                         # classes 2..3 alone: the same launch arithmetic
        whole = X1[0]
        assert ((Xc.sum(0) - whole).abs() <= 1e-13 * whole).all() and torch.equal(Xc.sum(0) == 0, whole == 0)
        assert ((tc.sum(0) - t1[0]).abs() <= 1e-13 * t1[0]).all()


@pytest.mark.parametrize("d", SWEEP_D)
def test_blocksum_geo_every_kp(hip_ops, d):
    """The descriptor-driven entry (``blocksum_apply_geo<KP>``, one per KP) in modes 1-5 returns bit for bit what the
    host-geometry entry returns over the same positions: the whole pool, and a shard that starts and ends mid-block."""
    i = SWEEP_D.index(d)
    family, with_wx = FAMILIES[i % 3], bool(i % 2)
    spec = _spec(family, d, bool(i % 4 >= 2))
    m, S, reg_blocks, C = 130, 64, 40, 8
    R = 46 * S + 6                                             # 6 irregular full blocks behind the regular region, tail of 6
    nb = R // S
    n_full, reg_hi, e = nb * S, reg_blocks * S, nb - reg_blocks
    nys, cand = _points(m, d, 21), _points(R, d, 22)
    mu, wx = _weights(R, 0, S, 23, with_wx)
    pa, pb = _pack(hip_ops, spec, nys, cand)
    mu_d = hip_ops.to_device(mu)
    wx_d = None if wx is None else hip_ops.to_device(wx)

    def host(lo, hi, n_ch, off=0, Rl=R, **kw):
        lo, hi = max(lo, off), min(hi, off + Rl)
        hi = max(hi, lo)
        return hip_ops.blocksum(spec, pa, m, pb[lo:], mu_d[lo:], None if wx_d is None else wx_d[lo:], hi - lo, lo, n_full, S,
                                n_ch, **kw)

    def same(a, b):
        return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

    for off, Rl in ((0, R), (333, 2100)):
        geo = _geo_row(hip_ops, R, S, reg_hi, off, Rl)
        pbs, mus, wxs = pb[off:], mu_d[off:], None if wx_d is None else wx_d[off:]
        assert same(hip_ops.blocksum_geo(spec, pa, m, pbs, mus, wxs, geo, 1, S, C, class_mod=C),
                    host(0, reg_hi, C, off, Rl, class_mod=C))
        assert same(hip_ops.blocksum_geo(spec, pa, m, pbs, mus, wxs, geo, 2, S, 1), host(reg_hi, R, 1, off, Rl))
        assert same(hip_ops.blocksum_geo(spec, pa, m, pbs, mus, wxs, geo, 3, S, 3), host(0, R, 3, off, Rl))
    geo = _geo_row(hip_ops, R, S, reg_hi)
    Xa, ta = hip_ops.blocksum_geo(spec, pa, m, pb, mu_d, wx_d, geo, 5, S, C - 1, class_mod=C)   # one chunk per irregular block
    for b in range(C - 1):
        if b < e:
            lo = reg_hi + b * S
            Xb, tb = hip_ops.blocksum(spec, pa, m, pb[lo:], mu_d[lo:], None if wx_d is None else wx_d[lo:], S, lo, n_full, S, 1)
            assert torch.equal(Xa[b], Xb[0]) and torch.equal(ta[b], tb[0])
        else:
            assert not Xa[b].any() and not ta[b].any()
    Xt, tt = hip_ops.blocksum_geo(spec, pa, m, pb, mu_d, wx_d, geo, 4, S, 1)                 # the tail: point k in set k
    Xh, th = hip_ops.blocksum(spec, pa, m, pb[n_full:], mu_d[n_full:], None if wx_d is None else wx_d[n_full:], R - n_full, 0,
                              S, S, 1)
    assert torch.equal(Xt, Xh) and torch.equal(tt, th)


SQ_SWEEP = [(d, fam) for d in SWEEP_D for fam in FAMILIES]


@pytest.mark.parametrize("d,family", SQ_SWEEP, ids=[f"d{d}-{f}" for d, f in SQ_SWEEP])
def test_blocksum_sq_and_cov_diag_vs_direct_covariance(hip_ops, d, family):
    """WSABI-M's squared-covariance block sums (``blocksum_sq_kernel``) and noise cross terms (``cov_diag_kernel``) at every
    KK x family against ``cov = s2 k(nys, y) - B ko + noise [j == kappa]`` built from the direct-difference kernel in float64.

    The bound is per entry and counts the cancellation honestly: ``1e-12 sum mu/2 (s2 k + sum_o |B| |ko| + noise)^2`` (the
    second term is what the n_obs products of the correction can round at, whatever their signed sum).  The descriptor-driven
    variants are bit-equal to the host-geometry entries."""
    spec = _spec(family, d, True)
    dev = hip_ops.to_device
    s2, m, n_obs, S, n_ch = spec.outputscale, 97, 37, 37, 2
    off, n_full = 50, 37 * 30
    Rl = n_full - off + 20                                     # starts mid-block, ragged tail of 20
    noise = 1e-3 if SWEEP_D.index(d) % 2 else 0.0
    nys, obs, cand = _points(m, d, 31), _points(n_obs, d, 32), _points(Rl, d, 33)
    g = torch.Generator().manual_seed(34)
    mu = torch.rand(Rl, generator=g, dtype=torch.float64) + 0.05
    mu[::7] = 0.0
    Bm = 0.1 * _points(m, n_obs, 35)
    ko = s2 * kernel_direct(family, obs, cand, spec.lengthscale)[0]        # an input: the same numbers on both sides
    n4, mp = (n_obs + 3) // 4 * 4, (m + 63) // 64 * 64
    pa, pb = _pack(hip_ops, spec, nys, cand)
    bT = hip_ops.zeros(n4, mp)
    bT[:n_obs, :m] = dev(Bm.t().contiguous())
    kobs = hip_ops.zeros(n4, Rl)
    kobs[:n_obs] = dev(ko)
    mud = dev(mu)
    E = hip_ops.blocksum_sq(spec, pa, m, pb, mud, Rl, off, n_full, S, n_ch, bT, kobs, n_obs, noise)
    val = hip_ops.cov_diag(spec, pa, m, pb, Rl, off, n_full, S, bT, kobs, n_obs, 1e-3)

    k = kernel_direct(family, nys, cand, spec.lengthscale)[0]
    pg = off + torch.arange(Rl)
    kappa = torch.where(pg < n_full, pg % S, pg - n_full)
    hit = kappa < m
    diag = torch.zeros(m, Rl, dtype=torch.float64)
    diag[kappa[hit], torch.arange(Rl)[hit]] = 1.0
    corr = Bm @ ko
    cov = s2 * k - corr + noise * diag
    mag = s2 * k + Bm.abs() @ ko.abs() + noise * diag
    sets = torch.where(pg < n_full, pg % S, torch.full_like(pg, S - 1))
    Er = torch.zeros(m, S, dtype=torch.float64).index_add_(1, sets, 0.5 * mu * cov * cov)
    bound = 1e-12 * torch.zeros(m, S, dtype=torch.float64).index_add_(1, sets, 0.5 * mu * mag * mag)
    err = (E.cpu().sum(0) - Er).abs()
    assert (err <= bound).all(), f"worst entry at {(err / bound).max().item():.2f} of its bound"
    print(f"d={d} {family}: squared sums' worst entry at {(err / bound).max().item():.3f} of its bound")

    cols = torch.arange(Rl)[hit]
    want = torch.zeros(Rl, dtype=torch.float64)
    want[hit] = 1e-3 * (s2 * k[kappa[hit], cols] - corr[kappa[hit], cols]) + 0.5e-6
    vb = 1e-12 * (1e-3 * mag[kappa[hit], cols] + 0.5e-6)
    got = val.cpu()[:Rl]
    assert (got[~hit] == 0).all() and ((got[hit] - want[hit]).abs() <= vb).all()

    # descriptor-driven: the same shard, read from a descriptor (mode 3: everything; mode 1: the regular region in classes)
    R, reg_hi, C = n_full + 20, 24 * S, 4
    geo = _geo_row(hip_ops, R, S, reg_hi, off, Rl)
    assert torch.equal(hip_ops.blocksum_sq_geo(spec, pa, m, pb, mud, geo, 3, S, n_ch, bT, kobs, n_obs, noise), E)
    Ec = hip_ops.blocksum_sq_geo(spec, pa, m, pb, mud, geo, 1, S, C, bT, kobs, n_obs, 0.0, class_mod=C)
    hi = reg_hi - off
    Eh = hip_ops.blocksum_sq(spec, pa, m, pb, mud, hi, off, n_full, S, C, bT, kobs, n_obs, 0.0, class_mod=C)
    assert torch.equal(Ec, Eh)
    va = hip_ops.cov_diag_geo(spec, pa, m, pb, geo, Rl, S, bT, kobs, n_obs, 1e-3)
    assert torch.equal(va[:Rl], val[:Rl])


@pytest.mark.parametrize("d", [2, 16, 38])
@pytest.mark.parametrize("family", FAMILIES)
def test_matvec_every_family_vs_direct_reference(hip_ops, d, family):
    """``basq_kernel_matvec_f64`` (the block sums with one set, accurate exponential) at KK 1, 5 and 10: every entry within
    ``1e-12 (|bias| + s2 sum_j k |v_j|)`` of the direct-difference reference -- per entry, the signed sum's own scale."""
    from basq_amd.kernels import StationaryKernel

    spec = StationaryKernel(family, 1.2 * math.sqrt(d), 1.3).spec(d)
    x, xo = _points(1000, d, 41), _points(202, d, 42)
    v = _points(202, 1, 43).reshape(-1)
    center = x.mean(0)
    dev = hip_ops.to_device
    out = hip_ops.matvec(spec, hip_ops.pack(spec, dev(x), dev(center), 0, pad_rows_to=64), 1000,
                         hip_ops.pack(spec, dev(xo), dev(center), 1), 202, dev(v), 0.7).cpu()
    k = kernel_direct(family, x, xo, spec.lengthscale)[0]
    want = 0.7 + spec.outputscale * (k @ v)
    scale = 0.7 + spec.outputscale * (k @ v.abs())
    assert ((out - want).abs() <= 1e-12 * scale).all(), ((out - want).abs() / scale).max().item()
