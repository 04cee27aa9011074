"""The oracle against the reference's golden vectors (committed outputs of the reference run in the
build container, see oracle/make_golden.py) -- runs anywhere, no GPU, no reference checkout."""
import pytest
import torch

from tests.cases import BY_NAME, CASES, build_oracle_kernel, build_pool, has_golden, load_golden

SMALL = [c["name"] for c in CASES if not c["slow"] and c["N"] <= 30_000]


@pytest.fixture(autouse=True)
def _f64_default():
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)       # the reference allocates in the default dtype
    yield
    torch.set_default_dtype(prev)


def test_known_answer_survey_8c():
    """SURVEY §8c known-answer test of the reference (recorded from BASQ/_rchq.py in fp64)."""
    from oracle.kernels_oracle import direct_rbf
    from oracle.rchq_oracle import recombination_oracle

    g = torch.Generator().manual_seed(1234)
    X = torch.randn(1000, 2, generator=g, dtype=torch.float64)
    torch.manual_seed(7)
    idx, w = recombination_oracle(X, X[:50], 10, direct_rbf)
    assert idx.tolist() == [27, 48, 147, 208, 266, 307, 348, 368, 528, 586]
    ref_w = torch.tensor([0.0652065411967, 0.119271503457, 0.0984233495763, 0.10017205585, 0.167531837628,
                          0.00661903613011, 0.186993262378, 0.0118420499484, 0.194040389823, 0.0498999740124])
    assert ((w - ref_w).abs() / ref_w).max().item() < 1e-9
    assert abs(w.sum().item() - 1.0) < 1e-14


@pytest.mark.parametrize("name", SMALL)
def test_oracle_reproduces_golden(name):
    """Bit-exact: indices, weights and the per-round surviving sets of the reference."""
    from basq_amd.pools import pool_digest
    from oracle.rchq_oracle import Trace, recombination_oracle

    if not has_golden(name):
        pytest.skip("fixture not generated")
    c, fx = BY_NAME[name], load_golden(name)
    pts, nys = build_pool(c)
    assert pool_digest(pts) == fx["pool_digest"], "pool generator is not bit-reproducible on this host"
    kern, _ = build_oracle_kernel(c)
    tr = Trace()
    torch.manual_seed(c["torch_seed"])
    idx, w = recombination_oracle(pts, nys, c["n"], kern, tr)
    assert idx.tolist() == fx["idx"]
    # torch.randn / MKL are the same binaries as in the build container; allow round-off if the CPU differs
    gw = torch.tensor(fx["w"], dtype=torch.float64)
    assert ((w - gw).abs() / gw).max().item() <= 1e-9 if len(gw) else True
    assert len(tr.rounds) == fx["n_rounds"]
    for mine, ref in zip(tr.rounds, fx["rounds"]):
        assert mine.kept_sets is None or mine.kept_sets.tolist() == ref["kept"]
    assert tr.tie_margin > 1e-7, f"{name}: a pivot within {tr.tie_margin:.1e} of a tie -- the golden is not a stable yardstick"


def test_selection_invariant_under_basis_sign_flips():
    """The property the GPU range finder relies on: flipping the sign of rows of U changes nothing, bit for bit."""
    from oracle.kernels_oracle import StationaryOracle
    from oracle.rchq_oracle import divide_and_recombine, nystrom_basis

    c = BY_NAME["rbf_ragged"]
    pts, nys = build_pool(c)
    k = StationaryOracle("rbf", 1.5, 0.7)
    torch.manual_seed(1)
    _, U = nystrom_basis(nys, c["n"] - 1, k)
    w0, i0 = divide_and_recombine(pts, U, nys, k)
    g = torch.Generator().manual_seed(3)
    D = (torch.randint(0, 2, (U.shape[0], 1), generator=g) * 2 - 1).double()
    w1, i1 = divide_and_recombine(pts, D * U, nys, k)
    assert torch.equal(i0, i1) and torch.equal(w0, w1)


def _orthogonal(k, seed, det):
    """A random orthogonal [k, k] matrix with the requested determinant sign (+1: a rotation, -1: a reflection)."""
    g = torch.Generator().manual_seed(seed)
    R = torch.linalg.qr(torch.randn(k, k, generator=g, dtype=torch.float64)).Q
    if float(torch.linalg.det(R)) * det < 0:
        R[0] = -R[0]
    assert abs(float(torch.linalg.det(R)) - det) < 1e-9
    return R


def _null_rows(bary):
    """The rows the elimination pivots on (``_rchq.py:138-143``): trailing rows of the full Vh of ``svd([1 | bary]^T)``."""
    X = torch.cat([torch.ones(bary.shape[0], 1, dtype=bary.dtype), bary], 1)
    M, s = X.shape
    return torch.linalg.svd(X.T)[2][-(M - s):]


def _rotation_case(name):
    """-> ``(run(U) -> (w, idx, Trace), U)`` on the REFERENCE'S OWN op sequence for a BASQ case or the SOBER variant."""
    from oracle.rchq_oracle import Trace, divide_and_recombine, divide_and_recombine_sober, nystrom_basis

    if name.startswith("sober_"):
        from oracle.kernels_oracle import StationaryOracle
        from oracle.make_golden_sober import CASES as SOBER_CASES, case_weights
        from oracle.rchq_oracle import make_cov_psd_sober
        from basq_amd.pools import gmm_pool

        c = [c for c in SOBER_CASES if c["name"] == name][0]
        pts = gmm_pool(c["N"], c["d"], c["pool_seed"])
        nys, w0 = pts[: c["m"]], case_weights(c)
        k = StationaryOracle(c["family"], c["lengthscale"], 1.0)
        torch.manual_seed(1)
        Uq, _, _ = torch.svd_lowrank(make_cov_psd_sober(k(nys, nys)), q=c["n"] - 1)
        U = -1 * Uq.T

        def run(Ux):
            tr = Trace()
            w, idx = divide_and_recombine_sober(pts, Ux, nys, k, None if w0 is None else w0.clone(), tr)
            return w, idx, tr

        return run, U
    c = BY_NAME[name]
    pts, nys = build_pool(c)
    k, _ = build_oracle_kernel(c)
    torch.manual_seed(c["torch_seed"])
    _, U = nystrom_basis(nys, c["n"] - 1, k)

    def run(Ux):
        tr = Trace()
        w, idx = divide_and_recombine(pts, Ux, nys, k, tr)
        return w, idx, tr

    return run, U


@pytest.mark.parametrize("name", ["rbf_ragged", "posterior_noise_ragged", "wsabim_noise_ragged", "sober_is_ragged", "rbf_1e4",
                                  "matern32_8e3", "cfg1_posterior_1e4"])
def test_selection_invariant_under_basis_rotations(name):
    """Round 4's shortcut (``_config.BASIS_SVD = False``: the engine stops at the range finder's orthonormal ``Q`` and skips the
    ``[q, m]`` SVD of ``torch.svd_lowrank``, ``_rchq.py:29``) rests on ONE property of the reference's own op sequence: the
    selection does not depend on WHICH orthonormal basis of the Nystrom feature space the rows of U are.

    Left-multiplying U by an orthogonal R turns every round's matrix X = [1 ; features] into diag(1, R) X: the same Gram X^T X and
    the same first row (the ones), hence the same Golub-Kahan right vectors -- LAPACK's right Householder reflectors, whose trailing
    rows are the null-space basis the elimination pivots on, are unchanged even by the sign flips that uniqueness leaves open
    (dlarfg: (alpha, x) -> (-alpha, -x) gives the same tau and v).

    Pinned here on the oracle (= the reference, bit for bit) for FIVE random orthogonal matrices of EACH determinant sign
    (rotations and reflections), on ragged / posterior-with-noise / WSABI-M / SOBER cases: in round 1 the null-space ROWS
    agree to 2e-10, in every later round to 1e-9 (they are NOT what another SVD algorithm would give: gesvd's differ at O(1)), the kept sets are identical,
    the final indices are identical and the weights agree to 1e-8."""
    run, U = _rotation_case(name)
    w0, i0, t0 = run(U)
    ns0 = [_null_rows(r.bary) for r in t0.rounds if r.bary is not None]
    assert ns0, "no traced round"
    worst_ns = worst_w = worst_first = 0.0
    n_rot = 5 if U.shape[0] <= 60 else 2                         # (the 1e4-point cases: two of each sign keep the CPU suite short)
    for det in (+1.0, -1.0):
        for seed in range(n_rot):
            R = _orthogonal(U.shape[0], 100 * seed + (7 if det > 0 else 13), det)
            w1, i1, t1 = run(R @ U)
            assert torch.equal(i0, i1), (name, det, seed)
            assert len(t1.rounds) == len(t0.rounds)
            for a, b in zip(t0.rounds, t1.rounds):
                assert (a.kept_sets is None) == (b.kept_sets is None)
                assert a.kept_sets is None or a.kept_sets.tolist() == b.kept_sets.tolist(), (name, det, seed, a.remaining)
            ns1 = [_null_rows(r.bary) for r in t1.rounds if r.bary is not None]
            worst_first = max(worst_first, float((ns0[0] - ns1[0]).abs().max()))
            for a, b in zip(ns0, ns1):
                worst_ns = max(worst_ns, float((a - b).abs().max()))
            worst_w = max(worst_w, float(((w0 - w1).abs() / w0).max()))
    # round 1 sees identical weights on both sides: the property itself (measured 7e-14 .. 9e-11, the Matern-3/2 case); later rounds inherit the earlier rounds' weight differences
    # (1e-13 .. 1e-10 relative) and amplify them by the conditioning of [1 | barycentres] (~1e3) -- measured 3e-10 at worst
    assert worst_first <= 2e-10, f"{name}: round-1 null-space rows move by {worst_first:.2e} under a rotation of the basis"
    assert worst_ns <= 1e-9, f"{name}: null-space rows move by {worst_ns:.2e} under a rotation of the basis"
    assert worst_w <= 1e-8, f"{name}: weights move by {worst_w:.2e}"


def test_tie_margins_recorded():
    """Golden cases are well separated from pivot ties (fp64 stability margin, SURVEY finding 3)."""
    from oracle.kernels_oracle import StationaryOracle
    from oracle.rchq_oracle import Trace, recombination_oracle

    c = BY_NAME["rbf_1e4"]
    pts, nys = build_pool(c)
    tr = Trace()
    torch.manual_seed(c["torch_seed"])
    recombination_oracle(pts, nys, c["n"], StationaryOracle("rbf", 2.0), tr)
    assert tr.tie_margin > 1e-7


@pytest.mark.reference
@pytest.mark.parametrize("name", ["kat_small", "rbf_ragged", "cfg1_posterior_1e4", "matern32_8e3", "wsabim_1e4"])
def test_oracle_vs_imported_reference(name):
    """oracle == BASQ._rchq.recombination, bit for bit: against the reference's own output, stored in the golden exactly as
    the reference returned it (``oracle/make_golden.py`` writes every float64 with a round-tripping repr)."""
    from oracle.rchq_oracle import recombination_oracle

    c, fx = BY_NAME[name], load_golden(name)
    pts, nys = build_pool(c)
    kern, _ = build_oracle_kernel(c)
    i0 = torch.tensor(fx["idx"], dtype=torch.int64)
    w0 = torch.tensor(fx["w"], dtype=torch.float64)
    torch.manual_seed(c["torch_seed"])
    i1, w1 = recombination_oracle(pts, nys, c["n"], kern)
    assert torch.equal(i0, i1) and torch.equal(w0, w1)
