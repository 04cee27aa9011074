"""Parity cases: how the inputs of every golden fixture are rebuilt from seeds.

A case is a plain dict (it is stored verbatim inside the fixture):

    name, N, d, m (n_nys), n (num_pts), pool_seed, torch_seed,
    kernel: {family, lengthscale, outputscale,
             posterior: {n_obs, noise, obs_seed} | None,
             warp: "none" | "wsabil" | "wsabim"}

Inputs are *regenerated* (``basq_amd.pools.gmm_pool`` is bit-reproducible across
hosts), only expected outputs are committed under ``tests/golden/``.
"""
from __future__ import annotations

import torch

from basq_amd.pools import gmm_pool


def K(family="rbf", lengthscale=2.0, outputscale=1.0, posterior=None, warp="none"):
    return dict(family=family, lengthscale=lengthscale, outputscale=outputscale, posterior=posterior, warp=warp)


def case(name, N, d, m, n, kernel, pool_seed=0, torch_seed=1, slow=False):
    return dict(name=name, N=N, d=d, m=m, n=n, pool_seed=pool_seed, torch_seed=torch_seed, kernel=kernel, slow=slow)


POST = dict(n_obs=102, noise=1e-10, obs_seed=11)
POST_W = dict(n_obs=202, noise=1e-10, obs_seed=12)

CASES = [
    # SURVEY §8c known-answer shape (N=1000, d=2, m=50, n=10) on the portable pool.
    case("kat_small", 1000, 2, 50, 10, K("rbf", 1.0)),
    # BASELINE config 1 shape: N=1e4, posterior-corrected RBF (vbq default kernel).
    case("cfg1_posterior_1e4", 10_000, 10, 100, 100, K("rbf", 2.0, 1.3, posterior=POST)),
    case("rbf_1e4", 10_000, 10, 100, 100, K("rbf", 2.0)),
    # BASQ defaults n_rec=20000, nys_ratio=1e-2, batch 100 (_parameters.py:38-41).
    case("rbf_2e4_defaults", 20_000, 10, 200, 100, K("rbf", 2.0), pool_seed=1),
    # ragged sizes: N not a multiple of 2n, m < 2n, odd d
    case("rbf_ragged", 12_345, 7, 123, 37, K("rbf", 1.5, 0.7), pool_seed=2),
    case("rbf_exact_blocks", 200 * 32, 3, 128, 100, K("rbf", 1.0), pool_seed=3),   # N = 32 * 2n exactly
    case("rbf_d1", 5_000, 1, 50, 20, K("rbf", 0.8), pool_seed=4),
    case("rbf_direct_car", 150, 3, 30, 60, K("rbf", 2.0), pool_seed=5),          # m < q: rank clipped to m
    case("rbf_tiny_final", 150, 3, 100, 100, K("rbf", 2.0), pool_seed=5),        # n < N <= 2n: single reduction
    case("rbf_all_kept", 90, 3, 90, 100, K("rbf", 2.0), pool_seed=6),            # N <= n: everything returned
    case("matern52_3e4_d32", 30_000, 32, 300, 200, K("matern52", 4.0), pool_seed=7),
    case("matern32_8e3", 8_000, 5, 80, 50, K("matern32", 3.0, 2.0), pool_seed=8),
    case("wsabil_2e4", 20_000, 10, 200, 100, K("rbf", 2.0, 1.0, posterior=POST_W, warp="wsabil"), pool_seed=9),
    case("wsabim_1e4", 10_000, 6, 100, 50, K("rbf", 2.0, 1.0, posterior=POST, warp="wsabim"), pool_seed=10),
    case("matern52_posterior", 9_000, 8, 90, 60, K("matern52", 3.0, 1.0, posterior=POST), pool_seed=13),
    # likelihood noise far above the reference's default 1e-10: the per-block diagonal terms of predictive_covariance
    # (full blocks, the ragged tail block, the squared term of WSABI-M) become visible in the selection
    case("posterior_noise_ragged", 9_123, 6, 90, 40, K("matern52", 2.5, 1.2, posterior=dict(n_obs=60, noise=1e-3, obs_seed=14)),
         pool_seed=14),
    case("wsabil_noise_ragged", 7_777, 5, 120, 30, K("rbf", 2.0, 1.0, posterior=dict(n_obs=80, noise=1e-3, obs_seed=15),
                                                      warp="wsabil"), pool_seed=15),
    case("wsabim_noise_ragged", 4_321, 4, 70, 25, K("rbf", 2.0, 1.0, posterior=dict(n_obs=50, noise=1e-2, obs_seed=16),
                                                     warp="wsabim"), pool_seed=16),
    # dimensions above 10: each routes the recombination's block sums through an instantiation no smaller case reaches
    # (KK = KP/4, KP = 4 ceil((d + 2)/4); XS 2 = stationary exponential, XS 1 = the accurate one of posteriors and WSABI)
    case("rbf_2e4_d24", 20_000, 24, 200, 100, K("rbf", 3.5), pool_seed=21),                    # KK 7, no kernel weights
    case("matern52_2e4_d20", 20_000, 20, 200, 100, K("matern52", 3.5), pool_seed=22),          # KK 6, no kernel weights
    case("matern32_2e4_d38", 20_000, 38, 200, 100, K("matern32", 5.0), pool_seed=23),          # KK 10, prefetch depth 1
    case("rbf_2e4_d36", 20_000, 36, 200, 100, K("rbf", 4.5), pool_seed=24),                    # KK 10, no kernel weights, depth 1
    case("posterior_1e4_d16", 10_000, 16, 100, 100, K("rbf", 3.0, 1.2, posterior=dict(n_obs=80, noise=1e-10, obs_seed=25)),
         pool_seed=25),                                                                        # KK 5, XS 1, two row tiles
    case("wsabil_1e4_d28", 10_000, 28, 100, 100, K("rbf", 4.0, 1.0, posterior=dict(n_obs=80, noise=1e-10, obs_seed=26),
                                                   warp="wsabil"), pool_seed=26),             # KK 8, XS 1, kernel weights
    case("wsabim_8e3_d20", 8_000, 20, 100, 50, K("rbf", 3.0, 1.0, posterior=dict(n_obs=60, noise=1e-3, obs_seed=27),
                                                 warp="wsabim"), pool_seed=27),               # squared sums at KK 6
    # BASELINE config 2: N=1e5, d=10, n=100, m=1e3.
    case("cfg2_rbf_1e5", 100_000, 10, 1_000, 100, K("rbf", 2.0)),
    # BASELINE config 3 / headline metric: N=1e6, d=10, n=100, m=1e4 (reference: ~2 min of CPU).
    case("cfg3_rbf_1e6", 1_000_000, 10, 10_000, 100, K("rbf", 2.0), slow=True),
    # the other four pools bench.py cycles through (pool seeds 0-4, torch.manual_seed(1) before every call):
    # every batch the headline number is measured on has a reference-generated golden
    case("cfg3_rbf_1e6_pool1", 1_000_000, 10, 10_000, 100, K("rbf", 2.0), pool_seed=1, slow=True),
    case("cfg3_rbf_1e6_pool2", 1_000_000, 10, 10_000, 100, K("rbf", 2.0), pool_seed=2, slow=True),
    case("cfg3_rbf_1e6_pool3", 1_000_000, 10, 10_000, 100, K("rbf", 2.0), pool_seed=3, slow=True),
    case("cfg3_rbf_1e6_pool4", 1_000_000, 10, 10_000, 100, K("rbf", 2.0), pool_seed=4, slow=True),
    # BASELINE config 4: Matern-5/2, N=1e6, d=32, n=200, m=1e4.
    case("cfg4_matern52_1e6_d32", 1_000_000, 32, 10_000, 200, K("matern52", 4.0), pool_seed=7, slow=True),
    # BASELINE config 5: WSABI-L, N=5e5, d=10, n=100, m=5e3, n_obs=202.
    case("cfg5_wsabil_5e5", 500_000, 10, 5_000, 100, K("rbf", 2.0, 1.0, posterior=POST_W, warp="wsabil"),
         pool_seed=9, slow=True),
    # the same size with the WSABI-M warp (tutorial 03's model): its 0.5 cov^2 term is not linear in the block sums
    case("cfg5m_wsabim_5e5", 500_000, 10, 5_000, 100, K("rbf", 2.0, 1.0, posterior=POST_W, warp="wsabim"),
         pool_seed=9, slow=True),
]

BY_NAME = {c["name"]: c for c in CASES}


def build_pool(c):
    """-> (pts_rec [N,d] f64 CPU, pts_nys = pts_rec[:m])  (prefix split: ``BASQ/_sampler.py:31-33``)."""
    pts = gmm_pool(c["N"], c["d"], c["pool_seed"])
    return pts, pts[: c["m"]]


def build_obs(c):
    p = c["kernel"]["posterior"]
    if p is None:
        return None
    return gmm_pool(p["n_obs"], c["d"], p["obs_seed"])


def build_oracle_kernel(c):
    """The CPU callable handed to the reference / oracle for this case (and its GP state, if any)."""
    from oracle.kernels_oracle import PosteriorOracle, StationaryOracle, WsabiOracle, synthetic_gp_state

    k = c["kernel"]
    base = StationaryOracle(k["family"], k["lengthscale"], k["outputscale"])
    if k["posterior"] is None:
        return base, None
    Xobs = build_obs(c)
    W, mean_const, mean_cache, _ = synthetic_gp_state(Xobs, base, k["posterior"]["noise"], k["posterior"]["obs_seed"])
    # "diag_noise": what the callable adds to entries [k][k] of every block -- the likelihood noise for BASQ/_gp.py:275-276
    # (the default), 0 for SOBER/_gp.py:281-305, whose predictive_covariance has that line commented out
    diag = k["posterior"].get("diag_noise", k["posterior"]["noise"])
    state = dict(Xobs=Xobs, W=W, mean_const=mean_const, mean_cache=mean_cache, noise=diag)
    post = PosteriorOracle(base, Xobs, W, diag)
    if k["warp"] == "none":
        return post, state
    return WsabiOracle(post, mean_const, mean_cache, k["warp"]), state


def seed_all(c):
    torch.manual_seed(c["torch_seed"])


def build_product_kernel(c, state=None):
    """The structured ``basq_amd.kernels`` object equivalent to ``build_oracle_kernel(c)``."""
    from basq_amd import kernels as BK

    k = c["kernel"]
    base = BK.StationaryKernel(k["family"], k["lengthscale"], k["outputscale"])
    if k["posterior"] is None:
        return base
    if state is None:
        _, state = build_oracle_kernel(c)
    post = BK.PosteriorKernel(base, state["Xobs"], state["W"], state["noise"])
    if k["warp"] == "none":
        return post
    return BK.WsabiKernel(post, state["mean_const"], state["mean_cache"], k["warp"])


def load_golden(name):
    import json
    import os

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".json")
    with open(path) as f:
        return json.load(f)


def has_golden(name):
    import os

    return os.path.exists(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".json"))


def structured_fuzz_cases(seed: int, count: int):
    """The configurations of the structured-kernel differential fuzz (stationary, GP posterior, WSABI-L, WSABI-M;
    likelihood noise 1e-10 / 1e-6 / 1e-3; random sizes), as ``tools/fuzz_structured.py`` draws them: a deterministic
    list of case dicts, shared by the GPU fuzz test and the CPU test of the ill-conditioned regime."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(count):
        N = int(torch.randint(50, 6000, (1,), generator=g))
        d = int(torch.randint(2, 12, (1,), generator=g))
        n = int(torch.randint(3, 70, (1,), generator=g))
        m = int(torch.randint(5, min(N, 250) + 1, (1,), generator=g))
        kind = i % 4
        fam = ["rbf", "matern52", "matern32"][i % 3]
        post = dict(n_obs=int(torch.randint(5, 120, (1,), generator=g)), noise=[1e-10, 1e-6, 1e-3][i % 3], obs_seed=50 + i)
        if kind == 0:
            kern = K(fam, 1.0 + 0.5 * (i % 4), 1.0 + 0.1 * (i % 3))
        elif kind == 1:
            kern = K(fam, 1.5 + 0.5 * (i % 3), 1.2, posterior=post)
        elif kind == 2:
            kern = K("rbf", 2.0, 1.0, posterior=post, warp="wsabil")
        else:
            kern = K("rbf", 2.0, 1.0, posterior=post, warp="wsabim")
        out.append(case(f"fz{seed}_{i}", N, d, m, n, kern, pool_seed=400 + i, torch_seed=i))
    return out


def observation_gram_condition(c, state):
    """2-norm condition number of ``K(X, X) + noise I`` of a posterior case (that of the Woodbury matrix), 1 without one."""
    if state is None:
        return 1.0
    W = state["W"]
    ev = torch.linalg.eigvalsh(0.5 * (W + W.T)).abs()
    lo = float(ev.min())
    return float(ev.max()) / lo if lo > 0 else float("inf")


class UlpPerturbed:
    """A base-kernel oracle whose values move by at most one ulp (``K * (1 + delta)``, ``|delta| <= 2^-52``, a fixed
    pseudo-random pattern per call shape): the yard-stick for "the reference's own sensitivity" in ill-conditioned regimes."""

    def __init__(self, base, seed: int):
        self.base, self.seed = base, int(seed)
        self.family, self.lengthscale, self.outputscale = base.family, base.lengthscale, base.outputscale

    def __call__(self, x, y):
        Kxy = self.base(x, y)
        g = torch.Generator().manual_seed(self.seed * 7919 + Kxy.numel() % 1000)
        return Kxy * (1.0 + 2.0 ** -52 * (2.0 * torch.rand(Kxy.shape, generator=g, dtype=torch.float64) - 1.0))


def build_perturbed_oracle_kernel(c, seed: int):
    """``build_oracle_kernel(c)`` with every base-kernel value moved by <= 1 ulp (the GP state -- Woodbury matrix, mean
    cache -- is the unperturbed one: the same fitted model, evaluated with a kernel that rounds differently)."""
    from oracle.kernels_oracle import PosteriorOracle, WsabiOracle

    ko, state = build_oracle_kernel(c)
    k = c["kernel"]
    if k["posterior"] is None:
        return UlpPerturbed(ko, seed)
    base = ko.base if k["warp"] == "none" else ko.post.base
    post = PosteriorOracle(UlpPerturbed(base, seed), state["Xobs"], state["W"], state["noise"])
    if k["warp"] == "none":
        return post
    return WsabiOracle(post, state["mean_const"], state["mean_cache"], k["warp"])
