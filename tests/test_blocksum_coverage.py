"""No GPU needed: the block-sum instantiation sweep (``tests/test_blocksum_instantiations_gpu.py``) against the kernels the build
actually contains, and the per-entry bound of ``tests/blocksum_reference.py`` against the CPU stand-in.

If an instantiation or a KK is added to the block sums without the sweep reaching it, ``test_sweep_reaches_every_instantiation``
fails.  The kernels' names come from the compiler's resource reports (``basq_amd._build.kernel_resources``)."""
import re

import pytest
import torch

from tests.blocksum_reference import FAMILY_ID, blocksum_direct, kp, worst_ratio
from tests.test_kernel_resources import res  # noqa: F401  (the module-scoped fixture)

FAMILY_NAME = {v: k for k, v in FAMILY_ID.items()}
BS = re.compile(r"^_Z15blocksum_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])E")
SQ = re.compile(r"^_Z18blocksum_sq_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])E")
GRAM = re.compile(r"^_Z11gram_kernelILi(\d+)ELi(\d+)EE")


def _gram_ds():
    from tests.test_kernels_gpu import test_gram_vs_oracle

    marks = [m for m in test_gram_vs_oracle.pytestmark if m.name == "parametrize" and m.args[0] == "d"]
    return list(marks[0].args[1])


def test_sweep_reaches_every_instantiation(res):  # noqa: F811
    from tests.test_blocksum_instantiations_gpu import FAMILIES, SQ_SWEEP, SWEEP

    reach = {}                                  # (KK, FAM, XS, with wx) -> the sweep case that launches it
    for d, fam, acc, wx in SWEEP:
        reach.setdefault((kp(d) // 4, FAMILY_ID[fam], 1 if acc else 2, wx), f"d{d}-{fam}-xs{1 if acc else 2}-{'wx' if wx else 'nowx'}")
    sq_reach = {}
    for d, fam in SQ_SWEEP:
        sq_reach.setdefault((kp(d) // 4, FAMILY_ID[fam]), f"d{d}-{fam}")
    gram_reach = {}
    for d in _gram_ds():
        for fam in FAMILIES:
            gram_reach.setdefault((kp(d) // 4, FAMILY_ID[fam]), f"d{d}-{fam}")

    table, bs_built = [], set()
    for name in sorted(res):
        m = BS.match(name)
        if m:
            KK, FAM, JT, XS, NOWX = (int(v) for v in m.groups())
            assert JT == (4 if KK <= 4 else 2), f"{name}: JT {JT} is not the one the launcher picks at KK {KK}"
            # the lean form runs when no kernel weights are given; the general form always runs with them
            key = (KK, FAM, XS, not NOWX)
            bs_built.add(key[:3])
            table.append((f"blocksum_kernel<KK={KK}, {FAMILY_NAME[FAM]}, JT={JT}, XS={XS}, NOWX={NOWX}>", reach.get(key)))
            continue
        m = SQ.match(name)
        if m:
            KK, FAM, JT, GEO = (int(v) for v in m.groups())
            if JT != (4 if KK <= 4 else 2):
                continue                        # JT 4 at KK >= 5 is never launched; JT 2 below only under BASQ_SQ_JT=2 (A/B knob)
            table.append((f"blocksum_sq_kernel<KK={KK}, {FAMILY_NAME[FAM]}, JT={JT}, GEO={GEO}>", sq_reach.get((KK, FAM))))
            continue
        m = GRAM.match(name)
        if m:
            KK, FAM = (int(v) for v in m.groups())
            table.append((f"gram_kernel<KK={KK}, {FAMILY_NAME[FAM]}>", gram_reach.get((KK, FAM))))
    print("\n".join(f"{k:60s} <- {v}" for k, v in table))
    missing = [k for k, v in table if v is None]
    assert not missing, f"instantiations no sweep case launches: {missing}"
    assert sum(1 for k, _ in table if k.startswith("blocksum_kernel")) >= 10 * 3 * 2, "block-sum instantiations not found"
    assert {k for k, _ in table if k.startswith("gram")} and {k for k, _ in table if k.startswith("blocksum_sq")}
    # and every general (KK, FAM, XS) the sweep asks for exists: the dispatcher has a kernel for each KK 1..10
    assert {key[:3] for key in reach} == bs_built


def _standin_case(family, d, accurate, far):
    import dataclasses

    from basq_amd.kernels import StationaryKernel
    from tests.cpu_stand_in import CpuStandInOps

    cpu = CpuStandInOps()
    spec = dataclasses.replace(StationaryKernel(family, 1.2 * d ** 0.5, 1.0).spec(d), accurate_exp=accurate)
    g = torch.Generator().manual_seed(7)
    m, S, Rl = 70, 37, 37 * 12 + 5
    nys = torch.randn(m, d, generator=g, dtype=torch.float64) * 1.5
    cand = torch.randn(Rl, d, generator=g, dtype=torch.float64) * 1.5
    if far:
        cand[torch.arange(Rl) % S == 5] += 6.0 * spec.lengthscale / d ** 0.5   # set 5: the far field of every row
    mu = torch.rand(Rl, generator=g, dtype=torch.float64) + 0.1
    center = nys.mean(0)
    X, _ = cpu.blocksum(spec, cpu.pack(spec, nys, center, 0, pad_rows_to=64), m, cpu.pack(spec, cand, center, 1), mu, None,
                        Rl, 0, 37 * 12, S, 2)
    Xr, _, bound = blocksum_direct(family, spec.lengthscale, nys, cand, mu, None, 0, 37 * 12, S, 2, accurate)
    return X, Xr, bound


@pytest.mark.parametrize("family", ["rbf", "matern52", "matern32"])
def test_direct_reference_bound_holds_for_the_expanded_product(family):
    """The stand-in forms distances by the kernels' expanded product with an exact exponential: it must sit inside the bound
    at every KK of the sweep (the bound has room for what the expansion loses), with the accurate scheme's tighter constant."""
    from tests.test_blocksum_instantiations_gpu import SWEEP_D

    for d in SWEEP_D:
        X, Xr, bound = _standin_case(family, d, True, far=False)
        assert worst_ratio(X, Xr, bound) <= 0.5, d


def test_per_entry_bound_rejects_what_a_max_normalised_bound_accepts():
    """A 1e-11 relative error planted in a far-field entry of a stand-in result: inside ``1e-12 * max|X|`` (the comparison the
    older block-sum tests make), outside the per-entry bound."""
    X, Xr, bound = _standin_case("rbf", 10, False, far=True)
    assert worst_ratio(X, Xr, bound) <= 1.0
    flat = Xr.reshape(-1)
    i = int(torch.argmin(torch.where(flat > 0, flat, torch.full_like(flat, float("inf")))))
    assert flat[i] < 1e-3 * flat.max()                          # a far-field entry
    bad = X.clone().reshape(-1)
    bad[i] *= 1.0 + 1e-11
    bad = bad.reshape(X.shape)
    assert (bad - Xr).abs().max() <= 1e-12 * Xr.abs().max()     # the max-normalised bound lets it through
    assert worst_ratio(bad, Xr, bound) > 1.0                    # the per-entry bound does not
