"""CPU: the two K-fold entry points (declared, bound, exported) and the refusals of the mirror, which reach no device."""
import numpy as np
import pytest


def test_the_two_entry_points_are_declared_bound_and_exported(agp):
    lib, P = agp._lib.load(), agp._lib.PROTOTYPES
    for name in ("gp_kfold", "gp_kfold_sum"):
        assert name in agp._lib.header_functions() and name in P and hasattr(lib, name), name
    assert P["gp_kfold_sum"][1][2:] == P["gp_kfold"][1][2:] and P["gp_kfold_sum"][1][0] == P["gp_kfold"][1][0] and len(P["gp_kfold"][1]) == 12
    assert P["gp_kfold_sum"][1][1] is P["gp_loo_sum"][1][1] and P["gp_kfold"][1][1] is P["gp_loo"][1][1]
    assert lib.gp_abi_version() == 4 and agp._lib.kfold_max_fold() == 1024
    assert callable(agp.kfold_logpdf) and callable(agp.kfold_mean_and_var)


@pytest.mark.parametrize("folds,n,exc,reason", [
    (np.zeros(7, dtype=np.int64), 8, ValueError, "one label per observation"),
    (np.array([0, 1, -1, 0, 1, 0, 1, 0]), 8, ValueError, "negative fold label"),
    (np.array([0, 2, 0, 2, 0, 2, 0, 2]), 8, ValueError, "empty fold 1"),
    (np.zeros(1025, dtype=np.int32), 1025, ValueError, "the limit is 1024"),
    (np.zeros(8), 8, TypeError, "integer array"),
])
def test_the_mirror_refuses_bad_fold_labels(agp, folds, n, exc, reason):
    fx = agp.GP(agp.SqExponentialKernel())(np.linspace(0.0, 1.0, n), 0.1)
    for call in (agp.kfold_logpdf, agp.kfold_mean_and_var):
        with pytest.raises(exc, match=reason):
            call(fx, np.zeros(n), folds)
