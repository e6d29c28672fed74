"""tests/adjoint_ref.py (the scatter form of the forward's definition, what the long cases of
tests/test_gpu_adjoint_forms.py are compared with) against the dense matrix from the oracle's forward on unit impulses.
No GPU.

Bound: 4e-15 |A|^T |gy| per element.  Both sides are float64 sums of the same at most Tt = ceil(T L / M) + 1 products
(at most 209 of them here), each of which carries a relative error of a few units of 1.1e-16 whatever the order, scaled
by the magnitude sum; the orders differ, the terms do not."""
import numpy as np
import pytest

import adjoint_ref

JOBS = [((48000, 44100, "LQ"), 701), ((44100, 8000, "QQ"), 3533), ((16000, 48000, "QQ"), 91), ((9973, 12289, "QQ"), 300)]


@pytest.mark.parametrize("case,n_x", JOBS, ids=lambda v: "%g-%g-%s" % v if isinstance(v, tuple) else str(v))
def test_scatter_form_is_the_dense_transpose(case, n_x):
    from oracle import oracle
    from soxr_amd import device as dev
    plan, pl = dev.Plan(*case), oracle.plan(*case)
    assert not plan.phases
    bank = plan.bank()
    A = adjoint_ref.dense(oracle, pl, bank, n_x)
    assert A.shape == (plan.out_len(n_x), n_x)
    rng = np.random.default_rng(21)
    gy = rng.standard_normal((A.shape[0], 3))
    gx, mag = adjoint_ref.scatter(plan.L, plan.M, bank, gy, n_x)
    want, want_mag = A.T @ gy, np.abs(A).T @ np.abs(gy)
    assert gx.shape == (n_x, 3)
    ratio = float((np.abs(gx - want) / (want_mag + 1e-300)).max())
    ratio_mag = float((np.abs(mag - want_mag) / (want_mag + 1e-300)).max())
    print("scatter reference %s n_x=%d: worst |error| / (|A|^T|gy|) %.3g (magnitude twin %.3g)" % (case, n_x, ratio, ratio_mag))
    assert ratio <= 4e-15 and ratio_mag <= 4e-15
    # a single column, and a truncated cotangent (fewer frames than the plan's output length)
    g1, m1 = adjoint_ref.scatter(plan.L, plan.M, bank, gy[:, 0], n_x)
    assert g1.shape == (n_x,) and np.array_equal(g1, gx[:, 0]) and np.array_equal(m1, mag[:, 0])
    n_t = A.shape[0] - 5
    gt, mt = adjoint_ref.scatter(plan.L, plan.M, bank, gy[:n_t, 1], n_x)
    assert (np.abs(gt - A[:n_t].T @ gy[:n_t, 1]) <= 4e-15 * (np.abs(A[:n_t]).T @ np.abs(gy[:n_t, 1])) + 1e-300).all()
