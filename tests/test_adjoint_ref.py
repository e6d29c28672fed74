"""tests/adjoint_ref.py (the scatter form of the forward's definition, what the long cases of
tests/test_gpu_adjoint_forms.py are compared with) against the dense matrix from the oracle's forward on unit impulses.
No GPU.

Bound: 4e-15 |A|^T |gy| per element.  Both sides are float64 sums of the same at most Tt = ceil(T L / M) + 1 products
(at most 209 of them here), each of which carries a relative error of a few units of 1.1e-16 whatever the order, scaled
by the magnitude sum; the orders differ, the terms do not.

`column` (one column of the dense matrix at any length, what tests/fuzz/fuzz_adjoint.py looks at long jobs through) is held
to `dense` bit for bit and to `scatter` within the same bound on two exact-bank plans, and bit for bit to the dense matrix of
tests/test_gpu_adjoint_interp.py (N_DENSE frames, both widths) on an interpolated-phase plan."""
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


@pytest.mark.parametrize("case,n_x", JOBS[:2], ids=lambda v: "%g-%g-%s" % v if isinstance(v, tuple) else str(v))
def test_column_is_the_dense_column_and_the_scatter_form(case, n_x):
    from oracle import oracle
    from soxr_amd import device as dev
    plan, pl = dev.Plan(*case), oracle.plan(*case)
    bank = plan.bank()
    n_y = plan.out_len(n_x)
    rng = np.random.default_rng(22)
    at = adjoint_ref.probes(n_x, [256, 512, 4 * plan.M], rng, 24)
    assert at[0] == 0 and at[-1] == n_x - 1 and len(at) == 24 and len(set(at)) == 24 and {255, 256, 511, 512} <= set(at)
    eye_cols = {a: adjoint_ref.column(oracle, pl, bank, a, n_x, "ref") for a in at}
    assert all(c.shape == (n_y,) and c.dtype == np.float64 for c in eye_cols.values())
    # dense: the same call on the same impulse, so the same bits (a narrower job: a column does not depend on the job's length)
    n_d = min(n_x, 600)
    A = adjoint_ref.dense(oracle, pl, bank, n_d)
    for a in [a for a in at if a < n_d]:
        assert np.array_equal(eye_cols[a][:A.shape[0]], A[:, a]), a
    assert sum(a < n_d for a in at) >= 3
    # scatter: A^T gy at the probed frames is the dot product with the column
    gy = rng.standard_normal(n_y)
    gx, mag = adjoint_ref.scatter(plan.L, plan.M, bank, gy, n_x)
    for a in at:
        assert abs(gx[a] - eye_cols[a] @ gy) <= 4e-15 * (np.abs(eye_cols[a]) @ np.abs(gy)) + 1e-300
        assert abs(mag[a] - np.abs(eye_cols[a]) @ np.abs(gy)) <= 4e-15 * mag[a] + 1e-300
    # the port modes on an exact bank: the bank's own values, and those rounded to float32
    for a in at[:3]:
        assert np.array_equal(adjoint_ref.column(oracle, pl, bank, a, n_x, "port_f64"), eye_cols[a])
        assert np.array_equal(adjoint_ref.column(oracle, pl, bank, a, n_x, "port_f32"), eye_cols[a].astype(np.float32).astype(np.float64))


def test_column_is_the_dense_column_of_an_interpolated_phase_plan():
    import test_gpu_adjoint_interp as ti
    from oracle import oracle
    case = ti.HQ
    plan, pl = ti._plan(case), oracle.plan(*case)
    assert plan.phases
    rng = np.random.default_rng(23)
    at = adjoint_ref.probes(ti.N_DENSE, [ti._w(), 2 * ti._w(), 3 * ti._w()], rng, 12)
    for kind, mode in ((ti.F64, "port_f64"), (ti.F32, "port_f32")):
        A = ti._dense_n(case, ti.N_DENSE, kind)
        for a in at:
            assert np.array_equal(adjoint_ref.column(oracle, pl, plan.bank(), a, ti.N_DENSE, mode), A[:, a]), (kind, a)
    # a longer job: the column is the shorter job's, continued (the signal is zero outside the job either way)
    a = at[5]
    long = adjoint_ref.column(oracle, pl, plan.bank(), a, 5000, "port_f64")
    assert long.shape == (plan.out_len(5000),) and np.array_equal(long[:A.shape[0]], ti._dense_n(case, ti.N_DENSE, ti.F64)[:, a])
    assert not long[A.shape[0] + plan.taps:].any()


def test_probes_are_deterministic_and_within_the_job():
    for n_x, seams, count in ((1, [256], 32), (2, [], 32), (5, [4], 4), (20000, range(256, 20000, 256), 32), (300, [256], 16)):
        a = adjoint_ref.probes(n_x, seams, np.random.default_rng(1), count)
        assert a == adjoint_ref.probes(n_x, seams, np.random.default_rng(1), count)
        assert a == sorted(set(a)) and a[0] == 0 and a[-1] == n_x - 1 and len(a) == min(n_x, max(count, min(n_x, 2)))
    a = adjoint_ref.probes(20000, range(256, 20000, 256), np.random.default_rng(1), 32)
    assert sum(p % 256 == 0 and p > 0 for p in a) >= 10 and sum(p % 256 == 255 for p in a) >= 10
