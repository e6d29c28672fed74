"""Float64 reference of the transposed polyphase operator that scales to long signals (numpy only, no GPU).

The ground truth of the adjoint tests is the dense matrix A [n_y, n_x] from the oracle's forward on unit impulses
(`dense`); at 20 000 frames it would take gigabytes.  `scatter` is the forward's own definition (csrc/plan.h locate())
read the other way round,

    y[k] = sum_{j<T} bank[p_k][j] x[n0_k + j],   n0_k = floor(k M / L) - (T/2 - 1),   p_k = (k M) mod L,   x zero outside [0, n_x)
    =>   gx[n0_k + j] += bank[p_k][j] gy[k],

accumulated with np.add.at in float64, together with its magnitude twin |A|^T |gy| (what error bounds are scaled by).
tests/test_adjoint_ref.py pins it to the dense matrix."""
import numpy as np


def scatter(L, M, bank, gy, n_x):
    """bank: [L][T] float64; gy: [n_y] or [n_y, columns] -> (A^T gy, |A|^T |gy|), each [n_x] or [n_x, columns], float64."""
    bank = np.asarray(bank, np.float64)
    g = np.asarray(gy, np.float64)
    mono = g.ndim == 1
    g = g.reshape(g.shape[0], -1)
    n_y, T = g.shape[0], bank.shape[1]
    assert bank.shape[0] == L
    gx, mag = np.zeros((n_x, g.shape[1])), np.zeros((n_x, g.shape[1]))
    step = max(1, (1 << 22) // (T * g.shape[1]))  # (rows of gy per pass: a few tens of MB of products at a time)
    for k0 in range(0, n_y, step):
        k = np.arange(k0, min(k0 + step, n_y), dtype=np.int64)
        n0, p = k * M // L - (T // 2 - 1), k * M % L
        idx = n0[:, None] + np.arange(T)[None, :]                      # [k, j]: the input frame tap j of output k reads
        ok = (idx >= 0) & (idx < n_x)
        c = bank[p]                                                     # [k, j]
        np.add.at(gx, idx[ok], (c[:, :, None] * g[k][:, None, :])[ok])
        np.add.at(mag, idx[ok], (np.abs(c)[:, :, None] * np.abs(g[k])[:, None, :])[ok])
    return (gx[:, 0], mag[:, 0]) if mono else (gx, mag)


def dense(oracle, pl, bank, n_x):
    """A [n_y, n_x] float64: the oracle's forward ("ref" mode, on `bank`) applied to the n_x unit impulses."""
    eye = np.eye(n_x)
    return np.stack([oracle.resample_channel(pl, eye[a], "ref", bank=bank) for a in range(n_x)], axis=1)
