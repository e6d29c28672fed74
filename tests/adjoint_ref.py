"""Float64 reference of the transposed polyphase operator that scales to long signals (numpy only, no GPU).

The ground truth of the adjoint tests is the dense matrix A [n_y, n_x] from the oracle's forward on unit impulses
(`dense`); at 20 000 frames it would take gigabytes.  `scatter` is the forward's own definition (csrc/plan.h locate())
read the other way round,

    y[k] = sum_{j<T} bank[p_k][j] x[n0_k + j],   n0_k = floor(k M / L) - (T/2 - 1),   p_k = (k M) mod L,   x zero outside [0, n_x)
    =>   gx[n0_k + j] += bank[p_k][j] gy[k],

accumulated with np.add.at in float64, together with its magnitude twin |A|^T |gy| (what error bounds are scaled by).
tests/test_adjoint_ref.py pins it to the dense matrix.

Interpolated-phase plans have no such closed form here, on purpose: `column` is ONE column of the dense matrix, the oracle's
forward on one unit impulse, at any length (about 10 ms at 20 000 frames) — the adjoint formula is not restated for them.
`probes` says which columns a long job is looked at: the ends, the seams of the kernel's tiling, and random ones."""
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


def column(oracle, pl, bank, a, n_x, mode):
    """Column a of A for a job of n_x frames, [out_len(n_x)] float64: the oracle's forward on the unit impulse e_a.
    pl: anything with L, M, T and phases (an oracle plan; a namespace will do).  mode "ref": float64 on `bank` as given;
    "port_f64" / "port_f32": the engine's own order and width — on a unit impulse every product but one is an exact zero, so
    with bank=Plan.bank() the column holds the very coefficients the engine multiplies by (tests/test_gpu_adjoint_interp.py
    argues this for its dense matrix), the float32 ones widened."""
    assert 0 <= a < n_x
    e = np.zeros(n_x, np.float32 if mode == "port_f32" else np.float64)
    e[a] = 1.0
    n_out = int(oracle.lib().oracle_out_len(int(n_x), int(pl.L), int(pl.M)))
    return oracle.resample_channel(pl, e, mode, n_out=n_out, bank=bank).astype(np.float64)


def probes(n_x, seams, rng, count):
    """Sorted frame positions of a job of n_x frames, at most `count` of them (at least the ends): 0, n_x - 1, every seam s
    (a tile edge of the kernel: the caller says where) with the frame before it, s - 1 — where the seams would take more
    than two thirds of the positions, a random choice of them — and random positions from `rng` (a numpy Generator) for the
    rest."""
    assert n_x >= 1
    seams = sorted(set(int(s) for s in seams if 0 < int(s) < n_x))
    pairs = max(count - 2, 0) // 3
    if len(seams) > pairs:
        seams = sorted(int(s) for s in rng.choice(seams, size=pairs, replace=False)) if pairs else []
    want = [0, n_x - 1]
    for s in seams:
        want += [s - 1, s]
    out = []
    for p in want:
        if 0 <= p < n_x and p not in out and len(out) < max(count, 2):
            out.append(p)
    free = n_x - len(out)
    extra = min(max(count - len(out), 0), free)
    if extra:
        if n_x <= 4 * count:
            rest = [p for p in range(n_x) if p not in out]
            out += [int(p) for p in rng.choice(rest, size=extra, replace=False)]
        else:
            while extra:
                p = int(rng.integers(0, n_x))
                if p not in out:
                    out.append(p)
                    extra -= 1
    return sorted(out)
