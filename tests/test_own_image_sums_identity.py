"""
The algebra behind the image-owning decoder build's transform-gradient sums (pv_sdec_fused_w8.hip, epilogue), in float64 numpy,
independent of the kernel.  Per row the coordinate layer's input gradient is d_k[row] = sum_j Wc[j][k] dpre0[row][j], the
transformed coordinates are x_k = sc u_k + t_k, and the latent backward consumes the sums over an image's rows of
    sc (d1 u0 - d0 u1)   d(phi)        d0 u0 + d1 u1   d(scale)        d0   d(tx)        d1   d(ty).
The kernel forms them from the column sums H_j = sum_rows dpre0, A_j = sum_rows dpre0 x_0, B_j = sum_rows dpre0 x_1 instead.
"""
import numpy as np
import pytest


def _per_row(dpre0, wc, u, sc, t):
    d = dpre0 @ wc                                    # (rows, 2)
    d0, d1, u0, u1 = d[:, 0], d[:, 1], u[:, 0], u[:, 1]
    return np.array([(sc * (d1 * u0 - d0 * u1)).sum(), (d0 * u0 + d1 * u1).sum(), d0.sum(), d1.sum()])


def _from_column_sums(dpre0, wc, u, sc, t, per_unit):
    x = sc * u + t
    H, A, B = dpre0.sum(0), dpre0.T @ x[:, 0], dpre0.T @ x[:, 1]
    w0, w1 = wc[:, 0], wc[:, 1]
    if per_unit:       # the translation taken out per hidden unit, before the dot product (what the kernel does)
        a, b = A - t[0] * H, B - t[1] * H
        return np.array([w1 @ a - w0 @ b, (w0 @ a + w1 @ b) / sc, w0 @ H, w1 @ H])
    T0, T1 = w0 @ H, w1 @ H
    P00, P01, P10, P11 = w0 @ A, w0 @ B, w1 @ A, w1 @ B
    return np.array([(P10 - t[0] * T1) - (P01 - t[1] * T0), ((P00 - t[0] * T0) + (P11 - t[1] * T1)) / sc, T0, T1])


@pytest.mark.parametrize("per_unit", [False, True])
@pytest.mark.parametrize("rows, sc, tmag, coord_dim", [(16, 1.0, 0.1, 1), (64, 0.83, 0.1, 2), (144, 1.21, 2.0, 2), (784, 1.0, 0.3, 2)])
def test_row_sums_from_column_sums(rows, sc, tmag, coord_dim, per_unit):
    rng = np.random.default_rng(rows)
    dpre0 = rng.standard_normal((rows, 128))
    wc = rng.standard_normal((128, 2))
    u = rng.uniform(-1.0, 1.0, (rows, 2))
    t = tmag * rng.standard_normal(2)
    if coord_dim == 1:                                # one coordinate: Wc's second column, u1 and ty do not exist — zeros
        wc[:, 1] = 0.0
        u[:, 1] = 0.0
        t[1] = 0.0
    want = _per_row(dpre0, wc, u, sc, t)
    got = _from_column_sums(dpre0, wc, u, sc, t, per_unit)
    scale = np.abs(dpre0 @ wc).sum() * (1.0 + np.abs(t).max())        # the size of the terms that are summed
    assert np.all(np.abs(got - want) <= 1e-12 * scale), (got, want)
    if coord_dim == 1:
        assert got[0] == 0.0 and got[3] == 0.0
