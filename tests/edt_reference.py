"""The closed form of the batch EDT with the tie rule the HIP passes implement, in plain numpy: shared by the tests that pin the
oracle against it (test_oracle_edt.py) and by the form table of the batch EDT (edt_forms.py, test_edt_forms.py)."""
import numpy as np


def tie_rule_reference(occ):
    """Closed form the HIP passes implement: pass Y nearest in column, ties -> LARGER y;
    pass X argmin_x' (x-x')^2+g^2, ties -> SMALLER x'; pass Z likewise ties -> SMALLER z'."""
    Z, Y, X = occ.shape
    BIG = 1 << 28
    cy = np.full((Z, Y, X), -1, np.int64)
    g2 = np.full((Z, Y, X), BIG, np.int64)
    ys = np.arange(Y)
    for z in range(Z):
        for x in range(X):
            sites = ys[occ[z, :, x]]
            if sites.size == 0:
                continue
            dist = np.abs(ys[:, None] - sites[None, :])
            best = dist.min(axis=1)
            # ties -> larger y': last index achieving the min
            idx = dist.shape[1] - 1 - np.argmin(dist[:, ::-1], axis=1)
            cy[z, :, x] = sites[idx]
            g2[z, :, x] = best ** 2
    xs = np.arange(X)
    cx2 = np.full((Z, Y, X), -1, np.int64)
    cy2 = np.full((Z, Y, X), -1, np.int64)
    d2 = np.full((Z, Y, X), BIG, np.int64)
    for z in range(Z):
        for y in range(Y):
            f = (xs[:, None] - xs[None, :]) ** 2 + g2[z, y, None, :]
            i = np.argmin(f, axis=1)  # first (smallest x') minimum
            ok = g2[z, y, i] < BIG
            d2[z, y, :] = np.where(ok, f[xs, i], BIG)
            cx2[z, y, :] = np.where(ok, i, -1)
            cy2[z, y, :] = np.where(ok, cy[z, y, i], -1)
    zs = np.arange(Z)
    out_d = np.full((Z, Y, X), BIG, np.int64)
    out_c = np.full((Z, Y, X, 3), -1, np.int64)
    for y in range(Y):
        for x in range(X):
            f = (zs[:, None] - zs[None, :]) ** 2 + d2[None, :, y, x]
            i = np.argmin(f, axis=1)
            ok = d2[i, y, x] < BIG
            out_d[:, y, x] = np.where(ok, f[zs, i], BIG)
            out_c[:, y, x, 0] = np.where(ok, cx2[i, y, x], -1)
            out_c[:, y, x, 1] = np.where(ok, cy2[i, y, x], -1)
            out_c[:, y, x, 2] = np.where(ok, i, -1)
    return out_d, out_c
