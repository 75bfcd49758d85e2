"""NumPy float64 restatement of ``snd_latent_mi`` (include/snd_vae.h, ABI 25): column ranges,
the bin rule, the joint counts, mi, hz and hf.  Plain NumPy: importable without a GPU.

Every step is the header's, on the same fp32 inputs: lo / hi are the fp32 minimum and maximum
of a column, a value goes to min(nb - 1, floor((v - lo) * nb / (hi - lo))) evaluated in float64
left to right (bin 0 for a constant column), and the sums over a joint block run a major, b
minor.
"""
from __future__ import annotations

import numpy as np


def column_range(x):
    """[columns, 2] float32 {lo, hi} of a float32 [rows, columns] matrix."""
    x = np.asarray(x, np.float32)
    return np.stack([x.min(axis=0), x.max(axis=0)], axis=1)


def bin_column(v, lo, hi, nb):
    """The bin of every value of one column (int64), by the header's rule."""
    v = np.asarray(v, np.float32).astype(np.float64)
    lo, hi = np.float64(np.float32(lo)), np.float64(np.float32(hi))
    if not hi > lo:
        return np.zeros(v.shape, np.int64)
    t = np.floor((v - lo) * np.float64(nb) / (hi - lo))
    return np.minimum(nb - 1, t.astype(np.int64))


def bin_matrix(x, nb):
    """Bins of a [rows, columns] matrix, column by column, and its ranges."""
    x = np.asarray(x, np.float32)
    rng = column_range(x)
    bins = np.stack([bin_column(x[:, c], rng[c, 0], rng[c, 1], nb) for c in range(x.shape[1])], axis=1)
    return bins, rng


def joint_counts(zb, fb, nbz, nbf):
    """joint [L, K, nbz, nbf] int64 from the bin labels zb [rows, L] and fb [rows, K]."""
    L, K = zb.shape[1], fb.shape[1]
    out = np.zeros((L, K, nbz, nbf), np.int64)
    cell = nbz * nbf
    for k in range(K):
        idx = np.arange(L)[None, :] * cell + zb * nbf + fb[:, k:k + 1]           # [rows, L]
        out[:, k] = np.bincount(idx.reshape(-1), minlength=L * cell).reshape(L, nbz, nbf)
    return out


def entropy_of(counts, rows):
    """-sum (r / rows) log(r / rows) over the non-empty bins, in index order."""
    acc = 0.0
    for r in counts:
        if r > 0:
            p = float(r) / float(rows)
            acc += p * np.log(p)
    return -acc


def mi_of(block, rows):
    """sum_{c > 0} (c / rows) log(c rows / (r_a s_b)) over one [nbz, nbf] block, a major."""
    r, s = block.sum(axis=1), block.sum(axis=0)
    n = float(rows)
    acc = 0.0
    for a in range(block.shape[0]):
        for b in range(block.shape[1]):
            c = int(block[a, b])
            if c > 0:
                acc += (float(c) / n) * np.log(float(c) * n / (float(r[a]) * float(s[b])))
    return acc


def mi_all(joint, rows):
    """``mi_of`` for every (l, k) at once: the same terms, added in the same order (one
    vector addition per cell, a major, b minor)."""
    L, K, nbz, nbf = joint.shape
    n = float(rows)
    c = joint.astype(np.float64)
    r = joint.sum(axis=3).astype(np.float64)[:, :, :, None]
    s = joint.sum(axis=2).astype(np.float64)[:, :, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = np.where(joint > 0, (c / n) * np.log(c * n / (r * s)), 0.0).reshape(L, K, nbz * nbf)
    acc = np.zeros((L, K))
    for i in range(nbz * nbf):
        acc += terms[:, :, i]
    return acc


def latent_mi_ref(z, f, nbz, nbf):
    """{'mi' [L, K], 'hz' [L], 'hf' [K], 'joint' [L, K, nbz, nbf] int64, 'range' [L + K, 2]
    float32, 'zb', 'fb' (the bin labels)} of float32 z [rows, L] and f [rows, K]."""
    z, f = np.asarray(z, np.float32), np.asarray(f, np.float32)
    rows = z.shape[0]
    assert f.shape[0] == rows and z.ndim == 2 and f.ndim == 2
    zb, zr = bin_matrix(z, nbz)
    fb, fr = bin_matrix(f, nbf)
    joint = joint_counts(zb, fb, nbz, nbf)
    L, K = z.shape[1], f.shape[1]
    mi = mi_all(joint, rows)
    hz = np.array([entropy_of(joint[l, 0].sum(axis=1), rows) for l in range(L)])
    hf = np.array([entropy_of(joint[0, k].sum(axis=0), rows) for k in range(K)])
    return {"mi": mi, "hz": hz, "hf": hf, "joint": joint, "range": np.concatenate([zr, fr]), "zb": zb, "fb": fb}


def random_case(rows, n_lat, n_fac, seed, levels=5):
    """Normal latents (a few of them correlated with a factor) and integer-coded factors."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, levels, size=(rows, n_fac)).astype(np.float32)
    z = rng.standard_normal((rows, n_lat)).astype(np.float32)
    for l in range(0, n_lat, 3):
        z[:, l] += f[:, l % n_fac]
    return z, f
