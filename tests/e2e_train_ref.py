"""Float64 restatement of exactly what ``snd_e2e_train`` (ABI 24) computes; importable
without a GPU.

The factorised layer 0 forward and backward, and the V_t form of a general layer (forward,
weight gradient, data gradient): every formula of include/snd_vae.h, written out in numpy.
``train_ref`` returns what ``oracle.ref_disent.structure_decoder_grads`` returns (which
differentiates the literal pair-tensor model with autograd), so the two can be compared
block by block (tests/test_e2e_train_cpu.py).  ``operands`` and ``kink_margins`` build the
test operands of the GPU tests and measure how far they sit from the relu kinks.
"""
from types import SimpleNamespace as NS

import numpy as np

from oracle import ref_disent as RD

BN_C = RD.BN_C
F = lambda a: np.asarray(a, np.float64)

# (B, N, D, hidden) of the CPU comparison (the issue's list, then N = 1 and N = 2)
CPU_SHAPES = ((2, 7, 3, (5, 4)), (1, 8, 5, (33, 32)), (2, 25, 6, (50, 20)), (2, 6, 4, (6,)), (2, 5, 2, (9, 7, 5)),
              (2, 1, 3, (4, 3)), (1, 2, 3, (4, 3)))


def shift(x, s, axis):
    """out[.., n, ..] = x[.., n + s, ..] along ``axis``, zero where n + s is out of range."""
    out = np.zeros_like(x)
    n = x.shape[axis]
    if abs(s) >= n:
        return out
    src = [slice(None)] * x.ndim
    dst = [slice(None)] * x.ndim
    src[axis] = slice(max(s, 0), n + min(s, 0))
    dst[axis] = slice(max(-s, 0), n + min(-s, 0))
    out[tuple(dst)] = x[tuple(src)]
    return out


def taps_in(x, t, pb):
    """V_t[b,i,j] = x[b, i, j+t-pb] + x[b, i+t-pb, j]: the two inputs of tap t, added first."""
    return shift(x, t - pb, 2) + shift(x, t - pb, 1)


def layer_fwd(x, w, b):
    N = x.shape[1]
    pb = (N - 1) // 2
    return sum(taps_in(x, t, pb) @ w[t] for t in range(N)) + 2 * b


def layer_bwd(x, w, g):
    """(dx, dw, db) of a general layer in the V_t form; g = dy."""
    N = x.shape[1]
    pb = (N - 1) // 2
    dw = np.stack([np.einsum("bijc,bijo->co", taps_in(x, t, pb), g) for t in range(N)])
    dx = sum(taps_in(g, pb - t, 0) @ w[t].T for t in range(N))   # g[b,i,j-t+pb] + g[b,i-t+pb,j]
    return dx, dw, 2 * g.sum((0, 1, 2))


def bn_relu_bwd(dx, y, gamma, beta):
    """dy, dgamma, dbeta of x = relu(gamma BN_C y + beta)."""
    dt = dx * (gamma * BN_C * y + beta > 0)
    red = tuple(range(y.ndim - 1))
    return dt * gamma * BN_C, (dt * BN_C * y).sum(red), dt.sum(red)


def layer0_fwd(z, l0):
    """y0 and what the backward reuses: a, a', Wsum."""
    B, N, D = z.shape
    g, be, w, b = F(l0["gamma"]), F(l0["beta"]), F(l0["w"]), F(l0["b"])
    pb = (N - 1) // 2
    a = np.maximum(g[:D] * BN_C * z + be[:D], 0)
    ap = np.maximum(g[D:] * BN_C * z + be[D:], 0)
    wsum = np.zeros_like(w)
    P, Q = np.zeros((B, N, w.shape[2])), np.zeros((B, N, w.shape[2]))
    for n in range(N):
        for t in range(N):
            m = n + t - pb
            if 0 <= m < N:
                wsum[n] += w[t]
                P[:, n] += a[:, m] @ w[t, :D]
                Q[:, n] += ap[:, m] @ w[t, D:]
    y = (np.einsum("bic,jco->bijo", a, wsum[:, :D]) + np.einsum("bjc,ico->bijo", ap, wsum[:, D:])
         + P[:, :, None, :] + Q[:, None, :, :] + 2 * b)
    return y, a, ap, wsum


def layer0_bwd(z, l0, a, ap, wsum, g):
    """(dz, {gamma, beta, w, b}) of the factorised layer 0; g = dy0 [B, N, N, O]."""
    B, N, D = z.shape
    gam, be, w = F(l0["gamma"]), F(l0["beta"]), F(l0["w"])
    pb = (N - 1) // 2
    R, S = g.sum(2), g.sum(1)                                   # [b,i,o], [b,j,o]
    da = np.einsum("bijo,jco->bic", g, wsum[:, :D])
    dap = np.einsum("bijo,ico->bjc", g, wsum[:, D:])
    dwsum = np.zeros_like(w)
    dwsum[:, :D] = np.einsum("bic,bino->nco", a, g)
    dwsum[:, D:] = np.einsum("bjc,bnjo->nco", ap, g)
    dw = np.zeros_like(w)
    for t in range(N):
        for n in range(N):
            m = n + t - pb                                      # tap t reads node m for output node n
            if 0 <= m < N:
                dw[t] += dwsum[n]
                dw[t, :D] += np.einsum("bc,bo->co", a[:, m], R[:, n])
                dw[t, D:] += np.einsum("bc,bo->co", ap[:, m], S[:, n])
                da[:, m] += R[:, n] @ w[t, :D].T                # da[b,i] += R[b,i-t+pb] w[t]^T with i = m
                dap[:, m] += S[:, n] @ w[t, D:].T
    dta = da * (gam[:D] * BN_C * z + be[:D] > 0)
    dtp = dap * (gam[D:] * BN_C * z + be[D:] > 0)
    dz = BN_C * (gam[:D] * dta + gam[D:] * dtp)
    dgamma = np.concatenate([(dta * BN_C * z).sum((0, 1)), (dtp * BN_C * z).sum((0, 1))])
    dbeta = np.concatenate([dta.sum((0, 1)), dtp.sum((0, 1))])
    return dz, {"gamma": dgamma, "beta": dbeta, "w": dw, "b": 2 * g.sum((0, 1, 2))}


def head_ce(y, adj, head):
    """(CE sum, correct, dy of the MEAN CE, head grads): relu(BN_adj(y)) W + b, the diagonal (1, 0)."""
    B, N = y.shape[:2]
    g, be, W, b = (F(head[k]) for k in ("gamma", "beta", "w", "b"))
    A = F(adj)
    t = g * BN_C * y + be
    x = np.maximum(t, 0)
    logits = x @ W + b
    eye = np.eye(N, dtype=bool)[None]
    l0 = np.where(eye, 1.0, logits[..., 0])
    l1 = np.where(eye, 0.0, logits[..., 1])
    mx = np.maximum(l0, l1)
    lse = mx + np.log(np.exp(l0 - mx) + np.exp(l1 - mx))
    ce = (lse - (1 - A) * l0 - A * l1).sum()
    correct = float(((l1 > l0).astype(np.float64) == A).sum())
    M = B * N * N
    d0 = np.where(eye, 0.0, (np.exp(l0 - lse) - (1 - A)) / M)
    d1 = np.where(eye, 0.0, (np.exp(l1 - lse) - A) / M)
    dl = np.stack([d0, d1], -1)
    dx = dl @ W.T
    dy, dgamma, dbeta = bn_relu_bwd(dx, y, g, be)
    return ce, correct, dy, {"gamma": dgamma, "beta": dbeta, "w": np.einsum("bijc,bijk->ck", x, dl),
                             "b": dl.sum((0, 1, 2))}


def train_ref(z, adj, layers, head):
    """(mean CE, correct, dz, layer grads, head grads) as snd_e2e_train computes them, float64."""
    z = F(z)
    B, N, D = z.shape
    y, a, ap, wsum = layer0_fwd(z, layers[0])
    ys = [y]
    for l in layers[1:]:
        x = np.maximum(F(l["gamma"]) * BN_C * ys[-1] + F(l["beta"]), 0)
        ys.append(layer_fwd(x, F(l["w"]), F(l["b"])))
    ce, correct, g, hg = head_ce(ys[-1], adj, head)
    grads = [None] * len(layers)
    for i in range(len(layers) - 1, 0, -1):
        l = layers[i]
        x = np.maximum(F(l["gamma"]) * BN_C * ys[i - 1] + F(l["beta"]), 0)
        dx, dw, db = layer_bwd(x, F(l["w"]), g)
        g, dgamma, dbeta = bn_relu_bwd(dx, ys[i - 1], F(l["gamma"]), F(l["beta"]))
        grads[i] = {"gamma": dgamma, "beta": dbeta, "w": dw, "b": db}
    dz, grads[0] = layer0_bwd(z, layers[0], a, ap, wsum, g)
    return ce / (B * N * N), correct, dz, grads, hg


# ---------------------------------------------------------------- operands, kink margins
def operands(B, N, D, hidden, seed, beta_far=0.0):
    """z, a random symmetric 0/1 adjacency with a zero diagonal, layers, head (float32 values).
    ``beta_far`` > 0 draws every BN beta as +-beta_far (1 + 0.1 |n|) and scales every gamma by
    0.1: whole channels on or off, for shapes with too many pre-activations for all of them to
    miss zero by chance."""
    rng = np.random.default_rng([B, N, D, *hidden, seed])
    nrm = lambda *s: rng.standard_normal(s).astype(np.float32)
    beta = lambda n: (np.sign(nrm(n)) * np.float32(beta_far) * (1 + 0.1 * np.abs(nrm(n)))).astype(np.float32) \
        if beta_far else 0.3 * nrm(n)
    gs = np.float32(0.1 if beta_far else 1.0)
    z = nrm(B, N, D)
    up = np.triu(rng.random((B, N, N)) < 0.4, 1)
    adj = (up | up.transpose(0, 2, 1)).astype(np.float32)
    layers, cin = [], 2 * D
    for co in hidden:
        gamma = gs * (1 + 0.3 * nrm(cin))
        gamma[::3] *= -1                              # negative gammas: relu kills where y is large
        layers.append({"gamma": gamma, "beta": beta(cin), "w": nrm(N, cin, co) / np.float32(np.sqrt(2 * N * cin)),
                       "b": 0.3 * nrm(co)})
        cin = co
    gamma = gs * (1 + 0.3 * nrm(cin))
    gamma[::3] *= -1
    head = {"gamma": gamma, "beta": beta(cin), "w": nrm(cin, 2) / np.float32(np.sqrt(cin)), "b": 0.1 * nrm(2)}
    return NS(B=B, N=N, D=D, hidden=tuple(hidden), z=z, adj=adj, layers=layers, head=head)


def preacts(z, layers, head, dtype):
    """Every BN pre-activation of the literal model (pair concat, e2e per layer) in ``dtype``:
    a list with one [B, N, N, C] tensor per layer and one for the head, as float64 numpy.

    This is ``disent_infer_ref.structure_literal`` line by line (the same pair concat, the same
    ``oracle.ref_disent.e2e_torch``, the same BN expression), returning the arguments of its
    relus: that helper, an existing test file, returns only the margin.  ``argmax_margin``
    below calls it for the margin; the two agree on the head's pre-activation by construction."""
    import torch
    tt = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dtype)
    z = tt(z)
    B, N, D = z.shape
    h = torch.cat([z[:, :, None, :].expand(B, N, N, D), z[:, None, :, :].expand(B, N, N, D)], -1)
    out = []
    for l in layers:
        t = tt(l["gamma"]) * h * RD.BN_C + tt(l["beta"])
        out.append(t.double().numpy())
        h = RD.e2e_torch(torch.relu(t), tt(l["w"]), tt(l["b"]))
    out.append((tt(head["gamma"]) * h * RD.BN_C + tt(head["beta"])).double().numpy())
    return out


def kink_margins(c):
    """Per BN stage (layers, then the head): (the smallest |float64 pre-activation|, the
    largest |float32 literal - float64| of that stage's pre-activations)."""
    import torch
    p64 = preacts(c.z, c.layers, c.head, torch.float64)
    p32 = preacts(c.z, c.layers, c.head, torch.float32)
    return [(float(np.abs(a).min()), float(np.abs(b - a).max())) for a, b in zip(p64, p32)]


def off_kinks(c):
    """No pre-activation closer to zero than 10x the stage's float32 error; no exclusions."""
    return all(lo > 10.0 * err for lo, err in kink_margins(c))


def block_errors(got, ref):
    """{block: max |got - ref| / max |ref|} over dz, every layer block and the head block;
    ``got`` / ``ref`` = (dz, layer grads, head grads)."""
    out = {}
    blocks = [("dz", got[0], ref[0])]
    for i, (a, b) in enumerate(zip(got[1], ref[1])):
        blocks += [(f"l{i}_{k}", a[k], b[k]) for k in ("gamma", "beta", "w", "b")]
    blocks += [(f"head_{k}", got[2][k], ref[2][k]) for k in ("gamma", "beta", "w", "b")]
    for name, a, b in blocks:
        a, b = F(a).reshape(-1), F(b).reshape(-1)
        assert a.shape == b.shape, name
        scale = np.abs(b).max()
        err = np.abs(a - b).max()
        out[name] = 0.0 if err == 0 else float(err / scale) if scale > 0 else np.inf
    return out


def argmax_margin(c):
    """(the smallest off-diagonal |l1 - l0| in float64, the largest |float32 literal - float64|
    of the margin): ``correct`` is an exact count only where every argmax is decidable."""
    import torch
    from disent_infer_ref import structure_literal
    m64 = structure_literal(c.z, c.layers, c.head, torch.float64)[0].numpy()
    m32 = structure_literal(c.z, c.layers, c.head, torch.float32)[0].double().numpy()
    offd = np.broadcast_to(~np.eye(c.N, dtype=bool), m64.shape)
    lo = float(np.abs(m64[offd]).min()) if offd.any() else np.inf
    return lo, float(np.abs(m32 - m64).max())
