"""snd_vae_amd.ops, the host wrappers of the fp32 C ABI ops, against float64 torch
restatements at shapes chosen for the wrappers' own risk: a wrong leading dimension or a
wrong transpose.  Operands are column slices of wider tensors where the wrapper takes a
leading dimension, and a given output lies inside a guard band that must stay untouched.
Tolerance: tests/test_gpu_autograd.py's, 1e-5 of the reference block's max-abs (fp32 sums in
a different order)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BNC = 1.0 / (1.0 + 1e-3) ** 0.5
GUARD = 777.0


@pytest.fixture(scope="module")
def ops(lib_built):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")
    from snd_vae_amd import ops
    return ops


def _close(got, ref, tol=1e-5):
    got, ref = got.detach().double().cpu(), ref.detach().double()
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) <= tol * max(float(ref.abs().max()), 1e-30)


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float()


def _sliced(t, pad=(2, 3)):
    """t as a column slice of a wider device tensor: (the view, its leading dimension, the wide tensor)."""
    wide = torch.full((t.shape[0], pad[0] + t.shape[1] + pad[1]), GUARD)
    wide[:, pad[0]:pad[0] + t.shape[1]] = t
    wide = wide.cuda()
    return wide[:, pad[0]:pad[0] + t.shape[1]], wide.shape[1], wide


def _guards_intact(wide, width, pad=(2, 3)):
    w = wide.cpu()
    assert bool((w[:, :pad[0]] == GUARD).all()) and bool((w[:, pad[0] + width:] == GUARD).all())


def _act(v, act):
    return v if act == 0 else (torch.relu(v) if act == 1 else F.leaky_relu(v, 0.2))


def _bn_act_ref(y, gamma, beta, act, first):
    return (_act(y, act) * (gamma * BNC) + beta) if first else _act(y * (gamma * BNC) + beta, act)


@pytest.mark.parametrize("sliced,bias", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("ta", [False, True])
@pytest.mark.parametrize("tb", [False, True])
@pytest.mark.parametrize("m,n,k", [(3, 5, 7), (33, 65, 17)])
def test_gemm(ops, m, n, k, ta, tb, sliced, bias):
    a = _rand(*((k, m) if ta else (m, k)), seed=1)
    b = _rand(*((n, k) if tb else (k, n)), seed=2)
    bv = _rand(n, seed=3) if bias else None
    ref = (a.double().T if ta else a.double()) @ (b.double().T if tb else b.double())
    if bias:
        ref = ref + bv.double()
    if not sliced:
        _close(ops.gemm(a.cuda(), b.cuda(), ta=ta, tb=tb), ref)
        return
    av, lda, _ = _sliced(a)
    bview, ldb, _ = _sliced(b)
    out, ldc, wide = _sliced(torch.full((m, n), GUARD))
    got = ops.gemm(av, bview, ta=ta, tb=tb, bias=bv.cuda() if bias else None, out=out, lda=lda, ldb=ldb, ldc=ldc)
    assert got is out
    _close(out, ref)
    _guards_intact(wide, n)


@pytest.mark.parametrize("rows", [1, 130])
def test_colsum(ops, rows):
    g = _rand(rows, 6, seed=4)
    gv, ld, _ = _sliced(g)
    ref = g.double().sum(0)
    _close(ops.colsum(gv, ld=ld), ref)
    out = torch.full((3, 6), GUARD).cuda()                              # a given row between two guard rows
    ops.colsum(gv, out=out[1], ones=torch.ones(rows + 5).cuda(), ld=ld)
    _close(out[1], ref)
    assert bool((out[0] == GUARD).all()) and bool((out[2] == GUARD).all())


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("first", [0, 1])
def test_bn_act_forward_and_backward(ops, act, first):
    rows, c = 37, 6
    y, dx = _rand(rows, c, seed=5), _rand(rows, c, seed=6)
    gamma, beta = 1.0 + 0.3 * _rand(c, seed=7), 0.2 * _rand(c, seed=8)
    yr, gr, br = (t.double().requires_grad_(True) for t in (y, gamma, beta))
    ref = _bn_act_ref(yr, gr, br, act, first)
    rdy, rdg, rdb = torch.autograd.grad(ref, (yr, gr, br), dx.double())
    yv, ldy, _ = _sliced(y)
    out, ldx, wide = _sliced(torch.full((rows, c), GUARD))
    ops.bn_act(yv, gamma.cuda(), beta.cuda(), act, first, out=out, ldy=ldy, ldx=ldx)
    _close(out, ref)
    _guards_intact(wide, c)
    _close(ops.bn_act(y.cuda(), gamma.cuda(), beta.cuda(), act, first), ref)
    dxv, lddx, _ = _sliced(dx)
    dg = torch.full((c,), GUARD).cuda()
    dy, dg2, db = ops.bn_act_bwd(dxv, yv, gamma.cuda(), beta.cuda(), act, first, dgamma=dg, lddx=lddx, ldy=ldy)
    assert dg2 is dg
    _close(dy, rdy)
    _close(dg, rdg)
    _close(db, rdb)


def _conv_ref(x, w, b, n):
    """conv1d(k=5, SAME) over each graph's n rows, w [5, cin, cout] (the TF kernel layout)."""
    g = x.shape[0] // n
    y = F.conv1d(x.view(g, n, -1).permute(0, 2, 1), w.permute(2, 1, 0), b, padding=2)
    return y.permute(0, 2, 1).reshape(g * n, -1)


@pytest.mark.parametrize("n", [7, 25])
def test_conv1d_same(ops, n):
    cin, cout, rows = 3, 5, 2 * n
    x, w, b, dy = _rand(rows, cin, seed=9), 0.3 * _rand(5, cin, cout, seed=10), _rand(cout, seed=11), \
        _rand(rows, cout, seed=12)
    gamma, beta = 1.0 + 0.3 * _rand(cout, seed=13), 0.2 * _rand(cout, seed=14)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    ref = _conv_ref(xr, wr, b.double(), n)
    rdx, rdw = torch.autograd.grad(ref, (xr, wr), dy.double())
    xd, wd, bd, dyd = x.cuda(), w.cuda(), b.cuda(), dy.cuda()
    out, pre = ops.conv1d_same(xd, wd, bd, n)
    assert pre is None
    _close(out, ref)
    xv, ldx, _ = _sliced(x)
    _close(ops.conv1d_same(xv, wd, bd, n, ldx=ldx)[0], ref)
    out, pre = ops.conv1d_same(xd, wd, bd, n, gamma.cuda(), beta.cuda())
    _close(pre, ref)
    _close(out, _bn_act_ref(ref.detach(), gamma.double(), beta.double(), 2, 0))
    _close(ops.conv1d_same_bwd_data(dyd, wd, n), rdx)
    _close(ops.conv1d_same_bwd_weight(xd, dyd, n), rdw)


def test_sigmoid_mse_and_sigmoid_linear(ops):
    rows, cin, cout = 50, 4, 3
    u, w, b = _rand(rows, cin, seed=15), _rand(cin, cout, seed=16), _rand(cout, seed=17)
    target = torch.sigmoid(_rand(rows, cout, seed=18))
    ur, wr, br = (t.double().requires_grad_(True) for t in (u, w, b))
    yhat = torch.sigmoid(ur @ wr + br)
    sse_ref = ((yhat - target.double()) ** 2).sum()
    rdu, rdw, rdb = torch.autograd.grad(sse_ref / (rows * cout), (ur, wr, br))
    sse, got, du, dw, db = ops.sigmoid_mse(u.cuda(), w.cuda(), b.cuda(), target.cuda())
    assert sse.dtype == torch.float64 and float(sse.sum()) == pytest.approx(float(sse_ref.detach()), rel=1e-5)
    for a, r in ((got, yhat), (du, rdu), (dw, rdw), (db, rdb)):
        _close(a, r)
    dw1, db1 = torch.ones(cin, cout).cuda(), torch.ones(cout).cuda()    # given gradients are added to
    ops.sigmoid_mse(u.cuda(), w.cuda(), b.cuda(), target.cuda(), dw=dw1, db=db1)
    _close(dw1, rdw + 1.0)
    _close(db1, rdb + 1.0)
    _close(ops.sigmoid_linear(u.cuda(), w.cuda(), b.cuda()), yhat)


@pytest.mark.parametrize("with_add", [False, True])
def test_reparam_kl_and_bwd(ops, with_add):
    rows, lat = 3, 5
    ms, eps, dz = 0.5 * _rand(rows, 2 * lat, seed=19), _rand(rows, lat, seed=20), _rand(rows, lat, seed=21)
    add_mu, add_s = (_rand(rows, lat, seed=22), _rand(rows, lat, seed=23)) if with_add else (None, None)
    mu, s = ms.double()[:, :lat], ms.double()[:, lat:]
    z, kl = ops.reparam_kl(ms.cuda(), eps.cuda())
    _close(z, mu + eps.double() * torch.exp(s))
    assert kl.dtype == torch.float64
    assert float(kl.sum()) == pytest.approx(float((1 + 2 * s - mu ** 2 - torch.exp(2 * s)).sum()), rel=1e-5)
    ref = torch.cat([dz.double(), dz.double() * eps.double() * torch.exp(s)], 1)
    if with_add:
        ref = ref + torch.cat([add_mu.double(), add_s.double()], 1)
    dev = lambda t: None if t is None else t.cuda()
    _close(ops.reparam_bwd(ms.cuda(), eps.cuda(), dz.cuda(), dev(add_mu), dev(add_s)), ref)


def test_add_strided(ops):
    rows, cols = 9, 4
    x, y = _rand(rows, cols, seed=24), _rand(rows, cols, seed=25)
    xv, ldx, _ = _sliced(x)
    yv, ldy, wide = _sliced(y, pad=(1, 6))
    assert ops.add_strided(xv, yv, alpha=0.5, ldx=ldx, ldy=ldy) is yv
    _close(yv, y.double() + 0.5 * x.double())
    _guards_intact(wide, cols, pad=(1, 6))
    yd = y.cuda()
    ops.add_strided(x.cuda(), yd)
    _close(yd, y.double() + x.double())


def test_spmm_with_an_isolated_row(ops):
    n, width = 6, 5
    adj = torch.zeros(n, n, dtype=torch.float64)
    for i, j in ((0, 1), (0, 4), (1, 2), (2, 5), (4, 5)):               # row 3 has no neighbour
        adj[i, j] = adj[j, i] = 1.0
    rowptr = torch.tensor([0] + adj.sum(1).cumsum(0).tolist(), dtype=torch.int32).cuda()
    colidx = adj.nonzero()[:, 1].to(torch.int32).cuda()
    h = _rand(n, width, seed=26)
    out = ops.spmm(rowptr, colidx, h.cuda())
    _close(out, adj @ h.double())
    assert float(out[3].abs().max()) == 0.0
    _close(ops.spmm(rowptr[:4].contiguous(), colidx, h.cuda(), n_out=3), (adj @ h.double())[:3])
