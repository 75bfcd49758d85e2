"""Hub graphs whose rows sit on every boundary of the row gathers (snd_gather.hpp
gather_rows16, the fused front's feature gather): shared by test_gpu_gather_rounds.py and
test_gather_rounds_cpu.py.

The gathers take a row's neighbour ids 16 per round (two per lane of the row's 8), request
the next round's ids under the current round's rows, and the fused front takes the ids of
the first 32 neighbours at once.  The code changes path at 8 (second id of a lane), 16
(second round), 24 / 32 (the front's prefetched ids end) and every further 16; a wrong
guard shows as a neighbour dropped, read twice, or read past the row's end.  Hub rows of
exactly HUB_DEGREES neighbours cover both sides of each of these; everything else is a
leaf of degree <= 4.

0 neighbours: GraphBatch is a plain CSR and accepts isolated nodes (``isolated=N_ISOLATED``),
but their P0 = (A X) W0 is exactly 0, on the lrelu kink, and the own-operand reference has
to exclude those elements of dP0 (64 per isolated row).  The cases checked against the
reference therefore have none ("nothing excluded" holds for them); the isolated rows are
checked fused against chain, bit for bit, and for their exact zeros.
"""
import numpy as np

from snd_vae_amd.data import GraphBatch, csr_from_pairs, stack_csr

HUB_DEGREES = (1, 15, 16, 17, 31, 32, 33, 48, 49, 65)
# (name, n, d, B): N = 328 is no multiple of 64 or 128; d = 64 runs the fused front, both fused
# heads and the gathered RC_ENC0; d = 128 the two-chunk (NQ = 2) gathers of the bf16 edge kernels
CASES = (("n328_d64", 328, 64, 2), ("n200_d128", 200, 128, 2))
# (batch seed: the first from 21 on for which the float32 / bf16 emulation of both cases puts
# no element on an lrelu kink, tests/test_gather_rounds_cpu.py)
BATCH_SEED, INIT_SEED, EPS_SEED = 24, 2, 9
N_ISOLATED = 8


def hub_positions(n):
    """Ten local rows: the first and the last row of 64-row tiles (every second one also of a
    128-row tile in graph 0; graph 1 starts at row n, so its hubs meet the 128-row tiles of
    the whole batch at other offsets), the last one the graph's last row."""
    if n >= 320:
        return [0, 63, 64, 127, 128, 191, 192, 255, 256, n - 1]
    return [0, 63, 64, 127, 128, 191, 192, 1, 126, n - 1]   # n = 200: four tiles, two inner rows


def hub_graph(n, degrees, rng, isolated=0):
    """Undirected pairs of one graph: hub i at hub_positions(n)[i] with exactly degrees[i]
    neighbours, all of them leaves (no two hubs adjacent).  The leaves are dealt out in turn,
    so a leaf serves at most ceil(sum(degrees) / leaves) hubs; ``isolated`` nodes get no edge."""
    pos = hub_positions(n)
    assert len(set(pos)) == len(degrees)
    leaves = rng.permutation(np.setdiff1d(np.arange(n), pos))
    pool, free = leaves[:len(leaves) - isolated], leaves[len(leaves) - isolated:]
    assert max(degrees) <= len(pool)
    pairs, at = [], 0
    for h, k in zip(pos, degrees):
        pairs += [(h, int(pool[(at + i) % len(pool)])) for i in range(k)]
        at += k
    for a, b in zip(pool[0::2], pool[1::2]):       # leaf-leaf edges: no leaf of the pool is isolated
        pairs.append((int(a), int(b)))
    if len(pool) % 2:
        pairs.append((int(pool[-1]), int(pool[0])))
    return np.array(pairs, np.int64), free


def make_batch(cfg, B, seed=BATCH_SEED, isolated=0):
    """B hub graphs (graph b's first nine hub degrees rotated by 5 b, the graph's -- and so
    the batch's -- last row always the largest hub) with synthetic_batch's features and
    targets."""
    n = cfg.n_nodes
    parts, feats, xs, ss = [], [], [], []
    for b in range(B):
        rng = np.random.default_rng(seed + b)
        deg = list(HUB_DEGREES[:-1])
        deg = deg[(5 * b) % 9:] + deg[:(5 * b) % 9] + [HUB_DEGREES[-1]]
        pairs, free = hub_graph(n, deg, rng, isolated)
        rp, cols = csr_from_pairs(n, pairs)
        d = np.diff(rp)
        assert list(d[hub_positions(n)]) == deg and not d[free].any()
        assert np.delete(d, hub_positions(n)).max() <= 4      # the rest: low-degree leaves
        parts.append((rp, cols))
        pos = rng.random((n, 2))
        x = rng.random((n, cfg.num_feature))
        s = pos[:, :cfg.spatial_dim]
        xs.append(x)
        ss.append(s)
        feats.append(np.concatenate([x, s], 1) if cfg.encoder_coords else x)
    rowptr, colidx = stack_csr(parts, n)
    return GraphBatch(B, n, rowptr, colidx,
                      np.ascontiguousarray(np.concatenate(feats), np.float32),
                      np.ascontiguousarray(np.concatenate(xs), np.float32),
                      np.ascontiguousarray(np.concatenate(ss), np.float32))


def make_case(n, d, B, isolated=0):
    """(cfg, batch, fp32-exact parameter blocks, fp32 eps) of a committed case."""
    from snd_vae_amd.config import tscale
    from snd_vae_amd.params import init_blocks
    cfg = tscale(n, d)
    batch = make_batch(cfg, B, isolated=isolated)
    deg = np.diff(batch.rowptr)
    assert (deg == 0).sum() == B * isolated
    assert sorted(HUB_DEGREES[1:]) == sorted(set(deg[deg > 4]))       # (the 1-hub is among the leaves)
    assert deg[-1] == deg.max() and batch.rowptr[-1] == batch.nnz  # the last row's ids end colidx
    p = {k: v.astype(np.float32).astype(np.float64) for k, v in init_blocks(cfg, INIT_SEED).items()}
    eps = np.random.default_rng(EPS_SEED).standard_normal((B * n, cfg.latent)).astype(np.float32)
    return cfg, batch, p, eps
