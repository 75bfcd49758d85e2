/*
 * snd_vae.h -- C ABI of the MI355X (gfx950) SND-VAE training hot path.
 *
 * One shared library, libsndvae.so, built by hipcc for gfx950.  Every entry
 * point takes caller-owned DEVICE pointers plus sizes and a HIP stream (passed
 * as an opaque pointer so FFI bindings need no HIP headers), launches
 * stream-ordered work, never allocates or synchronises (graph-capturable), and
 * returns 0 or a negative SND_ERR_* code; snd_last_error() gives the
 * thread-local message.  Layouts are row-major fp32 unless stated.  A batch of
 * B graphs with N nodes each is one block-diagonal CSR (int32 rowptr [B*N+1],
 * sorted int32 colidx with global column ids b*N+j) plus row-major node data
 * [B*N, width].
 *
 * Each function names the reference interface it replaces (file:line in
 * xguo7/SND-VAE, TensorFlow 1.x).  The reference is a TF graph-construction
 * API, not an FFI; INTEGRATION.md shows the ctypes binding a maintainer adds.
 */
#ifndef SND_VAE_H
#define SND_VAE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* snd_stream_t; /* hipStream_t */

enum {
  SND_OK = 0,
  SND_ERR_ARG = -1,         /* bad shape/pointer/enum */
  SND_ERR_HIP = -2,         /* HIP launch/runtime error */
  SND_ERR_UNSUPPORTED = -3  /* configuration not built for gfx950 path */
};

enum { SND_F32 = 0, SND_BF16 = 1 }; /* MFMA operand dtype; accumulation always fp32 */

const char* snd_last_error(void);
/* the ABI this header describes; snd_abi_version() returns it */
#define SND_ABI_VERSION 29
int snd_abi_version(void);

/* ---- a1: adjacency ingest ------------------------------------------------
 * Replaces the dense adj_truth feed (main.py:257, input_data.py:62-72):
 * converts B dense [N,N] float 0/1 matrices (diagonal ignored) into the
 * block-diagonal CSR, entries in np.where row-major order (bit-exact vs
 * scipy.sparse.csr_matrix).  *nnz_out (device int) receives the total.
 * Fails with SND_ERR_ARG (message set) via *nnz_out = -1 when colidx_cap is
 * too small.  workspace: snd_dense_to_csr_workspace() bytes. */
size_t snd_dense_to_csr_workspace(int n_graphs, int n);
int snd_dense_to_csr(const float* adj, int n_graphs, int n, int* rowptr,
                     int* colidx, long long colidx_cap, int* nnz_out,
                     void* workspace, size_t workspace_bytes, snd_stream_t stream);

/* ---- a2/a3/a4: CSR SpMM with GraphConvolution epilogue -------------------
 * Replaces tf.matmul(adj, new_x) + lrelu (layers.py:122-123) and the BN /
 * concat that follow it (model.py:107-112).
 *   acc = A @ h                      (A symmetric: also the backward A^T @ dy)
 *   epilogue SND_SPMM_PLAIN: out = acc
 *   epilogue SND_SPMM_GCN:   preact = acc;
 *       y = lrelu(acc) * gamma/sqrt(1.001) + beta        -> out[:, :width]
 *       out[:, width:width+fx] = concat_x                 (model.py:109)
 *       if out2: out2 = [y || concat_x] * g2/sqrt(1.001) + b2 (encoder_g BN) */
enum { SND_SPMM_PLAIN = 0, SND_SPMM_GCN = 1 };
int snd_csr_spmm(const int* rowptr, const int* colidx, int n_rows,
                 const float* h, int ldh, int width, float* out, int ldo,
                 int epilogue, const float* bn_gamma, const float* bn_beta,
                 float* preact, int ldp, const float* concat_x, int ldx, int fx,
                 const float* bn2_gamma, const float* bn2_beta, float* out2,
                 int ldo2, snd_stream_t stream);

/* a2 in the bf16 throughput mode (the SpMM of the fast path, layers.py:122 and
 * its backward): out = A @ h over bf16 rows with fp32 accumulation, rounded to
 * bf16.  width % 8 == 0 in 8..128; ldh, ldo % 8 == 0 (16-byte rows).  When
 * n_per_graph % 32 == 0 and n_graphs % 8 == 0 the row blocks are ordered so one
 * graph's rows stay on one XCD (its gathered rows then hit that XCD's L2);
 * otherwise natural order.  row_order (optional, NULL = 0..n_rows-1) is the
 * order rows are processed in, a permutation of 0..n_rows-1 that keeps each
 * graph's rows inside its own slot range (snd_vae_amd/data.py locality_order:
 * per-graph reverse Cuthill-McKee, so a workgroup's neighbour rows overlap in
 * L1); the result does not depend on it.  h and out are bf16 device buffers. */
int snd_csr_spmm_bf16(const int* rowptr, const int* colidx, int n_rows,
                      const void* h, int ldh, int width, void* out, int ldo,
                      int n_per_graph, int n_graphs, const int* row_order,
                      snd_stream_t stream);

/* Row tiles of a CSR (ABI 5): a per-batch companion format of the bf16 SpMM
 * that stages neighbour rows in LDS.  The schedule (row_order, or natural
 * order) is cut into tiles of tile_rows consecutive slots.  Per tile:
 *   rows[slot]   the tile's rows, by degree (descending, ties by schedule
 *                order), so a wavefront's rows have similar lengths;
 *   trp[slot]    row pointers in slot order into lcol ([n_rows+1]);
 *   lcol[k]      1 + each neighbour's index in its tile's set, every
 *                row's entries in colidx order (u16; 0 is never used);
 *   ucol[t*ustride + u]  the tile's set: ascending distinct neighbour rows,
 *                padded with -1 to ustride = the largest set.
 * The adjacency is static across training steps, so the tiles are built
 * once per batch, on the HOST (plain C++ over host arrays): call
 * snd_spmm_tile_plan with rows/trp/lcol/ucol NULL to size (*ustride), then
 * with them to fill; it returns the ucol length n_tiles*ustride (>= 0) or a
 * negative error.  A tile set of 65535 rows or more is an error.  The
 * SpMM relies on the degree order: a wavefront's first row is its longest. */
typedef struct snd_row_tiles {
  const int* rows;              /* [n_rows] device */
  const int* trp;               /* [n_rows+1] device */
  const uint16_t* lcol;         /* [nnz] device */
  const int* ucol;              /* [n_tiles*ustride] device */
  int tile_rows;                /* rows per tile (<= 128); 0 = no tiles */
  int ustride;                  /* largest tile set */
} snd_row_tiles_t;
long long snd_spmm_tile_plan(const int* rowptr, const int* colidx, int n_rows,
                             const int* row_order, int tile_rows, int* rows,
                             int* trp, uint16_t* lcol, int* ucol, int* ustride);
/* snd_csr_spmm_bf16 over row tiles: a persistent, software-pipelined kernel.
 * Each workgroup walks its tiles; while it sums tile i from LDS, the rows of
 * tile i+1 are in flight into registers and the set of tile i+2 is read.
 * A tile's rows are widened to fp32 in LDS once; every row accumulates its
 * neighbours from LDS in colidx order (the same fp32 sums as
 * snd_csr_spmm_bf16, bit for bit).  If ustride exceeds the LDS image
 * (319 rows) the launch runs snd_csr_spmm_bf16's kernel instead. */
int snd_csr_spmm_bf16_tiled(const int* rowptr, const int* colidx, int n_rows,
                            const snd_row_tiles_t* tiles, const void* h, int ldh,
                            int width, void* out, int ldo, int n_per_graph,
                            int n_graphs, const int* row_order, snd_stream_t stream);
/* snd_csr_spmm_bf16 streamed through a sliding window (ABI 7): out = A @ h,
 * width 64, bf16 rows, fp32 sums in colidx order (accumulated by
 * v_dot2c_f32_bf16: within one fp32 ulp per add of snd_csr_spmm_bf16, bitwise
 * equal on every tested batch).  A workgroup walks one graph's schedule positions (e.g.
 * the per-graph RCM order) in steps of 128 rows and keeps the h rows of
 * positions [p - beta, p + 127 + beta] in a 1096-row LDS ring, filled by
 * LDS-DMA two steps ahead: every h row is read from HBM once.  The plan
 * (snd_vae_amd/data.py window_plan, host-built once per batch):
 *   meta[q]  = (start8 << 6) | degree of the row at position q (degree <= 63)
 *   slots[]  = u16 ring slot (neighbour position % 1096) per neighbour, each
 *              row's list at 8 * start8, padded with the zero row's slot 1096
 *              to a multiple of 8 and to the largest degree (<= 32) of its
 *              wavefront group (8 consecutive rows of the listing below); the
 *              kernel reads 32 entries from every list start, so the array holds
 *              24 entries past the end of the last list, and 32 past the start
 *              of a trailing empty list (a row of an all-empty group)
 *   rows[q]  = the row whose sums position q computes, and meta[q] its meta:
 *              inside each aligned 128-position block listed by degree,
 *              descending (a wave's 8 rows then share their neighbour count)
 *   order[q] = the row at position q (the h row held at ring slot q % 1096)
 * beta = max |neighbour position - row position|; ceil8(beta) <= 352, else
 * SND_ERR_ARG (use snd_csr_spmm_bf16_tiled).  Replaces layers.py:122 (tf.matmul
 * of the dense adjacency). */
int snd_csr_spmm_bf16_window(const int* meta, const uint16_t* slots, const int* rows,
                             const int* order,
                             int n_rows, int n_per_graph, int n_graphs, int beta,
                             const void* h, int ldh, int width, void* out, int ldo,
                             snd_stream_t stream);
/* ---- a5: linear / dense GEMM on MFMA ---------------------------------------
 * Replaces linear() (layers.py:566-576) and the X@w of GraphConvolution
 * (layers.py:120-121; the tile() copy is not needed):
 *   C[m,n] = sum_k op(A)[m,k] op(B)[k,n] (+ bias[n])
 * op(A) = A (trans_a=0, A is [m,k] lda) or A^T (A is [k,m]); same for B. */
int snd_gemm(int trans_a, int trans_b, int m, int n, int k, const float* a,
             int lda, const float* b, int ldb, float* c, int ldc,
             const float* bias, int dtype, snd_stream_t stream);

/* ---- a8/a9: conv1d k=5 SAME over the node axis of each graph --------------
 * Replaces tf.layers.conv1d(k=5, stride 1, padding='SAME') + BN + lrelu
 * (model_joint.py:115-116, 138-139).  w is TF layout [5][cin][cout].
 *   fwd:  y_pre = conv(x) + bias;  out = lrelu(y_pre*g/sqrt(1.001) + b)
 *         (gamma == NULL: out = y_pre, no BN/lrelu)
 *   bwd_data:   dx = conv^T(dy)   (flipped taps, transposed channels)
 *   bwd_weight: dw[t,c,o] = sum_rows x[r+t-2,c] dy[r,o]  (deterministic
 *               split-K; workspace snd_conv1d_bwd_weight_workspace()).
 * rows = B*N, n_per_graph = N: taps never cross graph boundaries. */
int snd_conv1d_same_fwd(const float* x, int ldx, int rows, int n_per_graph,
                        int cin, const float* w, int cout, const float* bias,
                        const float* bn_gamma, const float* bn_beta,
                        float* y_pre, int ldy, float* out, int ldo, int dtype,
                        snd_stream_t stream);
int snd_conv1d_same_bwd_data(const float* dy, int lddy, int rows,
                             int n_per_graph, int cout, const float* w,
                             int cin, float* dx, int lddx, int dtype,
                             snd_stream_t stream);
size_t snd_conv1d_bwd_weight_workspace(int rows, int cin, int cout);
int snd_conv1d_same_bwd_weight(const float* x, int ldx, const float* dy,
                               int lddy, int rows, int n_per_graph, int cin,
                               int cout, float* dw, void* workspace,
                               size_t workspace_bytes, int dtype,
                               snd_stream_t stream);

/* ---- a6/a12: reparameterisation + KL --------------------------------------
 * Replaces get_z (model.py:153-161) and the KL term (optimizer.py:193).
 * ms = [mu || logstd] rows of width 2L (ld).  eps: injected [rows, L] or NULL
 * for the device Philox4x32-10 stream (seed, offset = *step_counter).
 *   z = mu + eps*exp(s)  -> z [rows, L]; eps written to eps_out if non-NULL.
 *   kl_part: snd_reparam_kl_blocks(rows, L) device doubles whose (fixed-order)
 *   sum is sum(1 + 2s - mu^2 - exp(s)^2). */
int snd_reparam_kl_blocks(int rows, int latent);
int snd_reparam_kl(const float* ms, int ldms, int rows, int latent,
                   const float* eps, unsigned long long seed,
                   const int* step_counter, float* eps_out, float* z,
                   double* kl_part, snd_stream_t stream);

/* ---- a7/a10: fused inner-product decoder + 2-class CE ----------------------
 * Replaces InnerProductDecoder (layers.py:407-409), the diagonal rule
 * (model.py:185,205-207), argmax (model.py:208), accuracy (main.py:334) and
 * softmax_cross_entropy (optimizer.py:142-144).  Logits never reach HBM.
 * For each graph b (z [B*N, d], d in {16,32,64,128}):
 *   L = z z^T; per off-diagonal pair CE = softplus(L) - A L (pos_weight,
 *   norm generalise to the weighted BCE of SURVEY §8 decision ii);
 *   diagonal pairs contribute softplus(-1) and no gradient.
 * Outputs (device): stats[0] = sum CE over all B*N*N pairs (double),
 *   stats[1] = number of pairs with argmax == A (as double),
 *   dz [B*N, d] = d(sum CE)/dz (unscaled; divide by B*N*N for the mean).
 * workspace: snd_zzt_ce_workspace() bytes.  z, dz and the workspace must be 16-byte
 * aligned (the kernels move them as 16-byte vectors; a row is at least 64 bytes);
 * SND_ERR_ARG otherwise, before anything is launched. */
size_t snd_zzt_ce_workspace(int n_graphs, int n, int d, int dtype);
int snd_zzt_ce(const float* z, int n_graphs, int n, int d,
               const int* rowptr, const int* colidx, float pos_weight,
               float norm, double* stats, float* dz, void* workspace,
               size_t workspace_bytes, int dtype, snd_stream_t stream);

/* ---- a7/a10 row-sharded (SURVEY §8e "beyond DP": one N = 16384 graph over ranks) --
 * The same CE and gradient for the rows [row0, row1) of ONE graph against all N
 * columns (layers.py:407-409, optimizer.py:142-144 restricted to a row block):
 *   z       [n, d] the whole graph's latent (all-gathered by the caller);
 *   rowptr  [row1 - row0 + 1] the range's CSR row pointers (a slice of the graph's
 *           CSR is fine: offsets index colidx), colidx global column ids;
 *   stats[0] = sum CE over the range's rows x N pairs, stats[1] = #correct there;
 *   dz [row1 - row0, d] = d(sum CE over ALL pairs)/dz for the range's rows -- L is
 *   symmetric, so a rank's rows need no reduction across ranks.
 * row0 % 128 == 0 and (row1 % 128 == 0 or row1 == n).  Summing stats over a
 * partition of [0, n) gives snd_zzt_ce's stats for the graph.  z, dz and the workspace
 * must be 16-byte aligned, as for snd_zzt_ce. */
size_t snd_zzt_ce_rows_workspace(int n, int d, int row0, int row1, int dtype);
int snd_zzt_ce_rows(const float* z, int n, int d, int row0, int row1,
                    const int* rowptr, const int* colidx, float pos_weight, float norm,
                    double* stats, float* dz, void* workspace, size_t workspace_bytes,
                    int dtype, snd_stream_t stream);

/* ---- edge-score evaluation of the inner-product decoder (forward only) -------
 * What the reference's post-training evaluation needs (main.py:13-14 roc_auc_score /
 * average_precision_score, main.py:423,467) without the logits or a dense predicted
 * adjacency in HBM.  z [B*N, d] fp32 with row stride ldz >= d, 1 <= d <= 128, any
 * N >= 1; the block-diagonal CSR as snd_zzt_ce takes it (colidx in any order within
 * a row).  L = z z^T per graph on the fp32 matrix cores, k ascending from zero: bit
 * for bit the fp32 fmaf chain snd_generate's generated_adj thresholds.
 * Per graph b over the N^2 - N ordered off-diagonal pairs:
 *   hist[b][label][bin] += 1   (int64 [B, 2, 2048]); label = 1 for a CSR entry,
 *     bin = clamp(floor(64 L) + 1024, 0, 2047): width 1/64 over [-16, 16), bins 0
 *     and 2047 collect the under- and overflow;
 *   counts[b] = {TP, FP, FN, TN} (int64 [B, 4]) at the rule L > 0 (model.py:208), the
 *     N diagonal pairs counted as TN: (TP + TN) / N^2 is main.py:334's accuracy.
 * accumulate = 0 clears hist and counts on the stream first, 1 adds to them.  Integer
 * sums only: the result does not depend on scheduling and is additive over batches
 * and ranks.  Non-finite z is unspecified.  workspace: snd_zzt_eval_workspace()
 * bytes (0 today; NULL is accepted then). */
size_t snd_zzt_eval_workspace(int n_graphs, int n, int d);
int snd_zzt_eval(const float* z, int ldz, int n_graphs, int n, int d,
                 const int* rowptr, const int* colidx, long long* hist,
                 long long* counts, int accumulate, void* workspace,
                 size_t workspace_bytes, snd_stream_t stream);

/* ---- edge extraction of the inner-product decoder (ABI 19; forward only) ------
 * The predicted graph of the decoder at a caller-chosen logit threshold, written as the
 * block-diagonal CSR of this header's preamble: what model.py:208's dense
 * tf.cast(L > 0) is converted into before anything here can consume it.  z [B*N, d]
 * fp32 with row stride ldz >= d, 1 <= d <= 128, any N >= 1 (the operand rules of
 * snd_zzt_eval).  L = z z^T per graph is the logit snd_zzt_eval bins:
 * v_mfma_f32_32x32x2_f32, k ascending from a zero accumulator, K zero-padded -- bit for
 * bit the fp32 fmaf chain snd_generate's generated_adj thresholds.  So at threshold 0
 * the CSR is np.nonzero(generated_adj) exactly, and at the threshold and rule that
 * snd_zzt_eval's histogram selects it holds exactly the pairs that histogram counted.
 *   (i, j) is an edge iff i != j and L_ij > threshold; L_ij >= threshold when
 *   inclusive != 0.  -inf gives the complete graph, +inf the empty one; a NaN threshold
 *   is SND_ERR_ARG before anything is launched.  Non-finite z is unspecified (no fault,
 *   no write outside the outputs).
 *   rowptr [B*N + 1] int32; colidx int32 global ids b*N + j, ascending within each row.
 *   *nnz_out (device int64) always receives the exact number of edges; rowptr is
 *   complete whenever that number is below 2^31.  colidx is written only when
 *   colidx != NULL and the number is at most colidx_cap (and below 2^31); otherwise not
 *   one element of it is touched and the call still returns 0 -- compare *nnz_out with
 *   the capacity.  colidx = NULL (colidx_cap ignored) is the sizing call: count only.
 * L is recomputed by the count and the fill pass; O(nnz) bytes reach HBM.  Integer
 * results only: two runs on the same operands are bitwise equal.  workspace:
 * snd_zzt_edges_workspace() bytes (0 for shapes the op rejects), 4-byte aligned. */
size_t snd_zzt_edges_workspace(int n_graphs, int n, int d);
int snd_zzt_edges(const float* z, int ldz, int n_graphs, int n, int d,
                  float threshold, int inclusive,
                  int* rowptr, int* colidx, long long colidx_cap,
                  long long* nnz_out, void* workspace, size_t workspace_bytes,
                  snd_stream_t stream);

/* ---- graph statistics of a CSR and coordinates (ABI 20; forward only) ----------
 * What the reference's reconstruct_evaluation / generation_evaluation (main.py:423,467;
 * their utils/evaluation package is not shipped) are given: the graphs and the node
 * coordinates.  Degree, triangle, local-clustering and edge-length statistics of B graphs
 * x N nodes in one launch, from the block-diagonal CSR of this header's preamble (what
 * snd_zzt_edges writes) without a host round trip.  1 <= N <= 32768.
 *   N(i) = the SET of columns of row i inside i's graph block, i itself left out: entries
 *   outside the block and self loops are ignored (as snd_zzt_eval ignores them), colidx in
 *   any order within a row.  Duplicate entries give an unspecified count (no fault, no
 *   store outside the outputs).
 * Per row (R = B*N; deg and tri2 may each be NULL):
 *   deg[i]  = |N(i)|
 *   tri2[i] = sum_{j in N(i)} |N(i) & N(j)|   -- twice the triangles at i on a symmetric
 *             CSR; the formula is the definition on an asymmetric one.
 * Per graph b, hist [B, 3, 256] int64:
 *   hist[b][0][min(deg, 255)] += 1                                    per node
 *   hist[b][1][min(floor(256 tri2 / (deg (deg - 1))), 255)] += 1      per node, in 64-bit
 *             integers; nodes with deg < 2 go to bin 0 (c = 0, networkx's convention)
 *   hist[b][2][min(floor(len * len_scale), 255)] += 1   per entry with global column > row
 *             inside the block, len = ||coords[i, :sd] - coords[j, :sd]||_2 in fp32
 *             (coords [R, ldc] fp32, 1 <= sd <= 3, ldc >= sd, any alignment).  Left at
 *             zero (unchanged under accumulate) when coords == NULL; sd, ldc and
 *             len_scale are ignored then.  Non-finite coordinates: unspecified bin.
 * totals [B, 4] int64 = {sum deg, sum tri2, sum deg (deg - 1), entries with column > row}:
 *   density, mean degree, transitivity (sum tri2 / sum deg (deg - 1)) and the undirected
 *   edge count follow.
 * accumulate = 0 clears hist and totals on the stream first, != 0 adds to them.  Integer
 * sums only: two runs are bitwise equal, and the result is additive over batches.
 * SND_ERR_ARG before anything is launched: n_graphs < 1, n < 1, n > 32768; coords given
 * with sd outside 1..3, ldc < sd or a NaN, negative or infinite len_scale; NULL rowptr,
 * hist or totals; a workspace below snd_graph_stats_workspace() bytes (0 today; NULL is
 * accepted then).  Work: sum_j deg(j)^2 column ids tested. */
size_t snd_graph_stats_workspace(int n_graphs, int n);
int snd_graph_stats(const int* rowptr, const int* colidx, int n_graphs, int n,
                    const float* coords, int ldc, int sd, float len_scale,
                    int* deg, int* tri2, long long* hist, long long* totals,
                    int accumulate, void* workspace, size_t workspace_bytes,
                    snd_stream_t stream);

/* ---- path statistics of a CSR and coordinates (ABI 26; forward only) ------------
 * Does a generated spatial network work as a network?  Component structure, shortest-path
 * hop counts and the detour (route factor, circuity) of the network route over the straight
 * line (Barthelemy, Spatial networks, Phys. Rep. 499 (2011); Latora & Marchiori 2001 for
 * the efficiency that follows from the hop histogram): what the reference's
 * generation_evaluation / reconstruct_evaluation (main.py:423,467) are given the graphs
 * and coordinates for.  B graphs x N nodes from the block-diagonal CSR of this header's
 * preamble (what snd_zzt_edges writes), without a host round trip.  1 <= N <= 16384.
 *   Edge rule (snd_graph_stats'): N(i) = the columns of row i inside i's graph block, i
 *   itself left out; out-of-block entries and self loops are ignored, colidx in any order.
 *   Duplicate entries are legal and change nothing (every operation below is idempotent).
 *   Arcs are followed row -> column: the undirected graph on a symmetric CSR; on an
 *   asymmetric one the formula is the definition.  colidx holds nnz_cap >= rowptr[B*N]
 *   entries (NULL only with nnz_cap = 0).
 * Sources of a graph: its local nodes 0, src_step, 2 src_step, ... (src_step >= 1);
 * n_src = ceil(N / src_step).  Outputs (comp, hops_out and route_out may each be NULL):
 *   comp [B*N] int32: the smallest local node id of the node's WEAKLY connected component
 *             (arcs used both ways).
 *   hops_out [B*n_src, N] int32: BFS arc count from each source; -1 where unreachable, 0
 *             at the source.
 *   route_out [B*n_src, N] fp32 (needs coords): the shortest route length, the least fixed
 *             point in fp32 of d[s] = 0, d[v] = min_u fl(d[u] + len(u, v)), len the edge
 *             length ||coords[u, :sd] - coords[v, :sd]||_2 formed once per CSR entry in fp32
 *             (coords [B*N, ldc] fp32, 1 <= sd <= 3, ldc >= sd); +inf where unreachable.
 *             fl(. + w) is monotone and w >= 0, so the fixed point is unique: it is what a
 *             float32 Dijkstra returns, whatever the order of relaxations.
 *   hist [B, 2, 256] int64:
 *     hist[b][0][min(hops, 255)] += 1   per ordered pair (source s, t != s, reachable)
 *     hist[b][1][min(max(floor((route / e - 1) detour_scale), 0), 255)] += 1   per such pair
 *             with Euclidean distance e > 0, both distances fp32.  Left at zero when
 *             coords == NULL; sd, ldc and detour_scale are ignored then.
 *   totals [B, 6] int64 = {weak components, size of the largest, sources used, reachable
 *             ordered pairs (s, t != s), sum of hops over them, largest hop count seen}.
 * Every call clears hist and totals on the stream first (no accumulate mode: callers
 * concatenate per batch).  Integer atomics only, no allocation, no host synchronisation:
 * two runs are bitwise equal and a HIP-graph replay equals the eager call.  Non-finite
 * coordinates: unspecified bins and routes, no fault, no store outside the outputs.
 * SND_ERR_ARG before anything is launched: n_graphs < 1, n < 1, n > 16384, src_step < 1,
 * nnz_cap < 0; route_out without coords; coords given with sd outside 1..3, ldc < sd or a
 * NaN, non-positive or infinite detour_scale; NULL rowptr, hist or totals; a workspace
 * below snd_graph_paths_workspace() bytes (one fp32 length per entry with coords, 0 and
 * NULL accepted without).  Work: sources x arcs column ids, and that per relaxation sweep. */
size_t snd_graph_paths_workspace(int n_graphs, int n, long long nnz_cap, int has_coords);
int snd_graph_paths(const int* rowptr, const int* colidx, long long nnz_cap, int n_graphs, int n,
                    const float* coords, int ldc, int sd, float detour_scale, int src_step,
                    int* comp, int* hops_out, float* route_out, long long* hist,
                    long long* totals, void* workspace, size_t workspace_bytes,
                    snd_stream_t stream);

/* ---- graphlet census of a CSR (ABI 27; forward only) ------------------------------
 * The orbit descriptor of the graph-generation literature (GraphRNN, You et al. 2018, and
 * its successors: degree, clustering and orbit counts) is, per graph, the mean over the nodes
 * of the fifteen 2- to 4-node graphlet orbit counts.  Summed over a graph's nodes these
 * follow exactly from nine induced subgraph counts, which this op leaves per graph, on the
 * device, from the block-diagonal CSR of this header's preamble.  1 <= N <= 16384.
 *   Entry rule (snd_graph_stats'): N(i) = the columns of row i inside i's graph block, i
 *   itself left out; out-of-block entries and self loops are ignored, colidx in any order.
 *   Duplicate entries: the first occurrence counts (the others are dropped on chip); the
 *   contract leaves their effect unspecified, but no fault and no store outside the
 *   outputs.  colidx holds nnz_cap >= rowptr[B*N] entries (NULL only with nnz_cap = 0).
 *   The graph that is counted: the undirected simple graph G_b with {i, j} an edge iff
 *   j in N(i) AND i in N(j).  On a symmetric CSR that is the graph itself; on an asymmetric
 *   one this is the definition: a one-way arc (j in N(i), i not in N(j)) is no edge and is
 *   counted in census[b][9].
 * census [B, 10] int64: the numbers of INDUCED subgraphs of G_b
 *   {0: E edges, 1: P2 open 2-paths, 2: T triangles, 3: P3 3-edge paths, 4: S3 claws
 *    (3-stars), 5: C4 chordless 4-cycles, 6: TT tailed triangles (paws), 7: D diamonds,
 *    8: K4 4-cliques} and 9: the one-way arcs.
 * work [B] int64, always written: with l_i = rowptr[i + 1] - rowptr[i] the length of CSR row
 *   i, and over the entries j of row i that count (in block, j != i; duplicates count here)
 *   a_i = sum l_j and c_i = sum over those with j > i of l_j min(l_i, l_j),
 *     work[b] = sum over the rows i of graph b of 9 l_i + 4 a_i + c_i,
 *   an upper bound on the column ids the counting kernels read for graph b (the degrees of
 *   G_b are at most the l_i; per triangle u < v < w the clique kernel reads one row w).  It
 *   is computed in one pass of O(N + nnz) before any counting.  A graph with
 *   work[b] > work_cap is NOT counted: its ten census entries are -1, every other graph of
 *   the call is unaffected (4-clique counting is Theta(N^4) on a dense graph).
 * Every call overwrites census and work (no accumulate mode).  Integer arithmetic and
 * integer atomics only, no allocation, no host synchronisation: two runs are bitwise equal
 * and a HIP-graph replay equals the eager call.
 * SND_ERR_ARG before anything is launched, buffers untouched: n_graphs < 1; n < 1 or
 * n > 16384; B N >= 2^31; nnz_cap < 0; work_cap < 0; NULL rowptr, census or work; NULL
 * colidx with nnz_cap > 0; a workspace that is NULL, not 8-byte aligned or below
 * snd_graph_motifs_workspace() bytes (the sums, one degree per row and the mutual-edge CSR:
 * 80 B + 4 N B + 4 nnz_cap bytes, each part rounded up to 16 bytes; 0 for a shape the op rejects). */
size_t snd_graph_motifs_workspace(int n_graphs, int n, long long nnz_cap);
int snd_graph_motifs(const int* rowptr, const int* colidx, long long nnz_cap, int n_graphs, int n,
                     long long work_cap, long long* census, long long* work, void* workspace,
                     size_t workspace_bytes, snd_stream_t stream);

/* ---- spectral density of a CSR (ABI 28; forward only) -----------------------------
 * The fourth descriptor of the graph-generation literature (GRAN, Liao et al. 2019: degree,
 * clustering, orbits and the spectrum of the normalised Laplacian), without an eigensolver:
 * the Chebyshev moments of the spectral density by the kernel polynomial method (Weisse et
 * al., Rev. Mod. Phys. 78, 2006), per graph, on the device, from the block-diagonal CSR of
 * this header's preamble.  1 <= N <= 16384.
 *   The graph (snd_graph_motifs'): N(i) = the columns of row i inside i's graph block, i
 *   itself left out; out-of-block entries and self loops are ignored, colidx in any order;
 *   {i, j} is an edge iff j in N(i) AND i in N(j); a one-way arc is no edge and is counted
 *   in info[b][2].  Duplicate entries: every copy counts as an entry of its own; the
 *   contract leaves their effect unspecified, but no fault and no store outside the
 *   outputs.  colidx holds nnz_cap >= rowptr[B*N] entries (NULL only with nnz_cap = 0).
 *   The operator: with d_i the degree in that graph, M = L - I, L = D^-1/2 (D - A) D^-1/2
 *   and d^-1/2 := 0 for an isolated node (networkx's and scipy's convention: an isolated
 *   node has eigenvalue 0 of L):
 *     (M x)_i = - sum_{j in N(i), mutual} x_j / sqrt(d_i d_j)  if d_i > 0,  else -x_i.
 *   The spectrum of M lies in [-1, 1].
 * moments [B, n_moments] double, 2 <= n_moments <= 512:
 *   n_probes = 0 (exact): moments[b][k] = tr T_k(M_b) = sum_i T_k(lambda_i - 1), T_k the
 *     Chebyshev polynomial, computed with the N unit vectors as probes;
 *   n_probes = R >= 1: (1 / R) sum_r v_r^T T_k(M_b) v_r with v_r[i] = +-1: -1 iff bit 0 of
 *     the first output word of Philox4x32-10 with counter (i, r, b, 0x53504543) and key
 *     (seed lo, seed hi) is set; i is the node's local index, b its graph's index in the
 *     call (a Hutchinson estimate: the error of a raw moment is about sqrt(2 N / R)).
 *   moments[b][0] = N exactly in both modes; in exact mode moments[b][1] = -isolated exactly.
 * info [B, 4] int64: {edges, isolated nodes, one-way arcs, probes used (N in exact mode)}.
 * Arithmetic: state, weights and sums in double.  With t_0 = v, t_1 = M t_0,
 *   t_{s+1} = 2 M t_s - t_{s-1}:  mu_{2s+1} = 2 <t_{s+1}, t_s> - mu_1 and
 *   mu_{2s+2} = 2 <t_{s+1}, t_{s+1}> - mu_0 (M is symmetric), so K moments take K / 2
 *   applications of M.  Probes run in column blocks of 32; for N <= 64 a workgroup per graph
 *   runs the whole recurrence in LDS in one launch per probe block, above that (or with
 *   SND_SPECTRUM_FORCE_GLOBAL in flags; every other bit must be 0) one fused launch and
 *   one fixed-order reduction per step.  No floating-point atomics: two runs are bitwise
 *   equal and a HIP-graph replay equals the eager call; the launch count depends on N,
 *   n_moments, n_probes and flags only.  No allocation, no host synchronisation.
 * Every call overwrites moments and info.
 * SND_ERR_ARG before anything is launched, buffers untouched: n_graphs < 1; n < 1 or
 * n > 16384; B N >= 2^31; nnz_cap < 0; n_moments outside [2, 512]; n_probes < 0; unknown
 * flag bits; NULL rowptr, moments or info; NULL colidx with nnz_cap > 0; a workspace that
 * is NULL, not 8-byte aligned or below snd_graph_spectrum_workspace() bytes (32 B per
 * graph, 8 B per entry, two state buffers of 256 B per row, 16 B per 8 rows of partial
 * dots, 4 B per row, each part rounded up to 16 bytes; 0 for a shape the op rejects). */
enum { SND_SPECTRUM_FORCE_GLOBAL = 1 };
size_t snd_graph_spectrum_workspace(int n_graphs, int n, long long nnz_cap);
int snd_graph_spectrum(const int* rowptr, const int* colidx, long long nnz_cap, int n_graphs, int n,
                       int n_moments, int n_probes, unsigned long long seed, int flags,
                       double* moments, long long* info, void* workspace, size_t workspace_bytes,
                       snd_stream_t stream);

/* ---- edge crossings of a CSR drawn at its coordinates (ABI 29; forward only) --------
 * SND-VAE generates spatial networks: is a generated network drawn like the data?  Edge
 * crossings are the canonical measure of how far a spatial network is from planar
 * (Barthelemy, Spatial networks, Phys. Rep. 499 (2011), section 2.1), the distribution of
 * edge directions is Boeing's orientation descriptor (Urban spatial order, Appl. Netw. Sci. 4
 * (2019)).  B graphs x N nodes, 1 <= N <= 16384, B N < 2^31, from the block-diagonal CSR of
 * this header's preamble.  coords [B N, ldc] fp32, ldc >= 2; only columns 0 and 1 are read (a
 * 3-D caller passes the projection it wants).
 *   The graph is snd_graph_motifs': N(i) = the columns of row i inside i's block, i itself
 *   left out; {i, j} is an edge iff j in N(i) AND i in N(j); a one-way arc is no edge and is
 *   counted apart; out-of-block entries and self loops are ignored; of duplicate entries the
 *   first occurrence counts (effect unspecified, no fault, no store outside the outputs).  An
 *   edge is written (a, b), a < b in local ids.
 *   The predicate is the whole definition.  Two edges e = (a, b) and f = (c, d) CROSS iff
 *     1. they share no endpoint;
 *     2. their bounding boxes overlap, by fp32 compares on the coordinates as stored: no
 *        crossing if max(ax, bx) < min(cx, dx), or the same with e and f swapped, or either of
 *        these in y;
 *     3. they straddle each other strictly: with orient(p, q, r) = (qx - px)(ry - py) -
 *        (qy - py)(rx - px) evaluated in double from the fp32 coordinates, each of its four
 *        differences, two products and the final subtraction rounded once (no contraction),
 *        orient(a, b, c) and orient(a, b, d) are non-zero with opposite signs, and so are
 *        orient(c, d, a) and orient(c, d, b).  Signs are compared, no product of orients is
 *        formed.
 *   Touching, T-junctions, collinear overlaps, coincident nodes and zero-length edges are
 *   therefore not crossings; the conjunction is symmetric in e and f.
 * work [B] int64, always written: E_b (E_b - 1) / 2, the pairs to test.  A graph with
 *   work[b] > work_cap is NOT counted: its counts row is -1, its hist rows are 0, its
 *   cross_out entries are -1; every other graph is unaffected.
 * counts [B, 7] int64: {0: E edges, 1: X crossing pairs, 2: edges with >= 1 crossing,
 *   3: independent pairs E (E - 1) / 2 - sum_v C(deg_v, 2) with deg in this graph (the
 *   denominator of the crossing ratio), 4: one-way arcs, 5: zero-length edges (both
 *   coordinates equal), 6: the largest crossing count of one edge}.
 * hist [B, 3, 256] int64:
 *   [0][min(c_e, 255)] += 1 per edge, c_e its crossing count;
 *   [1][k] += 1 per edge of non-zero length, for its direction folded to [0, pi): u = b - a
 *     per component (one fp32 rounding each), negated if uy < 0 or (uy == 0 and ux < 0),
 *     theta = atan2f(uy, ux), k = floor(theta (256 / pi) + 0.5) mod 256 in fp32: the bins are
 *     centred on 0, pi / 256, ..., so axis-aligned and diagonal edges fall in bin centres;
 *   [2][k] += 1 per crossing pair, for the acute angle phi = atan2f(|ux vy - uy vx|,
 *     |ux vx + uy vy|) in [0, pi / 2] (fp32, every operation rounded once),
 *     k = min(floor(phi (512 / pi)), 255).
 * cross_out [nnz_cap] int32, may be NULL: the entries p < rowptr[B N] that are a mutual edge
 *   with global column > row hold c_e, every other such entry 0 (-1 in a skipped graph);
 *   entries past rowptr[B N] are untouched.
 *   work_cap has no default at this level: the caller passes it.  The Python binding's
 *   default (layers.CROSSINGS_WORK_CAP = 4e11 pairs) is the rate measured on one MI355X on
 *   10^5 long random edges, where nearly every pair reaches the double predicate and a quarter
 *   cross, 3.7e11 pairs per second, to one digit: about a second for a graph at the cap.  On
 *   the N = 4096 bench graphs, where the box test rejects nearly every pair, the op ran 1.6e12
 *   pairs per second (tools/graph_crossings_timing.py, profiles/graph_crossings_timing.json).
 * Every call overwrites the outputs (no accumulate mode).  Integer atomics only, no
 * allocation, no host synchronisation; the launch count and every grid size depend only on
 * (B, N, nnz_cap); two runs are bitwise equal and a HIP-graph replay equals the eager call.
 * Non-finite coordinates: unspecified counts, no fault, no store outside the outputs.
 * SND_ERR_ARG before anything is launched, buffers untouched: n_graphs < 1; n < 1 or
 * n > 16384; B N >= 2^31; nnz_cap < 0; work_cap < 0; ldc < 2; NULL rowptr, coords, counts,
 * hist or work; NULL colidx with nnz_cap > 0; a workspace that is NULL, not 16-byte aligned
 * or below snd_graph_crossings_workspace() bytes (64 B per graph of sums, 8 (B + 1) B of
 * tile-pair prefix, each rounded up to 16 bytes, and 28 B per entry of max(nnz_cap, 1)
 * rounded up to 4 entries: the edge list; 0 for a shape the op rejects). */
size_t snd_graph_crossings_workspace(int n_graphs, int n, long long nnz_cap);
int snd_graph_crossings(const int* rowptr, const int* colidx, long long nnz_cap, int n_graphs, int n,
                        const float* coords, int ldc, long long work_cap,
                        long long* counts, long long* hist, long long* work, int* cross_out,
                        void* workspace, size_t workspace_bytes, snd_stream_t stream);

/* ---- a11: sigmoid head + MSE ----------------------------------------------
 * Replaces tf.nn.sigmoid(linear(...)) (model_joint.py:121,144) and the
 * squared-difference means (optimizer.py:149,153) with their gradients:
 *   yhat = sigmoid(u @ w + b);  sse += sum (yhat - y)^2  (device double)
 *   du = dpre @ w^T with dpre = 2 (yhat - y)/count * yhat (1 - yhat),
 *   count = rows*cout (the mean's denominator).  dw/db accumulate (+=).
 *   sse: snd_sigmoid_mse_blocks(rows) device doubles (per-block partials).
 *   workspace: blocks * (cin*cout + cout) floats. */
int snd_sigmoid_mse_blocks(int rows);
int snd_sigmoid_mse(const float* u, int ldu, int rows, int cin,
                    const float* w, const float* b, int cout,
                    const float* target, int ldt, double* sse, float* yhat,
                    float* du, int lddu, float* dw, float* db, void* workspace,
                    size_t workspace_bytes, snd_stream_t stream);

/* ---- a13: TF1 Adam over a flat buffer --------------------------------------
 * Replaces tf.train.AdamOptimizer(lr).minimize (optimizer.py:125,197):
 *   t = *step_counter (1-based, already advanced for this step)
 *   g = grad*grad_scale; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2
 *   param -= lr*sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps) */
int snd_adam_tf1(float* param, const float* grad, float* m, float* v,
                 long long n, float lr, float beta1, float beta2, float eps,
                 float grad_scale, const int* step_counter,
                 snd_stream_t stream);
/* The same update over n_ranges disjoint [offsets[k], offsets[k] + counts[k]) element
 * ranges of the same flat buffers in one launch (ABI 14; host arrays, read at call
 * time): the blocks a fused in-step update (snd_plan_fuse_adam) leaves to the caller
 * are not contiguous (C4: three ranges).  Offsets and counts that are multiples of 4
 * on 16-byte aligned buffers take one float4 launch for up to 16 ranges; anything
 * else falls back to one snd_adam_tf1 per range.  Same arithmetic either way. */
int snd_adam_tf1_ranges(float* param, const float* grad, float* m, float* v,
                        const long long* offsets, const long long* counts, int n_ranges,
                        float lr, float beta1, float beta2, float eps, float grad_scale,
                        const int* step_counter, snd_stream_t stream);

/* ---- SpatialGraphConvolution (layers.py:143-198) and the model_joint
 * spatial-graph encoder layer s' = lrelu(BN(SGConv(adj, s, rel)))
 * (model_joint.py:77-80), factorised to O(nnz (h0 + deg)) + row GEMMs (see
 * snd_sg.hip).  adj must be symmetric (spanning trees and adj_truth are;
 * input_data.py:31-37,67) with rel_dim 1 (Matrix1 has 3F+3 rows).
 * Per-layer parameter buffer (fp32, snd_sg_param_count floats), row-major:
 *   Matrix1 [3F+3][h0] (rows: x_i | x_j | x_k | rel_ij | rel_jk | dis_ik), bias1 [h0],
 *   Matrix2 [2F+1+h0][h1] (x_i | x_j | rel_ij | m3_sum), bias2 [h1],
 *   Matrix3 [F+h1][h2] (x | m2_sum), bias3 [h2], BN gamma [h2], BN beta [h2].
 * Gradients use the same layout (written, not accumulated). */
typedef struct snd_sg_graph {
  const int* rowptr;   /* [R+1] symmetric CSR, block-diagonal, sorted global ids */
  const int* colidx;   /* [nnz] */
  int n_rows;          /* R = B * n_per_graph */
  int n_per_graph;
  float* edge_lr;      /* [nnz] lrelu(rel_ij)                      (snd_sg_prep) */
  float* edge_q;       /* [nnz] sum_{k in N(j)} lrelu(rel_ik)      (snd_sg_prep) */
  int* edge_rev;       /* [nnz] index of the reverse edge (j, i)   (snd_sg_prep) */
  float* node_deg;     /* [R] degree                               (snd_sg_prep) */
  float* node_e;       /* [R] sum_{j in N(i)} lrelu(rel_ij)        (snd_sg_prep) */
} snd_sg_graph_t;
/* Edge / node scalars of a batch from rel [B, N, N] (the 'rel' feed, main.py:262,
 * /600 at load); *n_unmatched (device int) = edges without a reverse edge (must be 0). */
int snd_sg_prep(const snd_sg_graph_t* g, const float* rel, int* n_unmatched,
                snd_stream_t stream);
long long snd_sg_param_count(int f, int h0, int h1, int h2);
size_t snd_sg_workspace(int n_rows, int f, int h0, int h1, int h2);
/* y [R, h2] = SGConv(adj, x, rel); bn_act: out = lrelu(BN(y)) (frozen Keras BN).
 * The workspace keeps what snd_sg_layer_bwd needs: pass the same one. */
int snd_sg_layer_fwd(const snd_sg_graph_t* g, const float* x, int ldx, int f, int h0, int h1,
                     int h2, const float* params, int bn_act, float* y, float* out,
                     void* workspace, snd_stream_t stream);
/* dout = dL/d(out) (bn_act) or dL/dy; writes grads (param layout) and, if dx is
 * not NULL, dL/dx [R, f]. */
int snd_sg_layer_bwd(const snd_sg_graph_t* g, const float* x, int ldx, int f, int h0, int h1,
                     int h2, const float* params, int bn_act, const float* y,
                     const float* dout, float* dx, int lddx, float* grads, void* workspace,
                     snd_stream_t stream);

/* ---- SpatialGraphConvolution_3D (ABI 21; layers.py:200-277), the three-hop layer
 * the reference selects for its 3-D datasets (model.py:139-140; four widths per
 * layer, main.py:223,241; spatial_dim 3), and the encoder layer
 * s' = lrelu(BN(SGConv3D(adj, s, rel))).  The reference materialises
 * B x N x N x N x N x (4F+5) messages; here the layer is factorised to O(P2 h0)
 * vector work over the P2 = sum_j d_j^2 directed 2-paths, the two-hop layer's edge
 * and node work and row / edge GEMMs (see snd_sg3.hip).  fp32 forward and backward,
 * no floating-point atomics: two runs on the same operands are bitwise equal.
 * Path indices need not be distinct (k may equal i, p may equal i or j), as in the
 * reference.  adj must be symmetric with rel_dim 1; g is a prepared snd_sg_graph_t
 * (snd_sg_prep) and rel the same dense [B, N, N] array snd_sg_prep read.
 * Per-layer parameter buffer (fp32, snd_sg3_param_count floats), row-major:
 *   Matrix0 [4F+5][h0] (rows: x_i | x_j | x_k | x_p | rel_ij | rel_jk | rel_kp |
 *                       dis_ik | dis_ip), bias0 [h0],
 *   Matrix1 [3F+3+h0][h1] (x_i | x_j | x_k | rel_ij | rel_jk | dis_ik | m4_sum), bias1 [h1],
 *   Matrix2 [2F+1+h1][h2] (x_i | x_j | rel_ij | m3_sum), bias2 [h2],
 *   Matrix3 [F+h2][h3] (x | m2_sum), bias3 [h3], BN gamma [h3], BN beta [h3].
 * Gradients use the same layout (written, not accumulated).
 * nnz = rowptr[R]; n_paths = sum over directed edges (i, j) of d_j, computed by the
 * caller on the host (the kernels walk the paths from the CSR and recompute the
 * per-path scalars, so n_paths is validated and reserved: the workspace of this
 * version does not grow with it).  Every buffer is caller-owned; the entry points
 * neither allocate nor synchronise.
 * SND_ERR_ARG is returned before anything is launched, with a message naming the
 * entry point and no buffer touched, for: ldx < f or lddx < f, a width below 1,
 * bn_act without out, n_rows not a multiple of n_per_graph, nnz or n_paths below 0,
 * a NULL required pointer (dx alone may be NULL), or workspace_bytes below
 * snd_sg3_workspace().
 * The fused SND_SGJOINT plan stays two-hop (snd_config_t.sg_h holds three widths per
 * layer): a four-width configuration is SND_ERR_UNSUPPORTED there (a ValueError from
 * the Python plan builder); compose this layer per call instead. */
long long snd_sg3_param_count(int f, int h0, int h1, int h2, int h3);   /* -1: bad width */
size_t snd_sg3_workspace(int n_rows, long long nnz, long long n_paths, int f, int h0, int h1,
                         int h2, int h3);                               /* 0: bad argument */
/* y [R, h3] = SGConv3D(adj, x, rel); bn_act: out = lrelu(BN(y)) (frozen Keras BN).
 * The workspace keeps what snd_sg3_layer_bwd needs: pass the same one. */
int snd_sg3_layer_fwd(const snd_sg_graph_t* g, const float* rel, long long nnz, long long n_paths,
                      const float* x, int ldx, int f, int h0, int h1, int h2, int h3,
                      const float* params, int bn_act, float* y, float* out, void* workspace,
                      size_t workspace_bytes, snd_stream_t stream);
/* dout = dL/d(out) (bn_act) or dL/dy; writes grads (param layout) and, if dx is
 * not NULL, dL/dx [R, f] (row stride lddx). */
int snd_sg3_layer_bwd(const snd_sg_graph_t* g, const float* rel, long long nnz, long long n_paths,
                      const float* x, int ldx, int f, int h0, int h1, int h2, int h3,
                      const float* params, int bn_act, const float* y, const float* dout,
                      float* dx, int lddx, float* grads, void* workspace,
                      size_t workspace_bytes, snd_stream_t stream);

/* ---- §8f rank 4: disentangled-model pieces (ABI 8; not on the benchmarked path) -
 * e2e edge-to-edge filter of the structure decoder (layers.py:431-450), fp32:
 *   out[b,i,j,o] = 2 b1[o] + sum_t sum_c w1[t,c,o] (x[b,i,j+t-p,c] + x[b,i+t-p,j,c])
 * x [B, N, N, C] (NHWC), w1 [K, C, O] (the reference's [1, K, C, O] kernel; conv2
 * uses its transpose [K, 1, C, O]: the same taps), TF SAME padding p = (K-1)/2;
 * the decoder uses K = N (model.py:196).  Deterministic fixed-order sums. */
int snd_e2e_fwd(const float* x, int n_graphs, int n, int c, const float* w1, const float* b1,
                int k, int o, float* out, snd_stream_t stream);
/* dx [B, N, N, C], dw1 [K, C, O], db1 [O] of sum(out * dout). */
int snd_e2e_bwd(const float* x, int n_graphs, int n, int c, const float* w1, int k, int o,
                const float* dout, float* dx, float* dw1, float* db1, snd_stream_t stream);
/* The e2e structure decoder around the filters (model.py:193-208), fp32, frozen
 * Keras BN (y' = gamma y / sqrt(1.001) + beta) then relu:
 *   snd_e2e_pair_fwd: x0[b,i,j,:] = relu(BN0([z_i | z_j]))  (z [B, N, D] -> x0 [B, N, N, 2D])
 *   snd_bn_relu_fwd:  x = relu(BN(y)), y [rows, c]           (between e2e layers)
 *   snd_e2e_head_ce:  logits = relu(BN_adj(y)) W + b (d_e_lin2, W [c][2]), the diagonal
 *                     set to (1, 0) (model.py:200-203), CE against [1 - A, A] summed
 *                     over B N^2 (optimizer.py:142-144) into out[0], argmax == A count
 *                     (main.py:334) into out[1]; gradients of the MEAN CE: dy, dW, db,
 *                     dgamma, dbeta (c <= 32; adj dense [B, N, N] 0/1 floats)
 *   snd_bn_relu_bwd / snd_e2e_pair_bwd: the matching backward passes (per-channel
 *                     gamma / beta gradients in fixed order; the pair backward needs
 *                     snd_e2e_pair_bwd_workspace bytes). */
int snd_e2e_pair_fwd(const float* z, int n_graphs, int n, int d, const float* gamma, const float* beta,
                     float* x, snd_stream_t stream);
size_t snd_e2e_pair_bwd_workspace(int n_graphs, int n, int d);
int snd_e2e_pair_bwd(const float* dx0, const float* z, int n_graphs, int n, int d, const float* gamma,
                     const float* beta, float* dz, float* dgamma, float* dbeta, void* workspace,
                     snd_stream_t stream);
int snd_bn_relu_fwd(const float* y, long long rows, int c, const float* gamma, const float* beta, float* x,
                    snd_stream_t stream);
int snd_bn_relu_bwd(const float* dx, const float* y, long long rows, int c, const float* gamma,
                    const float* beta, float* dy, float* dgamma, float* dbeta, snd_stream_t stream);
int snd_e2e_head_ce(const float* y, const float* adj, int n_graphs, int n, int c, const float* gamma,
                    const float* beta, const float* w, const float* b, float* dy, float* dw, float* db,
                    float* dgamma, float* dbeta, double* out, snd_stream_t stream);
/* Frozen Keras BN (y' = gamma y / sqrt(1.001) + beta, model.py:41) with an activation
 * (ABI 12): act 0 identity, 1 relu, 2 lrelu(0.2) (layers.py:112-113); act_first = 1:
 * x = BN(act(y)) (GraphConvolution then BN, model.py:107), 0: x = act(BN(y)) (the
 * spatial encoder's relu after BN, model.py:123-124; identity for the disentangled
 * decoders' conv + BN, model.py:190,214).  Strided rows (ld >= c).  The backward
 * writes dy and, when non-NULL, the per-channel dgamma / dbeta (fixed-order sums). */
int snd_bn_act_fwd(const float* y, int ldy, long long rows, int c, const float* gamma,
                   const float* beta, int act, int act_first, float* x, int ldx, snd_stream_t stream);
int snd_bn_act_bwd(const float* dx, int lddx, const float* y, int ldy, long long rows, int c,
                   const float* gamma, const float* beta, int act, int act_first, float* dy, int lddy,
                   float* dgamma, float* dbeta, snd_stream_t stream);
/* Reparameterisation backward (model.py:155-159): dms = [dz + add_mu || dz eps e^s +
 * add_logstd] over ms = [mu || logstd] rows (dz / add_* may be NULL: zero). */
int snd_reparam_bwd(const float* ms, int ldms, int rows, int latent, const float* eps, const float* dz,
                    const float* add_mu, const float* add_logstd, float* dms, int lddms,
                    snd_stream_t stream);
/* y[r, c] += alpha x[r, c] over a strided [rows, cols] block: gradients of one tensor
 * reaching it along several branches (the disentangled decoders' concat inputs). */
int snd_add_strided(long long rows, int cols, float alpha, const float* x, int ldx, float* y, int ldy,
                    snd_stream_t stream);
/* Latent regularisers of one latent group (optimizer.py:7-58,159-190), mu / logstd /
 * z [batch, latent] fp32:
 *   term = w_kl kl  (cap_gamma > 0: cap_gamma relu(kl - cap_c), 'disentangled_C')
 *        + w_dip DIP(mu; lambda_od, lambda_d) + w_tc TC(z, mu, logstd)
 * kl = -0.5 mean(1 + 2s - mu^2 - e^{2s}) (optimizer.py:160); DIP optimizer.py:7-21;
 * TC the minibatch estimate of optimizer.py:29-58 (logvar = 2 logstd).  Writes
 * dmu / dlogstd = d term / d (mu, logstd) including the path through
 * z = mu + eps e^{logstd} (model.py:155-159), and out[4] (double) =
 * {kl, term, DIP, TC}.  The TC block runs in double on the fp32 operands (its gradient
 * weight is the difference of two softmaxes that nearly cancel at a small batch).
 * One workgroup: sized for the reference's batches (<= a few
 * hundred latents).  workspace >= snd_latent_reg_workspace(batch, latent) bytes
 * when w_dip or w_tc is nonzero. */
typedef struct {
  float w_kl, cap_gamma, cap_c, w_dip, lambda_od, lambda_d, w_tc;
} snd_latent_reg_t;
size_t snd_latent_reg_workspace(int batch, int latent);
int snd_latent_reg(const float* mu, const float* logstd, const float* z, int batch, int latent,
                   const snd_latent_reg_t* w, float* dmu, float* dlogstd, double* out,
                   void* workspace, snd_stream_t stream);

/* ---- forward-only e2e structure decoder (ABI 22) ------------------------------
 * The generated adjacency of model.py:193-208 from z [n_graphs, n, d] (row stride ldz),
 * without the CE and the gradients of snd_e2e_head_ce: reconstruction, sampling and
 * latent traversal (model.py:163-169,227-358).
 *   x0 = relu(BN0([z_i | z_j]));  per layer y = e2e(x) with K = n, TF SAME padding
 *   (n-1)/2 before;  the next x = relu(BN(y));  logits = relu(BN_adj(y_last)) W + b,
 *   the diagonal forced to (1, 0);  margin = l1 - l0 (-1 on the diagonal);  adj = 1 iff
 *   l1 > l0 (a tie is 0, as tf.argmax; so the diagonal is 0).
 * layers[l]: gamma / beta of the frozen Keras BN over the layer's INPUT channels (2 d for
 * layer 0, cout of layer l-1 after it), w [n, cin, cout] (model.py:202), b [cout].
 * head_gamma / head_beta [c_last] (decoder_adj), head_w [c_last][2], head_b [2] (d_e_lin2).
 * adj [n_graphs, n, n] bytes; margin [n_graphs, n, n] floats or NULL.
 * Layer 0 is factorised over the pair structure of its input (2 d multiply-adds per
 * output, the pair tensor is never formed); later layers add the row and the column
 * input before the shared taps.  BN + relu are applied as operands are loaded, the head
 * and the argmax in the last layer's epilogue: no pair tensor, no stand-alone BN pass
 * and no logits in device memory.  fp32 FMA, fixed summation order, no atomics (two runs
 * are bitwise equal); no host synchronisation and no allocation (capturable in a graph).
 * workspace >= snd_e2e_decode_workspace bytes (0 for a bad shape): at most two
 * activations [n_graphs, n, n, max cout] (one with two layers, none with one), the
 * per-node terms of layer 0 (2 n_graphs n cout_0 floats, sharing the second activation)
 * and one [n, 2 d, cout_0] weight image.
 * SND_ERR_ARG before anything touches the device: a null operand, n_layers < 1 (or > 16),
 * a width < 1, n or a cout > 512, ldz < d, c_last > 32 (as snd_e2e_head_ce), a short
 * workspace, n_graphs > 262140 (decode in chunks). */
typedef struct {
  const float *gamma, *beta;   /* frozen BN over the layer's input channels */
  const float *w, *b;          /* w [n, cin, cout], b [cout] */
  int cout;
} snd_e2e_layer_t;
size_t snd_e2e_decode_workspace(int n_graphs, int n, int d, const int* couts, int n_layers);
int snd_e2e_decode(const float* z, int ldz, int n_graphs, int n, int d,
                   const snd_e2e_layer_t* layers, int n_layers,
                   const float* head_gamma, const float* head_beta,
                   const float* head_w, const float* head_b,
                   unsigned char* adj, float* margin,
                   void* workspace, size_t workspace_bytes, snd_stream_t stream);

/* ---- factorised training engine of the e2e structure decoder (ABI 24) ----------
 * Forward, CE and every gradient of model.py:193-208 in one call, from z [n_graphs, n, d]
 * (row stride ldz) and the dense 0/1 float target adj [n_graphs, n, n] (as
 * snd_e2e_head_ce), without the pair tensor x0 [B, N, N, 2d] or its gradient.  Operands
 * as for snd_e2e_decode; layer_grads[l] holds the destinations of layer l's gradients.
 * Gradients of the MEAN CE (as snd_e2e_head_ce); every output is written, not
 * accumulated.  dz [n_graphs, n, d] (row stride lddz).  out[2] (device double) =
 * {CE summed over B N^2, correct}.
 * Forward: snd_e2e_decode's route; every layer's y_l stays in the workspace and the
 * backward recomputes relu(BN(.)) from it as operands are loaded.  The head, the CE and
 * dy_last are snd_e2e_head_ce's kernel.
 * Backward of a general layer (C -> O), g = dy_l, pb = (n-1)/2, x = relu(BN_l(y_{l-1})):
 *   dw[t,c,o] = sum_{b,i,j} (x[b,i,j+t-pb,c] + x[b,i+t-pb,j,c]) g[b,i,j,o]   (out of range: 0)
 *   db[o]     = 2 sum g
 *   dx[b,i,j,c] = sum_t sum_o w[t,c,o] (g[b,i,j-t+pb,o] + g[b,i-t+pb,j,o])
 *   dy_{l-1} = dx 1[BN_l(y_{l-1}) > 0] gamma_l BN_C;  dgamma_l, dbeta_l the per-channel sums
 * The weight gradient is reduced per (tap, group of graphs) into slabs that a second
 * kernel sums in index order.
 * Backward of layer 0 through the factorisation, g = dy_0 [B, N, N, O]:
 *   a = relu(BN0[:D](z)), a' = relu(BN0[D:](z)),
 *   Wsum_n[c,o] = sum_{t: 0 <= n+t-pb < N} w[t,c,o],  R[b,i,o] = sum_j g,  S[b,j,o] = sum_i g
 *   da[b,i,c]  = sum_j sum_o g[b,i,j,o] Wsum_j[c,o]   + sum_t sum_o R[b,i-t+pb,o] w[t,c,o]
 *   da'[b,j,c] = sum_i sum_o g[b,i,j,o] Wsum_i[D+c,o] + sum_t sum_o S[b,j-t+pb,o] w[t,D+c,o]
 *   dWsum_n[c,o]   = sum_{b,i} a[b,i,c] g[b,i,n,o];   dWsum_n[D+c,o] = sum_{b,j} a'[b,j,c] g[b,n,j,o]
 *   dw[t,c,o]   = sum_{n: 0 <= n+t-pb < N} dWsum_n[c,o]   + sum_{b,i} a[b,i+t-pb,c] R[b,i,o]
 *   dw[t,D+c,o] = sum_{n: 0 <= n+t-pb < N} dWsum_n[D+c,o] + sum_{b,j} a'[b,j+t-pb,c] S[b,j,o]
 *   db[o] = 2 sum g
 *   dz[b,n,c] = BN_C (gamma0[c] 1[a > 0] da[b,n,c] + gamma0[D+c] 1[a' > 0] da'[b,n,c])
 *   dgamma0, dbeta0: the matching per-channel sums over (b, n).
 * fp32 FMA, fixed summation order, no atomics (two runs are bitwise equal); no host
 * synchronisation and no allocation (capturable in a graph).
 * workspace >= snd_e2e_train_workspace bytes (0 for a bad shape): every layer's y, two
 * gradient activations [B, n, n, max cout], the forward's weight image and per-node terms,
 * R, S, dWsum, da | da', and the weight-gradient slabs (at most 32 of [n, cin, cout]).
 * SND_ERR_ARG before anything touches the device: a null operand (every gradient is
 * required), n_layers < 1 or > 16, a width < 1, n or a cout > 512, c_last > 32, ldz < d,
 * lddz < d, a short workspace, n_graphs < 1 or > 262140; and, d being unbounded otherwise, a d
 * whose layer-0 launches would not fit a grid (d > 2^24, or n 2 d cout_0 or n_graphs n 2 d
 * over 2^31 x 256 threads). */
typedef struct {
  float *dgamma, *dbeta;   /* [cin] */
  float *dw, *db;          /* [n, cin, cout], [cout] */
} snd_e2e_layer_grad_t;
size_t snd_e2e_train_workspace(int n_graphs, int n, int d, const int* couts, int n_layers);
int snd_e2e_train(const float* z, int ldz, const float* adj, int n_graphs, int n, int d,
                  const snd_e2e_layer_t* layers, int n_layers,
                  const float* head_gamma, const float* head_beta,
                  const float* head_w, const float* head_b,
                  float* dz, int lddz,
                  const snd_e2e_layer_grad_t* layer_grads,
                  float* d_head_gamma, float* d_head_beta, float* d_head_w, float* d_head_b,
                  double* out,
                  void* workspace, size_t workspace_bytes, snd_stream_t stream);

/* yhat = sigmoid(u w + b): the forward half of snd_sigmoid_mse for the decoders'
 * sigmoid heads at inference (no target).  u [rows, cin] (stride ldu), w [cin, cout],
 * yhat [rows, cout] (stride ldy). */
int snd_sigmoid_linear_fwd(const float* u, int ldu, long long rows, int cin, const float* w,
                           const float* b, int cout, float* yhat, int ldy, snd_stream_t stream);

/* ---- the disentangled step's loss tail and edge-score evaluation (ABI 23) -------
 * snd_disent_losses: the loss terms of one step of the disentangled model
 * (optimizer.py:146-203) from the partial results its ops leave on the device, so a step
 * reads nothing back and can be captured in a graph.
 * losses[8] (device double) = {cost, spatial_cost, adj_cost, node_cost, kl_g, kl_s, kl_sg, correct}
 * (optimizer.py:201 order, then main.py:334's count).
 *   node_cost    = (sum of sse_node[0..node_blocks)) / node_count   (snd_sigmoid_mse's sse)
 *   spatial_cost = likewise
 *   adj_cost     = ce_out[0] / pair_count;  correct = ce_out[1]     (snd_e2e_head_ce's out)
 *   cost = adj_cost + node_cost + spatial_cost + (term_s + term_g + term_sg), terms added in
 *   that order from 0.0 (reg_x[1] of snd_latent_reg's out[4]; kl_x = reg_x[0]).
 * reg_s / reg_g may be NULL ('base': their kl is written as 0 and their terms do not enter).
 * The partials are summed in index order, in double, by one thread: no atomics, no
 * allocation, no host synchronisation.  SND_ERR_ARG: a NULL sse_node, sse_spatial, ce_out,
 * reg_sg or losses, a block count < 1, a count <= 0 (or NaN). */
int snd_disent_losses(const double* sse_node, int node_blocks, double node_count,
                      const double* sse_spatial, int spatial_blocks, double spatial_count,
                      const double* ce_out, double pair_count,
                      const double* reg_s, const double* reg_g, const double* reg_sg,
                      double* losses, snd_stream_t stream);

/* snd_margin_eval: snd_zzt_eval's counters for the e2e structure decoder, whose edge score
 * is the margin l1 - l0 that snd_e2e_decode writes (main.py:13-14,423,467 for the
 * disentangled model).  margin and adj [B, N, N] contiguous fp32; the label is adj != 0.
 * The N diagonal pairs are skipped by index, whatever they hold (the decoder writes -1
 * there), and counted as TN.  Per graph b over the N^2 - N off-diagonal pairs:
 *   hist[b][label][clamp(floor(64 m) + 1024, 0, 2047)] += 1   (int64 [B, 2, 2048],
 *     snd_zzt_eval's bins; the clamp is done in float, so -inf / +inf land in bins 0 / 2047)
 *   counts[b] = {TP, FP, FN, TN} (int64 [B, 4]) at the rule m > 0: snd_e2e_decode's adj
 *     (a tie is 0), so TP + FP is the number of ones of that adj.
 * NaN margins are unspecified (no fault, no write outside the outputs).  accumulate = 0
 * clears hist and counts on the stream first, != 0 adds to them.  Integer sums only: the
 * result does not depend on scheduling and is additive over batches.  No allocation and
 * no host synchronisation.  Any pointer alignment (16-byte loads where a graph's chunk is
 * aligned, scalar loads otherwise).  workspace: snd_margin_eval_workspace() bytes (0 today;
 * NULL is accepted then).  SND_ERR_ARG before anything is launched: a NULL margin, adj,
 * hist or counts, n_graphs < 1, n < 1, a short workspace. */
size_t snd_margin_eval_workspace(int n_graphs, int n);
int snd_margin_eval(const float* margin, const float* adj, int n_graphs, int n,
                    long long* hist, long long* counts, int accumulate,
                    void* workspace, size_t workspace_bytes, snd_stream_t stream);

/* ---- disentanglement evaluation: latent-factor mutual information (ABI 25) ----
 * snd_latent_mi: the matrix of mutual information between every latent dimension and every
 * generative factor, estimated from joint histograms: the object MIG, avgMI and modularity
 * are host arithmetic on (metrics.LatentMI).  z [rows, n_lat] fp32 (row stride ldz >= n_lat)
 * holds one row per graph, the encoder means; f [rows, n_fac] fp32 (row stride ldf >= n_fac)
 * the generative factors, integer-coded ones passed as floats.  Any pointer alignment.
 *   Range.  Per column of z and of f: lo = min, hi = max over the rows (order-free, so
 *     deterministic; +-0 may come out with either sign).
 *   Bin.  Every value v goes to
 *       b = (hi > lo) ? min(nb - 1, (int)floor(((double)v - (double)lo) * nb / ((double)hi - (double)lo))) : 0
 *     evaluated in double, left to right; nb = nbz for a latent column, nbf for a factor
 *     column.  NumPy float64 on the same fp32 inputs gives the same bin, bit for bit (IEEE
 *     subtraction, multiplication and division on both sides, nothing to contract into an
 *     FMA).  k equally spaced factor values land in k distinct bins when nbf = k:
 *     floor(i k / (k - 1)) = i for i < k - 1, and the maximum is clamped to k - 1.  A
 *     constant column is all bin 0.  NaN inputs are unspecified (no fault, no write outside
 *     the outputs).
 *   Count and reduce.  joint[l][k][a][b] = #rows with bin(z[:, l]) = a and bin(f[:, k]) = b
 *     (int32).  With r, s the marginals of a joint block, natural logs, in double, summed in
 *     index order (a major, b minor):
 *       mi[l][k] = sum_{a,b: c > 0} (c / rows) log(c rows / (r_a s_b))
 *       hz[l] = - sum_a (r_a / rows) log(r_a / rows),   hf[k] likewise.
 * Outputs (device): mi [n_lat, n_fac], hz [n_lat], hf [n_fac] doubles; range
 * [n_lat + n_fac, 2] floats {lo, hi}, latent columns first (may be NULL); joint
 * [n_lat, n_fac, nbz, nbf] int32 (may be NULL: the counts then live in the workspace).
 * Counting is integer only (32-bit LDS and global atomics); there are no floating-point
 * atomics: two runs are bitwise equal, and a captured-graph replay equals an eager call.
 * No allocation, no host synchronisation.  workspace >= snd_latent_mi_workspace() bytes (0
 * for a bad shape): the row slices' ranges, the ranges and the joint counts.
 * SND_ERR_ARG before anything is launched: a NULL z, f, mi, hz or hf; rows < 1; n_lat not in
 * [1, 65536]; n_fac not in [1, 64]; nbz or nbf not in [1, 32]; ldz < n_lat; ldf < n_fac; a
 * short (or NULL) workspace. */
size_t snd_latent_mi_workspace(int rows, int n_lat, int n_fac, int nbz, int nbf);
int snd_latent_mi(const float* z, int ldz, const float* f, int ldf,
                  int rows, int n_lat, int n_fac, int nbz, int nbf,
                  double* mi, double* hz, double* hf,
                  float* range, int* joint,
                  void* workspace, size_t workspace_bytes, snd_stream_t stream);

/* ---- a14: the whole train step (main.py:315-334) ---------------------------
 * A plan fixes shapes; the step runs forward + backward of the SND-VAE
 * (SURVEY §8 "Composed step") for one batch in either decoder-input topology:
 *   SND_TSCALE  node latent: heads per node row, mu/logstd [B*N, L], J = z;
 *   SND_TREF    graph latent (model.py:113-115, model_joint.py:87-97):
 *               h = flat(G) Wh + bh per graph, z [B, L],
 *               J = reshape(z Wp + bp, [B, N, node_h]); at most 8 graphs
 *               per plan (the weight-streaming kernels keep B in registers);
 *   SND_SGJOINT the SND-VAE spatial-graph encoder (ABI 11; model_joint.py:72-85,
 *               model.py:134-151,172-180): two SpatialGraphConvolution layers
 *               (snd_sg_layer_fwd, BN + lrelu) over the B * sampling_num
 *               spanning-tree copies (batch tree_rowptr / tree_colidx / rel,
 *               features tiled per copy), flat heads per copy, z [B*S, L],
 *               J_b = mean_s reshape(z_{b,s} Wp + bp, [N, node_h]), then the
 *               graph-latent decoders; f_in = num_feature, h0/h1 unused, fp32
 *               generic engine (either dtype for the GEMM operands).
 * It writes the flat
 * gradient (same layout as params), advances *step_counter and writes
 * losses[0..7] = {cost, spatial_cost, adj_cost, node_cost, kl, acc,
 *                 adj_sum, correct} (device doubles; main.py:331-334
 * overall_loss order, optimizer.py:203).  It also writes the first six as
 * floats to grads[param_count .. +6) so one all-reduce averages them. */
typedef struct snd_config {
  int n_nodes;      /* N */
  int f_in;         /* encoder input width (num_feature + spatial_dim) */
  int num_feature;  /* node feature targets */
  int spatial_dim;  /* coordinate targets */
  int h0, h1;       /* g_conv_hidden */
  int g_hidden;     /* g_hidden_size */
  int latent;       /* L (g_latent_size) */
  int s1, s2, s3;   /* s_d_channel */
  int n1, n2;       /* n_d_channel[:2] */
  float beta;       /* KL weight */
  float pos_weight; /* 1 == reference */
  float norm;       /* 1 == reference */
  int dtype;        /* SND_F32 (parity) or SND_BF16 (throughput) */
  int topology;     /* SND_TSCALE or SND_TREF (ABI version 2) */
  int node_h;       /* width of J (node_h_size); == latent for SND_TSCALE */
  int sampling_num; /* SND_SGJOINT: spanning trees per graph (main.py:100) */
  int sg_h[6];      /* SND_SGJOINT: sg_conv_hidden [[h0,h1,h2],[h0,h1,h2]] (main.py:193) */
} snd_config_t;
enum { SND_TSCALE = 0, SND_TREF = 1, SND_SGJOINT = 2 };

/* The window SpMM's plan on the device (ABI 10; data.py window_plan, see
 * snd_csr_spmm_bf16_window): with it, the step's bf16 GraphConvolution backward
 * SpMM (A @ dP1, width 64) runs the window kernel.  meta NULL = none. */
typedef struct snd_window_plan {
  const int* meta;              /* [n_rows] */
  const uint16_t* slots;
  const int* rows;              /* [n_rows] */
  const int* order;             /* [n_rows] */
  int beta;
} snd_window_plan_t;

typedef struct snd_batch {
  const int* rowptr;           /* [B*N+1] */
  const int* colidx;           /* [nnz]   */
  const float* features;       /* [B*N, f_in] */
  const float* feature_truth;  /* [B*N, num_feature] */
  const float* spatial_truth;  /* [B*N, spatial_dim] */
  const int* row_order;        /* optional [B*N] locality schedule of the gather
                                  kernels (see snd_csr_spmm_bf16); NULL = natural */
  snd_row_tiles_t tiles;       /* optional row tiles over row_order (ABI 5; all
                                  zero = none): the bf16 encoder SpMMs stage
                                  neighbour rows in LDS */
  snd_window_plan_t window;    /* optional window SpMM plan over row_order (ABI 10) */
  /* SND_SGJOINT (ABI 11): the spanning trees of the B graphs, copy c = b * S + s of
   * graph b (input_data.py:76-83), one symmetric block-diagonal CSR over B*S*N rows;
   * rel [B*S, N, N] of each copy (the 'rel' feed / 600, input_data.py:59); features
   * are then [B*S*N, num_feature] (graph b's features in each of its copies) */
  const int* tree_rowptr;
  const int* tree_colidx;
  const float* rel;
} snd_batch_t;

typedef struct snd_plan snd_plan_t;

int snd_plan_create(const snd_config_t* cfg, int n_graphs, snd_plan_t** out);
void snd_plan_destroy(snd_plan_t* plan);
long long snd_plan_param_count(const snd_plan_t* plan);
int snd_plan_num_blocks(const snd_plan_t* plan);
int snd_plan_param_block(const snd_plan_t* plan, int idx, const char** name,
                         long long* offset, long long* numel);
size_t snd_plan_workspace_bytes(const snd_plan_t* plan);
/* Fused TF1 Adam (1 GPU: no all-reduce between gradient and update).  With m and
 * v set (flat buffers in the parameter layout), snd_train_step applies the Adam
 * update of optimizer.py:125,197 in place, through the params pointer, to the blocks
 * snd_plan_block_fused() reports nonzero; the caller's snd_adam_tf1 then covers the
 * other blocks (none on the node-latent plans).  m = v = NULL turns it off (default).
 * lr/betas/eps as snd_adam_tf1; grad_scale is 1.
 * snd_plan_block_fused (ABI 16): 0 = updated by the caller; 1 = updated inside the
 * weight-gradient stream that produces the gradient complete (graph-latent head weight,
 * d_sg_lin1 weight and bias) -- its gradient is NOT written; 2 = updated by the step's final
 * slab reduction, which writes the gradient and applies Adam to it in the same launch
 * (every block that launch writes complete), the gradient is written as usual.
 * The reduction reads the step index t = *step_counter + 1 that the step's
 * reparameterisation kernel publishes in the workspace, since the same launch's
 * finalize workgroup advances *step_counter. */
int snd_plan_fuse_adam(snd_plan_t* plan, float* m, float* v, float lr, float beta1,
                       float beta2, float eps);
int snd_plan_block_fused(const snd_plan_t* plan, int idx);
/* Bucketed data parallel (ABI 13).  Registers `event` (a hipEvent_t created by the
 * caller) to be recorded on the step's stream right after the kernel that writes
 * block idx's gradient complete, so the caller can start that bucket's collective on
 * another stream while the backward pass goes on (DP of optimizer.py:125,197 with
 * main.py:331's single update): the graph-latent d_sg_lin1 weight and
 * bias complete after the projection backward, the graph-latent head weight after
 * the head backward.  Returns k > 0, the block's completion point (blocks with the
 * same k complete together and share one event; points are reached in increasing k),
 * when it has one (the event is kept for every later snd_train_step; NULL unregisters
 * it), 0 when the block's gradient is completed by the step's final reduction
 * (nothing kept), <0 on a bad index. */
int snd_plan_grad_event(snd_plan_t* plan, int idx, void* event);
/* ABI 17: the event currently registered for block idx (NULL when none) in *event;
 * returns the block's completion point as snd_plan_grad_event does.  Lets a host
 * binding check that a freed optimizer did not unregister a newer one's events. */
int snd_plan_grad_event_get(const snd_plan_t* plan, int idx, void** event);
/* Data parallel (ABI 6): the device Philox normals of this plan's head rows start at
 * global head row `head_row_offset` (rank * n_graphs for SND_TREF, rank * n_graphs *
 * n_nodes for SND_TSCALE), so every rank of a sharded global batch draws exactly the
 * eps a single device would draw for those rows (model.py:155-159).  Default 0. */
int snd_plan_set_rng_offset(snd_plan_t* plan, long long head_row_offset);
/* Named intermediate buffers inside the workspace (tests / inspection). */
int snd_plan_buffer(const snd_plan_t* plan, const char* name,
                    long long* byte_offset, long long* numel);
int snd_train_step(const snd_plan_t* plan, const snd_batch_t* batch,
                   const float* params, float* grads, void* workspace,
                   const float* eps, unsigned long long seed,
                   int* step_counter, double* losses, snd_stream_t stream);
/* Forward-only evaluation / sampling on the plan's shapes and dtype, generic
 * kernels (main.py:358-469 generate_new / generate_new_train; model.py:163-169
 * get_random_z).  mode:
 *   SND_GEN_SAMPLE  encode `batch`, z = mu + eps exp(s) (eps_or_z = eps [RH, L]
 *                   or NULL: device Philox at (seed, *step_counter)), as in training
 *   SND_GEN_MEAN    encode `batch`, z = mu (z_mean_*, main.py:361,367)
 *   SND_GEN_PRIOR   z ~ N(0, 1) (eps_or_z = eps or NULL: Philox); batch unused
 *   SND_GEN_GIVEN   z = eps_or_z [RH, L]; batch unused
 * RH = n_graphs (SND_TREF) or n_graphs * n_nodes (SND_TSCALE).  Results stay in
 * the workspace (snd_plan_buffer): "MS" [mu || s], "Z" (node latent z / decoder
 * input J), "ZL" (graph latent z), "SHAT" generated_spatial, "XHAT"
 * generated_node_feat.  gen_adj (optional, uint8 [B, N, N]) receives
 * generated_adj: 1 iff i != j and (J J^T)_ij > 0 (argmax of the 2-class logits,
 * first index on ties, model.py:205-208).  Stream-ordered, no allocation;
 * *step_counter is read, not advanced. */
enum { SND_GEN_SAMPLE = 0, SND_GEN_MEAN = 1, SND_GEN_PRIOR = 2, SND_GEN_GIVEN = 3 };
int snd_generate(const snd_plan_t* plan, const snd_batch_t* batch, const float* params,
                 void* workspace, int mode, const float* eps_or_z, unsigned long long seed,
                 const int* step_counter, unsigned char* gen_adj, snd_stream_t stream);
/* Re-launch one kernel of the step on the workspace state left by the last
 * snd_train_step (measurement/profiling): "zzt_dense" (fused zz^T + CE),
 * "spmm_dxw1" (plain fp32 CSR SpMM, width h1; generic-engine plans),
 * "spmm_bf16" (the bf16 path's A @ dP1), "pack" / "dec:<k>" (bf16 weight
 * packing / k-th bf16 decoder kernel, k = 0..10), and on SND_TREF plans
 * "tref_head_fwd" / "tref_head_bwd" / "tref_proj_fwd" / "tref_proj_bwd"
 * (the weight-streaming heads and projection), "wgrad_multi" (the last step's
 * multi-segment weight-gradient launch) and "wgrad_multi:dims" (launches nothing:
 * returns 3 when that launch carries (row chunk, pair group, segment) as its block
 * indices, 1 when it takes the flattened grid). */
int snd_plan_launch(const snd_plan_t* plan, const snd_batch_t* batch,
                    void* workspace, const char* kernel, snd_stream_t stream);
/* Measurement only: bits that make the bf16 decoder kernels skip phases
 * (1 weight staging, 2 row staging, 4 MFMA, 8 stores, 16 column params,
 * 32 epilogue prefetch) and, read by snd_plan_create, 256 = generic-engine
 * plan, 512 = generic encoder; read by snd_train_step, 1024 = run the edge
 * terms and weight gradients on a side stream, 4096 = one weight-gradient launch
 * per weight, 1u << 31 = the multi-segment weight-gradient launch takes the flattened
 * 1-D grid even when its segments are uniform.  0 (default) = normal. */
int snd_debug_set(int flags);

/* Plan options (round 4).  "conc_decoder": 1 = run the fused decoder on a side stream
 * beside the zz^T kernel (whose column splits then leave the decoder's tiles their CUs),
 * 0 = serial, -1 = auto (the default: on for graphs of N >= 2048 with at most 64
 * decoder tiles -- one or two N = 4096 graphs, C3's per-rank batch -- where neither
 * kernel fills the chip).  The
 * side stream is created by the first non-capturing step.
 * "reduce_adam" (ABI 16): 1 (default) = with snd_plan_fuse_adam set, the blocks the
 * final reduction completes take their Adam update in that launch (snd_plan_block_fused
 * 2); 0 = they are left to the caller's snd_adam_tf1 (kind 0).  Set it before
 * snd_plan_fuse_adam / the optimizer reads the kinds.
 * Returns 1 when the option is in effect for this plan, 0 when the plan cannot use it,
 * SND_ERR_ARG for an unknown option. */
int snd_plan_set_option(snd_plan_t* plan, const char* name, int value);

#ifdef __cplusplus
}
#endif
#endif /* SND_VAE_H */
