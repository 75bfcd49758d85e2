// SpatialGraphConvolution_3D (layers.py:200-277), the three-hop spatial-graph layer of
// the reference's 3-D datasets (model.py:139-140), and the encoder layer
// lrelu(BN(SGConv3D)), forward and backward.
//
// The reference materialises B x N x N x N x N x (4F+5) message tensors.  lrelu acts on
// the CONCATENATED INPUTS of every message matmul, so the first message layer is a sum
// of per-node / per-edge / per-pair terms and its sum over p collapses (A binary,
// LX = lrelu(X), L_ab = lrelu(rel_ab), d = degree, e_k = sum_p A_kp L_kp,
// Q_ik = sum_{p in N(k)} L_ip; Matrix0 rows named by what they multiply):
//   a = LX M0i, b = LX M0j, G = [d LX | A LX] [M0k; M0p]
//   S4_ijk = d_k (a_i + b_j + L_ij m0_ij + L_jk m0_jk + L_ik m0_ik)
//            + G_k + e_k m0_kp + d_k bias0 + Q_ik m0_ip           per directed 2-path i-j-k
//   T_ij   = sum_{k in N(j)} lrelu(S4_ijk)                        [h0] per directed edge
//   S3_ij  = d_j (u_i + v_j + L_ij m1_ij + bias1) + w_j + e_j m1_jk + Q_ij m1_ik + T_ij M1s
//   P_i    = sum_{j in N(i)} lrelu(S3_ij)
//   m2_i   = d_i (LX_i M2i + bias2) + (A LX)_i M2j + e_i m2_r + P_i M2s
//   y_i    = [LX_i | lrelu(m2_i)] Matrix3 + bias3
// From S3 downwards this is the two-hop layer (snd_sg.hip) with one more term, T M1s.
// The new work is O(P2 h0) over the directed 2-paths plus the per-path scalars L_ik,
// Q_ik, which depend on the data only and are recomputed from rel where a path is walked.
// Every sum runs along a row's own edges or its reverse edges (edge_rev) in CSR order:
// no floating-point atomics, two runs are bitwise equal.  The dense products run on the
// generic MFMA GEMM (fp32 operands), weight gradients are split-K slabs over the R rows
// or the nnz edges, reduced in fixed order.  Backward derivation: DESIGN.md §7.
#include <algorithm>
#include <climits>

#include "snd_gemm.hpp"
#include "snd_sg3.hpp"

namespace snd {

Sg3POff sg3_poff(int F, int h0, int h1, int h2, int h3) {
  Sg3POff p{};
  p.M0 = 0;
  p.b0 = p.M0 + (long long)(4 * F + 5) * h0;
  p.M1 = p.b0 + h0;
  p.b1 = p.M1 + (long long)(3 * F + 3 + h0) * h1;
  p.M2 = p.b1 + h1;
  p.b2 = p.M2 + (long long)(2 * F + 1 + h1) * h2;
  p.M3 = p.b2 + h2;
  p.b3 = p.M3 + (long long)(F + h2) * h3;
  p.gamma = p.b3 + h3;
  p.beta = p.gamma + h3;
  p.total = p.beta + h3;
  return p;
}

namespace {

constexpr int NT = 256;

__device__ __forceinline__ float lr(float x) { return x >= 0.f ? x : kLeak * x; }
__device__ __forceinline__ float lrg(float x) { return x >= 0.f ? 1.f : kLeak; }

struct Geo {   // per-layer widths and workspace map (floats)
  int F, h0, h1, h2, h3, ld2, ld3;
  long long R, E;
  long long oZ2, oZ3, oABG, oUVW, oT, oTS, oM2P, oDY, oDTY, oDZ3, oDM2, oDZ2, oDUVW, oTM1, oGS,
      oDT, oDABG, oTM0, oDLX, oDAX, oSLAB;
  long long total;
  int splitsR, splitsE;
};

long long r64(long long n) { return (n + 63) / 64 * 64; }

Geo geo(long long R, long long nnz, int F, int h0, int h1, int h2, int h3) {
  Geo g{};
  g.F = F; g.h0 = h0; g.h1 = h1; g.h2 = h2; g.h3 = h3; g.R = R; g.E = nnz;
  g.ld2 = 2 * F + 2 + h1;      // [d LX | A LX | e | P | d]
  g.ld3 = F + h2 + 1;          // [LX | lrelu(m2) | 1]
  long long o = 0;
  auto take = [&](long long n) { long long r = o; o += r64(n); return r; };
  g.oZ2 = take(R * g.ld2);
  g.oZ3 = take(R * g.ld3);
  g.oABG = take(R * 3 * h0);
  g.oUVW = take(R * 3 * h1);
  g.oT = take(nnz * h0);
  g.oTS = take(nnz * h1);
  g.oM2P = take(R * h2);
  g.oDY = take(R * h3);
  g.oDTY = take(R * 2 * h3);
  g.oDZ3 = take(R * (F + h2));
  g.oDM2 = take(R * h2);
  g.oDZ2 = take(R * (2 * F + 1 + h1));
  g.oDUVW = take(R * 3 * h1);
  g.oTM1 = take(R * 4 * h1);
  g.oGS = take(nnz * h1);
  g.oDT = take(nnz * h0);
  g.oDABG = take(R * 3 * h0);
  g.oTM0 = take(R * 6 * h0);
  g.oDLX = take(R * F);
  g.oDAX = take(R * F);
  // split-K parts of 128 rows (at most 64 parts): the backward has 13 reductions over R or nnz,
  // each a serial K loop of one workgroup per output tile.  Measured at R = 2500 (100 trees of
  // 25 nodes, widths [10]*4) the backward took 1256 us with snd_sg.hip's 4096 rows per part,
  // 421 us with 512 and 261 us with 128
  g.splitsR = std::max(1, std::min(64, cdiv(R, 128)));
  g.splitsE = std::max(1, std::min(64, cdiv(nnz, 128)));
  const long long mnR = std::max<long long>({(long long)g.ld3 * h3, (long long)g.ld2 * h2,
                                             (long long)F * h1, 2LL * F * h0, 2LL * h3, 4LL * h1,
                                             6LL * h0});
  const long long mnE = (long long)h0 * h1;
  g.oSLAB = take(std::max(g.splitsR * mnR, g.splitsE * mnE));
  g.total = o;
  return g;
}

// Matrix0's scalar rows and bias0 (each [h0]); bias0 follows Matrix0 in the buffer
struct M0Rows { const float *ij, *jk, *kp, *ik, *ip, *b0; };
__device__ __forceinline__ M0Rows m0_rows(const float* prm, const Sg3POff& po, int F, int h0) {
  const float* r = prm + po.M0 + (long long)4 * F * h0;
  return {r, r + h0, r + 2 * h0, r + 3 * h0, r + 4 * h0, prm + po.b0};
}

// ------------------------------------------------------------------ forward
// thread per (row, f): LX, A LX; Z2e = [d LX | A LX | e | P (later) | d], Z3e = [LX | . | 1]
__global__ void __launch_bounds__(NT) sg3_gather_kernel(snd_sg_graph_t g, const float* x, int ldx,
                                                        Geo G, float* ws) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= G.R * G.F) return;
  const int i = (int)(idx / G.F), f = (int)(idx - (long long)i * G.F);
  const float l = lr(x[(long long)i * ldx + f]);
  float ax = 0.f;
  for (int q = g.rowptr[i]; q < g.rowptr[i + 1]; ++q) ax += lr(x[(long long)g.colidx[q] * ldx + f]);
  const float d = g.node_deg[i];
  float* z2 = ws + G.oZ2 + (long long)i * G.ld2;
  float* z3 = ws + G.oZ3 + (long long)i * G.ld3;
  z2[f] = d * l;
  z2[G.F + f] = ax;
  z3[f] = l;
  if (f == 0) {
    z2[2 * G.F] = g.node_e[i];
    z2[2 * G.F + 1 + G.h1] = d;
    z3[G.F + G.h2] = 1.f;
  }
}

// Q_ik = sum_{p in N(k)} lrelu(rel_ip), rrow = rel row of i, off = first id of the graph
__device__ __forceinline__ float q_of(const snd_sg_graph_t& g, const float* rrow, int off, int k) {
  float s = 0.f;
  for (int p = g.rowptr[k]; p < g.rowptr[k + 1]; ++p) s += lr(rrow[g.colidx[p] - off]);
  return s;
}

// S4 of the 2-path i-j-k, channel c.  ai = a_i[c], bj = b_j[c]; abg = [a | b | G] rows
__device__ __forceinline__ float s4_of(float ai, float bj, float lij, float ljk, float lik,
                                       float qik, float dk, float ek, float gk, const M0Rows& m,
                                       int c) {
  return dk * (ai + bj + lij * m.ij[c] + ljk * m.jk[c] + lik * m.ik[c] + m.b0[c]) + gk +
         ek * m.kp[c] + qik * m.ip[c];
}

// thread per (row i, c < h0): T_q = sum_{k in N(j)} lrelu(S4_ijk) for every edge q = (i -> j)
__global__ void __launch_bounds__(NT) sg3_path_fwd_kernel(snd_sg_graph_t g, const float* rel, Geo G,
                                                          const float* prm, Sg3POff po, float* ws) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= G.R * G.h0) return;
  const int i = (int)(idx / G.h0), c = (int)(idx - (long long)i * G.h0);
  const int n = g.n_per_graph, off = i / n * n;
  const float* rrow = rel + (long long)i * n;
  const M0Rows m = m0_rows(prm, po, G.F, G.h0);
  const float* abg = ws + G.oABG;
  const int h3w = 3 * G.h0;
  const float ai = abg[(long long)i * h3w + c];
  for (int q = g.rowptr[i]; q < g.rowptr[i + 1]; ++q) {
    const int j = g.colidx[q];
    const float bj = abg[(long long)j * h3w + G.h0 + c], lij = g.edge_lr[q];
    float acc = 0.f;
    for (int t = g.rowptr[j]; t < g.rowptr[j + 1]; ++t) {
      const int k = g.colidx[t];
      acc += lr(s4_of(ai, bj, lij, g.edge_lr[t], lr(rrow[k - off]), q_of(g, rrow, off, k),
                      g.node_deg[k], g.node_e[k], abg[(long long)k * h3w + 2 * G.h0 + c], m, c));
    }
    ws[G.oT + (long long)q * G.h0 + c] = acc;
  }
}

// S3 of edge q = (i -> j), channel c (ts = (T_ij M1s)[c])
__device__ __forceinline__ float s3_of(const float* uvw, int h1, int i, int j, int c, float dj,
                                       float ej, float lrq, float qq, float ts, const float* m1r,
                                       const float* m1s, const float* m1t, const float* b1) {
  const float* ui = uvw + (long long)i * 3 * h1;
  const float* uj = uvw + (long long)j * 3 * h1;
  return dj * (ui[c] + uj[h1 + c] + lrq * m1r[c] + b1[c]) + uj[2 * h1 + c] + ej * m1s[c] +
         qq * m1t[c] + ts;
}

// thread per (row i, c < h1): P_i = sum_j lrelu(S3_ij) -> Z2e[i, 2F+1+c]
__global__ void __launch_bounds__(NT) sg3_edge_fwd_kernel(snd_sg_graph_t g, Geo G, const float* prm,
                                                          Sg3POff po, float* ws) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= G.R * G.h1) return;
  const int i = (int)(idx / G.h1), c = (int)(idx - (long long)i * G.h1);
  const float* m1r = prm + po.M1 + (long long)3 * G.F * G.h1;
  const float* m1s = m1r + G.h1;
  const float* m1t = m1s + G.h1;
  const float* uvw = ws + G.oUVW;
  const float* ts = ws + G.oTS;
  float acc = 0.f;
  for (int q = g.rowptr[i]; q < g.rowptr[i + 1]; ++q) {
    const int j = g.colidx[q];
    acc += lr(s3_of(uvw, G.h1, i, j, c, g.node_deg[j], g.node_e[j], g.edge_lr[q], g.edge_q[q],
                    ts[(long long)q * G.h1 + c], m1r, m1s, m1t, prm + po.b1));
  }
  ws[G.oZ2 + (long long)i * G.ld2 + 2 * G.F + 1 + c] = acc;
}

// Z3e[:, F + c] = lrelu(m2)
__global__ void __launch_bounds__(NT) sg3_act_kernel(Geo G, float* ws) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= G.R * G.h2) return;
  const long long i = idx / G.h2;
  const int c = (int)(idx - i * G.h2);
  ws[G.oZ3 + i * G.ld3 + G.F + c] = lr(ws[G.oM2P + idx]);
}

// encoder epilogue: out = lrelu(BN(y))
__global__ void __launch_bounds__(NT) sg3_bn_fwd_kernel(long long n, int h3, const float* y,
                                                        const float* gamma, const float* beta,
                                                        float* out) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= n) return;
  const int c = (int)(idx % h3);
  out[idx] = lr(y[idx] * (gamma[c] * kBnC) + beta[c]);
}

// ------------------------------------------------------------------ backward
// DY = dout lrelu'(t) gamma c; DTY = [dT | dT y c] (column sums -> dbeta, dgamma)
__global__ void __launch_bounds__(NT) sg3_bn_bwd_kernel(Geo G, const float* y, const float* dout,
                                                        const float* gamma, const float* beta,
                                                        float* ws) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= G.R * G.h3) return;
  const long long i = idx / G.h3;
  const int c = (int)(idx - i * G.h3);
  const float yv = y[idx];
  const float dt = dout[idx] * lrg(yv * (gamma[c] * kBnC) + beta[c]);
  ws[G.oDY + idx] = dt * gamma[c] * kBnC;
  float* dty = ws + G.oDTY + i * 2 * G.h3;
  dty[c] = dt;
  dty[G.h3 + c] = dt * yv * kBnC;
}

// DM2 = dZ3[:, F:] lrelu'(m2)
__global__ void __launch_bounds__(NT) sg3_act_bwd_kernel(Geo G, float* ws) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= G.R * G.h2) return;
  const long long i = idx / G.h2;
  const int c = (int)(idx - i * G.h2);
  ws[G.oDM2 + idx] = ws[G.oDZ3 + i * (G.F + G.h2) + G.F + c] * lrg(ws[G.oM2P + idx]);
}

// thread per (row r, c < h1), G_ij = dP_i lrelu'(S3_ij), stored per edge in GS:
//   du_r = sum_n G_rn d_n;  dw_r = sum_n G_nr (reverse edges);  dv_r = d_r dw_r
//   TM1_r = [sum_n G_rn d_n lr_rn | du_r | sum_n G_rn e_n | sum_n G_rn Q_rn]
__global__ void __launch_bounds__(NT) sg3_edge_bwd_kernel(snd_sg_graph_t g, Geo G, const float* prm,
                                                          Sg3POff po, float* ws) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= G.R * G.h1) return;
  const int r = (int)(idx / G.h1), c = (int)(idx - (long long)r * G.h1);
  const float* m1r = prm + po.M1 + (long long)3 * G.F * G.h1;
  const float* m1s = m1r + G.h1;
  const float* m1t = m1s + G.h1;
  const float* b1 = prm + po.b1;
  const float* uvw = ws + G.oUVW;
  const float* ts = ws + G.oTS;
  const int ldz2 = 2 * G.F + 1 + G.h1;
  const float* dz2 = ws + G.oDZ2;
  const float dPr = dz2[(long long)r * ldz2 + 2 * G.F + 1 + c];
  const float dr = g.node_deg[r], er = g.node_e[r];
  float du = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f, dw = 0.f;
  for (int q = g.rowptr[r]; q < g.rowptr[r + 1]; ++q) {
    const int n = g.colidx[q];
    const float dn = g.node_deg[n], en = g.node_e[n];
    const float lq = g.edge_lr[q], qq = g.edge_q[q];
    const float Gf = dPr * lrg(s3_of(uvw, G.h1, r, n, c, dn, en, lq, qq,
                                     ts[(long long)q * G.h1 + c], m1r, m1s, m1t, b1));
    ws[G.oGS + (long long)q * G.h1 + c] = Gf;
    du += Gf * dn;
    t1 += Gf * dn * lq;
    t2 += Gf * en;
    t3 += Gf * qq;
    const int qr = g.edge_rev[q];               // edge (n -> r)
    if (qr < 0) continue;
    const float dPn = dz2[(long long)n * ldz2 + 2 * G.F + 1 + c];
    dw += dPn * lrg(s3_of(uvw, G.h1, n, r, c, dr, er, g.edge_lr[qr], g.edge_q[qr],
                          ts[(long long)qr * G.h1 + c], m1r, m1s, m1t, b1));
  }
  float* o = ws + G.oDUVW + (long long)r * 3 * G.h1;
  o[c] = du;
  o[G.h1 + c] = dr * dw;
  o[2 * G.h1 + c] = dw;
  float* t = ws + G.oTM1 + (long long)r * 4 * G.h1;
  t[c] = t1;
  t[G.h1 + c] = du;
  t[2 * G.h1 + c] = t2;
  t[3 * G.h1 + c] = t3;
}

// thread per (row r, c < h0), gS4_ijk = lrelu'(S4_ijk) dT_ij over every 2-path r is on:
//   r = i (paths r-j-n):  da_r = sum d_n gS4;  TM0_r[ij, jk, ik, ip] = sum gS4 {d_n L_rj,
//                         d_n L_jn, d_n L_rn, Q_rn}
//   r = k (paths n-j-r):  dG_r = sum gS4, walked over the reverse edges of j's row
//   r = j (paths i-r-k):  db_r = sum d_k gS4
//   TM0_r[kp] = e_r dG_r, TM0_r[bias0] = d_r dG_r   (columns in Matrix0's row order)
__global__ void __launch_bounds__(NT) sg3_path_bwd_kernel(snd_sg_graph_t g, const float* rel, Geo G,
                                                          const float* prm, Sg3POff po, float* ws) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= G.R * G.h0) return;
  const int r = (int)(idx / G.h0), c = (int)(idx - (long long)r * G.h0);
  const int n = g.n_per_graph, off = r / n * n;
  const float* rrow = rel + (long long)r * n;
  const M0Rows m = m0_rows(prm, po, G.F, G.h0);
  const float* abg = ws + G.oABG;
  const float* dT = ws + G.oDT;
  const int h3w = 3 * G.h0;
  const float ar = abg[(long long)r * h3w + c], br = abg[(long long)r * h3w + G.h0 + c];
  const float gr = abg[(long long)r * h3w + 2 * G.h0 + c];
  const float dr = g.node_deg[r], er = g.node_e[r];
  const int rs = g.rowptr[r], re = g.rowptr[r + 1];
  float da = 0.f, db = 0.f, dg = 0.f, tij = 0.f, tjk = 0.f, tik = 0.f, tip = 0.f;
  for (int q = rs; q < re; ++q) {
    const int j = g.colidx[q];
    const int qjr = g.edge_rev[q];              // edge (j -> r)
    if (qjr < 0) continue;
    const float lrj = g.edge_lr[q], ljr = g.edge_lr[qjr];
    const float bj = abg[(long long)j * h3w + G.h0 + c];
    const float dTq = dT[(long long)q * G.h0 + c];
    for (int t = g.rowptr[j]; t < g.rowptr[j + 1]; ++t) {
      const int v = g.colidx[t];
      const float ljv = g.edge_lr[t], dv = g.node_deg[v];
      // path r-j-v (i = r, k = v)
      const float lrv = lr(rrow[v - off]), qrv = q_of(g, rrow, off, v);
      const float gs = dTq * lrg(s4_of(ar, bj, lrj, ljv, lrv, qrv, dv, g.node_e[v],
                                       abg[(long long)v * h3w + 2 * G.h0 + c], m, c));
      da += dv * gs;
      tij += dv * lrj * gs;
      tjk += dv * ljv * gs;
      tik += dv * lrv * gs;
      tip += qrv * gs;
      // path v-j-r (i = v, k = r), its edge (v -> j) is the reverse of t
      const int qvj = g.edge_rev[t];
      if (qvj < 0) continue;
      const float* vrow = rel + (long long)v * n;
      dg += dT[(long long)qvj * G.h0 + c] *
            lrg(s4_of(abg[(long long)v * h3w + c], bj, g.edge_lr[qvj], ljr, lr(vrow[r - off]),
                      q_of(g, vrow, off, r), dr, er, gr, m, c));
    }
  }
  for (int q = rs; q < re; ++q) {               // paths i-r-k
    const int i = g.colidx[q];
    const int qir = g.edge_rev[q];
    if (qir < 0) continue;
    const float* irow = rel + (long long)i * n;
    const float ai = abg[(long long)i * h3w + c], lir = g.edge_lr[qir];
    const float dTq = dT[(long long)qir * G.h0 + c];
    for (int t = rs; t < re; ++t) {
      const int k = g.colidx[t];
      const float dk = g.node_deg[k];
      db += dk * dTq * lrg(s4_of(ai, br, lir, g.edge_lr[t], lr(irow[k - off]),
                                 q_of(g, irow, off, k), dk, g.node_e[k],
                                 abg[(long long)k * h3w + 2 * G.h0 + c], m, c));
    }
  }
  float* o = ws + G.oDABG + (long long)r * h3w;
  o[c] = da;
  o[G.h0 + c] = db;
  o[2 * G.h0 + c] = dg;
  float* t = ws + G.oTM0 + (long long)r * 6 * G.h0;
  t[c] = tij;
  t[G.h0 + c] = tjk;
  t[2 * G.h0 + c] = er * dg;
  t[3 * G.h0 + c] = tik;
  t[4 * G.h0 + c] = tip;
  t[5 * G.h0 + c] = dr * dg;
}

// thread per (row i, f):
//   dLX = dZ3[:, f] + d dZ2[:, f] + du M1i^T + dv M1j^T + da M0i^T + db M0j^T + d dG M0k^T
//   dAX = dZ2[:, F + f] + dw M1k^T + dG M0p^T
__global__ void __launch_bounds__(NT) sg3_bwd_node_kernel(snd_sg_graph_t g, Geo G, const float* prm,
                                                          Sg3POff po, float* ws) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= G.R * G.F) return;
  const int i = (int)(idx / G.F), f = (int)(idx - (long long)i * G.F);
  const float* m0 = prm + po.M0;
  const float* m1 = prm + po.M1;
  const float* duvw = ws + G.oDUVW + (long long)i * 3 * G.h1;
  const float* dabg = ws + G.oDABG + (long long)i * 3 * G.h0;
  const float* dz2 = ws + G.oDZ2 + (long long)i * (2 * G.F + 1 + G.h1);
  const float d = g.node_deg[i];
  float dlx = ws[G.oDZ3 + (long long)i * (G.F + G.h2) + f] + d * dz2[f];
  float dax = dz2[G.F + f];
  {
    const float* mx = m1 + (long long)f * G.h1;
    const float* my = m1 + (long long)(G.F + f) * G.h1;
    const float* mz = m1 + (long long)(2 * G.F + f) * G.h1;
    for (int c = 0; c < G.h1; ++c) {
      dlx += duvw[c] * mx[c] + duvw[G.h1 + c] * my[c];
      dax += duvw[2 * G.h1 + c] * mz[c];
    }
  }
  {
    const float* mi = m0 + (long long)f * G.h0;
    const float* mj = m0 + (long long)(G.F + f) * G.h0;
    const float* mk = m0 + (long long)(2 * G.F + f) * G.h0;
    const float* mp = m0 + (long long)(3 * G.F + f) * G.h0;
    float sk = 0.f;
    for (int c = 0; c < G.h0; ++c) {
      dlx += dabg[c] * mi[c] + dabg[G.h0 + c] * mj[c];
      sk += dabg[2 * G.h0 + c] * mk[c];
      dax += dabg[2 * G.h0 + c] * mp[c];
    }
    dlx += d * sk;
  }
  ws[G.oDLX + idx] = dlx;
  ws[G.oDAX + idx] = dax;
}

// dX = lrelu'(x) (dLX + A^T dAX), A symmetric
__global__ void __launch_bounds__(NT) sg3_bwd_x_kernel(snd_sg_graph_t g, Geo G, const float* x,
                                                       int ldx, const float* ws, float* dx, int lddx) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx >= G.R * G.F) return;
  const int i = (int)(idx / G.F), f = (int)(idx - (long long)i * G.F);
  float s = ws[G.oDLX + idx];
  for (int q = g.rowptr[i]; q < g.rowptr[i + 1]; ++q) s += ws[G.oDAX + (long long)g.colidx[q] * G.F + f];
  dx[(long long)i * lddx + f] = s * lrg(x[(long long)i * ldx + f]);
}

__global__ void __launch_bounds__(NT) sg3_zero_kernel(float* p, long long n) {
  const long long idx = (long long)blockIdx.x * NT + threadIdx.x;
  if (idx < n) p[idx] = 0.f;
}

unsigned nblk(long long n) { return (unsigned)((n + NT - 1) / NT); }

// C[M, N] (row-major, ldc) = A[M, K] B[K, N]
int mm(const float* A, int lda, int amode, const float* B, int ldb, int bmode, int M, int N, int K,
       float* C, int ldc, hipStream_t s) {
  GemmArgs a{};
  a.M = M; a.N = N; a.K = K; a.A = A; a.lda = lda; a.B = B; a.ldb = ldb; a.C = C; a.ldc = ldc;
  a.kchunk = (int)round_up(K > 0 ? K : 1, kGemmBK);
  return launch_gemm(a, amode, bmode, E_STORE, SND_F32, 1, s);
}

// weight gradient dst[m][n] (ld ld_dst) = sum_r A[r][m] D[r][n], split-K over the K rows
// (the R node rows or the nnz edges) into `splits` slabs reduced in fixed order
int wg(const Geo& G, float* ws, long long K, int splits, const float* A, int lda, int M,
       const float* D, int ldd_in, int N, float* dst, int ld_dst, hipStream_t s) {
  GemmArgs a{};
  a.M = M; a.N = N; a.K = (int)K; a.A = A; a.lda = lda; a.B = D; a.ldb = ldd_in;
  a.C = ws + G.oSLAB;
  a.kchunk = (int)round_up(cdiv(K, splits), kGemmBK);
  const int parts = cdiv(K, a.kchunk);
  SND_TRY(launch_gemm(a, A_COL, B_ROW, E_PART, SND_F32, parts, s));
  ReduceDesc rd{ws + G.oSLAB, dst, parts, N, (long long)M * N, 1.f, 0, M, N, ld_dst};
  return launch_reduce(&rd, 1, s);
}

// column sums of B [R, N] (ld N) as split-K partials [parts][N] in the slab; returns parts
int colsum(const Geo& G, float* ws, const float* ones, const float* B, int N, hipStream_t s) {
  GemmArgs a{};
  a.M = 1; a.N = N; a.K = (int)G.R; a.A = ones; a.lda = G.ld3; a.B = B; a.ldb = N;
  a.C = ws + G.oSLAB;
  a.kchunk = (int)round_up(cdiv(G.R, G.splitsR), kGemmBK);
  const int parts = cdiv(G.R, a.kchunk);
  SND_TRY(launch_gemm(a, A_COL, B_ROW, E_PART, SND_F32, parts, s));
  return parts;
}

int args_ok(const char* fn, const snd_sg_graph_t* g, const float* rel, long long nnz,
            long long n_paths, const float* x, int ldx, int f, int h0, int h1, int h2, int h3,
            const float* params, const void* workspace, size_t workspace_bytes) {
  SND_CHECK_ARG(g && g->rowptr && g->colidx && g->edge_lr && g->edge_q && g->edge_rev &&
                    g->node_deg && g->node_e,
                "%s: incomplete graph (run snd_sg_prep first)", fn);
  SND_CHECK_ARG(rel && x && params && workspace, "%s: null argument", fn);
  SND_CHECK_ARG(f >= 1 && f <= 4096 && h0 >= 1 && h1 >= 1 && h2 >= 1 && h3 >= 1,
                "%s: widths must be at least 1 (f at most 4096)", fn);
  SND_CHECK_ARG(g->n_rows >= 0 && g->n_per_graph > 0 && g->n_rows % g->n_per_graph == 0,
                "%s: n_rows must be a multiple of n_per_graph", fn);
  SND_CHECK_ARG(nnz >= 0 && nnz <= INT_MAX && n_paths >= 0, "%s: nnz / n_paths out of range", fn);
  SND_CHECK_ARG(ldx >= f, "%s: ldx (%d) < f (%d)", fn, ldx, f);
  const size_t need = (size_t)geo(g->n_rows, nnz, f, h0, h1, h2, h3).total * sizeof(float);
  SND_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes, snd_sg3_workspace needs %zu",
                fn, workspace_bytes, need);
  return 0;
}

}  // namespace
}  // namespace snd

using namespace snd;

extern "C" long long snd_sg3_param_count(int f, int h0, int h1, int h2, int h3) {
  if (f <= 0 || h0 <= 0 || h1 <= 0 || h2 <= 0 || h3 <= 0) return -1;
  return sg3_poff(f, h0, h1, h2, h3).total;
}

extern "C" size_t snd_sg3_workspace(int n_rows, long long nnz, long long n_paths, int f, int h0,
                                    int h1, int h2, int h3) {
  if (n_rows < 0 || nnz < 0 || n_paths < 0 || f <= 0 || h0 <= 0 || h1 <= 0 || h2 <= 0 || h3 <= 0)
    return 0;
  return (size_t)geo(n_rows, nnz, f, h0, h1, h2, h3).total * sizeof(float);
}

extern "C" int snd_sg3_layer_fwd(const snd_sg_graph_t* g, const float* rel, long long nnz,
                                 long long n_paths, const float* x, int ldx, int f, int h0, int h1,
                                 int h2, int h3, const float* params, int bn_act, float* y,
                                 float* out, void* workspace, size_t workspace_bytes,
                                 snd_stream_t stream) {
  const char* fn = "snd_sg3_layer_fwd";
  SND_TRY(args_ok(fn, g, rel, nnz, n_paths, x, ldx, f, h0, h1, h2, h3, params, workspace,
                  workspace_bytes));
  SND_CHECK_ARG(y, "%s: null argument", fn);
  SND_CHECK_ARG(!bn_act || out, "%s: bn_act needs out", fn);
  hipStream_t s = (hipStream_t)stream;
  const Geo G = geo(g->n_rows, nnz, f, h0, h1, h2, h3);
  const Sg3POff po = sg3_poff(f, h0, h1, h2, h3);
  float* ws = (float*)workspace;
  const int R = (int)G.R, E = (int)G.E;
  if (R == 0) return 0;
  hipLaunchKernelGGL(sg3_gather_kernel, dim3(nblk(G.R * f)), dim3(NT), 0, s, *g, x, ldx, G, ws);
  SND_LAUNCH_CHECK("sg3_gather_kernel");
  const float* m0 = params + po.M0;
  const float* m1 = params + po.M1;
  float* abg = ws + G.oABG;
  float* uvw = ws + G.oUVW;
  // a = LX M0i, b = LX M0j, G = [d LX | A LX] [M0k; M0p]
  SND_TRY(mm(ws + G.oZ3, G.ld3, A_ROW, m0, h0, B_ROW, R, h0, f, abg, 3 * h0, s));
  SND_TRY(mm(ws + G.oZ3, G.ld3, A_ROW, m0 + (long long)f * h0, h0, B_ROW, R, h0, f, abg + h0,
             3 * h0, s));
  SND_TRY(mm(ws + G.oZ2, G.ld2, A_ROW, m0 + (long long)2 * f * h0, h0, B_ROW, R, h0, 2 * f,
             abg + 2 * h0, 3 * h0, s));
  // u = LX M1i, v = LX M1j, w = (A LX) M1k
  SND_TRY(mm(ws + G.oZ3, G.ld3, A_ROW, m1, h1, B_ROW, R, h1, f, uvw, 3 * h1, s));
  SND_TRY(mm(ws + G.oZ3, G.ld3, A_ROW, m1 + (long long)f * h1, h1, B_ROW, R, h1, f, uvw + h1,
             3 * h1, s));
  SND_TRY(mm(ws + G.oZ2 + f, G.ld2, A_ROW, m1 + (long long)2 * f * h1, h1, B_ROW, R, h1, f,
             uvw + 2 * h1, 3 * h1, s));
  if (E > 0) {
    hipLaunchKernelGGL(sg3_path_fwd_kernel, dim3(nblk(G.R * h0)), dim3(NT), 0, s, *g, rel, G, params,
                       po, ws);
    SND_LAUNCH_CHECK("sg3_path_fwd_kernel");
    // TS = T M1s
    SND_TRY(mm(ws + G.oT, h0, A_ROW, m1 + (long long)(3 * f + 3) * h1, h1, B_ROW, E, h1, h0,
               ws + G.oTS, h1, s));
  }
  hipLaunchKernelGGL(sg3_edge_fwd_kernel, dim3(nblk(G.R * h1)), dim3(NT), 0, s, *g, G, params, po, ws);
  SND_LAUNCH_CHECK("sg3_edge_fwd_kernel");
  // m2 = [d LX | A LX | e | P | d] [M2; b2]
  SND_TRY(mm(ws + G.oZ2, G.ld2, A_ROW, params + po.M2, h2, B_ROW, R, h2, G.ld2, ws + G.oM2P, h2, s));
  hipLaunchKernelGGL(sg3_act_kernel, dim3(nblk(G.R * h2)), dim3(NT), 0, s, G, ws);
  SND_LAUNCH_CHECK("sg3_act_kernel");
  // y = [LX | lrelu(m2) | 1] [M3; b3]
  SND_TRY(mm(ws + G.oZ3, G.ld3, A_ROW, params + po.M3, h3, B_ROW, R, h3, G.ld3, y, h3, s));
  if (bn_act) {
    hipLaunchKernelGGL(sg3_bn_fwd_kernel, dim3(nblk(G.R * h3)), dim3(NT), 0, s, G.R * h3, h3, y,
                       params + po.gamma, params + po.beta, out);
    SND_LAUNCH_CHECK("sg3_bn_fwd_kernel");
  }
  return 0;
}

extern "C" int snd_sg3_layer_bwd(const snd_sg_graph_t* g, const float* rel, long long nnz,
                                 long long n_paths, const float* x, int ldx, int f, int h0, int h1,
                                 int h2, int h3, const float* params, int bn_act, const float* y,
                                 const float* dout, float* dx, int lddx, float* grads,
                                 void* workspace, size_t workspace_bytes, snd_stream_t stream) {
  const char* fn = "snd_sg3_layer_bwd";
  SND_TRY(args_ok(fn, g, rel, nnz, n_paths, x, ldx, f, h0, h1, h2, h3, params, workspace,
                  workspace_bytes));
  SND_CHECK_ARG(y && dout && grads, "%s: null argument", fn);
  SND_CHECK_ARG(!dx || lddx >= f, "%s: lddx (%d) < f (%d)", fn, lddx, f);
  hipStream_t s = (hipStream_t)stream;
  const Geo G = geo(g->n_rows, nnz, f, h0, h1, h2, h3);
  const Sg3POff po = sg3_poff(f, h0, h1, h2, h3);
  float* ws = (float*)workspace;
  const int R = (int)G.R, E = (int)G.E;
  if (R == 0) return 0;
  const float* dy = dout;
  const float* ones = ws + G.oZ3 + G.F + G.h2;   // Z3e's constant column (ld ld3)
  if (bn_act) {
    hipLaunchKernelGGL(sg3_bn_bwd_kernel, dim3(nblk(G.R * h3)), dim3(NT), 0, s, G, y, dout,
                       params + po.gamma, params + po.beta, ws);
    SND_LAUNCH_CHECK("sg3_bn_bwd_kernel");
    dy = ws + G.oDY;
    // [dbeta | dgamma] = 1^T [dT | dT y c]
    const int parts = colsum(G, ws, ones, ws + G.oDTY, 2 * h3, s);
    if (parts < 0) return parts;
    ReduceDesc rd[2] = {
        {ws + G.oSLAB, grads + po.beta, parts, h3, 2LL * h3, 1.f, 0, 0, 0, 0},
        {ws + G.oSLAB + h3, grads + po.gamma, parts, h3, 2LL * h3, 1.f, 0, 0, 0, 0}};
    SND_TRY(launch_reduce(rd, 2, s));
  } else {   // no BN in the graph: its gradient is zero (grads are written, not accumulated)
    hipLaunchKernelGGL(sg3_zero_kernel, dim3(nblk(2LL * h3)), dim3(NT), 0, s, grads + po.gamma,
                       2LL * h3);
    SND_LAUNCH_CHECK("sg3_zero_kernel");
  }
  // [dM3; db3] = Z3e^T dy ; dZ3 = dy M3^T
  SND_TRY(wg(G, ws, G.R, G.splitsR, ws + G.oZ3, G.ld3, G.ld3, dy, h3, h3, grads + po.M3, h3, s));
  SND_TRY(mm(dy, h3, A_ROW, params + po.M3, h3, B_COL, R, f + h2, h3, ws + G.oDZ3, f + h2, s));
  hipLaunchKernelGGL(sg3_act_bwd_kernel, dim3(nblk(G.R * h2)), dim3(NT), 0, s, G, ws);
  SND_LAUNCH_CHECK("sg3_act_bwd_kernel");
  // [dM2; db2] = Z2e^T dm2 ; dZ2 = dm2 M2^T
  SND_TRY(wg(G, ws, G.R, G.splitsR, ws + G.oZ2, G.ld2, G.ld2, ws + G.oDM2, h2, h2, grads + po.M2,
             h2, s));
  SND_TRY(mm(ws + G.oDM2, h2, A_ROW, params + po.M2, h2, B_COL, R, 2 * f + 1 + h1, h2,
             ws + G.oDZ2, 2 * f + 1 + h1, s));
  hipLaunchKernelGGL(sg3_edge_bwd_kernel, dim3(nblk(G.R * h1)), dim3(NT), 0, s, *g, G, params, po, ws);
  SND_LAUNCH_CHECK("sg3_edge_bwd_kernel");
  // dM1i = LX^T du, dM1j = LX^T dv, dM1k = (A LX)^T dw
  float* gm1 = grads + po.M1;
  const float* m1s = params + po.M1 + (long long)(3 * f + 3) * h1;
  SND_TRY(wg(G, ws, G.R, G.splitsR, ws + G.oZ3, G.ld3, f, ws + G.oDUVW, 3 * h1, h1, gm1, h1, s));
  SND_TRY(wg(G, ws, G.R, G.splitsR, ws + G.oZ3, G.ld3, f, ws + G.oDUVW + h1, 3 * h1, h1,
             gm1 + (long long)f * h1, h1, s));
  SND_TRY(wg(G, ws, G.R, G.splitsR, ws + G.oZ2 + f, G.ld2, f, ws + G.oDUVW + 2 * h1, 3 * h1, h1,
             gm1 + (long long)2 * f * h1, h1, s));
  // scalar rows: dm1_ij, db1, dm1_jk, dm1_ik = column sums of TM1
  {
    const int parts = colsum(G, ws, ones, ws + G.oTM1, 4 * h1, s);
    if (parts < 0) return parts;
    const long long st = 4LL * h1;
    float* m1row = gm1 + (long long)3 * f * h1;
    ReduceDesc rd[4] = {
        {ws + G.oSLAB, m1row, parts, h1, st, 1.f, 0, 0, 0, 0},
        {ws + G.oSLAB + h1, grads + po.b1, parts, h1, st, 1.f, 0, 0, 0, 0},
        {ws + G.oSLAB + 2 * h1, m1row + h1, parts, h1, st, 1.f, 0, 0, 0, 0},
        {ws + G.oSLAB + 3 * h1, m1row + 2 * h1, parts, h1, st, 1.f, 0, 0, 0, 0}};
    SND_TRY(launch_reduce(rd, 4, s));
  }
  float* gm0 = grads + po.M0;
  if (E > 0) {
    // dM1s = T^T GS (split-K over the edges) ; dT = GS M1s^T
    SND_TRY(wg(G, ws, G.E, G.splitsE, ws + G.oT, h0, h0, ws + G.oGS, h1, h1,
               gm1 + (long long)(3 * f + 3) * h1, h1, s));
    SND_TRY(mm(ws + G.oGS, h1, A_ROW, m1s, h1, B_COL, E, h0, h1, ws + G.oDT, h0, s));
  } else {
    hipLaunchKernelGGL(sg3_zero_kernel, dim3(nblk((long long)h0 * h1)), dim3(NT), 0, s,
                       gm1 + (long long)(3 * f + 3) * h1, (long long)h0 * h1);
    SND_LAUNCH_CHECK("sg3_zero_kernel");
  }
  hipLaunchKernelGGL(sg3_path_bwd_kernel, dim3(nblk(G.R * h0)), dim3(NT), 0, s, *g, rel, G, params,
                     po, ws);
  SND_LAUNCH_CHECK("sg3_path_bwd_kernel");
  // dM0i = LX^T da, dM0j = LX^T db, [dM0k; dM0p] = [d LX | A LX]^T dG
  SND_TRY(wg(G, ws, G.R, G.splitsR, ws + G.oZ3, G.ld3, f, ws + G.oDABG, 3 * h0, h0, gm0, h0, s));
  SND_TRY(wg(G, ws, G.R, G.splitsR, ws + G.oZ3, G.ld3, f, ws + G.oDABG + h0, 3 * h0, h0,
             gm0 + (long long)f * h0, h0, s));
  SND_TRY(wg(G, ws, G.R, G.splitsR, ws + G.oZ2, G.ld2, 2 * f, ws + G.oDABG + 2 * h0, 3 * h0, h0,
             gm0 + (long long)2 * f * h0, h0, s));
  // Matrix0's five scalar rows and bias0 (contiguous in the buffer) = column sums of TM0
  {
    const int parts = colsum(G, ws, ones, ws + G.oTM0, 6 * h0, s);
    if (parts < 0) return parts;
    ReduceDesc rd{ws + G.oSLAB, gm0 + (long long)4 * f * h0, parts, 6 * h0, 6LL * h0, 1.f, 0, 0, 0, 0};
    SND_TRY(launch_reduce(&rd, 1, s));
  }
  if (dx) {
    hipLaunchKernelGGL(sg3_bwd_node_kernel, dim3(nblk(G.R * f)), dim3(NT), 0, s, *g, G, params, po, ws);
    SND_LAUNCH_CHECK("sg3_bwd_node_kernel");
    hipLaunchKernelGGL(sg3_bwd_x_kernel, dim3(nblk(G.R * f)), dim3(NT), 0, s, *g, G, x, ldx, ws, dx,
                       lddx);
    SND_LAUNCH_CHECK("sg3_bwd_x_kernel");
  }
  return 0;
}
