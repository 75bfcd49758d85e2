// Kernels of the factorised e2e structure decoder shared by the forward-only decode
// (snd_e2e_dec.hip) and the training engine (snd_e2e_train.hip).  The maths and the
// kernel list are in snd_e2e_dec.hip's header comment.
#pragma once
#include "snd_common.hpp"

#include <algorithm>

namespace snd {
namespace {

constexpr int DT = 256;            // threads per workgroup
constexpr int DG = 4;              // graphs per workgroup of the factorised layer 0
constexpr int kHeadC = 32;         // head input channels at most (as snd_e2e_head_ce)
constexpr int kLdsFloats = 12288;  // 48 KiB of staging per workgroup: three workgroups per CU
constexpr int kMaxDim = 512;       // n and every cout at most (keeps a 4-channel chunk in LDS)

__host__ __device__ inline int up4(int v) { return (v + 3) & ~3; }

struct HeadArgs {
  const float *g, *be, *w, *b;   // BN_adj gamma / beta [O], d_e_lin2 W [O][2], b [2]
  unsigned char* adj;            // [B, N, N]
  float* margin;                 // [B, N, N] or nullptr
};

// Wsum[n][h][c][o] = sum_{t: 0 <= n+t-pb < N} w[t][h D + c][o], zero in the padding lanes
__global__ void __launch_bounds__(DT) e2e_wsum_kernel(const float* w, int N, int D, int O, float* img) {
  const int D4 = up4(D), O4 = up4(O);
  const long long idx = (long long)blockIdx.x * DT + threadIdx.x;
  if (idx >= (long long)N * 2 * D4 * O4) return;
  const int o = (int)(idx % O4);
  const int c = (int)((idx / O4) % D4);
  const int h = (int)((idx / ((long long)O4 * D4)) % 2);
  const int n = (int)(idx / ((long long)O4 * D4 * 2));
  float s = 0.f;
  if (o < O && c < D) {
    const int pb = (N - 1) / 2;
    const int t0 = max(0, pb - n), t1 = min(N - 1, N - 1 + pb - n);
    for (int t = t0; t <= t1; ++t) s += w[((long long)t * 2 * D + h * D + c) * O + o];
  }
  img[idx] = s;
}

// P[b,n,o] = sum_t sum_c a[b,n+t-pb,c] w[t,c,o];  Q the same over a' and w[t, D + c, o].
// One workgroup per (graph, group of NG nodes): 64 output lanes x 4 slices of the channel
// quads; a / a' of the graph staged in LDS in chunks of CK channels (row N stays zero: the
// taps SAME padding drops); nodes in register tiles of 4, so a weight load serves 4 nodes;
// the 4 slices are summed in index order through LDS.
constexpr int kPqRed = 4 * 4 * 2 * 64;
__global__ void __launch_bounds__(DT) e2e_pq_kernel(const float* z, int ldz, int N, int D, const float* g,
                                                    const float* be, const float* w, int O, int CK, int NG,
                                                    float* P, float* Q) {
  extern __shared__ float lds[];
  float* a = lds;                             // [N + 1][CK]
  float* ap = lds + (size_t)(N + 1) * CK;     // [N + 1][CK]
  float* red = lds + (size_t)2 * (N + 1) * CK;   // [4 slices][4 nodes][P, Q][64 lanes]
  const int b = blockIdx.x, n_lo = blockIdx.y * NG, n_hi = min(N, n_lo + NG), pb = (N - 1) / 2;
  const int lane = threadIdx.x & 63, ks = threadIdx.x >> 6, D4 = up4(D);
  const float* zb = z + (long long)b * N * ldz;
  for (int c0 = 0; c0 < D4; c0 += CK) {
    const int ck = min(CK, D4 - c0);          // a multiple of 4
    __syncthreads();
    for (int e = threadIdx.x; e < (N + 1) * ck; e += DT) {
      const int n = e / ck, cc = e - n * ck, c = c0 + cc;
      float va = 0.f, vp = 0.f;
      if (n < N && c < D) {
        const float v = zb[(long long)n * ldz + c];
        va = fmaxf(g[c] * kBnC * v + be[c], 0.f);
        vp = fmaxf(g[D + c] * kBnC * v + be[D + c], 0.f);
      }
      a[n * CK + cc] = va;
      ap[n * CK + cc] = vp;
    }
    __syncthreads();
    for (int o0 = 0; o0 < O; o0 += 64) {
      const int o = o0 + lane, oc = min(o, O - 1);
      for (int n0 = n_lo; n0 < n_hi; n0 += 4) {
        float p[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < N; ++t) {
          int row[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int m = n0 + k + t - pb;
            row[k] = (n0 + k < n_hi && m >= 0 && m < N) ? m : N;
          }
          const float* wl = w + ((long long)t * 2 * D + c0) * O + oc;
          const float* wr = wl + (long long)D * O;
          for (int cq = ks * 4; cq < ck; cq += 16) {
            float wlv[4], wrv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const bool cv = c0 + cq + r < D;
              wlv[r] = cv ? wl[(long long)(cq + r) * O] : 0.f;
              wrv[r] = cv ? wr[(long long)(cq + r) * O] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const f32x4 av = *(const f32x4*)(a + row[k] * CK + cq);
              const f32x4 pv = *(const f32x4*)(ap + row[k] * CK + cq);
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                p[k] = fmaf(av[r], wlv[r], p[k]);
                q[k] = fmaf(pv[r], wrv[r], q[k]);
              }
            }
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          red[((ks * 4 + k) * 2 + 0) * 64 + lane] = p[k];
          red[((ks * 4 + k) * 2 + 1) * 64 + lane] = q[k];
        }
        __syncthreads();
        if (ks == 0 && o < O) {
          for (int k = 0; k < 4 && n0 + k < n_hi; ++k) {
            float sp = 0.f, sq = 0.f;
            for (int sl = 0; sl < 4; ++sl) {
              sp += red[((sl * 4 + k) * 2 + 0) * 64 + lane];
              sq += red[((sl * 4 + k) * 2 + 1) * 64 + lane];
            }
            const long long at = ((long long)b * N + n0 + k) * O + o;
            P[at] = c0 ? P[at] + sp : sp;
            Q[at] = c0 ? Q[at] + sq : sq;
          }
        }
        __syncthreads();
      }
    }
  }
}

// Head of one output row (b, i) for the jn rows j0 .. j0+jn-1 of this pass: every thread
// holds yv[tj][q] = y[b, i, jbase + tj, 4 oq + q]; partial logits go through LDS and are
// summed over oq in index order by one thread per j.
template <int TJ>
__device__ __forceinline__ void head_rows(const HeadArgs& h, float (&yv)[TJ][4], bool active, int jloc, int oq,
                                          int nOq, int O, int N, int b, int i, int jpass0, int jpassn,
                                          float* part) {
  __syncthreads();   // the staging buffers are free
  if (active) {
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj) {
      float p0 = 0.f, p1 = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int o = oq * 4 + q;
        if (o < O) {
          const float x = fmaxf(h.g[o] * kBnC * yv[tj][q] + h.be[o], 0.f);
          p0 = fmaf(x, h.w[2 * o], p0);
          p1 = fmaf(x, h.w[2 * o + 1], p1);
        }
      }
      part[((jloc + tj) * nOq + oq) * 2] = p0;
      part[((jloc + tj) * nOq + oq) * 2 + 1] = p1;
    }
  }
  __syncthreads();
  for (int jl = threadIdx.x; jl < jpassn; jl += DT) {
    const int j = jpass0 + jl;
    float l0 = h.b[0], l1 = h.b[1];
    for (int k = 0; k < nOq; ++k) {
      l0 += part[(jl * nOq + k) * 2];
      l1 += part[(jl * nOq + k) * 2 + 1];
    }
    if (i == j) { l0 = 1.f; l1 = 0.f; }
    const long long at = ((long long)b * N + i) * N + j;
    h.adj[at] = l1 > l0 ? 1 : 0;
    if (h.margin) h.margin[at] = l1 - l0;
  }
  __syncthreads();
}

struct L0Args {
  const float* z;
  int ldz, B, N, D, O, CK;
  const float *g, *be, *bias;   // BN0 gamma / beta [2D], e2e bias [O]
  const float *img, *P, *Q;     // Wsum image, P / Q [B, N, O]
  float* y;                     // [B, N, N, O] (not LAST)
  HeadArgs h;                   // (LAST)
};

template <bool LAST>
__global__ void __launch_bounds__(DT) e2e_l0_kernel(L0Args A) {
  extern __shared__ float lds[];
  const int N = A.N, D = A.D, O = A.O, CK = A.CK;
  const int D4 = up4(D), O4 = up4(O), nOq = O4 / 4;
  const int i = blockIdx.x, b0 = blockIdx.y * DG;
  float* sa = lds;                         // [DG][CK]     a_i of the DG graphs
  float* sap = lds + DG * CK;              // [DG][N][CK]  a'_j
  const int JTP = DT / nOq;                // j rows per pass
  const int oq = threadIdx.x % nOq, jl = threadIdx.x / nOq;
  for (int jp0 = 0; jp0 < N; jp0 += JTP) {
    const int jpn = min(JTP, N - jp0);
    const bool active = jl < jpn;
    const int j = min(jp0 + jl, N - 1);
    float acc[DG][4];
#pragma unroll
    for (int gI = 0; gI < DG; ++gI)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[gI][q] = 0.f;
    for (int c0 = 0; c0 < D4; c0 += CK) {
      const int ck = min(CK, D4 - c0);     // multiple of 4
      __syncthreads();
      for (int e = threadIdx.x; e < DG * (N + 1) * ck; e += DT) {
        const int cc = e % ck, r = e / ck, n = r % (N + 1), gI = r / (N + 1);
        const int c = c0 + cc, b = min(b0 + gI, A.B - 1);
        float v = 0.f;
        if (c < D) {
          const int node = n < N ? n : i, ch = n < N ? D + c : c;
          v = fmaxf(A.g[ch] * kBnC * A.z[((long long)b * N + node) * A.ldz + c] + A.be[ch], 0.f);
        }
        if (n < N) sap[(gI * N + n) * CK + cc] = v;
        else sa[gI * CK + cc] = v;
      }
      __syncthreads();
      if (active) {
        const float* wl = A.img + (((long long)j * 2 + 0) * D4 + c0) * O4 + oq * 4;
        const float* wr = A.img + (((long long)i * 2 + 1) * D4 + c0) * O4 + oq * 4;
        for (int cc = 0; cc < ck; cc += 4) {
          f32x4 l[4], r[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            l[q] = *(const f32x4*)(wl + (long long)(cc + q) * O4);
            r[q] = *(const f32x4*)(wr + (long long)(cc + q) * O4);
          }
#pragma unroll
          for (int gI = 0; gI < DG; ++gI) {
            const f32x4 av = *(const f32x4*)(sa + gI * CK + cc);
            const f32x4 pv = *(const f32x4*)(sap + (gI * N + j) * CK + cc);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                acc[gI][k] = fmaf(av[q], l[q][k], acc[gI][k]);
                acc[gI][k] = fmaf(pv[q], r[q][k], acc[gI][k]);
              }
          }
        }
      }
    }
#pragma unroll
    for (int gI = 0; gI < DG; ++gI) {
      const int b = b0 + gI;
      if (b >= A.B) break;   // uniform over the workgroup
      float yv[1][4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int o = min(oq * 4 + q, O - 1);
        yv[0][q] = acc[gI][q] + A.P[((long long)b * N + i) * O + o] + A.Q[((long long)b * N + j) * O + o] +
                   2.f * A.bias[o];
      }
      if (LAST) {
        head_rows<1>(A.h, yv, active, jl, oq, nOq, O, N, b, i, jp0, jpn, lds);
      } else if (active) {
        float* out = A.y + (((long long)b * N + i) * N + j) * O;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (oq * 4 + q < O) out[oq * 4 + q] = yv[0][q];
      }
    }
  }
}

struct LayerArgs {
  const float* x;               // [B, N, N, C]: the previous layer's y
  int N, C, O, CK;
  const float *g, *be;          // BN over the C input channels (relu after it)
  const float *w, *bias;        // [N, C, O], [O]
  float* y;                     // [B, N, N, O] (not LAST)
  HeadArgs h;                   // (LAST)
};

template <int TJ, bool LAST>
__global__ void __launch_bounds__(DT) e2e_layer_kernel(LayerArgs A) {
  extern __shared__ float lds[];
  const int N = A.N, C = A.C, O = A.O, CK = A.CK;
  const int O4 = up4(O), nOq = O4 / 4, pb = (N - 1) / 2;
  const int b = blockIdx.x / N, i = blockIdx.x - b * N;
  float* xr = lds;                          // [N][CK]  relu(BN(x[b, i, :, chunk]))
  float* V = lds + (size_t)N * CK;          // [N][CK]  the tap's summed input
  float* ws = lds + (size_t)2 * N * CK;     // [CK][O4] the tap's weights
  float* gs = ws + (size_t)CK * O4;         // [CK] BN scale gamma c of the chunk's channels
  float* bs = gs + CK;                      // [CK] BN shift beta
  const float* xb = A.x + (long long)b * N * N * C;
  const int JTP = DT / nOq;                 // (TJ-row) tiles per pass
  const int oq = threadIdx.x % nOq, jt = threadIdx.x / nOq;
  for (int jp0 = 0; jp0 < N; jp0 += JTP * TJ) {
    const int jpn = min(JTP * TJ, N - jp0);
    const bool active = jt * TJ < jpn;
    int jr[TJ];
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj) jr[tj] = min(jp0 + jt * TJ + tj, N - 1);
    float acc[TJ][4];
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[tj][q] = 0.f;
    for (int c0 = 0; c0 < C; c0 += CK) {
      const int ck = min(CK, C - c0), ck4 = up4(ck), cq4 = ck4 / 4;
      __syncthreads();
      for (int cc = threadIdx.x; cc < ck4; cc += DT) {   // zero past ck: relu(0 x + 0) = 0
        gs[cc] = cc < ck ? A.g[c0 + cc] * kBnC : 0.f;
        bs[cc] = cc < ck ? A.be[c0 + cc] : 0.f;
      }
      __syncthreads();
      // staging walks float4 quads (one division per quad); x and w rows are only 4-byte
      // aligned in general (C, O odd; offset pointers), so their loads stay scalar
      for (int q = threadIdx.x; q < N * cq4; q += DT) {
        const int jj = q / cq4, cc = (q - jj * cq4) * 4;
        const float* src = xb + ((long long)i * N + jj) * C + c0 + cc;
        const f32x4 gv = *(const f32x4*)(gs + cc), bv = *(const f32x4*)(bs + cc);
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = cc + r < ck ? fmaxf(fmaf(gv[r], src[r], bv[r]), 0.f) : 0.f;
        *(f32x4*)(xr + jj * CK + cc) = v;
      }
      for (int t = 0; t < N; ++t) {
        const int ii = i + t - pb;
        const bool vi = ii >= 0 && ii < N;
        __syncthreads();   // xr is complete; the previous tap's V and ws have been read
        for (int q = threadIdx.x; q < N * cq4; q += DT) {
          const int j = q / cq4, cc = (q - j * cq4) * 4, jj = j + t - pb;
          f32x4 v = {0.f, 0.f, 0.f, 0.f};
          if (jj >= 0 && jj < N) v = *(const f32x4*)(xr + jj * CK + cc);
          if (vi) {
            const float* src = xb + ((long long)ii * N + j) * C + c0 + cc;
            const f32x4 gv = *(const f32x4*)(gs + cc), bv = *(const f32x4*)(bs + cc);
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (cc + r < ck) v[r] += fmaxf(fmaf(gv[r], src[r], bv[r]), 0.f);
          }
          *(f32x4*)(V + j * CK + cc) = v;
        }
        for (int q = threadIdx.x; q < ck4 * nOq; q += DT) {
          const int cc = q / nOq, o4 = (q - cc * nOq) * 4;
          f32x4 v = {0.f, 0.f, 0.f, 0.f};
          if (cc < ck) {
            const float* src = A.w + ((long long)t * C + c0 + cc) * O + o4;
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (o4 + r < O) v[r] = src[r];
          }
          *(f32x4*)(ws + cc * O4 + o4) = v;
        }
        __syncthreads();
        if (active) {
          for (int cc = 0; cc < ck4; cc += 4) {
            f32x4 wv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) wv[q] = *(const f32x4*)(ws + (cc + q) * O4 + oq * 4);
#pragma unroll
            for (int tj = 0; tj < TJ; ++tj) {
              const f32x4 v = *(const f32x4*)(V + jr[tj] * CK + cc);
#pragma unroll
              for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[tj][k] = fmaf(v[q], wv[q][k], acc[tj][k]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[tj][q] += 2.f * A.bias[min(oq * 4 + q, O - 1)];
    if (LAST) {
      head_rows<TJ>(A.h, acc, active, jt * TJ, oq, nOq, O, N, b, i, jp0, jpn, lds);
    } else if (active) {
#pragma unroll
      for (int tj = 0; tj < TJ; ++tj) {
        const int j = jp0 + jt * TJ + tj;
        if (j < N) {
          float* out = A.y + (((long long)b * N + i) * N + j) * O;
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (oq * 4 + q < O) out[oq * 4 + q] = acc[tj][q];
        }
      }
    }
  }
}

// channel chunk of a staging buffer with `per` floats per channel: the whole (padded)
// width when it fits, else the largest multiple of 4 that does
inline int chunk_of(int width4, long long per, int budget = kLdsFloats) {
  const long long fit = (budget / per) & ~3LL;
  return (int)std::min<long long>(width4, fit);
}

// Rows per register tile: the smallest whose (ceil(N / TJ) x ceil(O / 4)) tiles fit one pass
// of a workgroup.  The taps' staging wants the threads more than the FMAs want a wider tile
// (DESIGN.md section 7 has the measurements).
template <bool LAST>
void launch_layer(const LayerArgs& a, int B, hipStream_t st) {
  const int nOq = up4(a.O) / 4, jtp = DT / nOq;
  const size_t lds = sizeof(float) * std::max<size_t>((size_t)(2 * a.N + up4(a.O) + 2) * a.CK, 2 * DT * 4);
  const dim3 grid((unsigned)((long long)B * a.N));
  if (a.N <= jtp) hipLaunchKernelGGL((e2e_layer_kernel<1, LAST>), grid, dim3(DT), lds, st, a);
  else if (a.N <= 2 * jtp) hipLaunchKernelGGL((e2e_layer_kernel<2, LAST>), grid, dim3(DT), lds, st, a);
  else hipLaunchKernelGGL((e2e_layer_kernel<4, LAST>), grid, dim3(DT), lds, st, a);
}

}  // namespace
}  // namespace snd
