// Factorised training engine of the e2e structure decoder (ABI 24): forward, CE and every
// gradient of model.py:193-208 from z [B, N, D], without the pair tensor x0 [B, N, N, 2D]
// or its gradient.  The maths is in include/snd_vae.h; the forward kernels are
// snd_e2e_decode's (snd_e2e_dec.hpp), every layer's y kept in the workspace.
//
// Backward of a general layer (C -> O), g = dy_l, x = relu(BN_l(y_{l-1})) recomputed on load:
//   e2e_bias_grad_kernel  db[o] = 2 sum g: one workgroup per channel, fixed-order tree
//   e2e_wgrad_kernel      dw[t] = sum_{b,i,j} V_t[b,i,j,:]^T g[b,i,j,:]: one workgroup per
//                         (tap, group of graphs, 256 (c, 4 o) register tiles); rows of V_t and
//                         of g staged in LDS; one slab per group of graphs
//   e2e_slab_sum_kernel   the slabs summed in index order
//   e2e_dgrad_kernel      dx = the forward layer kernel with the taps mirrored and w read
//                         transposed (no BN on load)
//   snd_bn_relu_bwd       dx -> dy_{l-1} in place, dgamma_l, dbeta_l (the existing kernel)
// Backward of layer 0 through the factorisation, g = dy_0:
//   e2e_rs_kernel         R[b,i,:] = sum_j g, S[b,j,:] = sum_i g
//   e2e_dwsum_kernel      dWsum_n [2D, O]
//   e2e_dw0_kernel        dw_0 from dWsum and the per-node conv terms (a, R), (a', S)
//   e2e_da_kernel         da, da' [B, N, D]
//   e2e_dz_kernel         the relu masks and dz
//   e2e_bn0_grad_kernel   dgamma_0, dbeta_0: one workgroup per channel, fixed-order tree
// fp32 FMA, every sum in a fixed order, no atomics; nothing synchronises with or allocates
// on the host.
#include "snd_e2e_dec.hpp"

namespace snd {
namespace {

constexpr int kMaxParts = 32;   // weight-gradient slabs at most

// out[o] = scale * sum over rows of g[row, o]
__global__ void __launch_bounds__(DT) e2e_bias_grad_kernel(const float* g, long long rows, int O, float scale,
                                                           float* out) {
  __shared__ float red[DT];
  const int o = blockIdx.x;
  float s = 0.f;
  for (long long r = threadIdx.x; r < rows; r += DT) s += g[r * O + o];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = DT / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[o] = scale * red[0];
}

struct WgArgs {
  const float* y;        // [B, N, N, C]: the previous layer's y
  const float* g;        // [B, N, N, O]: dy of this layer
  int B, N, C, O, JK, CR, GP;
  const float *bg, *bb;  // BN over the C input channels
  float* slab;           // [parts][N, C, O]
};

__global__ void __launch_bounds__(DT) e2e_wgrad_kernel(WgArgs A) {
  extern __shared__ float lds[];
  const int N = A.N, C = A.C, O = A.O, JK = A.JK, CR = A.CR;
  const int O4 = up4(O), nOq = O4 / 4, pb = (N - 1) / 2;
  const int t = blockIdx.x, part = blockIdx.y;
  const int tile0 = blockIdx.z * DT, tile = tile0 + threadIdx.x;
  const bool valid = tile < C * nOq;
  const int c = valid ? tile / nOq : 0, oq = valid ? tile - c * nOq : 0;
  const int c_lo = tile0 / nOq, c_hi = min(C - 1, (tile0 + DT - 1) / nOq), cr = c_hi - c_lo + 1;
  float* gs = lds;                        // [JK][O4]
  float* V = lds + (size_t)JK * O4;       // [JK][CR]
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const int b_hi = min(A.B, (part + 1) * A.GP);
  for (int b = part * A.GP; b < b_hi; ++b) {
    const float* yb = A.y + (long long)b * N * N * C;
    const float* gb = A.g + (long long)b * N * N * O;
    for (int i = 0; i < N; ++i) {
      const int ii = i + t - pb;
      const bool vi = ii >= 0 && ii < N;
      for (int j0 = 0; j0 < N; j0 += JK) {
        const int jn = min(JK, N - j0);
        __syncthreads();
        for (int e = threadIdx.x; e < jn * O4; e += DT) {
          const int jl = e / O4, o = e - jl * O4;
          gs[e] = o < O ? gb[((long long)i * N + j0 + jl) * O + o] : 0.f;
        }
        for (int e = threadIdx.x; e < jn * cr; e += DT) {
          const int jl = e / cr, cc = e - jl * cr, ch = c_lo + cc, j = j0 + jl, jj = j + t - pb;
          const float sc = A.bg[ch] * kBnC, sh = A.bb[ch];
          float v = 0.f;
          if (jj >= 0 && jj < N) v = fmaxf(fmaf(sc, yb[((long long)i * N + jj) * C + ch], sh), 0.f);
          if (vi) v += fmaxf(fmaf(sc, yb[((long long)ii * N + j) * C + ch], sh), 0.f);
          V[jl * CR + cc] = v;
        }
        __syncthreads();
        if (valid) {
          for (int jl = 0; jl < jn; ++jl) {
            const float v = V[jl * CR + c - c_lo];
            const f32x4 gv = *(const f32x4*)(gs + jl * O4 + oq * 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = fmaf(v, gv[q], acc[q]);
          }
        }
      }
    }
  }
  if (valid) {
    float* out = A.slab + ((long long)part * N * C + (long long)t * C + c) * O;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (oq * 4 + q < O) out[oq * 4 + q] = acc[q];
  }
}

__global__ void __launch_bounds__(DT) e2e_slab_sum_kernel(const float* slab, long long count, int parts,
                                                          float* out) {
  const long long idx = (long long)blockIdx.x * DT + threadIdx.x;
  if (idx >= count) return;
  float s = slab[idx];
  for (int p = 1; p < parts; ++p) s += slab[(long long)p * count + idx];
  out[idx] = s;
}

struct DgArgs {
  const float* g;   // [B, N, N, Ci]: dy of the layer (Ci = its cout)
  int N, Ci, Co, CK;
  const float* w;   // [N, Co, Ci]: the layer's w [t, c, o], read transposed
  float* dx;        // [B, N, N, Co]
};

// dx[b,i,j,c] = sum_t sum_o w[t,c,o] (g[b,i,j-t+pb,o] + g[b,i-t+pb,j,o]): e2e_layer_kernel's
// structure, one workgroup per row (b, i), the two inputs added before the shared taps
template <int TJ>
__global__ void __launch_bounds__(DT) e2e_dgrad_kernel(DgArgs A) {
  extern __shared__ float lds[];
  const int N = A.N, Ci = A.Ci, Co = A.Co, CK = A.CK;
  const int Co4 = up4(Co), nCq = Co4 / 4, pb = (N - 1) / 2;
  const int b = blockIdx.x / N, i = blockIdx.x - b * N;
  float* xr = lds;                          // [N][CK]  g[b, i, :, chunk]
  float* V = lds + (size_t)N * CK;          // [N][CK]  the tap's summed input
  float* ws = lds + (size_t)2 * N * CK;     // [CK][Co4] the tap's weights, transposed
  const float* gb = A.g + (long long)b * N * N * Ci;
  const int JTP = DT / nCq;
  const int cq = threadIdx.x % nCq, jt = threadIdx.x / nCq;
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
    for (int c0 = 0; c0 < Ci; c0 += CK) {
      const int ck = min(CK, Ci - c0), ck4 = up4(ck), cq4 = ck4 / 4;
      __syncthreads();
      for (int q = threadIdx.x; q < N * cq4; q += DT) {
        const int jj = q / cq4, cc = (q - jj * cq4) * 4;
        const float* src = gb + ((long long)i * N + jj) * Ci + c0 + cc;
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = cc + r < ck ? src[r] : 0.f;
        *(f32x4*)(xr + jj * CK + cc) = v;
      }
      for (int t = 0; t < N; ++t) {
        const int ii = i - t + pb;
        const bool vi = ii >= 0 && ii < N;
        __syncthreads();   // xr is complete; the previous tap's V and ws have been read
        for (int q = threadIdx.x; q < N * cq4; q += DT) {
          const int j = q / cq4, cc = (q - j * cq4) * 4, jj = j - t + pb;
          f32x4 v = {0.f, 0.f, 0.f, 0.f};
          if (jj >= 0 && jj < N) v = *(const f32x4*)(xr + jj * CK + cc);
          if (vi) {
            const float* src = gb + ((long long)ii * N + j) * Ci + c0 + cc;
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (cc + r < ck) v[r] += src[r];
          }
          *(f32x4*)(V + j * CK + cc) = v;
        }
        for (int q = threadIdx.x; q < ck4 * nCq; q += DT) {
          const int cc = q / nCq, c4 = (q - cc * nCq) * 4;
          f32x4 v = {0.f, 0.f, 0.f, 0.f};
          if (cc < ck) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (c4 + r < Co) v[r] = A.w[((long long)t * Co + c4 + r) * Ci + c0 + cc];
          }
          *(f32x4*)(ws + cc * Co4 + c4) = v;
        }
        __syncthreads();
        if (active) {
          for (int cc = 0; cc < ck4; cc += 4) {
            f32x4 wv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) wv[q] = *(const f32x4*)(ws + (cc + q) * Co4 + cq * 4);
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
    if (active) {
#pragma unroll
      for (int tj = 0; tj < TJ; ++tj) {
        const int j = jp0 + jt * TJ + tj;
        if (j < N) {
          float* out = A.dx + (((long long)b * N + i) * N + j) * Co;
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (cq * 4 + q < Co) out[cq * 4 + q] = acc[tj][q];
        }
      }
    }
  }
}

void launch_dgrad(const DgArgs& a, int B, hipStream_t st) {
  const int nCq = up4(a.Co) / 4, jtp = DT / nCq;
  const size_t lds = sizeof(float) * (size_t)(2 * a.N + up4(a.Co)) * a.CK;
  const dim3 grid((unsigned)((long long)B * a.N));
  if (a.N <= jtp) hipLaunchKernelGGL(e2e_dgrad_kernel<1>, grid, dim3(DT), lds, st, a);
  else if (a.N <= 2 * jtp) hipLaunchKernelGGL(e2e_dgrad_kernel<2>, grid, dim3(DT), lds, st, a);
  else hipLaunchKernelGGL(e2e_dgrad_kernel<4>, grid, dim3(DT), lds, st, a);
}

// ---- layer 0 ---------------------------------------------------------------------------
struct Z0 {
  const float* z;
  int ldz, B, N, D, O;
  const float *g0, *b0;   // BN0 gamma / beta [2D]
};

// a (h = 0) or a' (h = 1) of node (b, n), channel c
__device__ __forceinline__ float act0(const Z0& Z, int b, int n, int h, int c) {
  const int ch = h * Z.D + c;
  return fmaxf(fmaf(Z.g0[ch] * kBnC, Z.z[((long long)b * Z.N + n) * Z.ldz + c], Z.b0[ch]), 0.f);
}

__global__ void __launch_bounds__(DT) e2e_rs_kernel(const float* g, int B, int N, int O, float* R, float* S) {
  const long long idx = (long long)blockIdx.x * DT + threadIdx.x;
  if (idx >= (long long)B * N * O) return;
  const int o = (int)(idx % O), n = (int)((idx / O) % N);
  const long long b = idx / ((long long)O * N);
  const float* gb = g + b * N * N * O + o;
  float r = 0.f, s = 0.f;
  for (int m = 0; m < N; ++m) {
    r += gb[((long long)n * N + m) * O];
    s += gb[((long long)m * N + n) * O];
  }
  R[idx] = r;
  S[idx] = s;
}

// dWsum[n][h D + c][o] = sum_{b,m} a[b,m,c] g[b,m,n,o]  (h = 0),  a'[b,m,c] g[b,n,m,o]  (h = 1)
__global__ void __launch_bounds__(DT) e2e_dwsum_kernel(Z0 Z, const float* g, float* dws) {
  const int N = Z.N, D = Z.D, O = Z.O;
  const long long idx = (long long)blockIdx.x * DT + threadIdx.x;
  if (idx >= (long long)N * 2 * D * O) return;
  const int o = (int)(idx % O), ch = (int)((idx / O) % (2 * D)), n = (int)(idx / ((long long)O * 2 * D));
  const int h = ch >= D, c = ch - h * D;
  float s = 0.f;
  for (int b = 0; b < Z.B; ++b) {
    const float* gb = g + (long long)b * N * N * O + o;
    for (int m = 0; m < N; ++m) {
      const float gv = h ? gb[((long long)n * N + m) * O] : gb[((long long)m * N + n) * O];
      s = fmaf(act0(Z, b, m, h, c), gv, s);
    }
  }
  dws[idx] = s;
}

// dw0[t][h D + c][o] = sum_{n kept by tap t} dWsum_n + sum_{b,i} a / a' [b, i+t-pb, c] R / S [b, i, o]
__global__ void __launch_bounds__(DT) e2e_dw0_kernel(Z0 Z, const float* dws, const float* R, const float* S,
                                                     float* dw) {
  const int N = Z.N, D = Z.D, O = Z.O, pb = (N - 1) / 2;
  const long long idx = (long long)blockIdx.x * DT + threadIdx.x;
  if (idx >= (long long)N * 2 * D * O) return;
  const int o = (int)(idx % O), ch = (int)((idx / O) % (2 * D)), t = (int)(idx / ((long long)O * 2 * D));
  const int h = ch >= D, c = ch - h * D;
  const int n0 = max(0, pb - t), n1 = min(N - 1, N - 1 + pb - t);
  float s = 0.f;
  for (int n = n0; n <= n1; ++n) s += dws[((long long)n * 2 * D + ch) * O + o];
  const float* T = h ? S : R;
  for (int b = 0; b < Z.B; ++b)
    for (int i = n0; i <= n1; ++i) s = fmaf(act0(Z, b, i + t - pb, h, c), T[((long long)b * N + i) * O + o], s);
  dw[idx] = s;
}

// da[b,n,c]  = sum_j sum_o g[b,n,j,o] Wsum_j[c,o]     + sum_t sum_o R[b,n-t+pb,o] w[t,c,o]
// da'[b,n,c] = sum_i sum_o g[b,i,n,o] Wsum_i[D+c,o]   + sum_t sum_o S[b,n-t+pb,o] w[t,D+c,o]
// into DA [B, N, 2D] (da | da')
__global__ void __launch_bounds__(DT) e2e_da_kernel(Z0 Z, const float* g, const float* img, const float* w,
                                                    const float* R, const float* S, float* DA) {
  const int N = Z.N, D = Z.D, O = Z.O, pb = (N - 1) / 2, D4 = up4(D), O4 = up4(O);
  const long long idx = (long long)blockIdx.x * DT + threadIdx.x;
  if (idx >= (long long)Z.B * N * 2 * D) return;
  const int ch = (int)(idx % (2 * D)), n = (int)((idx / (2 * D)) % N);
  const long long b = idx / ((long long)2 * D * N);
  const int h = ch >= D, c = ch - h * D;
  const float* gb = g + b * N * N * O;
  float s = 0.f;
  for (int m = 0; m < N; ++m) {
    const float* gr = gb + (h ? (long long)m * N + n : (long long)n * N + m) * O;
    const float* wr = img + (((long long)m * 2 + h) * D4 + c) * O4;
    for (int o = 0; o < O; ++o) s = fmaf(gr[o], wr[o], s);
  }
  const float* T = (h ? S : R) + b * N * O;
  for (int t = 0; t < N; ++t) {
    const int m = n - t + pb;
    if (m < 0 || m >= N) continue;
    const float* tr = T + (long long)m * O;
    const float* wr = w + ((long long)t * 2 * D + ch) * O;
    for (int o = 0; o < O; ++o) s = fmaf(tr[o], wr[o], s);
  }
  DA[idx] = s;
}

// masks DA in place (da 1[a > 0] | da' 1[a' > 0]) and writes dz
__global__ void __launch_bounds__(DT) e2e_dz_kernel(Z0 Z, float* DA, float* dz, int lddz) {
  const int D = Z.D;
  const long long idx = (long long)blockIdx.x * DT + threadIdx.x;
  if (idx >= (long long)Z.B * Z.N * D) return;
  const int c = (int)(idx % D);
  const long long r = idx / D;
  const float zv = Z.z[r * Z.ldz + c];
  const float ga = Z.g0[c] * kBnC, gp = Z.g0[D + c] * kBnC;
  const float ta = fmaf(ga, zv, Z.b0[c]), tp = fmaf(gp, zv, Z.b0[D + c]);
  const float da = ta > 0.f ? DA[r * 2 * D + c] : 0.f, dp = tp > 0.f ? DA[r * 2 * D + D + c] : 0.f;
  DA[r * 2 * D + c] = da;
  DA[r * 2 * D + D + c] = dp;
  dz[r * lddz + c] = ga * da + gp * dp;
}

// dgamma0[ch] = sum_{b,n} dt c z, dbeta0[ch] = sum dt: one workgroup per channel
__global__ void __launch_bounds__(DT) e2e_bn0_grad_kernel(Z0 Z, const float* DA, float* dg, float* db) {
  __shared__ float r1[DT], r2[DT];
  const int D = Z.D, ch = blockIdx.x, c = ch >= D ? ch - D : ch;
  const long long rows = (long long)Z.B * Z.N;
  float sg = 0.f, sb = 0.f;
  for (long long r = threadIdx.x; r < rows; r += DT) {
    const float dt = DA[r * 2 * D + ch];
    sg = fmaf(dt, kBnC * Z.z[r * Z.ldz + c], sg);
    sb += dt;
  }
  r1[threadIdx.x] = sg;
  r2[threadIdx.x] = sb;
  __syncthreads();
  for (int h = DT / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) { r1[threadIdx.x] += r1[threadIdx.x + h]; r2[threadIdx.x] += r2[threadIdx.x + h]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { dg[ch] = r1[0]; db[ch] = r2[0]; }
}

inline int wg_parts(int B, int* gp) {
  *gp = (B + kMaxParts - 1) / kMaxParts;
  return (B + *gp - 1) / *gp;
}

struct TrainLayout {
  size_t y[16], g[2], img, P, Q, R, S, dws, da, slab, total;   // float offsets; total in bytes
};

inline TrainLayout train_layout(int B, int n, int d, const int* couts, int L) {
  TrainLayout s{};
  size_t at = 0;
  auto take = [&](long long floats) {
    const size_t o = at;
    at += (size_t)round_up(floats, 4);
    return o;
  };
  int widest = 0, gp;
  const long long pairs = (long long)B * n * n;
  for (int l = 0; l < L; ++l) {
    s.y[l] = take(pairs * couts[l]);
    widest = std::max(widest, couts[l]);
  }
  s.g[0] = take(pairs * widest);
  s.g[1] = take(L >= 2 ? pairs * widest : 0);
  s.img = take((long long)n * 2 * up4(d) * up4(couts[0]));
  const long long node = (long long)B * n * couts[0];
  s.P = take(node);
  s.Q = take(node);
  s.R = take(node);
  s.S = take(node);
  s.dws = take((long long)n * 2 * d * couts[0]);
  s.da = take((long long)B * n * 2 * d);
  long long slab = 0;
  const int parts = wg_parts(B, &gp);
  for (int l = 1; l < L; ++l) slab = std::max(slab, (long long)parts * n * couts[l - 1] * couts[l]);
  s.slab = take(slab);
  s.total = at * sizeof(float) + 16;
  return s;
}

// every launch of layer 0 whose grid grows with d fits a grid (d itself is not bounded otherwise)
inline bool d_fits(int n_graphs, int n, int d, int cout0) {
  if (d > (1 << 24)) return false;
  const long long threads = std::max((long long)n * 2 * up4(d) * up4(cout0), (long long)n_graphs * n * 2 * d);
  return threads <= 0x7fffffffLL * DT;
}

bool train_shape_ok(int n_graphs, int n, int d, const int* couts, int n_layers) {
  if (n_graphs < 1 || n_graphs > 262140 || n < 1 || n > kMaxDim || d < 1 || n_layers < 1 || n_layers > 16 || !couts)
    return false;
  for (int l = 0; l < n_layers; ++l)
    if (couts[l] < 1 || couts[l] > kMaxDim) return false;
  return couts[n_layers - 1] <= kHeadC && d_fits(n_graphs, n, d, couts[0]);
}

}  // namespace
}  // namespace snd

using namespace snd;

extern "C" size_t snd_e2e_train_workspace(int n_graphs, int n, int d, const int* couts, int n_layers) {
  if (!train_shape_ok(n_graphs, n, d, couts, n_layers)) return 0;
  return train_layout(n_graphs, n, d, couts, n_layers).total;
}

extern "C" int snd_e2e_train(const float* z, int ldz, const float* adj, int n_graphs, int n, int d,
                             const snd_e2e_layer_t* layers, int n_layers, const float* head_gamma,
                             const float* head_beta, const float* head_w, const float* head_b, float* dz, int lddz,
                             const snd_e2e_layer_grad_t* layer_grads, float* d_head_gamma, float* d_head_beta,
                             float* d_head_w, float* d_head_b, double* out, void* workspace, size_t workspace_bytes,
                             snd_stream_t stream) {
  SND_CHECK_ARG(n_layers >= 1, "snd_e2e_train: n_layers %d < 1", n_layers);
  SND_CHECK_ARG(n_layers <= 16, "snd_e2e_train: n_layers %d > 16", n_layers);
  SND_CHECK_ARG(z && adj && layers && head_gamma && head_beta && head_w && head_b && dz && layer_grads &&
                    d_head_gamma && d_head_beta && d_head_w && d_head_b && out && workspace,
                "snd_e2e_train: null operand");
  SND_CHECK_ARG(n_graphs >= 1 && n >= 1 && d >= 1, "snd_e2e_train: empty shape (n_graphs %d, n %d, d %d)", n_graphs,
                n, d);
  int couts[16];
  for (int l = 0; l < n_layers; ++l) {
    SND_CHECK_ARG(layers[l].gamma && layers[l].beta && layers[l].w && layers[l].b && layer_grads[l].dgamma &&
                      layer_grads[l].dbeta && layer_grads[l].dw && layer_grads[l].db,
                  "snd_e2e_train: null operand in layer %d", l);
    SND_CHECK_ARG(layers[l].cout >= 1, "snd_e2e_train: layer %d has width %d < 1", l, layers[l].cout);
    SND_CHECK_ARG(layers[l].cout <= kMaxDim, "snd_e2e_train: layer %d has width %d > %d", l, layers[l].cout, kMaxDim);
    couts[l] = layers[l].cout;
  }
  SND_CHECK_ARG(n <= kMaxDim, "snd_e2e_train: n %d > %d", n, kMaxDim);
  SND_CHECK_ARG(couts[n_layers - 1] <= kHeadC, "snd_e2e_train: head channels must be in [1, %d], got %d", kHeadC,
                couts[n_layers - 1]);
  SND_CHECK_ARG(ldz >= d, "snd_e2e_train: ldz %d < d %d", ldz, d);
  SND_CHECK_ARG(lddz >= d, "snd_e2e_train: lddz %d < d %d", lddz, d);
  SND_CHECK_ARG(n_graphs <= 262140, "snd_e2e_train: n_graphs %d too large for one call (train in chunks)", n_graphs);
  SND_CHECK_ARG(d_fits(n_graphs, n, d, couts[0]), "snd_e2e_train: d %d too large for one launch of layer 0", d);
  const TrainLayout lay = train_layout(n_graphs, n, d, couts, n_layers);
  SND_CHECK_ARG(workspace_bytes >= lay.total, "snd_e2e_train: workspace %zu bytes < %zu", workspace_bytes, lay.total);

  hipStream_t st = (hipStream_t)stream;
  const int B = n_graphs, L = n_layers;
  float* base = (float*)(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
  float* Y[16];
  for (int l = 0; l < L; ++l) Y[l] = base + lay.y[l];
  float* G[2] = {base + lay.g[0], base + lay.g[1]};
  float *img = base + lay.img, *P = base + lay.P, *Q = base + lay.Q, *R = base + lay.R, *S = base + lay.S;
  float *dws = base + lay.dws, *DA = base + lay.da, *slab = base + lay.slab;
  const long long pairs = (long long)B * n * n;
  const HeadArgs nohead{};

  // ---- forward: snd_e2e_decode's route, every y kept
  const snd_e2e_layer_t& l0 = layers[0];
  const int O0 = couts[0], D4 = up4(d);
  const long long nimg = (long long)n * 2 * D4 * up4(O0);
  hipLaunchKernelGGL(e2e_wsum_kernel, dim3((unsigned)cdiv(nimg, DT)), dim3(DT), 0, st, l0.w, n, d, O0, img);
  SND_LAUNCH_CHECK("e2e_wsum_kernel");
  const int ckpq = chunk_of(D4, 2LL * (n + 1), kLdsFloats - kPqRed);
  const int ng = (int)std::min<long long>(n, std::max<long long>(1, cdiv((long long)B * n, 1024)));
  hipLaunchKernelGGL(e2e_pq_kernel, dim3((unsigned)B, (unsigned)cdiv(n, ng)), dim3(DT),
                     sizeof(float) * ((size_t)2 * (n + 1) * ckpq + kPqRed), st, z, ldz, n, d, l0.gamma, l0.beta, l0.w,
                     O0, ckpq, ng, P, Q);
  SND_LAUNCH_CHECK("e2e_pq_kernel");
  L0Args a0{z, ldz, B, n, d, O0, chunk_of(D4, (long long)DG * (n + 1)), l0.gamma, l0.beta, l0.b,
            img, P, Q, Y[0], nohead};
  hipLaunchKernelGGL(e2e_l0_kernel<false>, dim3((unsigned)n, (unsigned)((B + DG - 1) / DG)), dim3(DT),
                     sizeof(float) * std::max<size_t>((size_t)DG * (n + 1) * a0.CK, 2 * DT), st, a0);
  SND_LAUNCH_CHECK("e2e_l0_kernel");
  for (int l = 1; l < L; ++l) {
    const int C = couts[l - 1], O = couts[l];
    LayerArgs a{Y[l - 1], n, C, O, chunk_of(up4(C), 2LL * n + up4(O) + 2), layers[l].gamma, layers[l].beta,
                layers[l].w, layers[l].b, Y[l], nohead};
    launch_layer<false>(a, B, st);
    SND_LAUNCH_CHECK("e2e_layer_kernel");
  }

  // ---- head, CE and dy of the last layer (gradients of the mean CE)
  int cur = 0;
  SND_TRY(snd_e2e_head_ce(Y[L - 1], adj, B, n, couts[L - 1], head_gamma, head_beta, head_w, head_b, G[cur], d_head_w,
                          d_head_b, d_head_gamma, d_head_beta, out, stream));

  // ---- general layers, last to first
  int gp;
  const int parts = wg_parts(B, &gp);
  for (int l = L - 1; l >= 1; --l) {
    const int C = couts[l - 1], O = couts[l], O4 = up4(O), nOq = O4 / 4;
    const snd_e2e_layer_grad_t& gr = layer_grads[l];
    hipLaunchKernelGGL(e2e_bias_grad_kernel, dim3((unsigned)O), dim3(DT), 0, st, G[cur], pairs, O, 2.f, gr.db);
    SND_LAUNCH_CHECK("e2e_bias_grad_kernel");
    const int crmax = std::min(C, (DT - 1) / nOq + 2);
    const int jk = std::min(n, kLdsFloats / (crmax + O4));
    WgArgs wa{Y[l - 1], G[cur], B, n, C, O, jk, crmax, gp, layers[l].gamma, layers[l].beta, slab};
    hipLaunchKernelGGL(e2e_wgrad_kernel, dim3((unsigned)n, (unsigned)parts, (unsigned)cdiv((long long)C * nOq, DT)),
                       dim3(DT), sizeof(float) * (size_t)jk * (crmax + O4), st, wa);
    SND_LAUNCH_CHECK("e2e_wgrad_kernel");
    const long long nw = (long long)n * C * O;
    hipLaunchKernelGGL(e2e_slab_sum_kernel, dim3((unsigned)cdiv(nw, DT)), dim3(DT), 0, st, slab, nw, parts, gr.dw);
    SND_LAUNCH_CHECK("e2e_slab_sum_kernel");
    DgArgs da{G[cur], n, O, C, chunk_of(O4, 2LL * n + up4(C)), layers[l].w, G[cur ^ 1]};
    launch_dgrad(da, B, st);
    SND_LAUNCH_CHECK("e2e_dgrad_kernel");
    // dx -> dy_{l-1} in place (each element is read, then written, by one thread)
    SND_TRY(snd_bn_relu_bwd(G[cur ^ 1], Y[l - 1], pairs, C, layers[l].gamma, layers[l].beta, G[cur ^ 1], gr.dgamma,
                            gr.dbeta, stream));
    cur ^= 1;
  }

  // ---- layer 0 through the factorisation
  const snd_e2e_layer_grad_t& g0 = layer_grads[0];
  const float* g = G[cur];
  const Z0 Z{z, ldz, B, n, d, O0, l0.gamma, l0.beta};
  hipLaunchKernelGGL(e2e_bias_grad_kernel, dim3((unsigned)O0), dim3(DT), 0, st, g, pairs, O0, 2.f, g0.db);
  SND_LAUNCH_CHECK("e2e_bias_grad_kernel");
  hipLaunchKernelGGL(e2e_rs_kernel, dim3((unsigned)cdiv((long long)B * n * O0, DT)), dim3(DT), 0, st, g, B, n, O0, R,
                     S);
  SND_LAUNCH_CHECK("e2e_rs_kernel");
  const long long nw0 = (long long)n * 2 * d * O0;
  hipLaunchKernelGGL(e2e_dwsum_kernel, dim3((unsigned)cdiv(nw0, DT)), dim3(DT), 0, st, Z, g, dws);
  SND_LAUNCH_CHECK("e2e_dwsum_kernel");
  hipLaunchKernelGGL(e2e_dw0_kernel, dim3((unsigned)cdiv(nw0, DT)), dim3(DT), 0, st, Z, dws, R, S, g0.dw);
  SND_LAUNCH_CHECK("e2e_dw0_kernel");
  hipLaunchKernelGGL(e2e_da_kernel, dim3((unsigned)cdiv((long long)B * n * 2 * d, DT)), dim3(DT), 0, st, Z, g, img,
                     l0.w, R, S, DA);
  SND_LAUNCH_CHECK("e2e_da_kernel");
  hipLaunchKernelGGL(e2e_dz_kernel, dim3((unsigned)cdiv((long long)B * n * d, DT)), dim3(DT), 0, st, Z, DA, dz, lddz);
  SND_LAUNCH_CHECK("e2e_dz_kernel");
  hipLaunchKernelGGL(e2e_bn0_grad_kernel, dim3((unsigned)(2 * d)), dim3(DT), 0, st, Z, DA, g0.dgamma, g0.dbeta);
  SND_LAUNCH_CHECK("e2e_bn0_grad_kernel");
  return 0;
}
